// The image front end on the device (preprocessing.preprocess_image_device, U2netSession.predict_device): Pillow's 8-bit
// LANCZOS resample, U^2-Net's input and mask arithmetic, the cut-out's bounding box, and the cut-out + frame + grey composite
// as one gather.  Every kernel is integer or separately rounded IEEE arithmetic and is held bit for bit to the host library
// the existing path calls (tests/test_gpu_image_front.py); the contracts are stated in include/sculpt_hip.h.
#include <algorithm>
#include <mutex>
#include <vector>

#include "block_scan.h"
#include "common.h"
#include "resample_coeffs.h"

// No floating-point contraction anywhere in this file.  The compiler fuses a * b + c into one fused multiply-add by default, and
// the __fmul_rn / __fadd_rn wrappers are plain operators that inherit that default once inlined; the host formulas these kernels
// restate round every operation on its own (the grey composite over all 65 536 (value, alpha) pairs is the test).  The fp32 and
// fp64 divisions below are the compiler's correctly rounded ones.
#pragma clang fp contract(off)
// The exactness contract also needs IEEE arithmetic from the build: no fast-math, and the compiler's default correctly rounded
// fp32 division and square root (sculptmate_amd/build.py: _flags says so too).
#ifdef __FAST_MATH__
#error "image_front.hip must not be compiled with fast-math: its kernels are held bit for bit to the host library"
#endif

namespace sculpt {

static constexpr int IF_THREADS = 256;

// ---------------------------------------------------------------------------------------------
// (a) one pass of the resample: acc = 2^21 + sum pixel * k in int32, out = clamp(acc >> 22, 0, 255)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t resample_clip8(int acc) {
    const int v = acc >> RESAMPLE_PRECISION_BITS;   // arithmetic shift
    return (uint32_t)min(max(v, 0), 255);
}

// in [H][Win][C] -> out [H][Wout][C]; one thread per output byte, blockIdx.y = row
__global__ void __launch_bounds__(IF_THREADS) resample_h_kernel(const uint8_t *__restrict__ in, int Win, int C,
                                                                const int32_t *__restrict__ bounds, const int32_t *__restrict__ kk,
                                                                int ksize, uint8_t *__restrict__ out, int Wout) {
    const int j = blockIdx.x * IF_THREADS + threadIdx.x;
    if (j >= Wout * C) return;
    const int xo = j / C, c = j - xo * C;
    const int xmin = bounds[2 * xo], n = bounds[2 * xo + 1];
    const uint8_t *src = in + ((size_t)blockIdx.y * Win + xmin) * C + c;
    const int32_t *k = kk + (size_t)xo * ksize;
    int acc = 1 << (RESAMPLE_PRECISION_BITS - 1);
    for (int x = 0; x < n; ++x) acc += (int)src[(size_t)x * C] * k[x];
    out[(size_t)blockIdx.y * Wout * C + j] = (uint8_t)resample_clip8(acc);
}

// in [Hin][L] -> out [Hout][L], L = W * C bytes per row (all bytes of a row share the row's weights); blockIdx.y = output row.
// VEC: four bytes per thread through one aligned dword (L % 4 == 0 and both images 4-byte aligned).
template <bool VEC>
__global__ void __launch_bounds__(IF_THREADS) resample_v_kernel(const uint8_t *__restrict__ in, int L,
                                                                const int32_t *__restrict__ bounds, const int32_t *__restrict__ kk,
                                                                int ksize, uint8_t *__restrict__ out) {
    const int yo = blockIdx.y;
    const int ymin = bounds[2 * yo], n = bounds[2 * yo + 1];
    const int32_t *k = kk + (size_t)yo * ksize;
    const int j = (blockIdx.x * IF_THREADS + threadIdx.x) * (VEC ? 4 : 1);
    if (j >= L) return;
    const uint8_t *src = in + (size_t)ymin * L + j;
    if (VEC) {
        int a0 = 1 << (RESAMPLE_PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
        for (int y = 0; y < n; ++y) {
            const uint32_t p = *reinterpret_cast<const uint32_t *>(src + (size_t)y * L);
            const int w = k[y];
            a0 += (int)(p & 255u) * w;
            a1 += (int)((p >> 8) & 255u) * w;
            a2 += (int)((p >> 16) & 255u) * w;
            a3 += (int)(p >> 24) * w;
        }
        *reinterpret_cast<uint32_t *>(out + (size_t)yo * L + j) =
            resample_clip8(a0) | (resample_clip8(a1) << 8) | (resample_clip8(a2) << 16) | (resample_clip8(a3) << 24);
    } else {
        int acc = 1 << (RESAMPLE_PRECISION_BITS - 1);
        for (int y = 0; y < n; ++y) acc += (int)src[(size_t)y * L] * k[y];
        out[(size_t)yo * L + j] = (uint8_t)resample_clip8(acc);
    }
}

// ---------------------------------------------------------------------------------------------
// small reductions: the workspaces are set by a one-thread launch, then reduced per block in LDS and once per block in HBM
// ---------------------------------------------------------------------------------------------
__global__ void set4_kernel(int32_t *ws, int a, int b, int c, int d) {
    ws[0] = a;
    ws[1] = b;
    ws[2] = c;
    ws[3] = d;
}

// ws[0] = max over the first three channels of an [n][C] uint8 image
__global__ void __launch_bounds__(IF_THREADS) u8_max3_kernel(const uint8_t *__restrict__ img, long n, int C, int32_t *ws) {
    __shared__ int smax;
    if (threadIdx.x == 0) smax = 0;
    __syncthreads();
    int m = 0;
    for (long i = (long)blockIdx.x * IF_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * IF_THREADS) {
        const uint8_t *p = img + i * C;
        m = max(m, max((int)p[0], max((int)p[1], (int)p[2])));
    }
    atomicMax(&smax, m);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&ws[0], smax);
}

// (b) out[c][i] = (float)(((double)v / max - mean[c]) / std[c]): three fp64 operations rounded on their own, one rounding to fp32
__global__ void __launch_bounds__(IF_THREADS) u2net_input_kernel(const uint8_t *__restrict__ img, long n, int C,
                                                                 const int32_t *__restrict__ ws, double m0, double m1, double m2,
                                                                 double s0, double s1, double s2, float *__restrict__ out) {
    const long i = (long)blockIdx.x * IF_THREADS + threadIdx.x;
    if (i >= n) return;
    const double mx = (double)ws[0];
    const uint8_t *p = img + i * C;
    out[i] = (float)(((double)p[0] / mx - m0) / s0);
    out[n + i] = (float)(((double)p[1] / mx - m1) / s1);
    out[2 * n + i] = (float)(((double)p[2] / mx - m2) / s2);
}

// ws[0] = ordered key (f32_to_ordered) of the minimum, ws[1] = of the maximum (set to 0xffffffff / 0 before); NaNs take no part
__global__ void __launch_bounds__(IF_THREADS) f32_minmax_kernel(const float *__restrict__ d, long n, uint32_t *ws) {
    __shared__ uint32_t smin, smax;
    if (threadIdx.x == 0) {
        smin = 0xffffffffu;
        smax = 0u;
    }
    __syncthreads();
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (long i = (long)blockIdx.x * IF_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * IF_THREADS) {
        const float v = d[i];
        if (v == v) {
            const uint32_t k = f32_to_ordered(v);
            lo = min(lo, k);
            hi = max(hi, k);
        }
    }
    atomicMin(&smin, lo);
    atomicMax(&smax, hi);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(&ws[0], smin);
        atomicMax(&ws[1], smax);
    }
}

// (c) m = (uint8)(((d - mi) / (ma - mi)) * 255), every fp32 operation rounded on its own, truncating conversion; ma == mi -> 0
__global__ void __launch_bounds__(IF_THREADS) u2net_mask_kernel(const float *__restrict__ d, long n, const uint32_t *__restrict__ ws,
                                                                uint8_t *__restrict__ mask) {
    const long i = (long)blockIdx.x * IF_THREADS + threadIdx.x;
    if (i >= n) return;
    const float mi = ordered_to_f32(ws[0]), ma = ordered_to_f32(ws[1]);
    const float span = ma - mi;
    uint8_t m = 0;
    if (ma > mi) {   // false as well when the image holds no number at all (both keys untouched: NaN patterns)
        const float v = ((d[i] - mi) / span) * 255.0f;
        m = (uint8_t)min(max((int)v, 0), 255);   // (int) truncates; a NaN pixel gives 0
    }
    mask[i] = m;
}

// ---------------------------------------------------------------------------------------------
// (d), (e) the cut-out: Image.composite(img, transparent, mask) is, per byte, md255(value, M) with alpha 255 for RGB input
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int md255(int a, int b) {
    const int t = a * b + 128;
    return ((t >> 8) + t) >> 8;
}

// ws = {ymin, ymax, xmin, xmax} of alpha' > 0, both ends inclusive; set to {H, -1, W, -1} before.  blockIdx.y = row.
__global__ void __launch_bounds__(IF_THREADS) cutout_bbox_kernel(const uint8_t *__restrict__ img, const uint8_t *__restrict__ mask,
                                                                 int W, int C, int32_t *ws) {
    __shared__ int sxmin, sxmax;
    if (threadIdx.x == 0) {
        sxmin = W;
        sxmax = -1;
    }
    __syncthreads();
    const int y = blockIdx.y;
    int lo = W, hi = -1;
    for (int x = blockIdx.x * IF_THREADS + threadIdx.x; x < W; x += gridDim.x * IF_THREADS) {
        const size_t i = (size_t)y * W + x;
        const int a = C == 4 ? (int)img[i * 4 + 3] : 255;
        if (md255(a, (int)mask[i]) > 0) {
            lo = min(lo, x);
            hi = max(hi, x);
        }
    }
    if (hi >= 0) {
        atomicMin(&sxmin, lo);
        atomicMax(&sxmax, hi);
    }
    __syncthreads();
    if (threadIdx.x == 0 && sxmax >= 0) {
        atomicMin(&ws[0], y);
        atomicMax(&ws[1], y);
        atomicMin(&ws[2], sxmin);
        atomicMax(&ws[3], sxmax);
    }
}

// out [S][S][grey ? 3 : 4]: pixel (oy, ox) is the cut-out's pixel (y0 + oy - top, x0 + ox - left) inside the h x w box and
// transparent black outside; grey: composited on 0.5 grey as preprocess_image does in fp32, every operation rounded on its own.
__global__ void __launch_bounds__(IF_THREADS) cutout_frame_kernel(const uint8_t *__restrict__ img, const uint8_t *__restrict__ mask,
                                                                  int W, int C, int y0, int x0, int h, int w, int top, int left,
                                                                  int S, int grey, uint8_t *__restrict__ out) {
    const int ox = blockIdx.x * IF_THREADS + threadIdx.x, oy = blockIdx.y;
    if (ox >= S) return;
    const int by = oy - top, bx = ox - left;
    int r = 0, g = 0, b = 0, a = 0;
    if (by >= 0 && by < h && bx >= 0 && bx < w) {
        const size_t i = (size_t)(y0 + by) * W + (x0 + bx);
        const int m = mask[i];
        const uint8_t *p = img + i * C;
        r = md255(p[0], m);
        g = md255(p[1], m);
        b = md255(p[2], m);
        a = md255(C == 4 ? (int)p[3] : 255, m);
    }
    const size_t o = (size_t)oy * S + ox;
    if (!grey) {
        out[o * 4 + 0] = (uint8_t)r;
        out[o * 4 + 1] = (uint8_t)g;
        out[o * 4 + 2] = (uint8_t)b;
        out[o * 4 + 3] = (uint8_t)a;
        return;
    }
    const float fa = (float)a / 255.0f;
    const float back = (1.0f - fa) * 0.5f;
    const int v[3] = {r, g, b};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float rgb = ((float)v[c] / 255.0f) * fa + back;
        out[o * 3 + c] = (uint8_t)(int)(rgb * 255.0f);
    }
}

// (f) out = v / 255 in fp32, a rounded division
__global__ void __launch_bounds__(IF_THREADS) u8_to_unit_f32_kernel(const uint8_t *__restrict__ in, long n, float *__restrict__ out) {
    const long i = (long)blockIdx.x * IF_THREADS + threadIdx.x;
    if (i < n) out[i] = (float)in[i] / 255.0f;
}

// ---------------------------------------------------------------------------------------------
// The bounding box's way to the host: a copy of the four integers into a pinned slot behind the kernel, an event behind the
// copy, and a wait for THAT EVENT (as marching cubes reads its counts, mc.hip).  Slots are created on first use and reused; the
// library has no teardown, so they live as long as the process.  The mutex is never held across the wait.
// ---------------------------------------------------------------------------------------------
struct BboxSlot {
    int dev;
    int32_t *host;   // pinned, 4 words
    hipEvent_t ev;
    bool busy;
};
static std::mutex g_bbox_mu;
static std::vector<BboxSlot> g_bbox_slots;

static int bbox_slot_acquire(int *index) {
    int dev = 0;
    SC_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_bbox_mu);
    for (size_t i = 0; i < g_bbox_slots.size(); ++i)
        if (!g_bbox_slots[i].busy && g_bbox_slots[i].dev == dev) {
            g_bbox_slots[i].busy = true;
            *index = (int)i;
            return 0;
        }
    void *p = nullptr;
    SC_HIP(hipHostMalloc(&p, 4 * sizeof(int32_t), hipHostMallocDefault));
    hipEvent_t ev;
    if (hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) {
        (void)hipHostFree(p);
        set_error("hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
        return 1;
    }
    g_bbox_slots.push_back(BboxSlot{dev, reinterpret_cast<int32_t *>(p), ev, true});
    *index = (int)g_bbox_slots.size() - 1;
    return 0;
}

static void bbox_slot_release(int index) {
    std::lock_guard<std::mutex> lock(g_bbox_mu);
    g_bbox_slots[index].busy = false;
}

static int bbox_copy_and_wait(int index, const int32_t *ws, hipStream_t st, int32_t *out4) {
    int32_t *host;
    hipEvent_t ev;
    {
        std::lock_guard<std::mutex> lock(g_bbox_mu);   // the vector may grow under another thread
        host = g_bbox_slots[index].host;
        ev = g_bbox_slots[index].ev;
    }
    SC_HIP(hipMemcpyAsync(host, ws, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SC_HIP(hipEventRecord(ev, st));
    SC_HIP(hipEventSynchronize(ev));
    memcpy(out4, host, 4 * sizeof(int32_t));
    return 0;
}

static bool image_dims_ok(int H, int W) { return H >= 1 && W >= 1 && H <= RESAMPLE_MAX_SIZE && W <= RESAMPLE_MAX_SIZE; }

static int reduce_blocks(long n) { return (int)std::min<long>(std::max<long>(cdiv(n, IF_THREADS), 1), 4L * num_cus()); }

}  // namespace sculpt

using namespace sculpt;

extern "C" {

int sculpt_resample_lanczos_ksize(int in_size, int out_size) { return resample_lanczos_ksize(in_size, out_size); }

int sculpt_resample_lanczos_coeffs(int in_size, int out_size, int ksize, int32_t *bounds_host, int32_t *kk_host) {
    SC_REQUIRE(bounds_host && kk_host, "resample_lanczos_coeffs: null table");
    SC_REQUIRE(ksize >= 1 && ksize == resample_lanczos_ksize(in_size, out_size),
               "resample_lanczos_coeffs: ksize %d is not sculpt_resample_lanczos_ksize(%d, %d)", ksize, in_size, out_size);
    std::vector<double> scratch((size_t)ksize);
    SC_REQUIRE(resample_lanczos_fill(in_size, out_size, ksize, bounds_host, kk_host, scratch.data()) == 0,
               "resample_lanczos_coeffs: bad sizes %d -> %d", in_size, out_size);
    return 0;
}

int sculpt_resample_u8(const uint8_t *in_hwc, int Hin, int Win, int C, const int32_t *bounds_x, const int32_t *kk_x, int ksize_x,
                       const int32_t *bounds_y, const int32_t *kk_y, int ksize_y, uint8_t *tmp, uint8_t *out_hwc, int Hout, int Wout,
                       sculpt_stream_t stream) {
    SC_REQUIRE(in_hwc && out_hwc, "resample_u8: null image");
    SC_REQUIRE(C == 1 || C == 3 || C == 4, "resample_u8: %d channels (1, 3 or 4)", C);
    SC_REQUIRE(image_dims_ok(Hin, Win) && image_dims_ok(Hout, Wout), "resample_u8: %d x %d -> %d x %d is outside [1, %d]", Hin, Win,
               Hout, Wout, RESAMPLE_MAX_SIZE);
    const bool horiz = Win != Wout, vert = Hin != Hout;
    SC_REQUIRE(!horiz || (bounds_x && kk_x && ksize_x == resample_lanczos_ksize(Win, Wout)),
               "resample_u8: the horizontal pass needs the tables of %d -> %d (ksize %d)", Win, Wout, resample_lanczos_ksize(Win, Wout));
    SC_REQUIRE(!vert || (bounds_y && kk_y && ksize_y == resample_lanczos_ksize(Hin, Hout)),
               "resample_u8: the vertical pass needs the tables of %d -> %d (ksize %d)", Hin, Hout, resample_lanczos_ksize(Hin, Hout));
    SC_REQUIRE(!(horiz && vert) || tmp, "resample_u8: two passes need the Hin x Wout x C intermediate");
    hipStream_t st = as_stream(stream);
    if (!horiz && !vert) {
        SC_HIP(hipMemcpyAsync(out_hwc, in_hwc, (size_t)Hin * Win * C, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    const uint8_t *vin = in_hwc;
    if (horiz) {
        uint8_t *hout = vert ? tmp : out_hwc;
        resample_h_kernel<<<dim3(cdiv((long)Wout * C, IF_THREADS), Hin), IF_THREADS, 0, st>>>(in_hwc, Win, C, bounds_x, kk_x, ksize_x,
                                                                                              hout, Wout);
        SC_LAUNCH_CHECK();
        vin = hout;
    }
    if (vert) {
        const int L = Wout * C;
        const bool vec = L % 4 == 0 && ((uintptr_t)vin | (uintptr_t)out_hwc) % 4 == 0;
        if (vec)
            resample_v_kernel<true><<<dim3(cdiv(L / 4, IF_THREADS), Hout), IF_THREADS, 0, st>>>(vin, L, bounds_y, kk_y, ksize_y, out_hwc);
        else
            resample_v_kernel<false><<<dim3(cdiv(L, IF_THREADS), Hout), IF_THREADS, 0, st>>>(vin, L, bounds_y, kk_y, ksize_y, out_hwc);
        SC_LAUNCH_CHECK();
    }
    return 0;
}

int sculpt_u2net_input(const uint8_t *img_hwc, int H, int W, int C, const double *mean3_host, const double *std3_host, int32_t *ws,
                       float *out_chw, sculpt_stream_t stream) {
    SC_REQUIRE(img_hwc && mean3_host && std3_host && ws && out_chw, "u2net_input: null argument");
    SC_REQUIRE((C == 3 || C == 4) && image_dims_ok(H, W), "u2net_input: %d x %d x %d", H, W, C);
    hipStream_t st = as_stream(stream);
    const long n = (long)H * W;
    set4_kernel<<<1, 1, 0, st>>>(ws, 0, 0, 0, 0);
    u8_max3_kernel<<<reduce_blocks(n), IF_THREADS, 0, st>>>(img_hwc, n, C, ws);
    u2net_input_kernel<<<cdiv(n, IF_THREADS), IF_THREADS, 0, st>>>(img_hwc, n, C, ws, mean3_host[0], mean3_host[1], mean3_host[2],
                                                                    std3_host[0], std3_host[1], std3_host[2], out_chw);
    SC_LAUNCH_CHECK();
    return 0;
}

int sculpt_u2net_mask(const float *d0, int64_t n, uint32_t *ws, uint8_t *mask, sculpt_stream_t stream) {
    SC_REQUIRE(d0 && ws && mask, "u2net_mask: null argument");
    SC_REQUIRE(n >= 1 && n <= (int64_t)RESAMPLE_MAX_SIZE * RESAMPLE_MAX_SIZE, "u2net_mask: %lld elements", (long long)n);
    hipStream_t st = as_stream(stream);
    set4_kernel<<<1, 1, 0, st>>>(reinterpret_cast<int32_t *>(ws), -1, 0, 0, 0);
    f32_minmax_kernel<<<reduce_blocks(n), IF_THREADS, 0, st>>>(d0, n, ws);
    u2net_mask_kernel<<<cdiv(n, IF_THREADS), IF_THREADS, 0, st>>>(d0, n, ws, mask);
    SC_LAUNCH_CHECK();
    return 0;
}

int sculpt_cutout_bbox(const uint8_t *img_hwc, const uint8_t *mask, int H, int W, int C, int32_t *ws, int32_t *bbox_host,
                       sculpt_stream_t stream) {
    SC_REQUIRE(mask && ws && bbox_host, "cutout_bbox: null argument");
    SC_REQUIRE((C == 3 || (C == 4 && img_hwc)) && image_dims_ok(H, W), "cutout_bbox: %d x %d x %d", H, W, C);
    hipStream_t st = as_stream(stream);
    int slot = -1;
    if (int rc = bbox_slot_acquire(&slot)) return rc;
    set4_kernel<<<1, 1, 0, st>>>(ws, H, -1, W, -1);
    cutout_bbox_kernel<<<dim3(std::min(cdiv(W, IF_THREADS), 8), H), IF_THREADS, 0, st>>>(img_hwc, mask, W, C, ws);
    int rc = hipGetLastError() == hipSuccess ? 0 : 1;
    if (rc) set_error("cutout_bbox: the launch failed");
    if (!rc) rc = bbox_copy_and_wait(slot, ws, st, bbox_host);
    bbox_slot_release(slot);
    return rc;
}

int sculpt_cutout_frame(const uint8_t *img_hwc, const uint8_t *mask, int H, int W, int C, int y0, int x0, int h, int w, int top,
                        int left, int S, int grey, uint8_t *out, sculpt_stream_t stream) {
    SC_REQUIRE(img_hwc && mask && out, "cutout_frame: null argument");
    SC_REQUIRE((C == 3 || C == 4) && image_dims_ok(H, W) && S >= 1 && S <= RESAMPLE_MAX_SIZE, "cutout_frame: %d x %d x %d -> %d", H, W,
               C, S);
    SC_REQUIRE(h >= 0 && w >= 0 && y0 >= 0 && x0 >= 0 && y0 + h <= H && x0 + w <= W, "cutout_frame: the box [%d, %d) x [%d, %d) leaves the %d x %d image",
               y0, y0 + h, x0, x0 + w, H, W);
    SC_REQUIRE(top >= 0 && left >= 0 && top + h <= S && left + w <= S, "cutout_frame: the %d x %d box at (%d, %d) leaves the %d-pixel frame", h,
               w, top, left, S);
    cutout_frame_kernel<<<dim3(cdiv(S, IF_THREADS), S), IF_THREADS, 0, as_stream(stream)>>>(img_hwc, mask, W, C, y0, x0, h, w, top, left,
                                                                                           S, grey ? 1 : 0, out);
    SC_LAUNCH_CHECK();
    return 0;
}

int sculpt_u8_to_unit_f32(const uint8_t *in, int64_t n, float *out, sculpt_stream_t stream) {
    SC_REQUIRE(in && out && n >= 1 && n <= (int64_t)4 * RESAMPLE_MAX_SIZE * RESAMPLE_MAX_SIZE, "u8_to_unit_f32: %lld elements", (long long)n);
    u8_to_unit_f32_kernel<<<cdiv(n, IF_THREADS), IF_THREADS, 0, as_stream(stream)>>>(in, n, out);
    SC_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
