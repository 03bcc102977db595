// Gradient of the raw density with respect to the query point, and the unit normal of its iso-surfaces, for gfx950 (MI355X).
//
// Restates (reference file:line), differentiated with respect to `positions`:
//   TriplaneNeRFRenderer.query_triplane / _query_chunk   TripoSR/tsr/models/nerf_renderer.py:41-91
//   NeRFMLP.forward                                       TripoSR/tsr/models/network_utils.py:116-124
//
// Shape:
//   * forward mode.  A wave owns one 32-column MFMA tile = 8 points x 4 columns {value, d/dx, d/dy, d/dz}: lane
//     (p = lane & 31, h = lane >> 5) holds column p, of point p >> 2 and kind p & 3.  The two halves h split the layer-0
//     features and the neurons exactly as in query_points_kernel (csrc/triplane.hip).
//   * layer 0 is linear in the four bilinear tap weights, so a tangent column runs point_taps + layer0_channel_last with the
//     DERIVATIVES of the weights in their place and its accumulators started at 0 (the bias belongs to the value).  The
//     derivative is floor's one-sided one (torch autograd's): the cell of the point, also when it sits on a cell edge.
//   * the hidden layers are hidden_layers' MFMA sequence for all 32 columns; between two layers a value column takes SiLU and
//     a tangent column t = s'(a) * a_t, with a the pre-activation of the same neuron in the value column of its quad
//     (one DPP quad broadcast per register, no LDS).  Activations are carried scaled by log2(e) (triplane_mlp.h): s(y) = y * sg,
//     sg = 1 / (1 + 2^-y), s'(y) = sg * (1 + y ln2 (1 - sg)); scaled tangents stay consistent through the hidden weights and the
//     last layer's x ln2 restores true units.
//   * a column's bits depend on that column alone (an MFMA column reads its own B column), and a value column runs the point
//     query's own operations: `density` is ops.triplane_query's from channel-last planes bit for bit, and a point's result does
//     not depend on N or on where in which tile the point sits.
#include <algorithm>

#include "common.h"
#include "triplane_mlp.h"

namespace sculpt {

// value of lane (lane & ~3): v_mov_b32 with quad_perm:[K,K,K,K]
template <int K>
__device__ __forceinline__ float quad_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), K * 0x55, 0xf, 0xf, true));
}

// The weights a column of kind `kind` (0 = value, 1 + axis = tangent) hands to layer 0.  wt comes in from point_taps (the value's
// weights) and stays for kind 0.  A tangent along world axis a gets, per plane, d(weight)/d(pixel coordinate) * d(pixel
// coordinate)/d(world coordinate) on the plane axis that reads a, and 0 on a plane that does not read it.
template <bool AC>
__device__ __forceinline__ void tangent_weights(int kind, float px, float py, float pz, float radius, float span, int H, int W,
                                                float (&wt)[3][4]) {
    if (kind == 0) return;
    const int a = kind - 1;
    const float q[3] = {to_unit(px, radius, span), to_unit(py, radius, span), to_unit(pz, radius, span)};
    // d(unit)/d(world) = 2 / span; d(pixel)/d(unit) = size / 2, or (size - 1) / 2 with align_corners
    const float du = 2.0f / span;
    const float sx = du * ((float)(AC ? W - 1 : W) * 0.5f), sy = du * ((float)(AC ? H - 1 : H) * 0.5f);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        const int ia = pl == 2 ? 1 : 0, ib = pl == 0 ? 1 : 2;
        const Tap1 tx = tap_of<AC>(q[ia], W), ty = tap_of<AC>(q[ib], H);
        const float wx = tx.w1, ex = 1.0f - wx, wy = ty.w1, ey = 1.0f - wy;
        const int x0 = tx.i0, x1 = x0 + 1, y0 = ty.i0, y1 = y0 + 1;
        const bool vx0 = x0 >= 0 && x0 < W, vx1 = x1 >= 0 && x1 < W;
        const bool vy0 = y0 >= 0 && y0 < H, vy1 = y1 >= 0 && y1 < H;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
        if (a == ia) {  // d/dfx of (ey ex, ey wx, wy ex, wy wx)
            d0 = -ey * sx; d1 = ey * sx; d2 = -wy * sx; d3 = wy * sx;
        } else if (a == ib) {  // d/dfy
            d0 = -ex * sy; d1 = -wx * sy; d2 = ex * sy; d3 = wx * sy;
        }
        wt[pl][0] = (vy0 && vx0) ? d0 : 0.f;
        wt[pl][1] = (vy0 && vx1) ? d1 : 0.f;
        wt[pl][2] = (vy1 && vx0) ? d2 : 0.f;
        wt[pl][3] = (vy1 && vx1) ? d3 : 0.f;
    }
}

// The step between two layers on 16 accumulator registers: SiLU on a value column (silu16's operations, the same bits), the
// chain rule on a tangent column.  Every lane computes the sigmoid of its quad's value column.
__device__ __forceinline__ f32x16 act16(const f32x16 &acc, bool is_value) {
    f32x16 o;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float y = quad_bcast<0>(acc[i]);
        const float e = __builtin_amdgcn_exp2f(-y);
        const float sg = __builtin_amdgcn_rcpf(e + 1.0f);
        const float val = y * sg;
        const float der = sg * (1.0f + (y * 0.69314718055994530942f) * (1.0f - sg));
        o[i] = is_value ? val : der * acc[i];
    }
    return o;
}

// hidden_layers (triplane_mlp.h) with act16 between the layers; in: layer-0 accumulators, out: what the last layer reads
__device__ __forceinline__ void hidden_layers_fwd(const LdsView &L, int NH, int lane, int h, bool is_value, f32x16 &x0,
                                                  f32x16 &x1) {
    x0 = act16(x0, is_value);
    x1 = act16(x1, is_value);
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int l = 0; l < NH; ++l) {
        f32x16 acc0 = is_value ? lds_bias16(L.bacc, l + 1, h, 0) : zero;
        f32x16 acc1 = is_value ? lds_bias16(L.bacc, l + 1, h, 1) : zero;
        const f32x4 *A0 = reinterpret_cast<const f32x4 *>(L.hid) + ((l * 2 + 0) * 8) * 64 + lane;
        const f32x4 *A1 = reinterpret_cast<const f32x4 *>(L.hid) + ((l * 2 + 1) * 8) * 64 + lane;
#pragma unroll
        for (int s4 = 0; s4 < 8; ++s4) {
            f32x4 a0 = A0[s4 * 64];
            f32x4 a1 = A1[s4 * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int s = s4 * 4 + j;
                const float b = (s < 16) ? x0[s & 15] : x1[s & 15];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b, acc1, 0, 0, 0);
            }
        }
        x0 = act16(acc0, is_value);
        x1 = act16(acc1, is_value);
    }
}

// last_dot (triplane_mlp.h) of row 0 without the bias
__device__ __forceinline__ float last_dot0_nobias(const LdsView &L, int h, const f32x16 &x0, const f32x16 &x1) {
    const float *w = L.wlast + h * 32;
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) s = fmaf(w[r], x0[r], s);
#pragma unroll
    for (int r = 0; r < 16; ++r) s = fmaf(w[16 + r], x1[r], s);
    s += __shfl_xor(s, 32, 64);
    return s;
}

template <int C, bool AC>
__global__ __launch_bounds__(512) void density_grad_kernel(
    const float *__restrict__ planes, int H, int W, const float *__restrict__ blob, const float *__restrict__ pts, long N,
    float radius, float span, float *__restrict__ grad, float *__restrict__ normal, float *__restrict__ density, int a0_lds) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpPackHeader hd = *reinterpret_cast<const MlpPackHeader *>(blob);
    const int NH = hd.NH;
    float *a0s = smem + lds_floats_for(NH);
    if (a0_lds) stage_a0_in_lds<C>(a0s, blob, hd);
    load_weights_to_lds(smem, blob, hd);
    const LdsView L = lds_view(smem, NH);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const int p = lane & 31, h = lane >> 5;
    const int kind = p & 3;
    const bool is_value = kind == 0;
    const long ntiles = (N + 7) / 8;
    const float *A0g = blob + hd.off_a0;
    const long HW = (long)H * W;
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    for (long tile = (long)blockIdx.x * nwave + wave; tile < ntiles; tile += (long)gridDim.x * nwave) {
        long n = tile * 8 + (p >> 2);
        const bool valid = n < N;
        if (!valid) n = N - 1;
        const float px = pts[3 * n], py = pts[3 * n + 1], pz = pts[3 * n + 2];
        int off[3][4];
        float wt[3][4];
        point_taps<AC>(px, py, pz, radius, span, H, W, off, wt);
        tangent_weights<AC>(kind, px, py, pz, radius, span, H, W, wt);
        f32x16 x0 = is_value ? lds_bias16(L.bacc, 0, h, 0) : zero;
        f32x16 x1 = is_value ? lds_bias16(L.bacc, 0, h, 1) : zero;
        layer0_channel_last<C>(planes, HW, off, wt, a0s, A0g, a0_lds, lane, h, x0, x1);
        hidden_layers_fwd(L, NH, lane, h, is_value, x0, x1);
        const float s = last_dot0_nobias(L, h, x0, x1);
        const float d = s + L.blast[0];
        // the quad's three tangents into the point's lane
        const float gx = quad_bcast<1>(s), gy = quad_bcast<2>(s), gz = quad_bcast<3>(s);
        if (valid && is_value && h == 0) {
            if (density) density[n] = d;
            if (grad) { grad[3 * n] = gx; grad[3 * n + 1] = gy; grad[3 * n + 2] = gz; }
            if (normal) {
                // -g / |g|, with g scaled by a power of two first so that no square overflows or vanishes
                const float m = fmaxf(fmaxf(fabsf(gx), fabsf(gy)), fabsf(gz));
                float nx = 0.f, ny = 0.f, nz = 0.f;
                const bool finite = fabsf(gx) < INFINITY && fabsf(gy) < INFINITY && fabsf(gz) < INFINITY;
                if (finite && m > 0.f) {
                    const int e = -ilogbf(m);
                    const float ux = ldexpf(gx, e), uy = ldexpf(gy, e), uz = ldexpf(gz, e);
                    const float len = sqrtf(ux * ux + uy * uy + uz * uz);
                    nx = -ux / len; ny = -uy / len; nz = -uz / len;
                }
                normal[3 * n] = nx; normal[3 * n + 1] = ny; normal[3 * n + 2] = nz;
            }
        }
    }
}

}  // namespace sculpt

using namespace sculpt;

extern "C" int sculpt_triplane_density_grad(const float *planes_cl, int C, int H, int W, const void *mlp_packed, int n_hidden_64,
                                            const float *points, long long N, float radius, int flags, float *grad,
                                            float *normal, float *density, sculpt_stream_t stream) {
    SC_REQUIRE(C == 40, "triplane_density_grad: built for C=40 channels per plane (got %d)", C);
    SC_REQUIRE(planes_cl && mlp_packed, "triplane_density_grad: null input");
    SC_REQUIRE(H >= 1 && W >= 1, "triplane_density_grad: bad plane size %d x %d", H, W);
    SC_REQUIRE(N >= 0, "triplane_density_grad: negative point count %lld", N);
    SC_REQUIRE((flags & ~(int)SCULPT_QUERY_ALIGN_CORNERS) == 0, "triplane_density_grad: unknown flags %d", flags);
    SC_REQUIRE(n_hidden_64 >= 0, "triplane_density_grad: bad n_hidden_64");
    SC_REQUIRE(radius > 0.f, "triplane_density_grad: radius must be positive");
    if (N == 0) return 0;   // empty arrays have no address: nothing to refuse, nothing to launch
    SC_REQUIRE(grad || normal || density, "triplane_density_grad: no output asked for (grad, normal and density are all null)");
    SC_REQUIRE(points, "triplane_density_grad: null points");
    size_t lds = (size_t)lds_floats_for(n_hidden_64) * sizeof(float);
    SC_REQUIRE(lds <= 160 * 1024, "triplane_density_grad: %d hidden layers do not fit LDS", n_hidden_64);
    const size_t a0_bytes = (size_t)3 * C * 64 * sizeof(float);
    const int a0_lds = lds + a0_bytes <= 160 * 1024 ? 1 : 0;
    if (a0_lds) lds += a0_bytes;
    auto kern = (flags & (int)SCULPT_QUERY_ALIGN_CORNERS) ? density_grad_kernel<40, true> : density_grad_kernel<40, false>;
    SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long ntiles = ((long)N + 7) / 8;
    const int grid = (int)std::min<long>((ntiles + 7) / 8, num_cus());
    const float span = (float)((double)radius - (double)(-radius));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, as_stream(stream), planes_cl, H, W,
                       reinterpret_cast<const float *>(mlp_packed), points, (long)N, radius, span, grad, normal, density, a0_lds);
    SC_LAUNCH_CHECK();
    return 0;
}
