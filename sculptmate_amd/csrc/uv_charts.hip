// UV chart atlas on the device: charts that are connected pieces of surface, shelf-packed (sculpt_uv_chart_*; the rule is stated
// operation by operation in include/sculpt_hip.h and restated in tests/_chartref.py; sf3d/unwrap.py ChartUnwrapper drives it).
//
// Integer and bandwidth work, no MFMA.  What makes it reproducible:
//   * every fp64 value is a fixed sequence of IEEE operations on fp32 inputs (no contraction), every comparison is on those;
//   * the union-find is mesh_components.hip's (parent[x] <= x; links by CAS on roots, halving by relaxed stores): the label of a
//     chart is its smallest face, whatever the thread order;
//   * the rectangles are integer atomicMin / atomicMax on ordered-float keys, aggregated per wave (lanes that share a chart reduce
//     among themselves and one lane issues the four atomics: a chart of thousands of faces would queue on four addresses);
//   * the packer quantises once to units of 2^-20 and is integer prefix sums from there on.
// The packer is ONE workgroup: its scans use all 1024 threads, the row walk is thread 0 with a binary search per row (DESIGN.md
// says what that costs).  The root ranks are a three-launch scan over the faces (per-1024 totals, one workgroup over the totals,
// ranks), as in mesh_components.hip.
#include <algorithm>

#include "block_scan.h"
#include "common.h"

#pragma clang fp contract(off)

namespace sculpt {

static constexpr int UVC_BLOCK = 256;     // threads of the per-face / per-texel kernels
static constexpr int UVC_CHUNK = 1024;    // threads = elements of the kernels that take part in a scan
static constexpr long long UVC_ONE = 1ll << 20;   // the atlas side in packer units
static constexpr int UVC_MAX_HALVINGS = 80, UVC_REFINE_STEPS = 11;
static constexpr unsigned long long UVC_ERR_CAP = 1ull, UVC_ERR_PACK = 2ull;

struct UvcHeader {   // the eight int64 words at the start of the workspace
    long long n_charts;
    unsigned long long evicted, error;
    long long n_rows, evaluations;
    double scale;
    unsigned long long conflict_texels, spare;
};
static_assert(sizeof(UvcHeader) == 64, "UvcHeader is the 64-byte record the caller reads back");

struct UvcLayout {
    size_t off_parent, off_cid, off_totals, off_rect, off_cum, off_rowstart, off_rowy, total;
    int nbf;
};

static UvcLayout uvc_layout(long nf) {
    UvcLayout w;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    w.nbf = cdiv(nf, UVC_CHUNK);
    size_t o = al(sizeof(UvcHeader));
    w.off_parent = o;   o = al(o + 4 * (size_t)nf);
    w.off_cid = o;      o = al(o + 4 * (size_t)nf);
    w.off_totals = o;   o = al(o + 4 * (size_t)w.nbf);
    w.off_rect = o;     o = al(o + 16 * (size_t)nf);
    w.off_cum = o;      o = al(o + 8 * ((size_t)nf + 1));
    w.off_rowstart = o; o = al(o + 4 * (size_t)nf);
    w.off_rowy = o;     o = al(o + 8 * (size_t)nf);
    w.total = o;
    return w;
}

// ---- 1 direction ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(UVC_BLOCK) void uvc_direction_kernel(const float *__restrict__ P, int nv, const int *__restrict__ F, int nf,
                                                                  int *__restrict__ direction, float *__restrict__ pq) {
    const long f = (long)blockIdx.x * UVC_BLOCK + threadIdx.x;
    if (f >= nf) return;
    const unsigned ia = (unsigned)F[3 * f], ib = (unsigned)F[3 * f + 1], ic = (unsigned)F[3 * f + 2];
    float v[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    if (ia < (unsigned)nv && ib < (unsigned)nv && ic < (unsigned)nv) {   // (the caller validates; an index outside is not read through)
        const unsigned idx[3] = {ia, ib, ic};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            v[j][0] = P[3 * (size_t)idx[j]];
            v[j][1] = P[3 * (size_t)idx[j] + 1];
            v[j][2] = P[3 * (size_t)idx[j] + 2];
        }
    }
    const double ux = (double)v[1][0] - (double)v[0][0], uy = (double)v[1][1] - (double)v[0][1], uz = (double)v[1][2] - (double)v[0][2];
    const double wx = (double)v[2][0] - (double)v[0][0], wy = (double)v[2][1] - (double)v[0][1], wz = (double)v[2][2] - (double)v[0][2];
    const double n[3] = {uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx};
    int k = 0;
    double m = fabs(n[0]);
    if (fabs(n[1]) > m) { k = 1; m = fabs(n[1]); }
    if (fabs(n[2]) > m) k = 2;
    const bool neg = (k == 0 ? n[0] : k == 1 ? n[1] : n[2]) < 0.0;
    direction[f] = 2 * k + (neg ? 1 : 0);
    const int kp = (k + 1) % 3, kq = (k + 2) % 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float a = k == 0 ? v[j][1] : k == 1 ? v[j][2] : v[j][0];   // v[j][kp]
        const float b = k == 0 ? v[j][2] : k == 1 ? v[j][0] : v[j][1];   // v[j][kq]
        pq[6 * f + 2 * j] = neg ? b : a;
        pq[6 * f + 2 * j + 1] = neg ? a : b;
    }
    (void)kp; (void)kq;
}

// ---- 2 charts: the union-find of mesh_components.hip over the faces ----------------------------------------------------------
__device__ __forceinline__ int uvc_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root above x, halving the path.  Every trip replaces x by parent[x] < x: at most x trips.  -1 when the budget runs out.
__device__ __forceinline__ int uvc_find(int *__restrict__ parent, int x, unsigned &budget, unsigned long long *__restrict__ err) {
    int p = uvc_load(parent + x);
    while (p != x) {
        if (budget == 0) {
            atomicOr(err, UVC_ERR_CAP);
            return -1;
        }
        --budget;
        const int g = uvc_load(parent + p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // g <= p < x, x is not a root
        x = p;
        p = g;
    }
    return x;
}

// walks' trips + failed CASes <= u + v (every one lowers a cursor that stays >= 0): a budget of u + v + 2 cannot run out
__device__ __forceinline__ void uvc_union(int *__restrict__ parent, int u, int v, unsigned long long *__restrict__ err) {
    if (u == v) return;
    unsigned budget = (unsigned)u + (unsigned)v + 2u;
    int ru = uvc_find(parent, u, budget, err);
    if (ru < 0) return;
    int rv = uvc_find(parent, v, budget, err);
    if (rv < 0) return;
    while (ru != rv) {
        const int hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
        const int old = atomicCAS(parent + hi, hi, lo);   // succeeds only while hi is a root
        if (old == hi) return;
        if (budget == 0) {
            atomicOr(err, UVC_ERR_CAP);
            return;
        }
        --budget;
        ru = uvc_find(parent, old, budget, err);
        if (ru < 0) return;
        rv = lo;
    }
}

__global__ __launch_bounds__(UVC_BLOCK) void uvc_init_kernel(UvcHeader *__restrict__ hdr, int *__restrict__ parent, int nf) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        UvcHeader z;
        memset(&z, 0, sizeof(z));
        *hdr = z;
    }
    const long stride = (long)gridDim.x * UVC_BLOCK;
    for (long f = (long)blockIdx.x * UVC_BLOCK + threadIdx.x; f < nf; f += stride) parent[f] = (int)f;   // ceil(nf / stride) trips
}

// one thread per sorted half-edge position: the head of a key that occurs exactly twice joins its two faces
__global__ __launch_bounds__(UVC_BLOCK) void uvc_union_kernel(const long long *__restrict__ skeys, const long long *__restrict__ sperm,
                                                              const int *__restrict__ F, int nf, const int *__restrict__ direction,
                                                              const int *__restrict__ layer, int max_layers, int *__restrict__ parent,
                                                              UvcHeader *__restrict__ hdr) {
    const long nh = 3l * nf;
    const long i = (long)blockIdx.x * UVC_BLOCK + threadIdx.x;
    if (i >= nh) return;
    const long long key = skeys[i];
    if (i > 0 && skeys[i - 1] == key) return;
    if (i + 1 >= nh || skeys[i + 1] != key) return;
    if (i + 2 < nh && skeys[i + 2] == key) return;
    const long long h0 = sperm[i], h1 = sperm[i + 1];
    if (h0 < 0 || h0 >= nh || h1 < 0 || h1 >= nh) return;   // (a permutation of [0, 3 nf): never taken)
    if (F[h0] == F[h1]) return;                             // both run the same way
    const int f0 = (int)(h0 / 3), f1 = (int)(h1 / 3);
    if (f0 == f1) return;
    const int l0 = layer[f0];
    if (direction[f0] != direction[f1] || l0 != layer[f1] || l0 >= max_layers) return;
    uvc_union(parent, f0, f1, &hdr->error);
}

__global__ __launch_bounds__(UVC_BLOCK) void uvc_flatten_kernel(int *__restrict__ parent, int nf, int *__restrict__ label,
                                                                UvcHeader *__restrict__ hdr) {
    const long f = (long)blockIdx.x * UVC_BLOCK + threadIdx.x;
    if (f >= nf) return;
    unsigned budget = (unsigned)f + 1u;
    const int r = uvc_find(parent, (int)f, budget, &hdr->error);
    label[f] = r < 0 ? (int)f : r;   // (an error run: any in-range value; the caller refuses the result)
}

__global__ __launch_bounds__(UVC_CHUNK) void uvc_root_totals_kernel(const int *__restrict__ label, int nf, unsigned *__restrict__ totals) {
    __shared__ unsigned s_w[UVC_CHUNK / 64];
    const long f = (long)blockIdx.x * UVC_CHUNK + threadIdx.x;
    const unsigned n = block_flag_count<UVC_CHUNK / 64>(f < nf && label[f] == (int)f, s_w);
    if (threadIdx.x == 0) totals[blockIdx.x] = n;
}

__global__ __launch_bounds__(UVC_CHUNK) void uvc_scan_totals_kernel(unsigned *__restrict__ totals, int nbf, UvcHeader *__restrict__ hdr) {
    __shared__ unsigned s_w[UVC_CHUNK / 64];
    const unsigned n = block_scan_in_place<UVC_CHUNK / 64>(totals, nbf, s_w);
    if (threadIdx.x == 0) hdr->n_charts = (long long)n;
}

__global__ __launch_bounds__(UVC_CHUNK) void uvc_root_rank_kernel(const int *__restrict__ label, int nf, const unsigned *__restrict__ totals,
                                                                  int *__restrict__ cid) {
    __shared__ unsigned s_w[UVC_CHUNK / 64];
    const long f = (long)blockIdx.x * UVC_CHUNK + threadIdx.x;
    const bool root = f < nf && label[f] == (int)f;
    const unsigned r = totals[blockIdx.x] + block_flag_rank<UVC_CHUNK / 64>(root, s_w);
    if (f < nf) cid[f] = root ? (int)r : -1;
}

// ---- 3 rectangles --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(UVC_BLOCK) void uvc_rect_init_kernel(uint4 *__restrict__ rect_ord, int nf) {
    const long c = (long)blockIdx.x * UVC_BLOCK + threadIdx.x;
    if (c < nf) rect_ord[c] = make_uint4(0xffffffffu, 0u, 0xffffffffu, 0u);   // (min p, max p, min q, max q) as ordered keys
}

__global__ __launch_bounds__(UVC_BLOCK) void uvc_rect_kernel(const float *__restrict__ pq, const int *__restrict__ label,
                                                             const int *__restrict__ cid, int nf, int *__restrict__ chart,
                                                             unsigned *__restrict__ rect_ord) {
    const long f = (long)blockIdx.x * UVC_BLOCK + threadIdx.x;
    bool active = f < nf;
    int c = -1;
    unsigned pmn = 0xffffffffu, pmx = 0u, qmn = 0xffffffffu, qmx = 0u;
    if (active) {
        c = cid[label[f]];
        chart[f] = c;
        active = c >= 0 && c < nf;   // (a root always has a rank: never false)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const unsigned p = f32_to_ordered(pq[6 * f + 2 * j]), q = f32_to_ordered(pq[6 * f + 2 * j + 1]);
            pmn = min(pmn, p); pmx = max(pmx, p); qmn = min(qmn, q); qmx = max(qmx, q);
        }
    }
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(active);
    // every trip clears at least the leader's bit of `todo`: at most 64 trips
    for (int trip = 0; trip < 64 && todo; ++trip) {
        const int leader_lane = __ffsll((long long)todo) - 1;
        const int leader = __shfl(c, leader_lane, 64);
        const bool mine = active && c == leader;
        const unsigned long long same = __ballot(mine);
        unsigned a = mine ? pmn : 0xffffffffu, b = mine ? pmx : 0u, d = mine ? qmn : 0xffffffffu, e = mine ? qmx : 0u;
        if (__popcll(same) > 1) {   // wave-uniform
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                a = min(a, (unsigned)__shfl_xor((int)a, s, 64));
                b = max(b, (unsigned)__shfl_xor((int)b, s, 64));
                d = min(d, (unsigned)__shfl_xor((int)d, s, 64));
                e = max(e, (unsigned)__shfl_xor((int)e, s, 64));
            }
        }
        if (lane == leader_lane) {
            unsigned *r = rect_ord + 4 * (size_t)leader;
            atomicMin(r, a); atomicMax(r + 1, b); atomicMin(r + 2, d); atomicMax(r + 3, e);
        }
        if (mine) active = false;
        todo &= ~same;
    }
}

__global__ __launch_bounds__(UVC_BLOCK) void uvc_extent_kernel(const uint4 *__restrict__ rect_ord, int nf, const UvcHeader *__restrict__ hdr,
                                                               float4 *__restrict__ rect, double2 *__restrict__ extent,
                                                               long long *__restrict__ sort_key) {
    const long c = (long)blockIdx.x * UVC_BLOCK + threadIdx.x;
    if (c >= nf) return;
    if (c >= hdr->n_charts) {
        rect[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        extent[c] = make_double2(0.0, 0.0);
        sort_key[c] = 0x7fffffffffffffffll;
        return;
    }
    const uint4 o = rect_ord[c];
    const float pmin = ordered_to_f32(o.x), pmax = ordered_to_f32(o.y), qmin = ordered_to_f32(o.z), qmax = ordered_to_f32(o.w);
    double w = (double)pmax - (double)pmin, h = (double)qmax - (double)qmin;
    if (h > w) { const double t = w; w = h; h = t; }
    rect[c] = make_float4(pmin, pmax, qmin, qmax);
    extent[c] = make_double2(w, h);
    sort_key[c] = -__builtin_bit_cast(long long, h);   // h >= +0: its bits order like its value
}

// ---- 4 pack: one workgroup -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long uvc_quant(double s, double e, double g) { return (long long)ceil((s * e + g) * 1048576.0); }

// Is `s` feasible?  Leaves cum[0 .. C] (and, with `write`, rowstart / rowy) and *s_rows.  Called by every thread of the workgroup.
__device__ bool uvc_evaluate(double s, bool write, int C, const long long *__restrict__ order, const double *__restrict__ extent, double g,
                             long long *cum, int *rowstart, long long *rowy, long long *s_w, int *s_flag, int *s_rows) {
    bool wide = false;
    long long carry = 0;
    for (int base = 0; base < C; base += UVC_CHUNK) {   // ceil(C / 1024) trips
        const int i = base + (int)threadIdx.x;
        long long wq = 0;
        if (i < C) {
            wq = uvc_quant(s, extent[2 * order[i]], g);
            if (wq > UVC_ONE) wide = true;
        }
        long long tot;
        const long long ex = block_exclusive_add<UVC_CHUNK / 64>(wq, s_w, &tot);
        if (i < C) cum[i] = carry + ex;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) cum[C] = carry;
    const int bad = __syncthreads_or(wide ? 1 : 0);   // (also publishes cum to thread 0)
    if (threadIdx.x == 0) {
        int feasible = !bad, rows = 0, start = 0;
        long long y = 0;
        // every trip moves `start` up by at least 1 (a feasible width fits a row): at most C trips
        while (feasible && start < C) {
            if (write) { rowstart[rows] = start; rowy[rows] = y; }
            y += uvc_quant(s, extent[2 * order[start] + 1], g);
            ++rows;
            if (y > UVC_ONE) { feasible = 0; break; }
            const long long limit = cum[start] + UVC_ONE;
            int lo = start + 1, hi = C;   // the smallest j in [start + 1, C) with cum[j + 1] > limit, else C
            while (lo < hi) {             // <= 32 trips
                const int mid = lo + ((hi - lo) >> 1);
                if (cum[mid + 1] > limit) hi = mid; else lo = mid + 1;
            }
            start = lo;
        }
        *s_flag = feasible;
        *s_rows = rows;
    }
    __syncthreads();
    const bool ok = *s_flag != 0;
    __syncthreads();   // s_flag is read: the next call may write it
    return ok;
}

__global__ __launch_bounds__(UVC_CHUNK) void uvc_pack_kernel(const long long *__restrict__ order, const double *__restrict__ extent, int nf,
                                                             double g, UvcHeader *hdr, long long *cum, int *rowstart, long long *rowy,
                                                             long long *__restrict__ cell) {
    __shared__ long long s_w[UVC_CHUNK / 64];
    __shared__ double s_m[UVC_CHUNK / 64];
    __shared__ int s_flag, s_rows;
    const int tid = (int)threadIdx.x;
    const long long nc = hdr->n_charts;
    const int C = (int)(nc < 0 ? 0 : nc > nf ? nf : nc);
    double m = 0.0;
    for (int i = tid; i < C; i += UVC_CHUNK) m = fmax(m, extent[2 * i]);   // exact and order-free
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmax(m, __shfl_xor(m, d, 64));
    if ((tid & 63) == 0) s_m[tid >> 6] = m;
    __syncthreads();
    for (int w = 0; w < UVC_CHUNK / 64; ++w) m = fmax(m, s_m[w]);
    double s = 1.0;
    if (m > 0.0) {
        int e;
        (void)frexp(m, &e);
        s = ldexp(1.0, 1 - e);
    }
    int evals = 0, halvings = 0;
    bool failed = false;
    while (true) {   // <= UVC_MAX_HALVINGS + 1 trips
        ++evals;
        if (uvc_evaluate(s, false, C, order, extent, g, cum, rowstart, rowy, s_w, &s_flag, &s_rows)) break;
        if (halvings == UVC_MAX_HALVINGS) { failed = true; break; }
        ++halvings;
        s *= 0.5;
    }
    double chosen = s;
    if (!failed && halvings > 0) {
        double t = 2.0 * s;
        for (int k = 0; k < UVC_REFINE_STEPS; ++k) {
            t = t * 0.9375;
            ++evals;
            if (uvc_evaluate(t, false, C, order, extent, g, cum, rowstart, rowy, s_w, &s_flag, &s_rows)) { chosen = t; break; }
        }
    }
    ++evals;
    (void)uvc_evaluate(chosen, true, C, order, extent, g, cum, rowstart, rowy, s_w, &s_flag, &s_rows);
    const int rows = s_rows;
    if (!failed && rows > 0) {
        for (int j = tid; j < C; j += UVC_CHUNK) {   // ceil(C / 1024) trips
            int lo = 0, hi = rows;   // the last row that starts at or before j (row 0 starts at 0)
            while (hi - lo > 1) {    // <= 32 trips
                const int mid = lo + ((hi - lo) >> 1);
                if (rowstart[mid] <= j) lo = mid; else hi = mid;
            }
            const long long c = order[j];
            cell[2 * c] = cum[j] - cum[rowstart[lo]];
            cell[2 * c + 1] = rowy[lo];
        }
    }
    if (tid == 0) {
        hdr->n_rows = rows;
        hdr->evaluations = evals;
        hdr->scale = chosen;
        if (failed) atomicOr(&hdr->error, UVC_ERR_PACK);
    }
}

// ---- 5 place -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(UVC_BLOCK) void uvc_place_kernel(const float *__restrict__ pq, const int *__restrict__ chart,
                                                              const float4 *__restrict__ rect, const long long *__restrict__ cell, int nf,
                                                              double g, const UvcHeader *__restrict__ hdr, float *__restrict__ uv) {
    const long f = (long)blockIdx.x * UVC_BLOCK + threadIdx.x;
    if (f >= nf) return;
    const int c = chart[f];
    if (c < 0 || c >= nf) return;
    const float4 r = rect[c];
    const double w = (double)r.y - (double)r.x, h = (double)r.w - (double)r.z;
    const bool turned = h > w;
    const double s = hdr->scale;
    const double x0 = (double)cell[2 * (size_t)c] * (1.0 / 1048576.0) + 0.5 * g, y0 = (double)cell[2 * (size_t)c + 1] * (1.0 / 1048576.0) + 0.5 * g;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float p = pq[6 * f + 2 * j], q = pq[6 * f + 2 * j + 1];
        const double pp = turned ? (double)q - (double)r.z : (double)p - (double)r.x;
        const double qq = turned ? (double)r.y - (double)p : (double)q - (double)r.z;
        uv[6 * f + 2 * j] = (float)(x0 + s * pp);
        uv[6 * f + 2 * j + 1] = (float)(y0 + s * qq);
    }
}

// ---- 6 conflicts ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool uvc_strictly_inside(const float *__restrict__ uv, long t, double px, double py) {
    const double ax = uv[6 * t], ay = uv[6 * t + 1], bx = uv[6 * t + 2], by = uv[6 * t + 3], cx = uv[6 * t + 4], cy = uv[6 * t + 5];
    const double e0 = (bx - ax) * (py - ay) - (by - ay) * (px - ax);
    const double e1 = (cx - bx) * (py - by) - (cy - by) * (px - bx);
    const double e2 = (ax - cx) * (py - cy) - (ay - cy) * (px - cx);
    return (e0 > 0.0 && e1 > 0.0 && e2 > 0.0) || (e0 < 0.0 && e1 < 0.0 && e2 < 0.0);
}

__global__ __launch_bounds__(UVC_BLOCK) void uvc_conflict_kernel(const float4 *__restrict__ rast_low, const float4 *__restrict__ rast_high,
                                                                 int res, const float *__restrict__ uv, const int *__restrict__ chart, int nf,
                                                                 int *__restrict__ evicted, int *__restrict__ chart_conflict,
                                                                 UvcHeader *__restrict__ hdr) {
    const long t = (long)blockIdx.x * UVC_BLOCK + threadIdx.x;
    bool hit = false;
    if (t < (long)res * res) {
        const float wl = rast_low[t].w, wh = rast_high[t].w;
        if (wl >= 0.f && wh >= 0.f && wl < (float)nf && wh < (float)nf) {
            const int lo = (int)wl, hi = nf - 1 - (int)wh;
            if (lo < hi) {   // (lo > hi cannot be: both maps hold the same set of covering faces)
                const int x = (int)(t % res), y = (int)(t / res);
                const float R = (float)res;
                const float px = (float)x / R, py = 1.0f - (float)y / R;
                if (uvc_strictly_inside(uv, lo, (double)px, (double)py) && uvc_strictly_inside(uv, hi, (double)px, (double)py)) {
                    hit = true;
                    evicted[hi] = 1;   // every writer stores the same value
                    const int cl = chart[lo], ch = chart[hi];
                    if (cl >= 0 && cl < nf) chart_conflict[cl] = 1;
                    if (ch >= 0 && ch < nf) chart_conflict[ch] = 1;
                }
            }
        }
    }
    const unsigned long long m = __ballot(hit);
    if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&hdr->conflict_texels, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(UVC_BLOCK) void uvc_evict_kernel(const int *__restrict__ evicted, const int *__restrict__ chart_conflict,
                                                              const int *__restrict__ chart, int nf, int max_layers, int mode,
                                                              int *__restrict__ layer, UvcHeader *__restrict__ hdr) {
    const long f = (long)blockIdx.x * UVC_BLOCK + threadIdx.x;
    bool ev = false;
    if (f < nf) {
        ev = evicted[f] != 0;
        if (mode == 0) {
            if (ev) layer[f] += 1;
        } else if (mode == 1) {
            const int c = chart[f];
            if (c >= 0 && c < nf && chart_conflict[c]) layer[f] = max_layers;
        }
    }
    const unsigned long long m = __ballot(ev);
    if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&hdr->evicted, (unsigned long long)__popcll(m));
}

static int uvc_check_nf(const char *who, int64_t nf) {
    SC_REQUIRE(nf >= 0 && nf < (1 << 24), "%s: %lld faces (0 <= Nf < 2^24: the rasteriser carries face ids in fp32)", who, (long long)nf);
    return 0;
}

}  // namespace sculpt

using namespace sculpt;

extern "C" {

size_t sculpt_uv_chart_workspace_bytes(int64_t n_faces) {
    if (n_faces < 0 || n_faces >= (1 << 24)) return 0;
    return uvc_layout((long)n_faces).total;
}

int sculpt_uv_chart_directions(const float *P, int64_t nv, const int32_t *F, int64_t nf, int32_t *direction, float *pq,
                               sculpt_stream_t stream) {
    if (int rc = uvc_check_nf("uv_chart_directions", nf)) return rc;
    SC_REQUIRE(nv >= 0 && nv < 0x7fffffffLL, "uv_chart_directions: %lld vertices (0 <= Nv < 2^31)", (long long)nv);
    if (nf == 0) return 0;
    SC_REQUIRE(P && F && direction && pq, "uv_chart_directions: null argument");
    hipLaunchKernelGGL(uvc_direction_kernel, dim3(cdiv(nf, UVC_BLOCK)), dim3(UVC_BLOCK), 0, as_stream(stream), P, (int)nv, F, (int)nf,
                       direction, pq);
    SC_LAUNCH_CHECK();
    return 0;
}

int sculpt_uv_chart_label(const int64_t *skeys, const int64_t *sperm, const int32_t *F, int64_t n_faces, const int32_t *direction,
                          const int32_t *layer, int max_layers, int32_t *label, void *workspace, sculpt_stream_t stream) {
    hipStream_t st = as_stream(stream);
    if (int rc = uvc_check_nf("uv_chart_label", n_faces)) return rc;
    if (n_faces == 0) return 0;
    SC_REQUIRE(skeys && sperm && F && direction && layer && label && workspace, "uv_chart_label: null argument");
    SC_REQUIRE(max_layers >= 0, "uv_chart_label: max_layers %d (>= 0)", max_layers);
    const int nf = (int)n_faces;
    const UvcLayout w = uvc_layout(nf);
    char *ws = reinterpret_cast<char *>(workspace);
    UvcHeader *hdr = reinterpret_cast<UvcHeader *>(ws);
    int *parent = reinterpret_cast<int *>(ws + w.off_parent), *cid = reinterpret_cast<int *>(ws + w.off_cid);
    unsigned *totals = reinterpret_cast<unsigned *>(ws + w.off_totals);
    hipLaunchKernelGGL(uvc_init_kernel, dim3(std::max(1, std::min(cdiv(nf, UVC_BLOCK), 2048))), dim3(UVC_BLOCK), 0, st, hdr, parent, nf);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(uvc_union_kernel, dim3(cdiv(3l * nf, UVC_BLOCK)), dim3(UVC_BLOCK), 0, st, reinterpret_cast<const long long *>(skeys),
                       reinterpret_cast<const long long *>(sperm), F, nf, direction, layer, max_layers, parent, hdr);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(uvc_flatten_kernel, dim3(cdiv(nf, UVC_BLOCK)), dim3(UVC_BLOCK), 0, st, parent, nf, label, hdr);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(uvc_root_totals_kernel, dim3(w.nbf), dim3(UVC_CHUNK), 0, st, label, nf, totals);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(uvc_scan_totals_kernel, dim3(1), dim3(UVC_CHUNK), 0, st, totals, w.nbf, hdr);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(uvc_root_rank_kernel, dim3(w.nbf), dim3(UVC_CHUNK), 0, st, label, nf, totals, cid);
    SC_LAUNCH_CHECK();
    return 0;
}

int sculpt_uv_chart_rects(const float *pq, const int32_t *label, int64_t n_faces, int32_t *chart, float *rect, double *extent,
                          int64_t *sort_key, void *workspace, sculpt_stream_t stream) {
    hipStream_t st = as_stream(stream);
    if (int rc = uvc_check_nf("uv_chart_rects", n_faces)) return rc;
    if (n_faces == 0) return 0;
    SC_REQUIRE(pq && label && chart && rect && extent && sort_key && workspace, "uv_chart_rects: null argument");
    SC_REQUIRE((reinterpret_cast<uintptr_t>(rect) & 15) == 0 && (reinterpret_cast<uintptr_t>(extent) & 15) == 0,
               "uv_chart_rects: rect and extent must be 16-byte aligned");
    const int nf = (int)n_faces;
    const UvcLayout w = uvc_layout(nf);
    char *ws = reinterpret_cast<char *>(workspace);
    unsigned *rect_ord = reinterpret_cast<unsigned *>(ws + w.off_rect);
    hipLaunchKernelGGL(uvc_rect_init_kernel, dim3(cdiv(nf, UVC_BLOCK)), dim3(UVC_BLOCK), 0, st, reinterpret_cast<uint4 *>(rect_ord), nf);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(uvc_rect_kernel, dim3(cdiv(nf, UVC_BLOCK)), dim3(UVC_BLOCK), 0, st, pq, label,
                       reinterpret_cast<const int *>(ws + w.off_cid), nf, chart, rect_ord);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(uvc_extent_kernel, dim3(cdiv(nf, UVC_BLOCK)), dim3(UVC_BLOCK), 0, st, reinterpret_cast<const uint4 *>(rect_ord), nf,
                       reinterpret_cast<const UvcHeader *>(ws), reinterpret_cast<float4 *>(rect), reinterpret_cast<double2 *>(extent),
                       reinterpret_cast<long long *>(sort_key));
    SC_LAUNCH_CHECK();
    return 0;
}

int sculpt_uv_chart_pack(const int64_t *order, const double *extent, int64_t n_faces, double gutter, int64_t *cell, void *workspace,
                         sculpt_stream_t stream) {
    if (int rc = uvc_check_nf("uv_chart_pack", n_faces)) return rc;
    if (n_faces == 0) return 0;
    SC_REQUIRE(order && extent && cell && workspace, "uv_chart_pack: null argument");
    SC_REQUIRE(gutter >= 0.0 && gutter < 0.5, "uv_chart_pack: gutter %g (0 <= g < 0.5)", gutter);
    const int nf = (int)n_faces;
    const UvcLayout w = uvc_layout(nf);
    char *ws = reinterpret_cast<char *>(workspace);
    hipLaunchKernelGGL(uvc_pack_kernel, dim3(1), dim3(UVC_CHUNK), 0, as_stream(stream), reinterpret_cast<const long long *>(order), extent, nf,
                       gutter, reinterpret_cast<UvcHeader *>(ws), reinterpret_cast<long long *>(ws + w.off_cum),
                       reinterpret_cast<int *>(ws + w.off_rowstart), reinterpret_cast<long long *>(ws + w.off_rowy),
                       reinterpret_cast<long long *>(cell));
    SC_LAUNCH_CHECK();
    return 0;
}

int sculpt_uv_chart_place(const float *pq, const int32_t *chart, const float *rect, const int64_t *cell, int64_t n_faces, double gutter,
                          const void *workspace, float *uv, sculpt_stream_t stream) {
    if (int rc = uvc_check_nf("uv_chart_place", n_faces)) return rc;
    if (n_faces == 0) return 0;
    SC_REQUIRE(pq && chart && rect && cell && workspace && uv, "uv_chart_place: null argument");
    SC_REQUIRE((reinterpret_cast<uintptr_t>(rect) & 15) == 0, "uv_chart_place: rect must be 16-byte aligned");
    const int nf = (int)n_faces;
    hipLaunchKernelGGL(uvc_place_kernel, dim3(cdiv(nf, UVC_BLOCK)), dim3(UVC_BLOCK), 0, as_stream(stream), pq, chart,
                       reinterpret_cast<const float4 *>(rect), reinterpret_cast<const long long *>(cell), nf, gutter,
                       reinterpret_cast<const UvcHeader *>(workspace), uv);
    SC_LAUNCH_CHECK();
    return 0;
}

int sculpt_uv_chart_conflicts(const float *rast_low, const float *rast_high, int res, const float *uv, const int32_t *chart,
                              int64_t n_faces, int32_t *evicted, int32_t *chart_conflict, void *workspace, sculpt_stream_t stream) {
    hipStream_t st = as_stream(stream);
    if (int rc = uvc_check_nf("uv_chart_conflicts", n_faces)) return rc;
    if (n_faces == 0) return 0;
    SC_REQUIRE(rast_low && rast_high && uv && chart && evicted && chart_conflict && workspace, "uv_chart_conflicts: null argument");
    SC_REQUIRE(res >= 1 && res <= 16384, "uv_chart_conflicts: resolution %d (1 .. 16384)", res);
    SC_REQUIRE((reinterpret_cast<uintptr_t>(rast_low) & 15) == 0 && (reinterpret_cast<uintptr_t>(rast_high) & 15) == 0,
               "uv_chart_conflicts: the rasters must be 16-byte aligned");
    const int nf = (int)n_faces;
    SC_HIP(hipMemsetAsync(evicted, 0, 4 * (size_t)nf, st));
    SC_HIP(hipMemsetAsync(chart_conflict, 0, 4 * (size_t)nf, st));
    hipLaunchKernelGGL(uvc_conflict_kernel, dim3(cdiv((long)res * res, UVC_BLOCK)), dim3(UVC_BLOCK), 0, st,
                       reinterpret_cast<const float4 *>(rast_low), reinterpret_cast<const float4 *>(rast_high), res, uv, chart, nf, evicted,
                       chart_conflict, reinterpret_cast<UvcHeader *>(workspace));
    SC_LAUNCH_CHECK();
    return 0;
}

int sculpt_uv_chart_evict(const int32_t *evicted, const int32_t *chart_conflict, const int32_t *chart, int64_t n_faces, int max_layers,
                          int mode, int32_t *layer, void *workspace, sculpt_stream_t stream) {
    if (int rc = uvc_check_nf("uv_chart_evict", n_faces)) return rc;
    if (n_faces == 0) return 0;
    SC_REQUIRE(evicted && chart_conflict && chart && layer && workspace, "uv_chart_evict: null argument");
    SC_REQUIRE(mode >= 0 && mode <= 2, "uv_chart_evict: mode %d (0, 1 or 2)", mode);
    const int nf = (int)n_faces;
    hipLaunchKernelGGL(uvc_evict_kernel, dim3(cdiv(nf, UVC_BLOCK)), dim3(UVC_BLOCK), 0, as_stream(stream), evicted, chart_conflict, chart, nf,
                       max_layers, mode, layer, reinterpret_cast<UvcHeader *>(workspace));
    SC_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
