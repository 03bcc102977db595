// Mesh smoothing ON THE DEVICE: Taubin's lambda|mu filter (sculpt_smooth_*, include/sculpt_hip.h; driven by
// sculptmate_amd/sf3d/remesh_device.py smooth_device).  The faces do not change, so everything topological is built once per
// call and the iterations are a pure gather:
//   neighbour table   CSR over the vertices, row u = the distinct neighbours of u in ascending index order.  From the unique
//                     edges of the topology (sculpt_rmd_topo_t): edge_keys writes the two directed keys (u << 32 | v),
//                     (v << 32 | u) of every edge, the caller sorts them (the row offsets are a searchsorted of u << 32), and
//                     neighbours takes the low words.  A sort of distinct keys: no atomics, one possible result.
//   fixed vertices    the caller's flags (sculpt_rmd_boundary on zeroes: an edge at the vertex without exactly two faces)
//   half-step         one thread per vertex, factor k (lambda, then mu), positions in 16-byte rows (x y z -):
//                         s = p[nb[first]], then s = s + p[nb[j]] in row order      per component, fp32
//                         c = s / (float)deg                                         IEEE division
//                         q = p + k * (c - p)                                        three operations
//                     a fixed vertex and a vertex without neighbours keep p.  It reads one buffer and writes the other, so the
//                     result does not depend on scheduling; a neighbour costs one 16-byte load.
// The unit is compiled with floating-point contraction OFF (the pragma below, before the shared helpers): every value is a
// fixed sequence of IEEE fp32 operations, which tests/_smoothref.py restates in NumPy operation for operation -- positions are
// compared bit for bit.
#pragma clang fp contract(off)

#include "remesh_topo.h"

namespace {

__global__ void smooth_edge_keys_kernel(Topo T, int64_t *__restrict__ keys) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T.ne) return;
    int u, v;
    edge_ends(T, (int)e, u, v);
    keys[2 * e] = ((int64_t)u << 32) | (int64_t)(uint32_t)v;
    keys[2 * e + 1] = ((int64_t)v << 32) | (int64_t)(uint32_t)u;
}

__global__ void smooth_neighbours_kernel(const int64_t *__restrict__ skeys, long n, int32_t *__restrict__ nb) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    nb[i] = (int32_t)(skeys[i] & 0xffffffff);
}

__global__ void smooth_pack_kernel(const float *__restrict__ P, long nv, float4 *__restrict__ p4) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nv) return;
    p4[u] = make_float4(P[3 * u], P[3 * u + 1], P[3 * u + 2], 0.0f);
}

__global__ void smooth_unpack_kernel(const float4 *__restrict__ p4, long nv, float *__restrict__ P) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nv) return;
    const float4 p = p4[u];
    P[3 * u] = p.x, P[3 * u + 1] = p.y, P[3 * u + 2] = p.z;
}

__global__ void smooth_half_step_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ nb, const uint8_t *__restrict__ fixed,
                                        long nv, float k, const float4 *__restrict__ p, float4 *__restrict__ q) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nv) return;
    float4 pu = p[u];
    const int b = start[u], e = start[u + 1];
    if (e > b && !fixed[u]) {
        const float4 first = p[nb[b]];
        float sx = first.x, sy = first.y, sz = first.z;
#pragma unroll 4
        for (int j = b + 1; j < e; ++j) {  // any degree: the loads of an unrolled group are independent, the adds stay in row order
            const float4 t = p[nb[j]];
            sx = sx + t.x, sy = sy + t.y, sz = sz + t.z;
        }
        const float deg = (float)(e - b);
        const float cx = sx / deg, cy = sy / deg, cz = sz / deg;
        pu.x = pu.x + k * (cx - pu.x);
        pu.y = pu.y + k * (cy - pu.y);
        pu.z = pu.z + k * (cz - pu.z);
    }
    q[u] = pu;
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int sculpt_smooth_edge_keys(const sculpt_rmd_topo_t *topo, int64_t *keys, sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "smooth_edge_keys")) return rc;
    SC_REQUIRE(topo->ne <= 3 * topo->nf, "smooth_edge_keys: %lld edges on %lld faces", (long long)topo->ne, (long long)topo->nf);
    SC_REQUIRE(topo->ne == 0 || keys, "smooth_edge_keys: null keys");
    RMD_LAUNCH(smooth_edge_keys_kernel, topo->ne, topo_of(topo), keys);
    return 0;
}

int sculpt_smooth_neighbours(const int64_t *skeys, int64_t n, int32_t *nb, sculpt_stream_t stream) {
    SC_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "smooth_neighbours: n=%lld out of range", (long long)n);
    SC_REQUIRE(n == 0 || (skeys && nb), "smooth_neighbours: null array");
    RMD_LAUNCH(smooth_neighbours_kernel, n, skeys, (long)n, nb);
    return 0;
}

int sculpt_smooth_taubin(const int32_t *start, const int32_t *nb, const uint8_t *fixed, int64_t nv, int64_t n_nb, const float *P,
                         int iterations, double lam, double mu, float *work_a, float *work_b, float *out, sculpt_stream_t stream) {
    SC_REQUIRE(nv >= 0 && nv < ((int64_t)1 << 31) && n_nb >= 0 && n_nb < ((int64_t)1 << 31), "smooth_taubin: nv=%lld, n_nb=%lld out of range",
               (long long)nv, (long long)n_nb);
    SC_REQUIRE(iterations >= 1 && iterations <= 1000, "smooth_taubin: iterations=%d (1 .. 1000)", iterations);
    SC_REQUIRE(lam > 0 && lam <= 1, "smooth_taubin: lambda=%g (0 < lambda <= 1)", lam);  // a NaN fails every comparison
    SC_REQUIRE(mu == 0 || (mu >= -1 && mu < -lam), "smooth_taubin: mu=%g (0, or -1 <= mu < -lambda)", mu);
    if (nv == 0) return 0;
    SC_REQUIRE(start && fixed && P && work_a && work_b && out, "smooth_taubin: null array");
    SC_REQUIRE(n_nb == 0 || nb, "smooth_taubin: null neighbour table");
    SC_REQUIRE(aligned16(work_a) && aligned16(work_b) && work_a != work_b, "smooth_taubin: the two work buffers must be distinct and 16-byte aligned");
    float4 *a = reinterpret_cast<float4 *>(work_a), *b = reinterpret_cast<float4 *>(work_b);
    RMD_LAUNCH(smooth_pack_kernel, nv, P, (long)nv, a);
    const float k[2] = {(float)lam, (float)mu};
    for (int it = 0; it < iterations; ++it)
        for (int half = 0; half < (mu == 0 ? 1 : 2); ++half) {  // mu == 0: plain Laplacian, no second half-step
            RMD_LAUNCH(smooth_half_step_kernel, nv, start, nb, fixed, (long)nv, k[half], a, b);
            float4 *t = a;
            a = b;
            b = t;
        }
    RMD_LAUNCH(smooth_unpack_kernel, nv, a, (long)nv, out);
    return 0;
}

}  // extern "C"
