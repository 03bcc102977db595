// Surface nets ON THE DEVICE: the all-quad dual of marching cubes (sculpt_surface_nets_*, include/sculpt_hip.h has the rule;
// tests/_snref.py restates it in NumPy and vertices, quads and triangles are compared bit for bit).  One vertex inside every
// cell the surface passes through, one quad across every sign-changing lattice edge whose four cells exist.
//
// Everything is a bit mask over the lattice rows.  A ROW is (i0, i1), a WORD 32 points of it along axis 2; word L = row * W + w,
// W = ceil(n2 / 32), so the order of the words, then of the bits inside a word, IS the order of the vertices (cells (i0, i1, i2)
// lexicographic) and of the quads (key (linear point) * 3 + axis: within a point the axis is minor).  An id is therefore a
// popcount below a bit plus a prefix over the words before: no atomics, no dense cell -> vertex map, nothing that depends on
// the order the threads run in.
//   sign     one thread per point, 64-bit ballots of vol > levelf (the plain path; the signed path reads the caller's planes)
//   masks    one thread per word: the active-cell word (the 8 corner signs of a cell are 4 rows x {word, word shifted by one}),
//            the three eligible-edge words, their popcounts scanned over the workgroup's 256 words (block_scan.h) -> a packed
//            16 + 16 bit prefix per word and two totals per workgroup
//   scan     ONE workgroup: exclusive scan of the workgroup totals in place (block_scan_in_place), the two grand totals go into
//            the header, whose copy into a pinned slot + event (readback_ring.h) is what the host waits for
//   verts    one thread per point: an active cell loads its 8 corners and writes its vertex, in LATTICE UNITS
//   quads    one thread per point: an eligible edge looks its four vertex ids up by popcount, reads their lattice-unit positions
//            back for the shorter diagonal and writes the quad and its two triangles
//   affine   one thread per vertex, in place: mc.hip's map o / vert_div, rounded(o * vert_mul) + vert_add
// Workspace (deterministic, a function of the shape alone): 6 words per 32 points + 8 bytes per 8192 points + a header;
// 12.6 MB at 256^3.
#pragma clang fp contract(off)

#include <math.h>

#include <algorithm>

#include "block_scan.h"
#include "readback_ring.h"

namespace {

using namespace sculpt;

constexpr int SN_BLOCK = 256;    // threads of every kernel but the scan; also the words of one masks workgroup
constexpr int SN_SCAN = 1024;    // threads of the scan workgroup
static_assert(SN_BLOCK == 256, "bv / bq are indexed by word >> 8 and `pre` packs two 16-bit prefixes");

struct SnHeader {
    unsigned n_verts, n_quads;
    unsigned pad[14];
};

struct SnGrid {
    int n0, n1, n2, W;   // W: words per row
    long nwords;         // n0 * n1 * W
};

// the words of one shape, all of nwords uint32 unless noted
struct SnWs {
    SnHeader *hdr;
    unsigned *sign, *act, *e0, *e1, *e2;
    unsigned *pre;        // (vertices before this word in its workgroup) | (quads before it) << 16
    unsigned *bv, *bq;    // [nblocks] vertices / quads before the workgroup, after the scan
    int nblocks;
};

__device__ __forceinline__ unsigned low_bits(int k) {   // the k lowest bits, any k
    return k >= 32 ? 0xffffffffu : (k <= 0 ? 0u : ((1u << k) - 1u));
}

// -- sign: word L = row * W + w of `vol > levelf`, zero past n2.  Lane t of the wave holds point (L = t / 32, bit t % 32).
__global__ __launch_bounds__(SN_BLOCK) void sn_sign_kernel(const float *__restrict__ vol, SnGrid g, float levelf,
                                                           unsigned *__restrict__ sign) {
    const long t = (long)blockIdx.x * SN_BLOCK + threadIdx.x;
    const long L = t >> 5;
    const int bit = (int)(t & 31);
    bool in = false;
    if (L < g.nwords) {
        const long row = L / g.W;
        const int i2 = (int)(L - row * g.W) * 32 + bit;
        if (i2 < g.n2) in = vol[row * g.n2 + i2] > levelf;   // a NaN is outside
    }
    const unsigned long long m = __ballot(in);
    if (bit == 0 && L < g.nwords) sign[L] = (threadIdx.x & 32) ? (unsigned)(m >> 32) : (unsigned)m;
}

// -- masks: `sign` has `ld` words per row (the workspace's W, or the caller's planes)
__global__ __launch_bounds__(SN_BLOCK) void sn_masks_kernel(const unsigned *__restrict__ sign, int ld, SnGrid g, SnWs ws) {
    __shared__ unsigned s_w[SN_BLOCK / 64];
    const long L = (long)blockIdx.x * SN_BLOCK + threadIdx.x;
    unsigned act = 0u, e0 = 0u, e1 = 0u, e2 = 0u;
    if (L < g.nwords) {
        const long row = L / g.W;
        const int w = (int)(L - row * g.W), i0 = (int)(row / g.n1), i1 = (int)(row - (long)i0 * g.n1);
        const unsigned valid = low_bits(g.n2 - 32 * w);          // points of the row
        const unsigned cells = low_bits(g.n2 - 1 - 32 * w);      // i2 <= n2 - 2
        const unsigned inner = w == 0 ? cells & ~1u : cells;     // 1 <= i2 <= n2 - 2
        const bool up0 = i0 + 1 < g.n0, up1 = i1 + 1 < g.n1, in0 = i0 >= 1 && up0, in1 = i1 >= 1 && up1;
        const bool more = w + 1 < g.W;
        // the row's word and the same word one point on (bit b = point b + 1)
        auto word = [&](long r, unsigned &s, unsigned &sh) {
            const unsigned *p = sign + r * ld + w;
            s = p[0] & valid;
            const unsigned nxt = more ? p[1] & low_bits(g.n2 - 32 * (w + 1)) : 0u;
            sh = (s >> 1) | (nxt << 31);
        };
        unsigned s00, h00;
        word(row, s00, h00);
        unsigned any = s00 | h00, all = s00 & h00;
        if (in0 && in1) e2 = (s00 ^ h00) & cells;
        if (up1) {
            unsigned s, h;
            word(row + 1, s, h);
            any |= s | h, all &= s & h;
            if (in0) e1 = (s00 ^ s) & inner;
        }
        if (up0) {
            unsigned s, h;
            word(row + g.n1, s, h);
            any |= s | h, all &= s & h;
            if (in1) e0 = (s00 ^ s) & inner;
        }
        if (up0 && up1) {
            unsigned s, h;
            word(row + g.n1 + 1, s, h);
            any |= s | h, all &= s & h;
            act = (any & ~all) & cells;
        }
        ws.act[L] = act, ws.e0[L] = e0, ws.e1[L] = e1, ws.e2[L] = e2;
    }
    const unsigned nv = (unsigned)__popc(act), nq = (unsigned)(__popc(e0) + __popc(e1) + __popc(e2));
    unsigned tv, tq;
    const unsigned pv = block_exclusive_add<SN_BLOCK / 64>(nv, s_w, &tv);
    __syncthreads();   // s_w is used again
    const unsigned pq = block_exclusive_add<SN_BLOCK / 64>(nq, s_w, &tq);
    if (L < g.nwords) ws.pre[L] = pv | (pq << 16);   // at most 256 * 32 and 256 * 96
    if (threadIdx.x == 0) ws.bv[blockIdx.x] = tv, ws.bq[blockIdx.x] = tq;
}

__global__ __launch_bounds__(SN_SCAN) void sn_scan_kernel(SnWs ws) {
    __shared__ unsigned s_w[SN_SCAN / 64];
    const unsigned nv = block_scan_in_place<SN_SCAN / 64>(ws.bv, ws.nblocks, s_w);
    const unsigned nq = block_scan_in_place<SN_SCAN / 64>(ws.bq, ws.nblocks, s_w);
    if (threadIdx.x == 0) ws.hdr->n_verts = nv, ws.hdr->n_quads = nq;
}

// the point of thread t, or false
__device__ __forceinline__ bool point_of(const SnGrid &g, long t, long &L, int &bit, int &i0, int &i1, int &i2) {
    L = t >> 5, bit = (int)(t & 31);
    if (L >= g.nwords) return false;
    const long row = L / g.W;
    i0 = (int)(row / g.n1), i1 = (int)(row - (long)i0 * g.n1), i2 = (int)(L - row * g.W) * 32 + bit;
    return i2 < g.n2;
}

// id of the vertex of cell (c0, c1, c2), which is active
__device__ __forceinline__ unsigned vertex_id(const SnGrid &g, const SnWs &ws, int c0, int c1, int c2) {
    const long L = ((long)c0 * g.n1 + c1) * g.W + (c2 >> 5);
    return ws.bv[L >> 8] + (ws.pre[L] & 0xffffu) + (unsigned)__popc(ws.act[L] & ((1u << (c2 & 31)) - 1u));
}

// -- verts: lattice units
__global__ __launch_bounds__(SN_BLOCK) void sn_verts_kernel(const float *__restrict__ vol, SnGrid g, float levelf, double level, SnWs ws,
                                                            float *__restrict__ verts) {
    long L;
    int bit, i0, i1, i2;
    if (!point_of(g, (long)blockIdx.x * SN_BLOCK + threadIdx.x, L, bit, i0, i1, i2)) return;
    const unsigned act = ws.act[L];
    if (!((act >> bit) & 1u) || i0 + 1 >= g.n0 || i1 + 1 >= g.n1 || i2 + 1 >= g.n2) return;
    const unsigned id = ws.bv[L >> 8] + (ws.pre[L] & 0xffffu) + (unsigned)__popc(act & ((1u << bit) - 1u));
    const long s1 = g.n2, s0 = (long)g.n1 * g.n2;
    const float *c = vol + i0 * s0 + i1 * s1 + i2;
    double v[8];   // corner d0 * 4 + d1 * 2 + d2 (static indices below: the array stays in registers)
    bool in[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float f = c[(k >> 2) * s0 + ((k >> 1) & 1) * s1 + (k & 1)];
        in[k] = f > levelf;
        v[k] = (double)f;
    }
    double s[3] = {0.0, 0.0, 0.0}, n = 0.0;
    // the 12 edges: axis 0, 1, 2; within an axis the two other offsets (0,0) (0,1) (1,0) (1,1), the lower axis first
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int lo_a = j >> 1, lo_b = j & 1;   // offsets on the lower / the higher of the two other axes
            const int lo[3] = {axis == 0 ? 0 : lo_a, axis == 1 ? 0 : (axis == 0 ? lo_a : lo_b), axis == 2 ? 0 : lo_b};
            const int ka = lo[0] * 4 + lo[1] * 2 + lo[2], kb = ka + (4 >> axis);
            if (in[ka] != in[kb]) {
                double t = (level - v[ka]) / (v[kb] - v[ka]);
                if (!__builtin_isfinite(t)) t = 0.5;
#pragma unroll
                for (int k = 0; k < 3; ++k) s[k] = s[k] + ((double)lo[k] + (k == axis ? t : 0.0));
                n = n + 1.0;
            }
        }
    }
    verts[3 * (size_t)id + 0] = (float)((double)i0 + s[0] / n);
    verts[3 * (size_t)id + 1] = (float)((double)i1 + s[1] / n);
    verts[3 * (size_t)id + 2] = (float)((double)i2 + s[2] / n);
}

__device__ __forceinline__ double dist2(const float *__restrict__ P, unsigned a, unsigned b) {
    const double dx = (double)P[3 * (size_t)a] - (double)P[3 * (size_t)b], dy = (double)P[3 * (size_t)a + 1] - (double)P[3 * (size_t)b + 1],
                 dz = (double)P[3 * (size_t)a + 2] - (double)P[3 * (size_t)b + 2];
    return (dx * dx + dy * dy) + dz * dz;
}

// -- quads: `verts` still holds lattice units
template <typename IdxT>
__global__ __launch_bounds__(SN_BLOCK) void sn_quads_kernel(const float *__restrict__ vol, SnGrid g, float levelf, SnWs ws,
                                                            const float *__restrict__ verts, IdxT *__restrict__ quads,
                                                            IdxT *__restrict__ faces) {
    long L;
    int bit, i0, i1, i2;
    if (!point_of(g, (long)blockIdx.x * SN_BLOCK + threadIdx.x, L, bit, i0, i1, i2)) return;
    const unsigned e[3] = {ws.e0[L], ws.e1[L], ws.e2[L]};
    if (!(((e[0] | e[1] | e[2]) >> bit) & 1u)) return;
    const unsigned below = (1u << bit) - 1u;
    size_t q = (size_t)ws.bq[L >> 8] + (ws.pre[L] >> 16) + (unsigned)(__popc(e[0] & below) + __popc(e[1] & below) + __popc(e[2] & below));
    const bool inside = vol[((long)i0 * g.n1 + i1) * g.n2 + i2] > levelf;
    const int p[3] = {i0, i1, i2}, n[3] = {g.n0, g.n1, g.n2};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!((e[a] >> bit) & 1u)) continue;
        const int u = (a + 1) % 3, v = (a + 2) % 3;
        // (the masks say so already: nothing below reads a cell outside [0, n - 2])
        if (p[a] + 1 >= n[a] || p[u] < 1 || p[u] + 1 >= n[u] || p[v] < 1 || p[v] + 1 >= n[v]) continue;
        unsigned c[4];   // c(-1,-1), c(0,-1), c(0,0), c(-1,0)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int du = (k == 1 || k == 2) ? 0 : -1, dv = k >= 2 ? 0 : -1;
            int cell[3] = {p[0], p[1], p[2]};
            cell[u] += du, cell[v] += dv;
            c[k] = vertex_id(g, ws, cell[0], cell[1], cell[2]);
        }
        const unsigned q0 = inside ? c[0] : c[3], q1 = inside ? c[1] : c[2], q2 = inside ? c[2] : c[1], q3 = inside ? c[3] : c[0];
        if (quads) {
            IdxT *o = quads + 4 * q;
            o[0] = (IdxT)q0, o[1] = (IdxT)q1, o[2] = (IdxT)q2, o[3] = (IdxT)q3;
        }
        if (faces) {
            const double d02 = dist2(verts, q0, q2), d13 = dist2(verts, q1, q3);
            IdxT *o = faces + 6 * q;
            if (d13 < d02) {
                o[0] = (IdxT)q0, o[1] = (IdxT)q1, o[2] = (IdxT)q3, o[3] = (IdxT)q1, o[4] = (IdxT)q2, o[5] = (IdxT)q3;
            } else {
                o[0] = (IdxT)q0, o[1] = (IdxT)q1, o[2] = (IdxT)q2, o[3] = (IdxT)q0, o[4] = (IdxT)q2, o[5] = (IdxT)q3;
            }
        }
        ++q;
    }
}

// -- affine: mc.hip's map of the lattice-unit positions, operation for operation (contraction is off in this unit)
__global__ __launch_bounds__(SN_BLOCK) void sn_affine_kernel(const SnHeader *__restrict__ hdr, float vdiv, float vmul, float vadd,
                                                             float *__restrict__ verts) {
    const size_t n = 3 * (size_t)hdr->n_verts;
    for (size_t i = (size_t)blockIdx.x * SN_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * SN_BLOCK) {
        float o = verts[i] / vdiv;
        o = o * vmul;
        verts[i] = o + vadd;
    }
}

int make_grid(int n0, int n1, int n2, SnGrid *g) {
    SC_REQUIRE(n0 >= 2 && n1 >= 2 && n2 >= 2, "surface_nets: the volume must be at least 2x2x2, got %dx%dx%d", n0, n1, n2);
    // vertex ids are int32 and the quad count (at most 3 per point) a uint32
    SC_REQUIRE((long)n0 * n1 * n2 <= (1L << 30), "surface_nets: %dx%dx%d is more than 2^30 points", n0, n1, n2);
    g->n0 = n0, g->n1 = n1, g->n2 = n2, g->W = (n2 + 31) / 32;
    g->nwords = (long)n0 * n1 * g->W;
    // one thread per point of the padded rows: a launch takes fewer than 2^32 threads
    SC_REQUIRE(g->nwords < (1L << 27), "surface_nets: %dx%dx%d has %ld words of 32 points along axis 2, more than 2^27", n0, n1, n2, g->nwords);
    return 0;
}

size_t layout(const SnGrid &g, void *base, SnWs *ws) {
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    char *p = reinterpret_cast<char *>(base);
    const size_t words = al(sizeof(unsigned) * (size_t)g.nwords);
    const int nblocks = cdiv(g.nwords, SN_BLOCK);
    size_t o = al(sizeof(SnHeader));
    unsigned **arrays[] = {&ws->sign, &ws->act, &ws->e0, &ws->e1, &ws->e2, &ws->pre};
    for (unsigned **a : arrays) *a = reinterpret_cast<unsigned *>(p + o), o += words;
    ws->bv = reinterpret_cast<unsigned *>(p + o), o += al(sizeof(unsigned) * (size_t)nblocks);
    ws->bq = reinterpret_cast<unsigned *>(p + o), o += al(sizeof(unsigned) * (size_t)nblocks);
    ws->hdr = reinterpret_cast<SnHeader *>(p);
    ws->nblocks = nblocks;
    return o;
}

float level_float(double level) {   // float f > double level  <=>  f > (largest float <= level), as mc.hip has it
    float levelf = (float)level;
    if ((double)levelf > level) levelf = nextafterf(levelf, -INFINITY);
    return levelf;
}

ReadbackRing<SnHeader> g_ring{"surface_nets_count", SCULPT_ERR_MC_NO_COUNT};

}  // namespace

extern "C" {

size_t sculpt_surface_nets_workspace_bytes(int n0, int n1, int n2) {
    SnGrid g;
    SnWs ws;
    if (make_grid(n0, n1, n2, &g)) return 0;
    return layout(g, nullptr, &ws);
}

int sculpt_surface_nets_count(const float *vol, const uint32_t *sign_planes, int words_per_row, int n0, int n1, int n2, double level,
                              unsigned flags, void *workspace, int64_t *n_verts_host, int64_t *n_quads_host, sculpt_stream_t stream) {
    hipStream_t st = as_stream(stream);
    SnGrid g;
    SnWs ws;
    if (int rc = make_grid(n0, n1, n2, &g)) return rc;
    SC_REQUIRE(vol && workspace && n_verts_host && n_quads_host, "surface_nets_count: null argument");
    SC_REQUIRE(!(flags & ~SCULPT_SN_INDEX_I64), "surface_nets_count: unknown flags 0x%x", flags);
    SC_REQUIRE(((uintptr_t)workspace & 15) == 0, "surface_nets_count: the workspace must be 16-byte aligned");
    SC_REQUIRE(!sign_planes || words_per_row >= g.W, "surface_nets_count: sign plane rows too short (%d words for n2=%d)", words_per_row, n2);
    layout(g, workspace, &ws);
    *n_verts_host = *n_quads_host = 0;
    const unsigned *sign = sign_planes;
    int ld = words_per_row;
    if (!sign) {
        hipLaunchKernelGGL(sn_sign_kernel, dim3(cdiv(32 * g.nwords, SN_BLOCK)), dim3(SN_BLOCK), 0, st, vol, g, level_float(level), ws.sign);
        SC_LAUNCH_CHECK();
        sign = ws.sign, ld = g.W;
    }
    hipLaunchKernelGGL(sn_masks_kernel, dim3(ws.nblocks), dim3(SN_BLOCK), 0, st, sign, ld, g, ws);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(sn_scan_kernel, dim3(1), dim3(SN_SCAN), 0, st, ws);
    SC_LAUNCH_CHECK();
    if (int rc = g_ring.launch(workspace, ws.hdr, st)) return rc;
    SnHeader h;
    if (int rc = g_ring.read(workspace, &h)) return rc;
    *n_verts_host = (int64_t)h.n_verts;
    *n_quads_host = (int64_t)h.n_quads;
    if (h.n_verts == 0) {
        set_error("surface_nets: no cell of the volume has corners on both sides of the level");
        return SCULPT_ERR_SN_EMPTY;
    }
    return 0;
}

int sculpt_surface_nets_emit(const float *vol, int n0, int n1, int n2, double level, unsigned flags, void *workspace, float vert_div,
                             float vert_mul, float vert_add, float *verts, void *quads, void *faces, sculpt_stream_t stream) {
    hipStream_t st = as_stream(stream);
    SnGrid g;
    SnWs ws;
    if (int rc = make_grid(n0, n1, n2, &g)) return rc;
    SC_REQUIRE(vol && workspace && verts, "surface_nets_emit: null argument");
    SC_REQUIRE(!(flags & ~SCULPT_SN_INDEX_I64), "surface_nets_emit: unknown flags 0x%x", flags);
    layout(g, workspace, &ws);
    const float levelf = level_float(level);
    const int grid = cdiv(32 * g.nwords, SN_BLOCK);
    hipLaunchKernelGGL(sn_verts_kernel, dim3(grid), dim3(SN_BLOCK), 0, st, vol, g, levelf, level, ws, verts);
    SC_LAUNCH_CHECK();
    if (quads || faces) {
        if (flags & SCULPT_SN_INDEX_I64)
            hipLaunchKernelGGL(sn_quads_kernel<long long>, dim3(grid), dim3(SN_BLOCK), 0, st, vol, g, levelf, ws, (const float *)verts,
                               reinterpret_cast<long long *>(quads), reinterpret_cast<long long *>(faces));
        else
            hipLaunchKernelGGL(sn_quads_kernel<int>, dim3(grid), dim3(SN_BLOCK), 0, st, vol, g, levelf, ws, (const float *)verts,
                               reinterpret_cast<int *>(quads), reinterpret_cast<int *>(faces));
        SC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sn_affine_kernel, dim3(std::min(cdiv(3L * (g.nwords * 32), SN_BLOCK), 4096)), dim3(SN_BLOCK), 0, st, ws.hdr, vert_div,
                       vert_mul, vert_add, verts);
    SC_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
