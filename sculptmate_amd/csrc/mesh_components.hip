// Connected components of an indexed triangle mesh on the device, and the mesh without its small ones ("floaters").
//
// Input: faces [Nf][3] (int32 or int64) over Nv shared vertices, as marching cubes emits them; connectivity is through the vertex
// indices alone (no edge table, no sort).  Integer work only: every result is exact and the same from run to run.
//
// LABEL  Lock-free union-find over the vertices (the ECL-CC scheme).  parent[v] = v at the start; one thread per face unions
//        (f0, f1) and (f0, f2); a flatten pass -- a launch of its own, so that every link is visible -- writes
//        labels[v] = find(v) into a separate array.
//   THE INVARIANT: parent[x] <= x, always, and parent[x] is a vertex of x's tree.  A slot changes in two ways only:
//     (a) a LINK, atomicCAS(parent + hi, hi, lo) with lo < hi: it succeeds only while hi is still a root, so a root is linked at
//         most once and a vertex that stopped being a root never becomes one again;
//     (b) path HALVING, a relaxed agent-scope store of g = parent[parent[x]] into parent[x], with g <= parent[x] < x as they were
//         read: only on a vertex seen as a non-root (so it never meets a CAS that could still succeed on that slot), and only
//         to a vertex of x's own tree below x.  Two halvings of one slot may land in either order; either value is such a vertex.
//         (atomicMin in its place keeps the slot monotone and was measured slower: 0.25 against 0.20 ms of labelling on the
//         123 128-face sphere of tools/time_mesh_components.py.)
//   So every walk x -> parent[x] strictly descends and ends at a root after at most x steps, whatever the other threads do.
//   Every link puts the larger root under a smaller vertex, and the smallest vertex of a component can therefore never be linked:
//   when all unions are done it is the root of the component's one tree.  Labels depend on neither thread order nor face order,
//   without any ordering of the atomics.
//   Loads inside a walk are relaxed agent-scope atomic loads (they bypass the CU's L1).  A walk may still see an older parent
//   than the newest one: every value a slot ever held is a vertex of the same tree below x, and trees only merge.  The decision
//   "hi is a root, link it" is made by the CAS alone, and a failed CAS continues from the value the CAS returned, never from a
//   plain re-read.
//   EVERY LOOP HAS A BUDGET that cannot run out while the invariant holds (stated at each loop).  A thread whose budget runs out
//   sets CC_ERR_CAP in the header's error word and leaves; the host turns the word into sculpt_last_error() and a non-zero return.
//   A face with an index outside [0, Nv) is never read through: it is skipped everywhere and sets CC_ERR_INDEX.
//   A face with repeated indices is a no-op union and still counts as a face of its component.
// COUNT  faces and vertices per component at the root's slot.  The usual input is one giant component plus dust, so one atomic per
//        face would queue on one address: lanes of a wave that share a label add once with their number (ballot + popcount,
//        looping over the distinct labels left), and the first such group of every wave goes through LDS so that a workgroup
//        whose waves agree adds once.  Integer atomics only.
// SELECT "largest" = the maximum of (face count, then smallest root): one packed 64-bit atomicMax over the roots, reduced per
//        workgroup first.  min_faces: count >= min_faces.  fraction x: (double)count >= x * (double)largest_count.
//        A component without faces (a vertex no face references) is never kept.
// COMPACT, stable: flags -> per-1024 totals -> one workgroup scans the totals -> the compact kernels recompute the flag, rank it
//        inside the 1024 with ballots and add the scanned base.  Order is preserved: the result is the input with rows deleted.
//        (The count, rank and scan are block_scan.h's.)
#include <algorithm>

#include "block_scan.h"
#include "common.h"
#include "readback_ring.h"

namespace sculpt {

static constexpr int CC_BLOCK = 256;     // threads of the per-face kernels (one face per thread)
static constexpr int CC_CHUNK = 1024;    // threads = elements of the kernels that take part in a scan
static constexpr unsigned CC_ERR_INDEX = 1u, CC_ERR_CAP = 2u;

struct CcHeader {                  // first 64 bytes of the workspace; what the host reads back
    unsigned long long best;       // max over the roots of (face count << 32) | (0xffffffff - root)
    double fraction;               // rule 3
    unsigned n_components;         // roots, isolated vertices included
    unsigned kept_nv, kept_nf;
    unsigned error;                // CC_ERR_*
    unsigned rule, min_faces;      // SCULPT_CC_KEEP_*, rule 2
    unsigned pad[6];
};
static_assert(sizeof(CcHeader) == 64, "CcHeader is the 64-byte read-back record");

struct CcLayout {
    size_t off_parent, off_labels, off_fcount, off_vcount, off_bt_root, off_bt_keepv, off_bt_keepf, total;
    int nbv, nbf;                  // 1024-element chunks of the vertices / faces
};

static CcLayout cc_layout(long nv, long nf) {
    CcLayout w;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    w.nbv = cdiv(nv, CC_CHUNK);
    w.nbf = cdiv(nf, CC_CHUNK);
    size_t o = al(sizeof(CcHeader));
    w.off_parent = o;   o = al(o + 4 * (size_t)nv);     // after the scans: the new index of every kept vertex, -1 elsewhere
    w.off_labels = o;   o = al(o + 4 * (size_t)nv);
    w.off_fcount = o;   o = al(o + 4 * (size_t)nv);
    w.off_vcount = o;   o = al(o + 4 * (size_t)nv);
    w.off_bt_root = o;  o = al(o + 4 * (size_t)w.nbv);
    w.off_bt_keepv = o; o = al(o + 4 * (size_t)w.nbv);
    w.off_bt_keepf = o; o = al(o + 4 * (size_t)w.nbf);
    w.total = o;
    return w;
}

__device__ __forceinline__ int cc_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root above x, halving the path on the way.  Returns -1 (and sets CC_ERR_CAP) when `budget` runs out.
// Bound: every trip replaces x by parent[x] < x (the invariant), so a walk from x makes at most x trips.
__device__ __forceinline__ int cc_find(int *__restrict__ parent, int x, unsigned &budget, unsigned *__restrict__ err) {
    int p = cc_load(parent + x);
    while (p != x) {
        if (budget == 0) {
            atomicOr(err, CC_ERR_CAP);
            return -1;
        }
        --budget;
        const int g = cc_load(parent + p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (b): g <= p < x, x is not a root
        x = p;
        p = g;
    }
    return x;
}

// Bound of the whole union: two cursors start at u and v; every trip of a walk lowers one of them by at least 1, and so does a
// failed CAS (it returns parent[hi] < hi, and the walk goes on from there); both stay >= 0.  So walks' trips + failed CASes
// <= u + v, and a budget of u + v + 2 cannot run out.
__device__ __forceinline__ void cc_union(int *__restrict__ parent, int u, int v, unsigned *__restrict__ err) {
    if (u == v) return;
    unsigned budget = (unsigned)u + (unsigned)v + 2u;
    int ru = cc_find(parent, u, budget, err);
    if (ru < 0) return;
    int rv = cc_find(parent, v, budget, err);
    if (rv < 0) return;
    while (ru != rv) {
        const int hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
        const int old = atomicCAS(parent + hi, hi, lo);   // (a)
        if (old == hi) return;
        if (budget == 0) {
            atomicOr(err, CC_ERR_CAP);
            return;
        }
        --budget;
        ru = cc_find(parent, old, budget, err);   // hi was no root any more: go on from what the CAS returned
        if (ru < 0) return;
        rv = lo;   // (it may have been linked meanwhile: linking under a non-root of the other tree merges the trees all the same)
    }
}

// the three indices of face i, or false when one is outside [0, nv)
template <typename IdxT>
__device__ __forceinline__ bool cc_face(const IdxT *__restrict__ faces, long i, int nv, int &a, int &b, int &c) {
    const long long x = faces[3 * i], y = faces[3 * i + 1], z = faces[3 * i + 2];
    const unsigned long long n = (unsigned long long)nv;
    if ((unsigned long long)x >= n || (unsigned long long)y >= n || (unsigned long long)z >= n) return false;
    a = (int)x; b = (int)y; c = (int)z;
    return true;
}

__global__ __launch_bounds__(CC_BLOCK) void cc_init_kernel(CcHeader *__restrict__ hdr, CcHeader init, int *__restrict__ parent,
                                                           unsigned *__restrict__ fcount, unsigned *__restrict__ vcount, int nv) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *hdr = init;
    const int stride = gridDim.x * CC_BLOCK;
    for (long v = (long)blockIdx.x * CC_BLOCK + threadIdx.x; v < nv; v += stride) {   // ceil(nv / stride) trips
        parent[v] = (int)v;
        if (fcount) { fcount[v] = 0u; vcount[v] = 0u; }
    }
}

template <typename IdxT>
__global__ __launch_bounds__(CC_BLOCK) void cc_union_kernel(const IdxT *__restrict__ faces, int nf, int nv, int *__restrict__ parent,
                                                            CcHeader *__restrict__ hdr) {
    const long i = (long)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (i >= nf) return;
    int a, b, c;
    if (!cc_face(faces, i, nv, a, b, c)) {
        atomicOr(&hdr->error, CC_ERR_INDEX);
        return;
    }
    cc_union(parent, a, b, &hdr->error);
    cc_union(parent, a, c, &hdr->error);
}

__global__ __launch_bounds__(CC_BLOCK) void cc_flatten_kernel(int *__restrict__ parent, int nv, int *__restrict__ labels,
                                                              CcHeader *__restrict__ hdr) {
    const long v = (long)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (v >= nv) return;
    unsigned budget = (unsigned)v + 1u;   // a walk from v makes at most v trips
    const int r = cc_find(parent, (int)v, budget, &hdr->error);
    labels[v] = r < 0 ? (int)v : r;       // (an error run: any in-range value; the host refuses the result)
}

// counts[lab] += 1 for every active thread, with one atomic per distinct label of a wave, and the first group of every wave
// merged across the workgroup in LDS.  Called by every thread of the workgroup (it has a barrier inside).
template <int NWAVES>
__device__ __forceinline__ void cc_aggregated_add(unsigned *__restrict__ counts, int lab, bool active, int *s_lab, unsigned *s_cnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long todo = __ballot(active);
    if (lane == 0) { s_lab[wave] = -1; s_cnt[wave] = 0u; }
    bool first = true;
    // every trip clears at least the leader's bit of `todo`: at most 64 trips
    for (int trip = 0; trip < 64 && todo; ++trip) {
        const int leader_lane = __ffsll((long long)todo) - 1;
        const int leader = __shfl(lab, leader_lane, 64);
        const bool mine = active && lab == leader;
        const unsigned long long same = __ballot(mine);
        if (lane == leader_lane) {
            if (first) { s_lab[wave] = leader; s_cnt[wave] = (unsigned)__popcll(same); }
            else atomicAdd(counts + leader, (unsigned)__popcll(same));
        }
        if (mine) active = false;
        todo &= ~same;
        first = false;
    }
    __syncthreads();
    if (threadIdx.x < NWAVES) {
        const int my = s_lab[threadIdx.x];
        unsigned sum = 0u;
        bool lowest = true;
        for (int j = 0; j < NWAVES; ++j)   // NWAVES trips
            if (s_lab[j] == my) {
                sum += s_cnt[j];
                if (j < (int)threadIdx.x) lowest = false;
            }
        if (my >= 0 && lowest) atomicAdd(counts + my, sum);
    }
}

template <typename IdxT>
__global__ __launch_bounds__(CC_BLOCK) void cc_count_faces_kernel(const IdxT *__restrict__ faces, int nf, int nv,
                                                                  const int *__restrict__ labels, unsigned *__restrict__ fcount) {
    __shared__ int s_lab[CC_BLOCK / 64];
    __shared__ unsigned s_cnt[CC_BLOCK / 64];
    const long i = (long)blockIdx.x * CC_BLOCK + threadIdx.x;
    int a = 0, b, c;
    const bool ok = i < nf && cc_face(faces, i, nv, a, b, c);
    cc_aggregated_add<CC_BLOCK / 64>(fcount, ok ? labels[a] : -1, ok, s_lab, s_cnt);
}

// vertex counts at the roots, the number of roots per 1024 vertices, and the "largest" key
__global__ __launch_bounds__(CC_CHUNK) void cc_count_verts_kernel(const int *__restrict__ labels, int nv,
                                                                  const unsigned *__restrict__ fcount, unsigned *__restrict__ vcount,
                                                                  unsigned *__restrict__ bt_root, CcHeader *__restrict__ hdr) {
    __shared__ int s_lab[CC_CHUNK / 64];
    __shared__ unsigned s_cnt[CC_CHUNK / 64];
    __shared__ unsigned s_w[CC_CHUNK / 64];
    __shared__ unsigned long long s_best[CC_CHUNK / 64];
    const long v = (long)blockIdx.x * CC_CHUNK + threadIdx.x;
    const bool ok = v < nv;
    const int lab = ok ? labels[v] : -1;
    const bool root = ok && lab == (int)v;
    unsigned long long key = root ? (((unsigned long long)fcount[v] << 32) | (0xffffffffull - (unsigned long long)v)) : 0ull;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = key;
    cc_aggregated_add<CC_CHUNK / 64>(vcount, lab, ok, s_lab, s_cnt);   // (its barrier also publishes s_best)
    if (threadIdx.x == 0) {
        unsigned long long best = 0ull;
        for (int w = 0; w < CC_CHUNK / 64; ++w) best = s_best[w] > best ? s_best[w] : best;   // 16 trips
        if (best) atomicMax(&hdr->best, best);
    }
    const unsigned nroot = block_flag_count<CC_CHUNK / 64>(root, s_w);
    if (threadIdx.x == 0) bt_root[blockIdx.x] = nroot;
}

// is the component of root `root` kept?  `cnt` = its face count
__device__ __forceinline__ bool cc_keep(unsigned rule, unsigned min_faces, double fraction, unsigned long long best, unsigned cnt, int root) {
    if (cnt == 0u) return false;
    if (rule == SCULPT_CC_KEEP_LARGEST) return (unsigned)root == 0xffffffffu - (unsigned)(best & 0xffffffffull);
    if (rule == SCULPT_CC_KEEP_MIN_FACES) return cnt >= min_faces;
    if (rule == SCULPT_CC_KEEP_FRACTION) return (double)cnt >= fraction * (double)(unsigned)(best >> 32);
    return false;
}

struct CcRule { unsigned rule, min_faces; double fraction; unsigned long long best; };
__device__ __forceinline__ CcRule cc_rule(const CcHeader *__restrict__ hdr) { return CcRule{hdr->rule, hdr->min_faces, hdr->fraction, hdr->best}; }

__device__ __forceinline__ bool cc_vertex_kept(const CcRule &r, const int *__restrict__ labels, const unsigned *__restrict__ fcount, long v, int nv) {
    if (v >= nv) return false;
    const int lab = labels[v];
    return cc_keep(r.rule, r.min_faces, r.fraction, r.best, fcount[lab], lab);
}

template <typename IdxT>
__device__ __forceinline__ bool cc_face_kept(const CcRule &r, const IdxT *__restrict__ faces, const int *__restrict__ labels,
                                             const unsigned *__restrict__ fcount, long i, int nf, int nv, int &a, int &b, int &c) {
    if (i >= nf || !cc_face(faces, i, nv, a, b, c)) return false;
    const int lab = labels[a];
    return cc_keep(r.rule, r.min_faces, r.fraction, r.best, fcount[lab], lab);
}

// kept vertices / faces per 1024: workgroups [0, nbv) take the vertices, [nbv, nbv + nbf) the faces
template <typename IdxT>
__global__ __launch_bounds__(CC_CHUNK) void cc_keep_totals_kernel(const IdxT *__restrict__ faces, int nf, int nv, int nbv,
                                                                  const int *__restrict__ labels, const unsigned *__restrict__ fcount,
                                                                  const CcHeader *__restrict__ hdr, unsigned *__restrict__ bt_keepv,
                                                                  unsigned *__restrict__ bt_keepf) {
    __shared__ unsigned s_w[CC_CHUNK / 64];
    const CcRule r = cc_rule(hdr);
    const bool verts = (int)blockIdx.x < nbv;   // workgroup-uniform
    const int blk = verts ? (int)blockIdx.x : (int)blockIdx.x - nbv;
    const long i = (long)blk * CC_CHUNK + threadIdx.x;
    int a, b, c;
    const bool kept = verts ? cc_vertex_kept(r, labels, fcount, i, nv) : cc_face_kept(r, faces, labels, fcount, i, nf, nv, a, b, c);
    const unsigned total = block_flag_count<CC_CHUNK / 64>(kept, s_w);
    if (threadIdx.x == 0) (verts ? bt_keepv : bt_keepf)[blk] = total;
}

__global__ __launch_bounds__(CC_CHUNK) void cc_scan_totals_kernel(unsigned *__restrict__ bt_root, unsigned *__restrict__ bt_keepv,
                                                                  unsigned *__restrict__ bt_keepf, int nbv, int nbf,
                                                                  CcHeader *__restrict__ hdr) {
    __shared__ unsigned s_w[CC_CHUNK / 64];
    const unsigned nroot = block_scan_in_place<CC_CHUNK / 64>(bt_root, nbv, s_w);
    unsigned kv = 0u, kf = 0u;
    if (bt_keepv) {
        kv = block_scan_in_place<CC_CHUNK / 64>(bt_keepv, nbv, s_w);
        kf = block_scan_in_place<CC_CHUNK / 64>(bt_keepf, nbf, s_w);
    }
    if (threadIdx.x == 0) {
        hdr->n_components = nroot;
        hdr->kept_nv = kv;
        hdr->kept_nf = kf;
    }
}

// kept vertex rows, their old indices, and new_id[v] (the old `parent` array) = the new index or -1
__global__ __launch_bounds__(CC_CHUNK) void cc_compact_verts_kernel(const float *__restrict__ vertices, int nv, const int *__restrict__ labels,
                                                                    const unsigned *__restrict__ fcount, const CcHeader *__restrict__ hdr,
                                                                    const unsigned *__restrict__ bt_keepv, int *__restrict__ new_id,
                                                                    float *__restrict__ out_v, long long *__restrict__ vertex_index,
                                                                    unsigned long long cap) {
    __shared__ unsigned s_w[CC_CHUNK / 64];
    const CcRule r = cc_rule(hdr);
    const long v = (long)blockIdx.x * CC_CHUNK + threadIdx.x;
    const bool keep = cc_vertex_kept(r, labels, fcount, v, nv);
    const unsigned long long dst = (unsigned long long)bt_keepv[blockIdx.x] + block_flag_rank<CC_CHUNK / 64>(keep, s_w);
    if (v < nv) new_id[v] = (keep && dst < cap) ? (int)dst : -1;
    if (keep && dst < cap) {
        out_v[3 * dst] = vertices[3 * v];
        out_v[3 * dst + 1] = vertices[3 * v + 1];
        out_v[3 * dst + 2] = vertices[3 * v + 2];
        vertex_index[dst] = (long long)v;
    }
}

template <typename IdxT>
__global__ __launch_bounds__(CC_CHUNK) void cc_compact_faces_kernel(const IdxT *__restrict__ faces, int nf, int nv, const int *__restrict__ labels,
                                                                    const unsigned *__restrict__ fcount, const CcHeader *__restrict__ hdr,
                                                                    const unsigned *__restrict__ bt_keepf, const int *__restrict__ new_id,
                                                                    IdxT *__restrict__ out_f, long long *__restrict__ face_index,
                                                                    unsigned long long cap) {
    __shared__ unsigned s_w[CC_CHUNK / 64];
    const CcRule r = cc_rule(hdr);
    const long i = (long)blockIdx.x * CC_CHUNK + threadIdx.x;
    int a = 0, b = 0, c = 0;
    const bool keep = cc_face_kept(r, faces, labels, fcount, i, nf, nv, a, b, c);
    const unsigned long long dst = (unsigned long long)bt_keepf[blockIdx.x] + block_flag_rank<CC_CHUNK / 64>(keep, s_w);
    if (keep && dst < cap) {   // (a kept face's three vertices carry its label: all three have a new index)
        out_f[3 * dst] = (IdxT)new_id[a];
        out_f[3 * dst + 1] = (IdxT)new_id[b];
        out_f[3 * dst + 2] = (IdxT)new_id[c];
        face_index[dst] = (long long)i;
    }
}

// every root ascending, with its counts
__global__ __launch_bounds__(CC_CHUNK) void cc_report_kernel(const int *__restrict__ labels, int nv, const unsigned *__restrict__ fcount,
                                                             const unsigned *__restrict__ vcount, const unsigned *__restrict__ bt_root,
                                                             int *__restrict__ roots, int *__restrict__ face_counts,
                                                             int *__restrict__ vertex_counts, unsigned long long cap) {
    __shared__ unsigned s_w[CC_CHUNK / 64];
    const long v = (long)blockIdx.x * CC_CHUNK + threadIdx.x;
    const bool root = v < nv && labels[v] == (int)v;
    const unsigned long long dst = (unsigned long long)bt_root[blockIdx.x] + block_flag_rank<CC_CHUNK / 64>(root, s_w);
    if (root && dst < cap) {
        roots[dst] = (int)v;
        face_counts[dst] = (int)fcount[v];
        vertex_counts[dst] = (int)vcount[v];
    }
}

static ReadbackRing<CcHeader> g_cc_ring{"mesh_components", SCULPT_ERR_MESH_COMPONENTS};

static int cc_check_sizes(const char *who, int64_t nv, int64_t nf) {
    SC_REQUIRE(nv >= 0 && nv < 0x7fffffffLL, "%s: %lld vertices (0 <= Nv < 2^31)", who, (long long)nv);
    SC_REQUIRE(nf >= 0 && nf < 0x7fffffffLL, "%s: %lld faces (0 <= Nf < 2^31)", who, (long long)nf);
    return 0;
}

// init + union + flatten into `labels`
static int cc_label(const void *faces, int faces_i64, int nf, int nv, const CcHeader &init, char *ws, const CcLayout &w, int *labels,
                    bool with_counts, hipStream_t st) {
    CcHeader *hdr = reinterpret_cast<CcHeader *>(ws);
    int *parent = reinterpret_cast<int *>(ws + w.off_parent);
    const int igrid = std::max(1, std::min(cdiv(nv, CC_BLOCK), 2048));
    hipLaunchKernelGGL(cc_init_kernel, dim3(igrid), dim3(CC_BLOCK), 0, st, hdr, init, parent,
                       with_counts ? reinterpret_cast<unsigned *>(ws + w.off_fcount) : nullptr,
                       with_counts ? reinterpret_cast<unsigned *>(ws + w.off_vcount) : nullptr, nv);
    SC_LAUNCH_CHECK();
    if (faces_i64)
        hipLaunchKernelGGL(cc_union_kernel<long long>, dim3(cdiv(nf, CC_BLOCK)), dim3(CC_BLOCK), 0, st,
                           reinterpret_cast<const long long *>(faces), nf, nv, parent, hdr);
    else
        hipLaunchKernelGGL(cc_union_kernel<int>, dim3(cdiv(nf, CC_BLOCK)), dim3(CC_BLOCK), 0, st, reinterpret_cast<const int *>(faces),
                           nf, nv, parent, hdr);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(cdiv(nv, CC_BLOCK)), dim3(CC_BLOCK), 0, st, parent, nv, labels, hdr);
    SC_LAUNCH_CHECK();
    return 0;
}

static int cc_read(const void *workspace, CcHeader *res) {
    if (int rc = g_cc_ring.read(workspace, res)) return rc;
    if (res->error & CC_ERR_INDEX) {
        set_error("mesh_components: a face names a vertex outside [0, Nv)");
        return SCULPT_ERR_MESH_COMPONENTS;
    }
    if (res->error & CC_ERR_CAP) {
        set_error("mesh_components: a union-find walk ran out of its step budget (parent[x] <= x did not hold): a defect, the "
                  "result is not valid");
        return SCULPT_ERR_MESH_COMPONENTS;
    }
    return 0;
}

}  // namespace sculpt

using namespace sculpt;

extern "C" {

size_t sculpt_mesh_components_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    if (n_vertices < 0 || n_vertices >= 0x7fffffffLL || n_faces < 0 || n_faces >= 0x7fffffffLL) return 0;
    return cc_layout((long)n_vertices, (long)n_faces).total;
}

int sculpt_mesh_components_launch(const void *faces, int faces_i64, int64_t n_faces, int64_t n_vertices, int rule, int64_t min_faces,
                                  double fraction, void *workspace, sculpt_stream_t stream) {
    hipStream_t st = as_stream(stream);
    if (int rc = cc_check_sizes("mesh_components", n_vertices, n_faces)) return rc;
    SC_REQUIRE(n_faces > 0 && n_vertices > 0, "mesh_components: nothing to launch for %lld faces over %lld vertices (the caller "
               "returns the empty result)", (long long)n_faces, (long long)n_vertices);
    SC_REQUIRE(faces && workspace, "mesh_components: null argument");
    SC_REQUIRE(rule >= SCULPT_CC_KEEP_NONE && rule <= SCULPT_CC_KEEP_FRACTION, "mesh_components: unknown rule %d", rule);
    SC_REQUIRE(rule != SCULPT_CC_KEEP_MIN_FACES || min_faces >= 1, "mesh_components: min_faces %lld (>= 1)", (long long)min_faces);
    SC_REQUIRE(rule != SCULPT_CC_KEEP_FRACTION || (fraction > 0.0 && fraction < 1.0), "mesh_components: fraction %g (0 < x < 1)", fraction);
    const int nv = (int)n_vertices, nf = (int)n_faces;
    const CcLayout w = cc_layout(nv, nf);
    char *ws = reinterpret_cast<char *>(workspace);
    CcHeader *hdr = reinterpret_cast<CcHeader *>(ws);
    CcHeader init;
    memset(&init, 0, sizeof(init));
    init.rule = (unsigned)rule;
    init.min_faces = rule == SCULPT_CC_KEEP_MIN_FACES ? (unsigned)std::min<int64_t>(min_faces, 0xffffffffLL) : 0u;
    init.fraction = rule == SCULPT_CC_KEEP_FRACTION ? fraction : 0.0;
    int *labels = reinterpret_cast<int *>(ws + w.off_labels);
    unsigned *fcount = reinterpret_cast<unsigned *>(ws + w.off_fcount), *vcount = reinterpret_cast<unsigned *>(ws + w.off_vcount);
    unsigned *bt_root = reinterpret_cast<unsigned *>(ws + w.off_bt_root);
    unsigned *bt_keepv = reinterpret_cast<unsigned *>(ws + w.off_bt_keepv), *bt_keepf = reinterpret_cast<unsigned *>(ws + w.off_bt_keepf);
    if (int rc = cc_label(faces, faces_i64, nf, nv, init, ws, w, labels, true, st)) return rc;
    if (faces_i64)
        hipLaunchKernelGGL(cc_count_faces_kernel<long long>, dim3(cdiv(nf, CC_BLOCK)), dim3(CC_BLOCK), 0, st,
                           reinterpret_cast<const long long *>(faces), nf, nv, labels, fcount);
    else
        hipLaunchKernelGGL(cc_count_faces_kernel<int>, dim3(cdiv(nf, CC_BLOCK)), dim3(CC_BLOCK), 0, st,
                           reinterpret_cast<const int *>(faces), nf, nv, labels, fcount);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_count_verts_kernel, dim3(w.nbv), dim3(CC_CHUNK), 0, st, labels, nv, fcount, vcount, bt_root, hdr);
    SC_LAUNCH_CHECK();
    if (rule != SCULPT_CC_KEEP_NONE) {
        if (faces_i64)
            hipLaunchKernelGGL(cc_keep_totals_kernel<long long>, dim3(w.nbv + w.nbf), dim3(CC_CHUNK), 0, st,
                               reinterpret_cast<const long long *>(faces), nf, nv, w.nbv, labels, fcount, hdr, bt_keepv, bt_keepf);
        else
            hipLaunchKernelGGL(cc_keep_totals_kernel<int>, dim3(w.nbv + w.nbf), dim3(CC_CHUNK), 0, st,
                               reinterpret_cast<const int *>(faces), nf, nv, w.nbv, labels, fcount, hdr, bt_keepv, bt_keepf);
        SC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(cc_scan_totals_kernel, dim3(1), dim3(CC_CHUNK), 0, st, bt_root, rule != SCULPT_CC_KEEP_NONE ? bt_keepv : nullptr,
                       bt_keepf, w.nbv, w.nbf, hdr);
    SC_LAUNCH_CHECK();
    return g_cc_ring.launch(workspace, hdr, st);
}

int sculpt_mesh_components_read(const void *workspace, int64_t *counts_host) {
    SC_REQUIRE(workspace && counts_host, "mesh_components_read: null argument");
    CcHeader res;
    if (int rc = cc_read(workspace, &res)) return rc;
    counts_host[0] = (int64_t)res.n_components;
    counts_host[1] = (int64_t)(res.best >> 32);
    counts_host[2] = (int64_t)(0xffffffffull - (res.best & 0xffffffffull));
    counts_host[3] = (int64_t)res.kept_nv;
    counts_host[4] = (int64_t)res.kept_nf;
    return 0;
}

int sculpt_mesh_components_compact(const float *vertices, const void *faces, int faces_i64, int64_t n_faces, int64_t n_vertices,
                                   void *workspace, float *out_vertices, int64_t cap_vertices, void *out_faces, int64_t cap_faces,
                                   int64_t *vertex_index, int64_t *face_index, sculpt_stream_t stream) {
    hipStream_t st = as_stream(stream);
    if (int rc = cc_check_sizes("mesh_components_compact", n_vertices, n_faces)) return rc;
    SC_REQUIRE(n_faces > 0 && n_vertices > 0 && cap_vertices >= 0 && cap_faces >= 0, "mesh_components_compact: bad sizes");
    SC_REQUIRE(vertices && faces && workspace, "mesh_components_compact: null argument");
    SC_REQUIRE((cap_vertices == 0 || (out_vertices && vertex_index)) && (cap_faces == 0 || (out_faces && face_index)),
               "mesh_components_compact: null output");
    const int nv = (int)n_vertices, nf = (int)n_faces;
    const CcLayout w = cc_layout(nv, nf);
    char *ws = reinterpret_cast<char *>(workspace);
    const CcHeader *hdr = reinterpret_cast<const CcHeader *>(ws);
    const int *labels = reinterpret_cast<const int *>(ws + w.off_labels);
    const unsigned *fcount = reinterpret_cast<const unsigned *>(ws + w.off_fcount);
    int *new_id = reinterpret_cast<int *>(ws + w.off_parent);
    hipLaunchKernelGGL(cc_compact_verts_kernel, dim3(w.nbv), dim3(CC_CHUNK), 0, st, vertices, nv, labels, fcount, hdr,
                       reinterpret_cast<const unsigned *>(ws + w.off_bt_keepv), new_id, out_vertices,
                       reinterpret_cast<long long *>(vertex_index), (unsigned long long)cap_vertices);
    SC_LAUNCH_CHECK();
    const unsigned *bt_keepf = reinterpret_cast<const unsigned *>(ws + w.off_bt_keepf);
    if (faces_i64)
        hipLaunchKernelGGL(cc_compact_faces_kernel<long long>, dim3(w.nbf), dim3(CC_CHUNK), 0, st, reinterpret_cast<const long long *>(faces),
                           nf, nv, labels, fcount, hdr, bt_keepf, new_id, reinterpret_cast<long long *>(out_faces),
                           reinterpret_cast<long long *>(face_index), (unsigned long long)cap_faces);
    else
        hipLaunchKernelGGL(cc_compact_faces_kernel<int>, dim3(w.nbf), dim3(CC_CHUNK), 0, st, reinterpret_cast<const int *>(faces), nf, nv,
                           labels, fcount, hdr, bt_keepf, new_id, reinterpret_cast<int *>(out_faces),
                           reinterpret_cast<long long *>(face_index), (unsigned long long)cap_faces);
    SC_LAUNCH_CHECK();
    return 0;
}

int sculpt_mesh_components_report(const void *workspace, int64_t n_vertices, int64_t n_faces, int64_t n_components, int32_t *labels,
                                  int32_t *roots, int32_t *face_counts, int32_t *vertex_counts, sculpt_stream_t stream) {
    hipStream_t st = as_stream(stream);
    if (int rc = cc_check_sizes("mesh_components_report", n_vertices, n_faces)) return rc;
    SC_REQUIRE(n_faces > 0 && n_vertices > 0 && n_components >= 0, "mesh_components_report: bad sizes");
    SC_REQUIRE(workspace && (n_components == 0 || (roots && face_counts && vertex_counts)), "mesh_components_report: null argument");
    const int nv = (int)n_vertices;
    const CcLayout w = cc_layout(nv, (long)n_faces);
    const char *ws = reinterpret_cast<const char *>(workspace);
    const int *ws_labels = reinterpret_cast<const int *>(ws + w.off_labels);
    if (labels) SC_HIP(hipMemcpyAsync(labels, ws_labels, 4 * (size_t)nv, hipMemcpyDeviceToDevice, st));
    if (n_components > 0) {
        hipLaunchKernelGGL(cc_report_kernel, dim3(w.nbv), dim3(CC_CHUNK), 0, st, ws_labels, nv,
                           reinterpret_cast<const unsigned *>(ws + w.off_fcount), reinterpret_cast<const unsigned *>(ws + w.off_vcount),
                           reinterpret_cast<const unsigned *>(ws + w.off_bt_root), roots, face_counts, vertex_counts,
                           (unsigned long long)n_components);
        SC_LAUNCH_CHECK();
    }
    return 0;
}

int sculpt_mesh_component_labels(const void *faces, int faces_i64, int64_t n_faces, int64_t n_vertices, int32_t *labels, void *workspace,
                                 sculpt_stream_t stream) {
    hipStream_t st = as_stream(stream);
    if (int rc = cc_check_sizes("mesh_component_labels", n_vertices, n_faces)) return rc;
    SC_REQUIRE(n_faces > 0 && n_vertices > 0, "mesh_component_labels: nothing to launch for %lld faces over %lld vertices",
               (long long)n_faces, (long long)n_vertices);
    SC_REQUIRE(faces && labels && workspace, "mesh_component_labels: null argument");
    const CcLayout w = cc_layout((long)n_vertices, (long)n_faces);
    CcHeader init;
    memset(&init, 0, sizeof(init));
    char *ws = reinterpret_cast<char *>(workspace);
    if (int rc = cc_label(faces, faces_i64, (int)n_faces, (int)n_vertices, init, ws, w, labels, false, st)) return rc;
    if (int rc = g_cc_ring.launch(workspace, reinterpret_cast<const CcHeader *>(ws), st)) return rc;
    CcHeader res;
    return cc_read(workspace, &res);
}

}  // extern "C"
