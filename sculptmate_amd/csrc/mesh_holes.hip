// Fill holes ON THE DEVICE: the border loops of a triangle mesh, and a fan over each one that is short enough
// (sculpt_mesh_border_mark .. sculpt_mesh_holes_emit, include/sculpt_hip.h; driven by sculptmate_amd/ops.py mesh_border_loops /
// mesh_fill_holes).  Every existing vertex and face stays exactly as it is; vertices and faces are only appended.  Everything up
// to the centroids is integers; the centroids are fixsum.h's order-independent sums.  The unit is compiled with floating-point
// contraction OFF (the pragma below, before the shared helpers), and tests/_holesref.py restates all of it in NumPy by plain
// walking of `next`.
//
// ---- the rule (the contract) ------------------------------------------------------------------------------------------------
// Half-edge h = 3 f + k runs from start(h) = F[f][k] to end(h) = F[f][(k + 1) % 3].  It is a BORDER half-edge when its undirected
// edge has exactly one half-edge (the census' definition, csrc/mesh_report.hip).  Edges with >= 3 half-edges, or with 2 in the same
// direction, are not border and are never touched.  Over the border half-edges:
//   - out(v), in(v) count those that start and end at v.  A vertex they touch is PINCHED unless out(v) == 1 and in(v) == 1 (a
//     bow-tie, where two holes meet in a vertex; inconsistent winding beside a hole);
//   - a border half-edge is BLOCKED when its start or its end is pinched;
//   - next(h) of an unblocked h is the one border half-edge that starts at end(h): unique, and injective on the unblocked ones, so
//     an unblocked half-edge lies on a pure cycle of unblocked half-edges, or its chain runs into a blocked one;
//   - a LOOP is such a cycle, its LEADER its smallest h, its length n the number of its half-edges (n >= 3: faces with a repeated
//     index are refused by the input check).  Every other border half-edge is OPEN and stays open;
//   - a loop is FILLED when n <= limit (limit = max_edges when given) and in any case n <= 2^22 - 1, the number of terms the
//     fixed-point sum below cannot overflow at.
// Result (V', F'):
//   - V' = V followed by one CENTROID per filled loop with n >= 4, in ascending leader order;
//   - F' = F followed by the new faces in ascending order of the half-edge that emits them: in a filled loop with n >= 4 every
//     h = (a -> b) emits (b, a, c), c the loop's centroid; in a filled loop with n == 3 the leader alone emits
//     (b, a, end(next(h))), and no vertex is made.
// The new faces traverse the border edges in the opposite direction, so the winding stays consistent; every new edge ends at a new
// vertex, so no non-manifold edge can arise.
// The centroid, per coordinate, over the n starts of the loop's half-edges (fixsum.h): pass 1 takes the largest |x| bits with
// atomicMax (fx_note); pass 2 rounds every term once onto the grid 2^(e - 40) and adds it as a 64-bit integer (fx_add); the value
// is (float)(ldexp((double)acc, e - 40) / (double)n) (fx_mean).  The integer sum is exact, so no order enters.  A per-vertex
// attribute [Nv, C <= 8] gets the same mean for the new rows; a non-finite attribute term gives NaN by fixsum.h's rule.
//
// What is NOT claimed: a fan is a good cap for a short or roughly planar, star-shaped loop, and nothing more.  A long loop that
// wraps round an edge or a corner of the extraction box gets a fan that cuts through the mesh: max_edges is the caller's control,
// the mesh report (self-intersections) is the check, and the voxel remesh remains the answer for the box-wrapping loops.
//
// ---- the labels ------------------------------------------------------------------------------------------------------------------
// Over the list of the nb border half-edges in ascending order (a list index orders like the half-edge it names), pointer doubling
// over PING-PONG buffers: element i holds (jump, low, open) = where 2^r steps of next lead, the smallest index among the first 2^r
// elements of its chain, and whether one of them is blocked; a blocked element jumps to itself.  A round reads only the other
// buffer -- updated in place, a thread would read a jump that another has already advanced in the same round, and skip elements.
// ceil(log2(nb)) + 1 rounds cover every cycle and every chain (none is longer than nb), so the labels are a function of the input
// alone.  Every loop in this file is bounded by a list length, a channel count or that round count; nothing waits on another thread.
#pragma clang fp contract(off)

#include "remesh_topo.h"
#include "block_scan.h"
#include "fixsum.h"

namespace {

constexpr int kWaves = kThreads / 64;
constexpr int kNoStart = 0x7f7f7f7f;           // start_of of a vertex no border half-edge starts at (the memset's byte, four times)
constexpr int kMaxLoop = (1 << 22) - 1;        // fixsum.h: fewer than 2^(62 - FX_BITS) terms
constexpr int kMaxChannels = 8;
constexpr unsigned kOpenBit = 0x80000000u;
enum { kPinched = 0, kLoops = 1, kOpenEdges = 2, kFilledLoops = 3, kFilledEdges = 4, kSkippedLoops = 5, kNewVertices = 6, kNewFaces = 7,
       kCountWords = 8 };

__device__ inline int end_of(const int32_t *F, int h) { return F[h - h % 3 + (h % 3 + 1) % 3]; }

// one thread per undirected edge: the flag of its half-edge when it is alone, out / in of its two ends, the start-of table
__global__ void __launch_bounds__(kThreads)
mark_kernel(Topo T, int32_t *__restrict__ flag, int32_t *__restrict__ vout, int32_t *__restrict__ vin, int32_t *__restrict__ start_of) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T.ne) return;
    const int first = T.es[e];
    if (T.es[e + 1] - first != 1) return;
    const int h = T.she[first];
    if (h < 0 || h >= 3 * T.nf) return;
    const int a = T.F[h], b = end_of(T.F, h);
    if (a < 0 || a >= T.nv || b < 0 || b >= T.nv) return;
    flag[h] = 1;
    atomicAdd(&vout[a], 1);
    atomicAdd(&vin[b], 1);
    atomicMin(&start_of[a], h);   // one writer wherever the table is read (out == 1); the minimum keeps the rest reproducible too
}

// incl = the inclusive scan of flag: border half-edge h is element incl[h] - 1 of the list
__global__ void __launch_bounds__(kThreads)
list_kernel(const int32_t *__restrict__ flag, const int32_t *__restrict__ incl, long nh, int32_t *__restrict__ list, long nb) {
    const long h = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= nh || !flag[h]) return;
    const long i = (long)incl[h] - 1;
    if (i >= 0 && i < nb) list[i] = (int32_t)h;
}

__device__ inline bool pinched(const int32_t *vout, const int32_t *vin, int v) { return !(vout[v] == 1 && vin[v] == 1); }

// threads 0 .. nb: next (list index, -1 when blocked); threads 0 .. nv: the pinched vertices, counted
__global__ void __launch_bounds__(kThreads)
next_kernel(Topo T, const int32_t *__restrict__ list, const int32_t *__restrict__ incl, long nb, const int32_t *__restrict__ vout,
            const int32_t *__restrict__ vin, const int32_t *__restrict__ start_of, int32_t *__restrict__ next,
            unsigned long long *__restrict__ counts) {
    __shared__ unsigned s_w[kWaves];
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nb) {
        const int h = list[t], a = T.F[h], b = end_of(T.F, h);
        int j = -1;
        if (!pinched(vout, vin, a) && !pinched(vout, vin, b)) {
            const int g = start_of[b];                 // out(b) == 1: the one border half-edge that starts at b
            if (g >= 0 && g < 3 * T.nf) j = incl[g] - 1;
            if (j < 0 || j >= nb) j = -1;
        }
        next[t] = j;
    }
    const bool p = t < T.nv && (vout[t] | vin[t]) != 0 && pinched(vout, vin, (int)t);
    const unsigned np = block_flag_count<kWaves>(p, s_w);
    if (threadIdx.x == 0 && np) atomicAdd(&counts[kPinched], (unsigned long long)np);
}

// state: x = jump, y = low | kOpenBit when a blocked element is among those covered
__global__ void __launch_bounds__(kThreads) jump_init_kernel(const int32_t *__restrict__ next, long nb, uint2 *__restrict__ state) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const int j = next[i];
    state[i] = j < 0 ? make_uint2((unsigned)i, (unsigned)i | kOpenBit) : make_uint2((unsigned)j, (unsigned)i);
}

__global__ void __launch_bounds__(kThreads) jump_round_kernel(const uint2 *__restrict__ from, uint2 *__restrict__ to, long nb) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const uint2 s = from[i];
    const uint2 o = from[s.x < nb ? s.x : i];
    const unsigned low = min(s.y & ~kOpenBit, o.y & ~kOpenBit);
    to[i] = make_uint2(o.x < nb ? o.x : (unsigned)i, low | ((s.y | o.y) & kOpenBit));
}

// leader [nb] = the list index of the loop's leader, -1 when open; length[leader] counts the loop's half-edges
__global__ void __launch_bounds__(kThreads)
label_kernel(const uint2 *__restrict__ state, long nb, int32_t *__restrict__ leader, int32_t *__restrict__ length) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const unsigned y = state[i].y, low = y & ~kOpenBit;
    const bool open = (y & kOpenBit) != 0 || low >= nb;
    leader[i] = open ? -1 : (int)low;
    if (!open) atomicAdd(&length[low], 1);
}

// per border half-edge: does it emit a face, is it the leader of a loop, of a loop that gets a centroid; and the totals
__global__ void __launch_bounds__(kThreads)
decide_kernel(const int32_t *__restrict__ leader, const int32_t *__restrict__ length, long nb, int limit, int32_t *__restrict__ emits,
              int32_t *__restrict__ centre, int32_t *__restrict__ heads, unsigned long long *__restrict__ counts) {
    __shared__ unsigned s_w[6][kWaves];
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool open = false, head = false, filled = false, emit = false, vertex = false;
    int n = 0;
    if (i < nb) {
        const int l = leader[i];
        open = l < 0;
        if (!open) {
            n = length[l];
            head = l == i;
            filled = n <= limit;
            emit = filled && (n >= 4 || head);
            vertex = filled && head && n >= 4;
        }
        emits[i] = emit;
        centre[i] = vertex;
        heads[i] = head;
    }
    const unsigned n_open = block_flag_count<kWaves>(open, s_w[0]);
    const unsigned n_head = block_flag_count<kWaves>(head, s_w[1]);
    const unsigned n_fill = block_flag_count<kWaves>(head && filled, s_w[2]);
    const unsigned n_edge = block_flag_count<kWaves>(!open && filled, s_w[3]);
    const unsigned n_emit = block_flag_count<kWaves>(emit, s_w[4]);
    const unsigned n_vert = block_flag_count<kWaves>(vertex, s_w[5]);
    if (threadIdx.x == 0) {
        if (n_open) atomicAdd(&counts[kOpenEdges], (unsigned long long)n_open);
        if (n_head) atomicAdd(&counts[kLoops], (unsigned long long)n_head);
        if (n_fill) atomicAdd(&counts[kFilledLoops], (unsigned long long)n_fill);
        if (n_head - n_fill) atomicAdd(&counts[kSkippedLoops], (unsigned long long)(n_head - n_fill));
        if (n_edge) atomicAdd(&counts[kFilledEdges], (unsigned long long)n_edge);
        if (n_emit) atomicAdd(&counts[kNewFaces], (unsigned long long)n_emit);
        if (n_vert) atomicAdd(&counts[kNewVertices], (unsigned long long)n_vert);
    }
}

// the labels as half-edges, and the leaders with their lengths in ascending leader order (heads_incl = the scan of heads)
__global__ void __launch_bounds__(kThreads)
loops_kernel(const int32_t *__restrict__ list, const int32_t *__restrict__ leader, const int32_t *__restrict__ length,
             const int32_t *__restrict__ heads_incl, long nb, long n_loops, int32_t *__restrict__ label, int32_t *__restrict__ leaders,
             int32_t *__restrict__ lengths) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const int l = leader[i];
    label[i] = l < 0 ? -1 : list[l];
    if (l == i) {
        const long r = (long)heads_incl[i] - 1;
        if (r >= 0 && r < n_loops) {
            leaders[r] = list[i];
            lengths[r] = length[i];
        }
    }
}

// value k of vertex v: a coordinate for k < 3, else channel k - 3 of the attributes
__device__ inline float term(const float *__restrict__ P, const float *__restrict__ A, int C, int v, int k) {
    return k < 3 ? P[3 * (long)v + k] : A[(long)C * v + (k - 3)];
}

// the centroid row of border element i (centre_incl = the scan of centre), or -1 when its loop gets none
__device__ inline long centre_row(const int32_t *leader, const int32_t *centre, const int32_t *centre_incl, long i, long n_new) {
    const int l = leader[i];
    if (l < 0 || !centre[l]) return -1;
    const long c = (long)centre_incl[l] - 1;
    return c >= 0 && c < n_new ? c : -1;
}

template <bool kAdd>
__global__ void __launch_bounds__(kThreads)
sum_kernel(Topo T, const float *__restrict__ P, const float *__restrict__ A, int C, const int32_t *__restrict__ list,
           const int32_t *__restrict__ leader, const int32_t *__restrict__ centre, const int32_t *__restrict__ centre_incl, long nb, long n_new,
           unsigned *__restrict__ mag, long long *__restrict__ acc) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const long c = centre_row(leader, centre, centre_incl, i, n_new);
    if (c < 0) return;
    const int v = T.F[list[i]], K = 3 + C;
    for (int k = 0; k < K; ++k) {
        const float x = term(P, A, C, v, k);
        if (kAdd)
            fx_add(&acc[c * K + k], mag[c * K + k], x);
        else
            fx_note(&mag[c * K + k], x);
    }
}

// one thread per loop leader with a centroid: rows Nv + c of the vertices and of the attributes
__global__ void __launch_bounds__(kThreads)
mean_kernel(const int32_t *__restrict__ leader, const int32_t *__restrict__ length, const int32_t *__restrict__ centre,
            const int32_t *__restrict__ centre_incl, long nb, long n_new, int C, const unsigned *__restrict__ mag,
            const long long *__restrict__ acc, float *__restrict__ Pn, float *__restrict__ An) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb || leader[i] != i) return;
    const long c = centre_row(leader, centre, centre_incl, i, n_new);
    if (c < 0) return;
    const int n = length[i], K = 3 + C;
    for (int k = 0; k < K; ++k) {
        const float m = fx_mean(acc[c * K + k], mag[c * K + k], n);
        if (k < 3)
            Pn[3 * c + k] = m;
        else
            An[(long)C * c + (k - 3)] = m;
    }
}

// the new faces, rows emits_incl[i] - 1 of Fn
__global__ void __launch_bounds__(kThreads)
emit_kernel(Topo T, const int32_t *__restrict__ list, const int32_t *__restrict__ next, const int32_t *__restrict__ leader,
            const int32_t *__restrict__ length, const int32_t *__restrict__ emits, const int32_t *__restrict__ emits_incl,
            const int32_t *__restrict__ centre, const int32_t *__restrict__ centre_incl, long nb, long n_new, long n_faces,
            int32_t *__restrict__ Fn) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb || !emits[i]) return;
    const long r = (long)emits_incl[i] - 1;
    if (r < 0 || r >= n_faces) return;
    const int h = list[i], a = T.F[h], b = end_of(T.F, h), l = leader[i];
    if (l < 0) return;
    int c;
    if (length[l] >= 4) {
        const long row = centre_row(leader, centre, centre_incl, i, n_new);
        if (row < 0) return;
        c = (int)(T.nv + row);
    } else {
        const int j = next[i];
        if (j < 0 || j >= nb) return;
        c = end_of(T.F, list[j]);
    }
    Fn[3 * r] = b;
    Fn[3 * r + 1] = a;
    Fn[3 * r + 2] = c;
}

int check_border(const sculpt_rmd_topo_t *topo, const char *who, int64_t nb) {
    if (int rc = check_topo(topo, who)) return rc;
    SC_REQUIRE(nb >= 0 && nb <= 3 * topo->nf, "%s: %lld border half-edges of %lld half-edges", who, (long long)nb, (long long)(3 * topo->nf));
    return 0;
}

}  // namespace

extern "C" {

int sculpt_mesh_border_mark(const sculpt_rmd_topo_t *topo, int32_t *flag, int32_t *vout, int32_t *vin, int32_t *start_of,
                            sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "mesh_border_mark")) return rc;
    if (topo->nf == 0) return 0;
    SC_REQUIRE(flag && vout && vin && start_of, "mesh_border_mark: null array");
    SC_REQUIRE(topo->nv > 0, "mesh_border_mark: faces without vertices");
    SC_HIP(hipMemsetAsync(flag, 0, 3 * topo->nf * sizeof(int32_t), as_stream(stream)));
    SC_HIP(hipMemsetAsync(vout, 0, topo->nv * sizeof(int32_t), as_stream(stream)));
    SC_HIP(hipMemsetAsync(vin, 0, topo->nv * sizeof(int32_t), as_stream(stream)));
    SC_HIP(hipMemsetAsync(start_of, kNoStart & 0xff, topo->nv * sizeof(int32_t), as_stream(stream)));
    RMD_LAUNCH(mark_kernel, topo->ne, topo_of(topo), flag, vout, vin, start_of);
    return 0;
}

int sculpt_mesh_border_next(const sculpt_rmd_topo_t *topo, const int32_t *flag, const int32_t *incl, int64_t nb, const int32_t *vout,
                            const int32_t *vin, const int32_t *start_of, int32_t *list, int32_t *next, int64_t *counts,
                            sculpt_stream_t stream) {
    if (int rc = check_border(topo, "mesh_border_next", nb)) return rc;
    SC_REQUIRE(counts, "mesh_border_next: null counts");
    SC_HIP(hipMemsetAsync(counts, 0, kCountWords * sizeof(int64_t), as_stream(stream)));
    if (topo->nf == 0) return 0;
    SC_REQUIRE(flag && incl && vout && vin && start_of, "mesh_border_next: null array");
    SC_REQUIRE(nb == 0 || (list && next), "mesh_border_next: null list");
    const Topo T = topo_of(topo);
    RMD_LAUNCH(list_kernel, 3 * T.nf, flag, incl, 3 * T.nf, list, (long)nb);
    RMD_LAUNCH(next_kernel, std::max((long)nb, T.nv), T, list, incl, (long)nb, vout, vin, start_of, next,
               reinterpret_cast<unsigned long long *>(counts));
    return 0;
}

int sculpt_mesh_border_label(const int32_t *next, int64_t nb, int64_t *state_a, int64_t *state_b, int32_t *leader, int32_t *length,
                             sculpt_stream_t stream) {
    SC_REQUIRE(nb >= 0 && nb < ((int64_t)1 << 31), "mesh_border_label: nb=%lld", (long long)nb);
    if (nb == 0) return 0;
    SC_REQUIRE(next && state_a && state_b && leader && length, "mesh_border_label: null array");
    SC_REQUIRE(state_a != state_b, "mesh_border_label: the two state buffers must differ (a round reads one and writes the other)");
    uint2 *from = reinterpret_cast<uint2 *>(state_a), *to = reinterpret_cast<uint2 *>(state_b);
    SC_HIP(hipMemsetAsync(length, 0, nb * sizeof(int32_t), as_stream(stream)));
    RMD_LAUNCH(jump_init_kernel, nb, next, (long)nb, from);
    int rounds = 1;   // ceil(log2(nb)) + 1
    while (((int64_t)1 << (rounds - 1)) < nb) ++rounds;
    for (int r = 0; r < rounds; ++r) {
        RMD_LAUNCH(jump_round_kernel, nb, from, to, (long)nb);
        std::swap(from, to);
    }
    RMD_LAUNCH(label_kernel, nb, from, (long)nb, leader, length);
    return 0;
}

int sculpt_mesh_border_decide(const int32_t *leader, const int32_t *length, int64_t nb, int64_t max_edges, int32_t *emits, int32_t *centre,
                              int32_t *heads, int64_t *counts, sculpt_stream_t stream) {
    SC_REQUIRE(nb >= 0 && nb < ((int64_t)1 << 31), "mesh_border_decide: nb=%lld", (long long)nb);
    SC_REQUIRE(max_edges == 0 || max_edges >= 3, "mesh_border_decide: max_edges=%lld (0: every loop, else at least 3)", (long long)max_edges);
    if (nb == 0) return 0;
    SC_REQUIRE(leader && length && emits && centre && heads && counts, "mesh_border_decide: null array");
    const int limit = (int)(max_edges == 0 ? kMaxLoop : std::min<int64_t>(max_edges, kMaxLoop));
    RMD_LAUNCH(decide_kernel, nb, leader, length, (long)nb, limit, emits, centre, heads, reinterpret_cast<unsigned long long *>(counts));
    return 0;
}

int sculpt_mesh_border_loops(const int32_t *list, const int32_t *leader, const int32_t *length, const int32_t *heads_incl, int64_t nb,
                             int64_t n_loops, int32_t *label, int32_t *leaders, int32_t *lengths, sculpt_stream_t stream) {
    SC_REQUIRE(nb >= 0 && nb < ((int64_t)1 << 31) && n_loops >= 0 && n_loops <= nb, "mesh_border_loops: nb=%lld, n_loops=%lld",
               (long long)nb, (long long)n_loops);
    if (nb == 0) return 0;
    SC_REQUIRE(list && leader && length && heads_incl && label, "mesh_border_loops: null array");
    SC_REQUIRE(n_loops == 0 || (leaders && lengths), "mesh_border_loops: null loop list");
    RMD_LAUNCH(loops_kernel, nb, list, leader, length, heads_incl, (long)nb, (long)n_loops, label, leaders, lengths);
    return 0;
}

int sculpt_mesh_holes_centroids(const sculpt_rmd_topo_t *topo, const float *P, const float *A, int channels, const int32_t *list,
                                const int32_t *leader, const int32_t *length, const int32_t *centre, const int32_t *centre_incl, int64_t nb,
                                int64_t n_new, uint32_t *mag, int64_t *acc, float *Pn, float *An, sculpt_stream_t stream) {
    if (int rc = check_border(topo, "mesh_holes_centroids", nb)) return rc;
    SC_REQUIRE(channels >= 0 && channels <= kMaxChannels, "mesh_holes_centroids: %d attribute channels (at most %d)", channels, kMaxChannels);
    SC_REQUIRE(n_new >= 0 && n_new <= nb, "mesh_holes_centroids: n_new=%lld", (long long)n_new);
    if (nb == 0 || n_new == 0) return 0;
    SC_REQUIRE(P && list && leader && length && centre && centre_incl && mag && acc && Pn, "mesh_holes_centroids: null array");
    SC_REQUIRE(channels == 0 || (A && An), "mesh_holes_centroids: null attributes");
    const Topo T = topo_of(topo);
    const int64_t words = n_new * (3 + channels);
    SC_HIP(hipMemsetAsync(mag, 0, words * sizeof(uint32_t), as_stream(stream)));
    SC_HIP(hipMemsetAsync(acc, 0, words * sizeof(int64_t), as_stream(stream)));
    RMD_LAUNCH((sum_kernel<false>), nb, T, P, A, channels, list, leader, centre, centre_incl, (long)nb, (long)n_new, mag,
               reinterpret_cast<long long *>(acc));
    RMD_LAUNCH((sum_kernel<true>), nb, T, P, A, channels, list, leader, centre, centre_incl, (long)nb, (long)n_new, mag,
               reinterpret_cast<long long *>(acc));
    RMD_LAUNCH(mean_kernel, nb, leader, length, centre, centre_incl, (long)nb, (long)n_new, channels, mag,
               reinterpret_cast<const long long *>(acc), Pn, An);
    return 0;
}

int sculpt_mesh_holes_emit(const sculpt_rmd_topo_t *topo, const int32_t *list, const int32_t *next, const int32_t *leader,
                           const int32_t *length, const int32_t *emits, const int32_t *emits_incl, const int32_t *centre,
                           const int32_t *centre_incl, int64_t nb, int64_t n_new, int64_t n_faces, int32_t *Fn, sculpt_stream_t stream) {
    if (int rc = check_border(topo, "mesh_holes_emit", nb)) return rc;
    SC_REQUIRE(n_new >= 0 && n_new <= nb && n_faces >= 0 && n_faces <= nb, "mesh_holes_emit: n_new=%lld, n_faces=%lld", (long long)n_new,
               (long long)n_faces);
    SC_REQUIRE(topo->nv + n_new < ((int64_t)1 << 31), "mesh_holes_emit: %lld vertices do not fit int32 indices", (long long)(topo->nv + n_new));
    if (nb == 0 || n_faces == 0) return 0;
    SC_REQUIRE(list && next && leader && length && emits && emits_incl && centre && centre_incl && Fn, "mesh_holes_emit: null array");
    RMD_LAUNCH(emit_kernel, nb, topo_of(topo), list, next, leader, length, emits, emits_incl, centre, centre_incl, (long)nb, (long)n_new,
               (long)n_faces, Fn);
    return 0;
}

}  // extern "C"
