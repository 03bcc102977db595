// The forward-mode evaluator of the raw density: the pieces that turn the point query's MFMA tile (triplane_mlp.h) into
// 8 points x 4 columns {value, d/dx, d/dy, d/dz} (the shape is described in csrc/field_normal.hip and DESIGN.md section 3.1d),
// and field_eval_fwd, the ONE evaluation of a point made of them.  Its callers evaluate a point with the same operations and
// give the same bits: density_grad_kernel (csrc/field_normal.hip), project_kernel and project_along_kernel
// (csrc/mesh_project.hip), bake_scene_normal_kernel (csrc/bake_normal.hip), bake_scene_surface_kernel (csrc/bake_surface.hip)
// and render_passes_kernel (csrc/render.hip).  The two bakes also share the span compaction at the end of this file.  Units that
// include this are compiled with -fno-slp-vectorize (build.py).
#pragma once

#include "common.h"
#include "field_kernel.h"
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

// One evaluation at (px, py, pz) of the column of kind `kind` (0 = value, 1 + axis = tangent; p & 3 in the tile): layer 0 with the
// column's weights, its accumulators started at the bias for a value and at 0 for a tangent, the hidden layers, row 0 of the last
// layer.  -> the raw density without the last bias (value) or its derivative along the axis (tangent); x0, x1 are left holding
// what the last layer read, for a caller that wants its other rows.
template <int C, bool AC>
__device__ __forceinline__ float field_eval_fwd(const FieldCtx &c, const float *planes, int H, int W, float radius, float span,
                                                int a0_lds, int kind, float px, float py, float pz, f32x16 &x0, f32x16 &x1) {
    const bool is_value = kind == 0;
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int off[3][4];
    float wt[3][4];
    point_taps<AC>(px, py, pz, radius, span, H, W, off, wt);
    tangent_weights<AC>(kind, px, py, pz, radius, span, H, W, wt);
    x0 = is_value ? lds_bias16(c.L.bacc, 0, c.h, 0) : zero;
    x1 = is_value ? lds_bias16(c.L.bacc, 0, c.h, 1) : zero;
    layer0_channel_last<C>(planes, (long)H * W, off, wt, c.a0s, c.A0g, a0_lds, c.lane, c.h, x0, x1);
    hidden_layers_fwd(c.L, c.NH, c.lane, c.h, is_value, x0, x1);
    return last_dot0_nobias(c.L, c.h, x0, x1);
}

template <int C, bool AC>
__device__ __forceinline__ float field_eval_fwd(const FieldCtx &c, const float *planes, int H, int W, float radius, float span,
                                                int a0_lds, int kind, float px, float py, float pz) {
    f32x16 x0, x1;
    return field_eval_fwd<C, AC>(c, planes, H, W, radius, span, a0_lds, kind, px, py, pz, x0, x1);
}

// The unit normal of the iso-surface through a point with density gradient g: -g / |g|, with g scaled by a power of two first
// so that no square overflows or vanishes; exactly 0 where g is 0 or not finite.  One copy, so that density_grad_kernel and the
// renderer's render_passes_kernel (csrc/render.hip) give the same bits.
__device__ __forceinline__ void unit_normal_of(float gx, float gy, float gz, float &nx, float &ny, float &nz) {
    const float m = fmaxf(fmaxf(fabsf(gx), fabsf(gy)), fabsf(gz));
    nx = 0.f; ny = 0.f; nz = 0.f;
    const bool finite = fabsf(gx) < INFINITY && fabsf(gy) < INFINITY && fabsf(gz) < INFINITY;
    if (finite && m > 0.f) {
        const int e = -ilogbf(m);
        const float ux = ldexpf(gx, e), uy = ldexpf(gy, e), uz = ldexpf(gz, e);
        const float len = sqrtf(ux * ux + uy * uy + uz * uz);
        nx = -ux / len; ny = -uy / len; nz = -uz / len;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The span compaction of the bakes.  A wave owns a span of 64 texels, one per lane, of which some are
// covered.  span_compact brings the covered texels' positions to the low lanes in rank order; the wave then runs
// ceil(count / 8) forward-mode tiles, tile k over ranks 8k .. 8k + 7 (span_tile_point); span_gather brings a tile's results to
// lanes 8k .. 8k + 7, and after the last tile span_return sends what lane `rank` holds back to its texel's lane.  Lane
// permutes only, no LDS.  Call with at least one lane covered (the ballot is wave-uniform: a span with none runs no tile).
// ---------------------------------------------------------------------------------------------------------------------------
struct SpanRanks {
    int count;          // covered texels of the span
    int slot;           // covered lane -> its rank; uncovered lane -> count + its rank among the uncovered: a permutation of 0 .. 63
    float cx, cy, cz;   // lane `rank` holds the position of the covered texel of that rank
};

__device__ __forceinline__ SpanRanks span_compact(unsigned long long m, bool covered, int lane, const float (&x)[3]) {
    SpanRanks s;
    s.count = __popcll(m);
    const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    s.slot = covered ? below : s.count + (lane - below);
    s.cx = __int_as_float(__builtin_amdgcn_ds_permute(s.slot * 4, __float_as_int(x[0])));
    s.cy = __int_as_float(__builtin_amdgcn_ds_permute(s.slot * 4, __float_as_int(x[1])));
    s.cz = __int_as_float(__builtin_amdgcn_ds_permute(s.slot * 4, __float_as_int(x[2])));
    return s;
}

__device__ __forceinline__ int span_tiles(const SpanRanks &s) { return (s.count + 7) >> 3; }  // <= 8

// the point of column p in tile k -> its rank (< 64).  A rank >= count is an uncovered texel's position (the box centre): the
// column evaluates with the wave and nothing of its result is kept.
__device__ __forceinline__ int span_tile_point(const SpanRanks &s, int k, int p, float &px, float &py, float &pz) {
    const int src = k * 8 + (p >> 2);
    px = __shfl(s.cx, src, 64), py = __shfl(s.cy, src, 64), pz = __shfl(s.cz, src, 64);
    return src;
}

// point j of a tile sits in lane 4 j: lane 8 k + j <- v of point j (float or int); the lanes 8k .. 8k + 7 keep it (span_keeps)
template <class T>
__device__ __forceinline__ T span_gather(T v, int lane) {
    return __shfl(v, 4 * (lane & 7), 64);
}

__device__ __forceinline__ bool span_keeps(int k, int lane) { return (lane >> 3) == k; }

// what lane `rank` holds, back in the texel's own lane (float or int)
template <class T>
__device__ __forceinline__ T span_return(const SpanRanks &s, T r) {
    return __builtin_bit_cast(T, __builtin_amdgcn_ds_bpermute(s.slot * 4, __builtin_bit_cast(int, r)));
}

}  // namespace sculpt
