// Fused triplane sample + NeRF-MLP kernels for gfx950 (MI355X).
//
// Replaces (reference file:line):
//   TriplaneNeRFRenderer.query_triplane / _query_chunk   TripoSR/tsr/models/nerf_renderer.py:41-91
//   NeRFMLP.forward                                       TripoSR/tsr/models/network_utils.py:116-124
//   dense query over MarchingCubeHelper.grid_vertices     TripoSR/tsr/system.py:171-183
//
// Design (see DESIGN.md "fused sample+MLP"):
//   * one wave owns a tile of 32 points; the point index lives on the MFMA column (lane & 31).
//   * hidden layers run on v_mfma_f32_32x32x2_f32 (exact fp32 == fmaf chain).  The 32x32
//     accumulator of layer l has the point on the lane and 16 neurons in registers, which is
//     exactly the B-operand shape of layer l+1 when the k order of layer l+1 is permuted to
//     neuron(t,r,h) = 32t + 8(r>>2) + 4h + (r&3).  The weights are stored pre-permuted
//     (sculpt_mlp_pack), so activations never leave registers: no LDS, no cross-lane traffic.
//   * all hidden weights (NH*64*64 fp32 = 128 KiB) sit in LDS once per workgroup; A operands
//     are fetched with conflict-free ds_read_b128 (4 k-steps per read).
//   * dense grid: the lattice is separable, so layer 0 (linear in the bilinear samples) is
//     evaluated once per lattice *pair* and plane (plane_features_kernel) and the per-point
//     layer-0 pre-activation is the sum of three table rows.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "triplane_mlp.h"

namespace sculpt {

static inline uint16_t host_f32_to_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
static inline float host_bf16_to_f32(uint16_t v) {
    uint32_t u = (uint32_t)v << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

static void pack_layout(int K0, int NH, MlpPackHeader *hd) {
    memset(hd, 0, sizeof(*hd));
    hd->magic = PACK_MAGIC;
    hd->K0 = K0;
    hd->NH = NH;
    int o = 16;  // header words
    hd->off_w0raw = o; o += HID * K0;
    hd->off_b0raw = o; o += HID;
    hd->off_a0 = o;    o += 2 * (K0 / 2) * 64;
    hd->off_bacc = o;  o += (NH + 1) * 64;
    hd->off_hid = o;   o += NH * 2 * 8 * 64 * 4;
    hd->off_wlast = o; o += 4 * 64;
    hd->off_blast = o; o += 4;
    o = (o + 3) & ~3;
    hd->off_x3 = o;    o += NH * 4096;
    hd->off_x3h = o;   o += NH * 4096;
    hd->off_w3 = o;    o += NH * 2048;
    hd->total_floats = (o + 3) & ~3;
}


// ---------------------------------------------------------------------------------------------
// General query at arbitrary points (C = 40 channels per plane).
// lane (p = lane&31, h = lane>>5) samples features k = h*60 + s, s = 0..59, of point p.
// ---------------------------------------------------------------------------------------------
// CL = planes are channel-last [3][H][W][C]: a tap is C contiguous floats (160 B), read as float4 groups of four
// channels -- 60 vector loads per lane instead of 240 scalar gathers from 40 channel planes 4*H*W bytes apart
// (the reference layout [3][C][H][W] touches ~480 cache lines per point, channel-last ~24).
template <int C, bool AC, bool CL>
__global__ __launch_bounds__(512) void query_points_kernel(
    const float *__restrict__ planes, int H, int W, const float *__restrict__ blob,
    const float *__restrict__ pts, long N, float radius, float span, float density_bias,
    float *__restrict__ density, float *__restrict__ features, float *__restrict__ density_act,
    float *__restrict__ color, int a0_lds) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int S0 = 3 * C / 2;
    const MlpPackHeader hd = *reinterpret_cast<const MlpPackHeader *>(blob);
    const int NH = hd.NH;
    float *a0s = smem + lds_floats_for(NH);
    if (CL && a0_lds) stage_a0_in_lds<C>(a0s, blob, hd);
    load_weights_to_lds(smem, blob, hd);
    const LdsView L = lds_view(smem, NH);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const int p = lane & 31, h = lane >> 5;
    const long ntiles = (N + 31) / 32;
    const float *A0g = blob + hd.off_a0;
    const long HW = (long)H * W;

    for (long tile = (long)blockIdx.x * nwave + wave; tile < ntiles; tile += (long)gridDim.x * nwave) {
        long n = tile * 32 + p;
        const bool valid = n < N;
        if (!valid) n = N - 1;
        int off[3][4];
        float wt[3][4];
        point_taps<AC>(pts[3 * n], pts[3 * n + 1], pts[3 * n + 2], radius, span, H, W, off, wt);
        // layer 0 on MFMA: step s consumes feature k = h*S0 + s of point p
        f32x16 acc0 = lds_bias16(L.bacc, 0, h, 0);
        f32x16 acc1 = lds_bias16(L.bacc, 0, h, 1);
        if (CL) {
            layer0_channel_last<C>(planes, HW, off, wt, a0s, A0g, a0_lds, lane, h, acc0, acc1);
        } else {
#pragma unroll 4
        for (int s = 0; s < S0; ++s) {
            const int f = h * S0 + s;
            const int pl = f / C, ch = f - pl * C;
            const float *P = planes + ((long)pl * C + ch) * HW;
            const int o0 = pl == 0 ? off[0][0] : (pl == 1 ? off[1][0] : off[2][0]);
            const int o1 = pl == 0 ? off[0][1] : (pl == 1 ? off[1][1] : off[2][1]);
            const int o2 = pl == 0 ? off[0][2] : (pl == 1 ? off[1][2] : off[2][2]);
            const int o3 = pl == 0 ? off[0][3] : (pl == 1 ? off[1][3] : off[2][3]);
            const float w0 = pl == 0 ? wt[0][0] : (pl == 1 ? wt[1][0] : wt[2][0]);
            const float w1 = pl == 0 ? wt[0][1] : (pl == 1 ? wt[1][1] : wt[2][1]);
            const float w2 = pl == 0 ? wt[0][2] : (pl == 1 ? wt[1][2] : wt[2][2]);
            const float w3 = pl == 0 ? wt[0][3] : (pl == 1 ? wt[1][3] : wt[2][3]);
            // same tap order as torch: nw + ne + sw + se
            float v = P[o0] * w0;
            v += P[o1] * w1;
            v += P[o2] * w2;
            v += P[o3] * w3;
            const float a0 = A0g[(0 * S0 + s) * 64 + lane];
            const float a1 = A0g[(1 * S0 + s) * 64 + lane];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, v, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, v, acc1, 0, 0, 0);
        }
        }
        f32x16 x0 = silu16(acc0), x1 = silu16(acc1);
        hidden_layers(L, NH, lane, h, x0, x1);
        const float d = last_dot(L, 0, h, x0, x1);
        const float f0 = last_dot(L, 1, h, x0, x1);
        const float f1 = last_dot(L, 2, h, x0, x1);
        const float f2 = last_dot(L, 3, h, x0, x1);
        if (valid && h == 0) {
            if (density) density[n] = d;
            if (density_act) density_act[n] = density_act_f(d, density_bias);
            if (features) { features[3 * n] = f0; features[3 * n + 1] = f1; features[3 * n + 2] = f2; }
            if (color) {
                color[3 * n] = color_f(f0);
                color[3 * n + 1] = color_f(f1);
                color[3 * n + 2] = color_f(f2);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Separable dense grid, step 1: per lattice pair (a -> W axis, b -> H axis) and plane k,
//   F_k[a][b][j] = sum_c W0[n(j)][k*C + c] * bilinear(P_k; a, b)[c]   (+ b0 on plane 0)
// stored in accumulator order j = h*32 + t*16 + r  <->  neuron nrow(t,r,h).
//   table 0 (FA): a = ix (local), b = iy     rows nx x R
//   table 1 (FB): a = ix (local), b = iz     rows nx x R
//   table 2 (FC): a = iy,         b = iz     rows R  x R
// ---------------------------------------------------------------------------------------------
// A wave takes 64 consecutive a (the coordinate along W, contiguous in memory) at one b: the four bilinear taps of a
// channel are then coalesced loads from the channel-first planes (64 lanes cover ~17 neighbouring pixels of one row) instead
// of one cache line per lane.  A lane keeps its pair's 64 pre-activations in registers and runs, channel by channel, the
// same fmaf chain (c ascending) one thread per (pair, neuron) would run; the weights of the workgroup's table sit in LDS
// (wl[c][j], j in accumulator order) and are read as broadcasts.  Four waves = four consecutive b.
template <int C, bool AC = false>
__global__ __launch_bounds__(256) void plane_features_kernel(
    const float *__restrict__ planes, int H, int W, const float *__restrict__ blob,
    const float *__restrict__ axis, int R, int x_begin, int nx, float radius, float span,
    float *__restrict__ FA, float *__restrict__ FB, float *__restrict__ FC) {
    __shared__ __attribute__((aligned(16))) float wl[C][64];
    __shared__ __attribute__((aligned(16))) float bl[64];
    const MlpPackHeader hd = *reinterpret_cast<const MlpPackHeader *>(blob);
    const int K0 = hd.K0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // workgroup -> (table k, chunk of 64 a, group of 4 b)
    const int bgroups = (R + 3) / 4;
    const long perA = (long)((nx + 63) / 64) * bgroups, perC = (long)((R + 63) / 64) * bgroups;
    int k, na;
    long rest;
    float *dst;
    {
        const long blk = blockIdx.x;
        if (blk < perA) { k = 0; rest = blk; na = nx; dst = FA; }
        else if (blk < 2 * perA) { k = 1; rest = blk - perA; na = nx; dst = FB; }
        else { k = 2; rest = blk - 2 * perA; na = R; dst = FC; }
    }
    (void)perC;
    const int a = (int)(rest / bgroups) * 64 + lane;
    const int b = (int)(rest % bgroups) * 4 + w;
    for (int i = threadIdx.x; i < C * 64; i += 256) {
        const int c = i >> 6, jj = i & 63;
        const int hh = jj >> 5, tt = (jj >> 4) & 1, rr = jj & 15;
        wl[c][jj] = blob[hd.off_w0raw + (long)nrow(tt, rr, hh) * K0 + k * C + c];
    }
    if (threadIdx.x < 64) {
        const int jj = threadIdx.x, hh = jj >> 5, tt = (jj >> 4) & 1, rr = jj & 15;
        bl[jj] = (k == 0) ? blob[hd.off_b0raw + nrow(tt, rr, hh)] : 0.f;
    }
    __syncthreads();
    if (b >= R) return;                                           // wave-uniform
    const bool live = a < na;
    const int ac = live ? a : na - 1;
    const int ia = (k == 2) ? ac : ac + x_begin;
    const float gx = to_unit(axis[ia], radius, span), gy = to_unit(axis[b], radius, span);
    Tap1 tx = tap_of<AC>(gx, W), ty = tap_of<AC>(gy, H);
    const float wx = tx.w1, ex = 1.0f - wx, wy = ty.w1, ey = 1.0f - wy;
    const int x0 = tx.i0, x1 = x0 + 1, y0 = ty.i0, y1 = y0 + 1;
    const bool vx0 = x0 >= 0 && x0 < W, vx1 = x1 >= 0 && x1 < W;
    const bool vy0 = y0 >= 0 && y0 < H, vy1 = y1 >= 0 && y1 < H;
    const int cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x1, 0), W - 1);
    const int cy0 = min(max(y0, 0), H - 1), cy1 = min(max(y1, 0), H - 1);
    const float wnw = (vy0 && vx0) ? ey * ex : 0.f, wne = (vy0 && vx1) ? ey * wx : 0.f;
    const float wsw = (vy1 && vx0) ? wy * ex : 0.f, wse = (vy1 && vx1) ? wy * wx : 0.f;
    const int o00 = cy0 * W + cx0, o01 = cy0 * W + cx1, o10 = cy1 * W + cx0, o11 = cy1 * W + cx1;
    float s[64];
#pragma unroll
    for (int jj = 0; jj < 64; ++jj) s[jj] = bl[jj];
    const float *P = planes + (long)k * C * H * W;
#pragma unroll 2
    for (int c = 0; c < C; ++c, P += (long)H * W) {
        float v = P[o00] * wnw;
        v += P[o01] * wne;
        v += P[o10] * wsw;
        v += P[o11] * wse;
        const f32x4 *wr = reinterpret_cast<const f32x4 *>(&wl[c][0]);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const f32x4 ww = wr[q];
            s[4 * q] = fmaf(ww[0], v, s[4 * q]);
            s[4 * q + 1] = fmaf(ww[1], v, s[4 * q + 1]);
            s[4 * q + 2] = fmaf(ww[2], v, s[4 * q + 2]);
            s[4 * q + 3] = fmaf(ww[3], v, s[4 * q + 3]);
        }
    }
    if (live) {
        f32x4 *o = reinterpret_cast<f32x4 *>(dst + ((long)a * R + b) * 64);
#pragma unroll
        for (int q = 0; q < 16; ++q) o[q] = f32x4{s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]};
    }
}

// ---------------------------------------------------------------------------------------------
// Separable dense grid, step 2: per tile of 32 consecutive iz at fixed (ix, iy):
//   x = silu(FA[ix,iy] + FB[ix,iz] + FC[iy,iz]); NH hidden layers on MFMA; density row of the
//   last layer on VALU; out = exp(d + density_bias).
// ---------------------------------------------------------------------------------------------

template <int NT>
__global__ __launch_bounds__(NT) void density_grid_kernel(
    const float *__restrict__ blob, const float *__restrict__ FA, const float *__restrict__ FB,
    const float *__restrict__ FC, int R, int nx, float density_bias, float out_add, float *__restrict__ out,
    int xcd_band) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpPackHeader hd = *reinterpret_cast<const MlpPackHeader *>(blob);
    const int NH = hd.NH;
    load_weights_to_lds(smem, blob, hd);
    const LdsView L = lds_view(smem, NH);

    const int lane = threadIdx.x & 63, nwave = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // tile bookkeeping stays on the scalar unit
    const int p = lane & 31, h = lane >> 5;
    // Measured (rocprofv3 PMC, profiles/round1/pmc_density_counters.txt): the matrix pipe is busy 78 % of
    // the kernel at 2.38 GHz; the rest is the SiLU VALU work (v_exp/v_rcp + 3 full-rate ops per value),
    // which does NOT overlap the fp32 MFMAs of the other waves on the SIMD -- removing the transcendental
    // part of SiLU brings the kernel to 93 % MFMA-busy, static per-wave priorities change nothing.  The
    // fp32-input MFMA runs at exactly the fp32 VALU rate, i.e. it appears to share that datapath.
    const int nzb = (R + 31) / 32;
    const long ntiles = (long)nx * nzb * R;
    // contiguous tile range per wave: consecutive tiles share (ix, zb) and walk iy
    const long nw_total = (long)gridDim.x * nwave;
    // XCD-aware wave order: the workgroups of one XCD (same blockIdx % 8) take one contiguous band of ix, so that
    // XCD's L2 streams only its band of the FA / FB tables (FC is indexed by (iy, iz) and is read by every XCD)
    long wid = (long)blockIdx.x * nwave + wave;
    if (xcd_band && gridDim.x % 8 == 0)
        wid = ((long)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3)) * nwave + wave;
    const long t_begin = ntiles * wid / nw_total, t_end = ntiles * (wid + 1) / nw_total;
    // (iy, zb, ixl) of the first tile by division once, then carried incrementally (all wave-uniform)
    int iy = (int)(t_begin % R);
    int zb = (int)((t_begin / R) % nzb), ixl = (int)((t_begin / R) / nzb);

    for (long t = t_begin; t < t_end; ++t, ++iy) {
        if (iy == R) {
            iy = 0;
            if (++zb == nzb) { zb = 0; ++ixl; }
        }
        const int iz = zb * 32 + p;
        const int izc = min(iz, R - 1);
        f32x16 x0, x1, y0, y1;
        load_row32(FA + ((long)ixl * R + iy) * 64 + h * 32, x0, x1);
        load_row32(FB + ((long)ixl * R + izc) * 64 + h * 32, y0, y1);
        x0 += y0; x1 += y1;
        load_row32(FC + ((long)iy * R + izc) * 64 + h * 32, y0, y1);
        x0 += y0; x1 += y1;
        x0 = silu16(x0); x1 = silu16(x1);
        hidden_layers(L, NH, lane, h, x0, x1);
        const float d = last_dot(L, 0, h, x0, x1);
        if (h == 0 && iz < R) out[((long)ixl * R + iy) * R + iz] = exp_f(d + density_bias) + out_add;
    }
}

// ---------------------------------------------------------------------------------------------
// The same step for a decoder head of StableFast-3D on its marching-tetrahedra lattice (sculpt_grid_decode): few hidden
// layers (one), so the launch is bound by its table reads, not by the matrix pipe, and R = 161 is not a multiple of 32.
// A tile is therefore 32 consecutive points of the flattened (iy, iz) plane of one ix -- no ragged sixth tile per row
// (-16 % tiles), the FC rows of a tile are consecutive -- and writes density_act (row 0) and / or the three raw feature rows.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void lattice_decode_kernel(
    const float *__restrict__ blob, const float *__restrict__ FA, const float *__restrict__ FB,
    const float *__restrict__ FC, int R, int nx, float density_bias, float out_add, float *__restrict__ out,
    float *__restrict__ features) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpPackHeader hd = *reinterpret_cast<const MlpPackHeader *>(blob);
    const int NH = hd.NH;
    load_weights_to_lds(smem, blob, hd);
    const LdsView L = lds_view(smem, NH);
    const int lane = threadIdx.x & 63, nwave = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = lane & 31, h = lane >> 5;
    const long plane = (long)R * R;
    const long tpx = (plane + 31) / 32, ntiles = (long)nx * tpx;
    const long nw_total = (long)gridDim.x * nwave;
    // XCD band order as in density_grid_kernel: one XCD streams one band of ix (FA / FB rows)
    long wid = (long)blockIdx.x * nwave + wave;
    if (gridDim.x % 8 == 0) wid = ((long)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3)) * nwave + wave;
    const long t_begin = ntiles * wid / nw_total, t_end = ntiles * (wid + 1) / nw_total;
    for (long t = t_begin; t < t_end; ++t) {
        const int ixl = (int)(t / tpx);
        const long flat = (t - (long)ixl * tpx) * 32 + p;
        const long fc = min(flat, plane - 1);
        const int iy = (int)(fc / R), iz = (int)(fc - (long)iy * R);
        f32x16 x0, x1, y0, y1;
        load_row32(FA + ((long)ixl * R + iy) * 64 + h * 32, x0, x1);
        load_row32(FB + ((long)ixl * R + iz) * 64 + h * 32, y0, y1);
        x0 += y0; x1 += y1;
        load_row32(FC + fc * 64 + h * 32, y0, y1);
        x0 += y0; x1 += y1;
        x0 = silu16(x0); x1 = silu16(x1);
        hidden_layers(L, NH, lane, h, x0, x1);
        const float d = last_dot(L, 0, h, x0, x1);
        const float f0 = last_dot(L, 1, h, x0, x1), f1 = last_dot(L, 2, h, x0, x1), f2 = last_dot(L, 3, h, x0, x1);
        if (h == 0 && flat < plane) {
            const long idx = (long)ixl * plane + flat;
            if (out) out[idx] = exp_f(d + density_bias) + out_add;
            if (features) { features[3 * idx] = f0; features[3 * idx + 1] = f1; features[3 * idx + 2] = f2; }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// bf16 THREE-LIMB mode of the dense grid (SCULPT_DENSITY_BF16L3, the default of TSR.extract_meshes): the eight 64x64
// hidden layers on v_mfma_f32_32x32x16_bf16 with both operands split into three bf16 limbs,
//     x = x1 + x2 + x3,  W = W1 + W2 + W3        EXACTLY (8 + 8 + 8 = 24 significant bits, fp32 exponent range:
//                                                 every limb is the round-to-nearest bf16 of the exact remainder, and
//                                                 the last remainder has at most 8 significant bits)
//     W.x = W1.x3 + W3.x1 + W2.x2 + W1.x2 + W2.x1 + W1.x1   (+ W2.x3 + W3.x2 + W3.x3 < 2^-23 |W||x|, dropped)
// Every bf16 x bf16 product is exact in fp32 and the matrix pipe accumulates in fp32, so this is fp32 arithmetic with the
// operands carried to 24 bits -- not a narrower format: no range limit, no fallback.  48 bf16 MFMAs (1536 cycles) per
// layer and 32 points instead of 64 fp32 MFMAs (4096 cycles).  Tables, SiLU, the last layer and exp stay fp32; the
// accumulator of layer l is the B operand of layer l+1 after the split, so activations still never leave registers.
// W1 | W2 of all layers sit in LDS (128 KiB); the 8 KiB of W3 a layer needs come from L2 (64 KiB for all layers, read by
// every wave of the chip): the loads are issued before the SiLU + split of the previous layer's output and land under it.
// ---------------------------------------------------------------------------------------------

template <int NT>
__global__ __launch_bounds__(NT) void density_grid_l3_kernel(
    const float *__restrict__ blob, const float *__restrict__ FA, const float *__restrict__ FB,
    const float *__restrict__ FC, int R, int nx, float density_bias, float out_add, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // [W1 | W2: NH*4096][bacc][wlast][blast]
    const MlpPackHeader hd = *reinterpret_cast<const MlpPackHeader *>(blob);
    const int NH = hd.NH;
    l3_load_lds(smem, blob, hd);
    const LdsView L = lds_view(smem, NH);
    const int lane = threadIdx.x & 63, nwave = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = lane & 31, h = lane >> 5;
    const int nzb = (R + 31) / 32;
    const long ntiles = (long)nx * nzb * R;
    const long nw_total = (long)gridDim.x * nwave;
    long wid = (long)blockIdx.x * nwave + wave;
    if (gridDim.x % 8 == 0) wid = ((long)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3)) * nwave + wave;
    const long t_begin = ntiles * wid / nw_total, t_end = ntiles * (wid + 1) / nw_total;
    int iy = (int)(t_begin % R);
    int zb = (int)((t_begin / R) % nzb), ixl = (int)((t_begin / R) / nzb);
    const tbf16x8 *A = reinterpret_cast<const tbf16x8 *>(smem) + lane;               // [l][part][T][s][lane]
    const tbf16x8 *A3 = reinterpret_cast<const tbf16x8 *>(blob + hd.off_w3) + lane;  // [l][T][s][lane], global (L2)

    for (long t = t_begin; t < t_end; ++t, ++iy) {
        if (iy == R) {
            iy = 0;
            if (++zb == nzb) { zb = 0; ++ixl; }
        }
        const int iz = zb * 32 + p;
        const int izc = min(iz, R - 1);
        f32x16 x0, x1, y0, y1;
        load_row32(FA + ((long)ixl * R + iy) * 64 + h * 32, x0, x1);
        load_row32(FB + ((long)ixl * R + izc) * 64 + h * 32, y0, y1);
        x0 += y0; x1 += y1;
        load_row32(FC + ((long)iy * R + izc) * 64 + h * 32, y0, y1);
        x0 += y0; x1 += y1;
        for (int l = 0; l < NH; ++l) {
            // third-limb weights of this layer: in flight while the VALU work below runs
            tbf16x8 c0[4], c1[4];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                c0[s4] = A3[(long)l * 512 + (0 * 4 + s4) * 64];
                c1[s4] = A3[(long)l * 512 + (1 * 4 + s4) * 64];
            }
            // keep the eight loads HERE: left alone, hipcc sinks each one to just before the MFMA that consumes it and
            // waits vmcnt(0) there -- eight exposed L2 round trips per layer
            __builtin_amdgcn_sched_barrier(0);
            const tbf16x8 *Al = A + (long)l * 16 * 64;
            f32x16 acc0, acc1;
            {
                x0 = silu16_scalar(x0);
                x1 = silu16_scalar(x1);
                tbf16x8 b1[4], b2[4], b3[4];  // B operands of the four k-steps: tiles (x0: s = 0,1), (x1: s = 2,3)
                split16_l3(x0, b1, b2, b3);
                split16_l3(x1, b1 + 2, b2 + 2, b3 + 2);
                acc0 = lds_bias16(L.bacc, l + 1, h, 0);
                acc1 = lds_bias16(L.bacc, l + 1, h, 1);
                // small terms first (order 2^-16 of the result), the leading product last
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) {
                    const tbf16x8 a10 = Al[((0 * 2 + 0) * 4 + s4) * 64], a11 = Al[((0 * 2 + 1) * 4 + s4) * 64];
                    const tbf16x8 a20 = Al[((1 * 2 + 0) * 4 + s4) * 64], a21 = Al[((1 * 2 + 1) * 4 + s4) * 64];
                    acc0 = mfma16(a10, b3[s4], acc0);
                    acc1 = mfma16(a11, b3[s4], acc1);
                    acc0 = mfma16(c0[s4], b1[s4], acc0);
                    acc1 = mfma16(c1[s4], b1[s4], acc1);
                    acc0 = mfma16(a20, b2[s4], acc0);
                    acc1 = mfma16(a21, b2[s4], acc1);
                    acc0 = mfma16(a10, b2[s4], acc0);
                    acc1 = mfma16(a11, b2[s4], acc1);
                    acc0 = mfma16(a20, b1[s4], acc0);
                    acc1 = mfma16(a21, b1[s4], acc1);
                    acc0 = mfma16(a10, b1[s4], acc0);
                    acc1 = mfma16(a11, b1[s4], acc1);
                }
            }
            x0 = acc0;
            x1 = acc1;
        }
        x0 = silu16_scalar(x0);
        x1 = silu16_scalar(x1);
        const float d = last_dot(L, 0, h, x0, x1);
        if (h == 0 && iz < R) out[((long)ixl * R + iy) * R + iz] = exp_f(d + density_bias) + out_add;
    }
}

// ---------------------------------------------------------------------------------------------
// The same arithmetic, scheduled inside the wave (density_grid_l3k_kernel, the default).  The kernel above leaves the overlap
// of the vector work (SiLU + split: 304 instructions per layer and tile) with the matrix work (48 MFMAs) to the four waves
// of a SIMD being out of phase; measured (profiles/round3/pmc_density_l3.txt) the SIMD is EITHER issuing vector instructions
// OR running MFMAs, 2 670 cycles per tile and layer against 1 536 of MFMA, and neither per-wave priorities, a raised
// priority in the matrix phase nor a start-up stagger change that.  What does overlap is a wave's OWN vector work issued
// right behind its MFMAs (tools/micro/mfma_fill.hip: six plain or three transcendental instructions per MFMA are free).
// So the layer runs as a k-step software pipeline: while the twelve MFMAs of k-step g run, the SiLU + split of the eight
// values of k-step g + 1 is issued in their shadow -- one MFMA, then one "chunk" of eight plain / four transcendental
// vector instructions, fenced by sched_barrier so that hipcc keeps the interleave.  A and W3 fragments are fetched (LDS / L2)
// a few slots ahead of their first use.
// ---------------------------------------------------------------------------------------------

template <int NT>
__global__ __launch_bounds__(NT) void density_grid_l3k_kernel(
    const float *__restrict__ blob, const float *__restrict__ FA, const float *__restrict__ FB,
    const float *__restrict__ FC, int R, int nx, float density_bias, float out_add, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // [W1 | W2: NH*4096][bacc][wlast][blast]
    const MlpPackHeader hd = *reinterpret_cast<const MlpPackHeader *>(blob);
    const int NH = hd.NH;  // >= 1 (the launcher sends NH == 0 to the plain kernel)
    l3_load_lds(smem, blob, hd);
    const LdsView L = lds_view(smem, NH);
    const int lane = threadIdx.x & 63, nwave = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = lane & 31, h = lane >> 5;
    const int nzb = (R + 31) / 32;
    const long ntiles = (long)nx * nzb * R;
    const long nw_total = (long)gridDim.x * nwave;
    long wid = (long)blockIdx.x * nwave + wave;
    if (gridDim.x % 8 == 0) wid = ((long)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3)) * nwave + wave;
    const long t_begin = ntiles * wid / nw_total, t_end = ntiles * (wid + 1) / nw_total;
    int iy = (int)(t_begin % R);
    int zb = (int)((t_begin / R) % nzb), ixl = (int)((t_begin / R) / nzb);
    const tbf16x8 *A = reinterpret_cast<const tbf16x8 *>(smem) + lane;               // [l][part][T][s][lane]
#ifdef SCULPT_L3_W3_LDS_EXPERIMENT
    // TIMING EXPERIMENT ONLY (wrong values): every third-limb fragment read from LDS (the W1 | W2 image) instead of L2 -- an upper
    // bound on what keeping W3 on chip could return (only three of the eight layers' W3 would really fit beside W1 | W2);
    // tools/micro/density_shape_experiment.sh, profiles/round4/density_levers.txt
    const tbf16x8 *A3 = reinterpret_cast<const tbf16x8 *>(smem) + lane;
#else
    const tbf16x8 *A3 = reinterpret_cast<const tbf16x8 *>(blob + hd.off_w3) + lane;  // [l][T][s][lane], global (L2)
#endif

    for (long t = t_begin; t < t_end; ++t, ++iy) {
        if (iy == R) {
            iy = 0;
            if (++zb == nzb) { zb = 0; ++ixl; }
        }
        const int iz = zb * 32 + p;
        f32x16 x0, x1;
        l3_table_sum(FA, FB, FC, R, ixl, iy, min(iz, R - 1), h, x0, x1);
        l3k_hidden(L, NH, A, A3, h, x0, x1);
        const float d = last_dot(L, 0, h, x0, x1);
        if (h == 0 && iz < R) out[((long)ixl * R + iy) * R + iz] = exp_f(d + density_bias) + out_add;
    }
}

}  // namespace sculpt

namespace sculpt {
// planes [3][C][H][W] -> [3][H][W][C] through an LDS tile (coalesced on both sides)
__global__ __launch_bounds__(256) void planes_channel_last_kernel(const float *__restrict__ in, float *__restrict__ out, int C,
                                                                  long HW) {
    __shared__ float tile[64][65];
    const int pl = blockIdx.z;
    const long p0 = (long)blockIdx.x * 64;
    const int c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int c = c0 + r;
        const long p = p0 + tx;
        tile[r][tx] = (c < C && p < HW) ? in[((long)pl * C + c) * HW + p] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const long p = p0 + r;
        const int c = c0 + tx;
        if (c < C && p < HW) out[((long)pl * HW + p) * C + c] = tile[tx][r];
    }
}
}  // namespace sculpt

using namespace sculpt;

extern "C" {

int sculpt_planes_channel_last(const float *planes, int C, int H, int W, float *out, sculpt_stream_t stream) {
    SC_REQUIRE(planes && out && C >= 1 && H >= 1 && W >= 1, "planes_channel_last: bad argument");
    const long HW = (long)H * W;
    hipLaunchKernelGGL(planes_channel_last_kernel, dim3(cdiv(HW, 64), cdiv(C, 64), 3), dim3(256), 0, as_stream(stream), planes,
                       out, C, HW);
    SC_LAUNCH_CHECK();
    return 0;
}

size_t sculpt_mlp_packed_bytes(int in_channels, int n_hidden_64) {
    MlpPackHeader hd;
    pack_layout(in_channels, n_hidden_64, &hd);
    return (size_t)hd.total_floats * sizeof(float);
}

int sculpt_mlp_pack(const float *const *Wh, const float *const *bh, int n_layers, const int *dims,
                    void *packed_host, size_t packed_bytes) {
    SC_REQUIRE(n_layers >= 2, "mlp_pack: need at least 2 layers");
    const int K0 = dims[0], NH = n_layers - 2;
    SC_REQUIRE(K0 % 2 == 0 && K0 > 0, "mlp_pack: in_channels must be even");
    for (int l = 1; l < n_layers; ++l) SC_REQUIRE(dims[l] == HID, "mlp_pack: hidden width must be 64 (got %d)", dims[l]);
    SC_REQUIRE(dims[n_layers] == 4, "mlp_pack: last layer must have 4 outputs");
    MlpPackHeader hd;
    pack_layout(K0, NH, &hd);
    SC_REQUIRE(packed_bytes >= (size_t)hd.total_floats * 4, "mlp_pack: buffer too small");
    float *o = reinterpret_cast<float *>(packed_host);
    memset(o, 0, (size_t)hd.total_floats * 4);
    memcpy(o, &hd, sizeof(hd));
    // activations are carried scaled by log2(e) (silu_f): fold the scale into layer 0, the hidden biases and the last layer
    const double LOG2E = 1.4426950408889634074, LN2 = 0.69314718055994530942;
    auto up = [&](float w) { return (float)((double)w * LOG2E); };
    for (size_t i = 0; i < (size_t)HID * K0; ++i) o[hd.off_w0raw + i] = up(Wh[0][i]);
    for (int i = 0; i < HID; ++i) o[hd.off_b0raw + i] = up(bh[0][i]);
    const int S0 = K0 / 2;
    for (int T = 0; T < 2; ++T)
        for (int s = 0; s < S0; ++s)
            for (int lane = 0; lane < 64; ++lane)
                o[hd.off_a0 + (T * S0 + s) * 64 + lane] = up(Wh[0][(size_t)(32 * T + (lane & 31)) * K0 + (lane >> 5) * S0 + s]);
    for (int l = 0; l <= NH; ++l)
        for (int h = 0; h < 2; ++h)
            for (int t = 0; t < 2; ++t)
                for (int r = 0; r < 16; ++r) o[hd.off_bacc + ((l * 2 + h) * 2 + t) * 16 + r] = up(bh[l][nrow(t, r, h)]);
    for (int l = 0; l < NH; ++l) {
        const float *Wl = Wh[l + 1];
        for (int T = 0; T < 2; ++T)
            for (int s = 0; s < 32; ++s)
                for (int lane = 0; lane < 64; ++lane) {
                    const int k = nrow(s >> 4, s & 15, lane >> 5);
                    o[hd.off_hid + ((((l * 2 + T) * 8 + (s >> 2)) * 64 + lane) * 4) + (s & 3)] =
                        Wl[(size_t)(32 * T + (lane & 31)) * HID + k];
                }
    }
    const float *WL = Wh[n_layers - 1];
    for (int oo = 0; oo < 4; ++oo)
        for (int h = 0; h < 2; ++h)
            for (int t = 0; t < 2; ++t)
                for (int r = 0; r < 16; ++r)
                    o[hd.off_wlast + ((oo * 2 + h) * 2 + t) * 16 + r] = (float)((double)WL[(size_t)oo * HID + nrow(t, r, h)] * LN2);
    for (int oo = 0; oo < 4; ++oo) o[hd.off_blast + oo] = bh[n_layers - 1][oo];
    // W = W1 + W2 (+ W3 below) as bf16 limbs, round-to-nearest-even (the three-limb kernels; pass A of the filtered grid multiplies
    // by W1 alone), k order = the accumulator order of the previous
    // layer seen as a 32x32x16 B operand: k(s, kg, j) = 16 s + 8 (j >> 2) + 4 kg + (j & 3)
    uint16_t *x3 = reinterpret_cast<uint16_t *>(o + hd.off_x3);
    for (int l = 0; l < NH; ++l) {
        const float *Wl = Wh[l + 1];
        for (int part = 0; part < 2; ++part)
            for (int T = 0; T < 2; ++T)
                for (int s4 = 0; s4 < 4; ++s4)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int k = 16 * s4 + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3);
                            const float w = Wl[(size_t)(32 * T + (lane & 31)) * HID + k];
                            const uint16_t hi = host_f32_to_bf16(w);
                            const uint16_t lo = host_f32_to_bf16(w - host_bf16_to_f32(hi));
                            x3[(size_t)l * 8192 + ((((part * 2 + T) * 4 + s4) * 64 + lane) * 8) + j] = part ? lo : hi;
                        }
    }
    // bf16 3-limb mode: W = W1 + W2 + W3 EXACTLY (W1, W2 are the two parts above; a 24-bit significand minus two
    // round-to-nearest 8-bit limbs leaves at most 8 significant bits, so W3 = W - W1 - W2 is itself a bf16 value)
    uint16_t *w3 = reinterpret_cast<uint16_t *>(o + hd.off_w3);
    for (int l = 0; l < NH; ++l) {
        const float *Wl = Wh[l + 1];
        for (int T = 0; T < 2; ++T)
            for (int s4 = 0; s4 < 4; ++s4)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int k = 16 * s4 + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3);
                        const float w = Wl[(size_t)(32 * T + (lane & 31)) * HID + k];
                        const float w1 = host_bf16_to_f32(host_f32_to_bf16(w));
                        const float r1 = w - w1;
                        const float w2 = host_bf16_to_f32(host_f32_to_bf16(r1));
                        w3[(size_t)l * 4096 + (((T * 4 + s4) * 64 + lane) * 8) + j] = host_f32_to_bf16(r1 - w2);
                    }
    }
    // the same with IEEE half parts (11-bit significands): pass A's fp16 operands are the leading part
    _Float16 *x3h = reinterpret_cast<_Float16 *>(o + hd.off_x3h);
    for (int l = 0; l < NH; ++l) {
        const float *Wl = Wh[l + 1];
        for (int part = 0; part < 2; ++part)
            for (int T = 0; T < 2; ++T)
                for (int s4 = 0; s4 < 4; ++s4)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int k = 16 * s4 + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3);
                            const float w = Wl[(size_t)(32 * T + (lane & 31)) * HID + k];
                            const _Float16 hi = (_Float16)w;
                            const _Float16 lo = (_Float16)(w - (float)hi);
                            x3h[(size_t)l * 8192 + ((((part * 2 + T) * 4 + s4) * 64 + lane) * 8) + j] = part ? lo : hi;
                        }
    }
    return 0;
}

static size_t lds_bytes_for(int NH) { return (size_t)(NH * 4096 + (NH + 1) * 64 + 256 + 4) * sizeof(float); }

int sculpt_triplane_query(const float *planes, int C, int H, int W, const void *mlp_packed,
                          int n_hidden_64, const float *points, int64_t N, float radius, float density_bias,
                          float *density, float *features, float *density_act, float *color,
                          sculpt_stream_t stream) {
    return sculpt_triplane_query_ex(planes, C, H, W, mlp_packed, n_hidden_64, points, N, radius, density_bias, 0u,
                                    density, features, density_act, color, stream);
}

int sculpt_triplane_query_ex(const float *planes, int C, int H, int W, const void *mlp_packed,
                             int n_hidden_64, const float *points, int64_t N, float radius, float density_bias,
                             unsigned flags, float *density, float *features, float *density_act, float *color,
                             sculpt_stream_t stream) {
    hipStream_t st = as_stream(stream);
    SC_REQUIRE(C == 40, "triplane_query: built for C=40 channels per plane (got %d)", C);
    SC_REQUIRE(planes && mlp_packed, "triplane_query: null input");
    if (N <= 0) return 0;
    SC_REQUIRE(points, "triplane_query: null points");
    SC_REQUIRE(n_hidden_64 >= 0, "triplane_query: bad n_hidden_64");
    size_t lds = lds_bytes_for(n_hidden_64);
    SC_REQUIRE(lds <= 160 * 1024, "triplane_query: %d hidden layers do not fit LDS", n_hidden_64);
    const bool ac = flags & SCULPT_QUERY_ALIGN_CORNERS, cl = flags & SCULPT_QUERY_CHANNEL_LAST;
    const size_t a0_bytes = (size_t)3 * C * 64 * sizeof(float);
    const int a0_lds = (cl && lds + a0_bytes <= 160 * 1024) ? 1 : 0;
    if (a0_lds) lds += a0_bytes;
    auto kern = cl ? (ac ? query_points_kernel<40, true, true> : query_points_kernel<40, false, true>)
                   : (ac ? query_points_kernel<40, true, false> : query_points_kernel<40, false, false>);
    SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long ntiles = (N + 31) / 32;
    const int grid = (int)std::min<long>((ntiles + 7) / 8, num_cus());
    const float span = (float)((double)radius - (double)(-radius));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, planes, H, W,
                       reinterpret_cast<const float *>(mlp_packed), points, (long)N, radius, span,
                       density_bias, density, features, density_act, color, a0_lds);
    SC_LAUNCH_CHECK();
    return 0;
}

size_t sculpt_density_grid_workspace_bytes(int R, int nx) {
    return ((size_t)2 * nx * R + (size_t)R * R) * 64 * sizeof(float);
}

int sculpt_plane_features(const float *planes, int C, int H, int W, const void *mlp_packed,
                          const float *axis_coords, int R, int x_begin, int x_end, float radius,
                          void *workspace, sculpt_stream_t stream) {
    return sculpt_plane_features_ex(planes, C, H, W, mlp_packed, axis_coords, R, x_begin, x_end, radius, 0u, workspace, stream);
}

int sculpt_plane_features_ex(const float *planes, int C, int H, int W, const void *mlp_packed,
                             const float *axis_coords, int R, int x_begin, int x_end, float radius, unsigned flags,
                             void *workspace, sculpt_stream_t stream) {
    hipStream_t st = as_stream(stream);
    SC_REQUIRE((flags & ~SCULPT_QUERY_ALIGN_CORNERS) == 0, "plane_features: planes are channel-first [3][C][H][W]; unknown flags %u", flags);
    SC_REQUIRE(C == 40, "plane_features: built for C=40 channels per plane (got %d)", C);
    SC_REQUIRE(planes && mlp_packed && axis_coords && workspace, "plane_features: null argument");
    SC_REQUIRE(R >= 2 && x_begin >= 0 && x_end <= R && x_begin < x_end, "plane_features: bad range [%d,%d) of %d", x_begin, x_end, R);
    const int nx = x_end - x_begin;
    float *FA = reinterpret_cast<float *>(workspace);
    float *FB = FA + (size_t)nx * R * 64;
    float *FC = FB + (size_t)nx * R * 64;
    const float span = (float)((double)radius - (double)(-radius));
    const long pairs = 2L * nx * R + (long)R * R;
    (void)pairs;
    const long pf_bg = (R + 3) / 4;
    const long pf_blocks = 2 * (long)((nx + 63) / 64) * pf_bg + (long)((R + 63) / 64) * pf_bg;
    if (flags & SCULPT_QUERY_ALIGN_CORNERS)
        hipLaunchKernelGGL((plane_features_kernel<40, true>), dim3((unsigned)pf_blocks), dim3(256), 0, st, planes, H, W,
                           reinterpret_cast<const float *>(mlp_packed), axis_coords, R, x_begin, nx, radius,
                           span, FA, FB, FC);
    else
        hipLaunchKernelGGL((plane_features_kernel<40, false>), dim3((unsigned)pf_blocks), dim3(256), 0, st, planes, H, W,
                           reinterpret_cast<const float *>(mlp_packed), axis_coords, R, x_begin, nx, radius,
                           span, FA, FB, FC);
    SC_LAUNCH_CHECK();
    return 0;
}

int sculpt_density_grid(const void *mlp_packed, int n_hidden_64, int R, int x_begin, int x_end,
                        float density_bias, float out_add, const void *workspace, float *out,
                        sculpt_stream_t stream) {
    return sculpt_density_grid_ex(mlp_packed, n_hidden_64, R, x_begin, x_end, density_bias, out_add, workspace, out, 0u,
                                  stream);
}

int sculpt_density_grid_ex(const void *mlp_packed, int n_hidden_64, int R, int x_begin, int x_end,
                           float density_bias, float out_add, const void *workspace, float *out, unsigned flags,
                           sculpt_stream_t stream) {
    hipStream_t st = as_stream(stream);
    SC_REQUIRE(mlp_packed && workspace && out, "density_grid: null argument");
    SC_REQUIRE((flags & ~SCULPT_DENSITY_BF16L3) == 0, "density_grid: unknown flags %u (the two-limb modes 1 / 2 were removed)", flags);
    SC_REQUIRE(R >= 2 && x_begin >= 0 && x_end <= R && x_begin < x_end, "density_grid: bad range [%d,%d) of %d", x_begin, x_end, R);
    SC_REQUIRE(n_hidden_64 >= 0, "density_grid: bad n_hidden_64");
    const size_t lds = lds_bytes_for(n_hidden_64);
    SC_REQUIRE(lds <= 160 * 1024, "density_grid: %d hidden layers do not fit LDS", n_hidden_64);
    const int nx = x_end - x_begin;
    const float *FA = reinterpret_cast<const float *>(workspace);
    const float *FB = FA + (size_t)nx * R * 64;
    const float *FC = FB + (size_t)nx * R * 64;
    const long ntiles = (long)nx * ((R + 31) / 32) * R;
    if ((flags & SCULPT_DENSITY_BF16L3) && n_hidden_64 >= 1) {  // without hidden layers there is nothing to split: fp32 kernel
        // SCULPT_DENSITY_FORM=nokstep (read per call): the phase-separated kernel instead of the k-step pipeline -- the same
        // arithmetic in the same order, the reference the pipelined kernel is pinned to bit for bit (tests/test_gpu_triplane.py)
        const bool kstep = !form_has("SCULPT_DENSITY_FORM", "nokstep");
        constexpr int nt = 1024;
        auto kern = kstep ? density_grid_l3k_kernel<1024> : density_grid_l3_kernel<1024>;
        SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const int nwave = nt / 64;
        const int grid = (int)std::min<long>((ntiles + nwave - 1) / nwave, num_cus());
        hipLaunchKernelGGL(kern, dim3(grid), dim3(nt), lds, st, reinterpret_cast<const float *>(mlp_packed), FA, FB, FC, R, nx,
                           density_bias, out_add, out);
        SC_LAUNCH_CHECK();
        return 0;
    }
    {
        SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(density_grid_kernel<1024>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const int grid = (int)std::min<long>((ntiles + 15) / 16, num_cus());
        hipLaunchKernelGGL(density_grid_kernel<1024>, dim3(grid), dim3(1024), lds, st,
                           reinterpret_cast<const float *>(mlp_packed), FA, FB, FC, R, nx, density_bias, out_add, out, 1);
    }
    SC_LAUNCH_CHECK();
    return 0;
}

int sculpt_grid_decode(const void *mlp_packed, int n_hidden_64, int R, int x_begin, int x_end, float density_bias,
                       float out_add, const void *workspace, float *density_act, float *features, sculpt_stream_t stream) {
    hipStream_t st = as_stream(stream);
    SC_REQUIRE(mlp_packed && workspace && (density_act || features), "grid_decode: null argument");
    SC_REQUIRE(R >= 2 && x_begin >= 0 && x_end <= R && x_begin < x_end, "grid_decode: bad range [%d,%d) of %d", x_begin, x_end, R);
    SC_REQUIRE(n_hidden_64 >= 0, "grid_decode: bad n_hidden_64");
    const size_t lds = lds_bytes_for(n_hidden_64);
    SC_REQUIRE(lds <= 160 * 1024, "grid_decode: %d hidden layers do not fit LDS", n_hidden_64);
    const int nx = x_end - x_begin;
    const float *FA = reinterpret_cast<const float *>(workspace);
    const float *FB = FA + (size_t)nx * R * 64;
    const float *FC = FB + (size_t)nx * R * 64;
    const long ntiles = (long)nx * (((long)R * R + 31) / 32);
    SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(lattice_decode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int grid = (int)std::min<long>((ntiles + 15) / 16, num_cus());
    hipLaunchKernelGGL(lattice_decode_kernel, dim3(grid), dim3(1024), lds, st, reinterpret_cast<const float *>(mlp_packed), FA, FB, FC,
                       R, nx, density_bias, out_add, density_act, features);
    SC_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
