// Fused attention for the fast parity mode (TSR(precision="bf16l3")): fp32 Q / K / V^T in, fp32 O out, fp32 ARITHMETIC on the bf16
// matrix pipe -- both products, S = (c q) . k and O = P . v, take their operands split EXACTLY into three bf16 limbs and sum
// the six limb products of order >= 2^-16 in fp32 (gemm_l3.hip has the argument); the softmax (running maximum, exp2, row sums,
// rescale) is plain fp32 in registers.  Replaces the parity modes' three launches per attention (scores into an fp32
// [heads][Tq][Tk] scratch, row softmax, P V: 600 MB written and re-read three times per backbone self-attention) by one.
// Reference: F.scaled_dot_product_attention, TripoSR/tsr/models/transformer/attention.py:629-631 (fp32, no autocast); HF
// ViTSelfAttention's eager softmax(QK^T / 8) V.
//
// One workgroup = 4 waves = 128 queries of one head; a wave owns 32 queries (the query is the MFMA column, lane & 31, so a
// lane holds 2 x 16 scores of ONE query per 64-key tile and the softmax statistics are in-register + one cross-half exchange).
// Per 64-key tile:  K rows and V^T rows arrive as fp32 through registers (loaded one tile ahead), are split and written as
// limbs into a [limb][8-wide k chunk][row] LDS image (gemm_l3.hip's: a fragment is 512 contiguous bytes);
//   S^T = K . Q^T     48 MFMAs (2 row tiles x 4 k-steps x 6 limb products); the Q limbs stay in registers for the whole loop;
//                     key row m of a 32-row tile sits at LDS row m with bits 2 and 3 swapped, so that a lane's accumulator
//                     registers 8 g .. 8 g + 7 hold 8 CONTIGUOUS keys -- exactly one B fragment of the second product;
//   P = exp2(S - M)   fp32; split into three limbs in registers (no LDS round trip);
//   O^T += V^T . P^T  48 MFMAs.
// One 49-KiB LDS buffer, two barriers per tile; two workgroups per CU overlap one's split / softmax with the other's MFMAs.
//
// Two kernels share the prologue, the ragged-tile mask with the row maximum, and the output epilogue below:
//   attention_l3_kernel        4 waves, the plain loop above (small launches: the image tokenizer);
//   attention_l3_pipe_kernel   8 waves, the vector work in the shadows of the wave's own MFMAs (the backbone).
// Splits, limb products and the MFMA come from limbs.h (Limb<LT_BF16X3>).  The two-fp16-limb form of the pipelined kernel is
// attention_l2.hip.
#include <stdlib.h>

#include "attention_tile.h"
#include "limbs.h"

namespace sculpt {

static constexpr int AL_CS = 64 * 16 + 16;    // bytes from one k-chunk plane (64 rows x 16 B) to the next (+16: the 8-byte writes
                                              // of a 16-lane group land on 16 different 8-byte slots of the 128-byte bank row)
static constexpr int AL_LT = 8 * AL_CS;       // one limb of one operand tile (64 rows x 64 k)
template <int FMT> static constexpr int AL_OP = Limb<FMT>::NL * AL_LT;   // one operand tile, all limbs

// What a lane is given: its query = MFMA column qc (lane & 31) of its wave's 32, k-half h (lane >> 5); its staging row sr and
// quad sq (thread t: quad t % 16 of rows t / 16 + ..) with the head's K / V^T pointers at them; the batch entry's outputs
struct AttnL3Lane {
    int tid, qc, h, head, q, sr, sq;
    const float *Kh, *Vh;   // + key * ldk;  + rows * ldvt + key0
    float *O;
    int o_row0;
};

// The batch entry (blockIdx.z), the lane's place among the NW * 32 queries of the workgroup, and its Q limbs (B operand of the
// first product: B[k = 8 h + j][column = query]), scaled by softmax_scale * log2(e) in fp32
template <int FMT, int NW>
__device__ __forceinline__ AttnL3Lane attn_l3_prologue(const float *Q, int ldq, const float *K, const float *Vt, int ldvt, float *O,
                                                       int o_row0, int Tq, float scale_log2e, const AttnL3Batch &ab,
                                                       typename Limb<FMT>::frag (&qf)[4][Limb<FMT>::NL]) {
    AttnL3Lane a;
    Q += blockIdx.z * ab.q_bs; K += blockIdx.z * ab.k_bs; Vt += blockIdx.z * ab.vt_bs;
    if (O) O += blockIdx.z * ab.o_bs;
    a.O = O;
    a.o_row0 = o_row0 + blockIdx.z * ab.o_row_bs;
    a.tid = threadIdx.x;
    const int lane = a.tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(a.tid >> 6);
    a.qc = lane & 31; a.h = lane >> 5;
    a.head = blockIdx.y;
    a.q = blockIdx.x * (NW * 32) + wave * 32 + a.qc;
    const int qld = min(a.q, Tq - 1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const float4 u = *reinterpret_cast<const float4 *>(Q + (long)qld * ldq + a.head * 64 + ks * 16 + a.h * 8);
        const float4 v = *reinterpret_cast<const float4 *>(Q + (long)qld * ldq + a.head * 64 + ks * 16 + a.h * 8 + 4);
        const float x[8] = {u.x * scale_log2e, u.y * scale_log2e, u.z * scale_log2e, u.w * scale_log2e,
                            v.x * scale_log2e, v.y * scale_log2e, v.z * scale_log2e, v.w * scale_log2e};
        Limb<FMT>::split8(x, qf[ks]);
    }
    a.sr = a.tid >> 4; a.sq = a.tid & 15;
    a.Kh = K + a.head * 64 + 4 * a.sq;
    a.Vh = Vt + (long)(a.head * 64 + a.sr) * ldvt + 4 * a.sq;
    return a;
}

// The scores of tile t as the lane holds them: s{rt}[8 g + j] = key 64 t + 32 rt + 16 g + 8 h + j.  Keys past Tk (ragged last
// tile, wave-uniform) score -inf; the row maximum joins the running one.  Returns the new maximum (finite from the first tile on:
// every tile has at least one valid key); alpha = the rescale of what was summed under the old one (exp2(-inf) = 0 on the first tile)
__device__ __forceinline__ float attn_l3_row_max(f32x16 &s0, f32x16 &s1, int t, int Tk, int h, float &m_run, float &alpha) {
    if (t * 64 + 64 > Tk) {
        const int kb = t * 64 + 8 * h;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kb + (r & 7) + 16 * (r >> 3);
            if (key >= Tk) s0[r] = -INFINITY;
            if (key + 32 >= Tk) s1[r] = -INFINITY;
        }
    }
    float mx = fmaxf(s0[0], s1[0]);
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, fmaxf(s0[r], s1[r]));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    return m_new;
}

// O = O^T accumulators / row sum: fp32 rows, or -- O_lt given -- limbs in the limb-tiled layout (limbs.h): the operand of the to_out
// Linear (gemm_l3p.hip); row o_row0 + q of a matrix with o_k8 chunks per row, columns head * 64 ..
__device__ __forceinline__ void attn_l3_store(const f32x16 &o0, const f32x16 &o1, float l_run, const AttnL3Lane a, int ldo, int Tq,
                                              unsigned char *O_lt, int o_k8, int o_fmt) {
    const int q = a.q, h = a.h, head = a.head;
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    if (q < Tq && O_lt) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const float u[4] = {o0[4 * g4] * inv, o0[4 * g4 + 1] * inv, o0[4 * g4 + 2] * inv, o0[4 * g4 + 3] * inv};
            const float v[4] = {o1[4 * g4] * inv, o1[4 * g4 + 1] * inv, o1[4 * g4 + 2] * inv, o1[4 * g4 + 3] * inv};
            lt_store4(O_lt, o_k8, (long)a.o_row0 + q, head * 64 + 8 * g4 + 4 * h, u, o_fmt);
            lt_store4(O_lt, o_k8, (long)a.o_row0 + q, head * 64 + 32 + 8 * g4 + 4 * h, v, o_fmt);
        }
    } else if (q < Tq) {
        float *orow = a.O + (long)q * ldo + head * 64;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {   // registers 4 g4 .. 4 g4 + 3 = d 8 g4 + 4 h + {0..3} (+ 32 for o1)
            *reinterpret_cast<float4 *>(orow + 8 * g4 + 4 * h) =
                make_float4(o0[4 * g4] * inv, o0[4 * g4 + 1] * inv, o0[4 * g4 + 2] * inv, o0[4 * g4 + 3] * inv);
            *reinterpret_cast<float4 *>(orow + 32 + 8 * g4 + 4 * h) =
                make_float4(o1[4 * g4] * inv, o1[4 * g4 + 1] * inv, o1[4 * g4 + 2] * inv, o1[4 * g4 + 3] * inv);
        }
    }
}

// The fragment of limb l for k-step ks (chunk 2 ks + h), rows 32 up + (lane & 31); src = the operand tile + the lane's h * AL_CS + qc * 16
template <int FMT>
__device__ __forceinline__ typename Limb<FMT>::frag attn_l3_frag(const unsigned char *src, int l, int ks, int up) {
    return *reinterpret_cast<const typename Limb<FMT>::frag *>(src + l * AL_LT + 2 * ks * AL_CS + up * (32 * 16));
}

__global__ __launch_bounds__(256, 2) void attention_l3_kernel(const float *__restrict__ Q, int ldq, const float *__restrict__ K, int ldk,
                                                              const float *__restrict__ Vt, int ldvt, float *__restrict__ O, int ldo,
                                                              int Tq, int Tk, float scale_log2e, unsigned char *__restrict__ O_lt,
                                                              int o_row0, int o_k8, AttnL3Batch ab) {
    typedef Limb<LT_BF16X3> L;
    constexpr int OP = AL_OP<LT_BF16X3>;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * OP];   // [K limbs | V^T limbs]
    L::frag qf[4][3];
    const AttnL3Lane a = attn_l3_prologue<LT_BF16X3, 4>(Q, ldq, K, Vt, ldvt, O, o_row0, Tq, scale_log2e, ab, qf);
    const int sr = a.sr, sq = a.sq;

    // staging: a tile is 64 rows x 64 fp32 = 1024 float4 per operand; thread t takes quad t % 16 of rows t / 16 + 16 i
    // LDS byte offsets of this thread's 8-byte pieces: chunk = sq / 2, half = sq % 2; K rows go to their permuted position
    int kofs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int kk = sr + 16 * i, m = kk & 31;
        const int pos = (kk & 32) | (m & 0x13) | ((m & 4) << 1) | ((m & 8) >> 1);
        kofs[i] = (sq >> 1) * AL_CS + pos * 16 + (sq & 1) * 8;
    }
    const int vofs = OP + (sq >> 1) * AL_CS + sr * 16 + (sq & 1) * 8;   // + 16 i rows = + 256 i bytes
    const int fro = a.h * AL_CS + a.qc * 16;                            // fragment reads (attn_l3_frag)

    const int nt = (Tk + 63) / 64;
    float4 rk[4], rv[4];
    auto gload = [&](int t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = min(t * 64 + sr + 16 * i, Tk - 1);
            rk[i] = *reinterpret_cast<const float4 *>(a.Kh + (long)key * ldk);
            rv[i] = *reinterpret_cast<const float4 *>(a.Vh + (long)(16 * i) * ldvt + t * 64);
        }
    };
    auto six = [&](f32x16 &acc, const L::frag (&x)[3], const L::frag (&y)[3]) {
#pragma unroll
        for (int s = 0; s < L::NP; ++s) acc = L::mfma(acc, x[L::PROD[s][0]], y[L::PROD[s][1]]);
    };

    f32x16 o0, o1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { o0[i] = 0.f; o1[i] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;

    gload(0);
    for (int t = 0; t < nt; ++t) {
        if (t > 0) __syncthreads();   // every wave has read the previous tile's fragments
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint2 p[3];
            L::split4(rk[i].x, rk[i].y, rk[i].z, rk[i].w, p);
#pragma unroll
            for (int l = 0; l < 3; ++l) *reinterpret_cast<uint2 *>(smem + kofs[i] + l * AL_LT) = p[l];
            L::split4(rv[i].x, rv[i].y, rv[i].z, rv[i].w, p);
#pragma unroll
            for (int l = 0; l < 3; ++l) *reinterpret_cast<uint2 *>(smem + vofs + i * 256 + l * AL_LT) = p[l];
        }
        __syncthreads();
        if (t + 1 < nt) gload(t + 1);   // the next tile travels while this one is multiplied

        // ---- S^T = K . Q^T (exponents of 2)
        f32x16 s0, s1;
#pragma unroll
        for (int i = 0; i < 16; ++i) { s0[i] = 0.f; s1[i] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            L::frag k0[3], k1[3];
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                k0[l] = attn_l3_frag<LT_BF16X3>(smem + fro, l, ks, 0);
                k1[l] = attn_l3_frag<LT_BF16X3>(smem + fro, l, ks, 1);
            }
            six(s0, k0, qf[ks]);
            six(s1, k1, qf[ks]);
        }
        float alpha;
        const float m_new = attn_l3_row_max(s0, s1, t, Tk, a.h, m_run, alpha);
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s0[r] = __builtin_amdgcn_exp2f(s0[r] - m_new);
            s1[r] = __builtin_amdgcn_exp2f(s1[r] - m_new);
            ps += s0[r] + s1[r];
        }
        l_run = l_run * alpha + ps;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }

        // ---- O^T += V^T . P^T: k-step kstep = 2 rt + g takes P registers 8 g .. 8 g + 7 of s{rt} (contiguous keys)
#pragma unroll
        for (int kstep = 0; kstep < 4; ++kstep) {
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = (kstep < 2) ? s0[8 * (kstep & 1) + j] : s1[8 * (kstep & 1) + j];
            L::frag p[3], v0[3], v1[3];
            L::split8(x, p);
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                v0[l] = attn_l3_frag<LT_BF16X3>(smem + OP + fro, l, kstep, 0);
                v1[l] = attn_l3_frag<LT_BF16X3>(smem + OP + fro, l, kstep, 1);
            }
            six(o0, v0, p);
            six(o1, v1, p);
        }
    }
    attn_l3_store(o0, o1, l_run, a, ldo, Tq, O_lt, o_k8, ab.o_fmt);
}


// ---------------------------------------------------------------------------------------------------------------------
// The same attention with the vector work issued in the shadows of the wave's own MFMAs (the default).  In the plain kernel a
// tile costs 96 MFMAs (3 072 matrix cycles) plus ~500 vector instructions that run while the matrix pipe waits (split of the next
// K / V^T rows 176, softmax ~160, split of P 176); a wave's own vector instructions right behind its own MFMA are free up to ~6
// per MFMA (tools/micro/mfma_fill.hip), another wave's are not (mfma_phase.hip).  So:
//   QK phase   8 groups of 6 MFMAs (k-step ks, key row tile rt); group g carries the split of float4 g of the NEXT tile's rows
//              (g < 4: K rows, else V^T rows) -- the limbs wait in 48 registers for the barrier at the end of the iteration;
//              the fragments of the following group are read into the registers of the one before it as they die;
//   softmax    as before (exposed: it needs all scores of the tile);
//   PV phase   4 k-steps of 2 x 6 MFMAs; the split of the 8 probabilities of k-step + 1 rides in k-step's groups.
// Stages are pinned inside their slots by empty asm statements and fenced with sched_barrier (gemm_l3.hip has the reasons).
// Same operands and the same order of every matrix sum as attention_l3_kernel; the softmax updates are written without fused
// multiply-adds here (fp contract off for the exact splits), so the two agree to fp32 rounding, not bit for bit.
// Measured (tools/time_l3_attention.py): 3072 x 3072 x 16 heads 262 -> 244 us = 0.38 of the bf16 peak by executed
// FLOPs -- the same region as the pipelined three-limb GEMM (0.43) and the density kernel (0.45): with every CU issuing MFMAs plus
// the split's vector work the chip is clock-bound, a tighter issue stream returns little.
// ---------------------------------------------------------------------------------------------------------------------
#define AL_FENCE __builtin_amdgcn_sched_barrier(0)
#define AL_PIN4(a, b, c, d) asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d))
#define AL_PIN2(a, b) asm volatile("" : "+v"(a), "+v"(b))

// One group: the format's MFMAs acc += A[i] . B[j] (smallest terms first), each followed by a fence.  X given: the stages of the
// split of the float4 *X into P[limb] ride behind them, one stage per MFMA -- limb l: convert + expand, then the exact
// remainder; the last limb: convert only.  rd given: the fragment reads rd[l] = limb l of k-step rd_ks, one behind each of the
// first NL MFMAs (the group after next's operand, into registers that died).
template <int FMT>
__device__ __forceinline__ void attn_l3_group(f32x16 &acc, const typename Limb<FMT>::frag (&A)[Limb<FMT>::NL],
                                              const typename Limb<FMT>::frag (&B)[Limb<FMT>::NL], const float4 *X, uint2 *P,
                                              typename Limb<FMT>::frag *rd = nullptr, const unsigned char *rd_src = nullptr,
                                              int rd_ks = 0) {
#pragma clang fp contract(off)
    typedef Limb<FMT> L;
    constexpr int NL = L::NL;
    float x0, x1, x2, x3, t0, t1, t2, t3;
    unsigned a[NL], b[NL];
    if (X) {
        x0 = X->x; x1 = X->y; x2 = X->z; x3 = X->w;
        AL_PIN4(x0, x1, x2, x3);
    }
#pragma unroll
    for (int s = 0; s < L::NP; ++s) {
        acc = L::mfma(acc, A[L::PROD[s][0]], B[L::PROD[s][1]]);
        const int l = s >> 1;
        if (X && s == 2 * (NL - 1)) {
            a[l] = L::cvt_pk(x0, x1); b[l] = L::cvt_pk(x2, x3);
            AL_PIN2(a[l], b[l]);
        } else if (X && s < 2 * (NL - 1) && !(s & 1)) {
            a[l] = L::cvt_pk(x0, x1); b[l] = L::cvt_pk(x2, x3);
            L::unpack(a[l], t0, t1);
            L::unpack(b[l], t2, t3);
            AL_PIN4(t0, t1, t2, t3);
        } else if (X && s < 2 * (NL - 1)) {
            x0 = x0 - t0; x1 = x1 - t1; x2 = x2 - t2; x3 = x3 - t3;   // exact
            AL_PIN4(x0, x1, x2, x3);
        }
        if (rd && s < NL) rd[s] = attn_l3_frag<FMT>(rd_src, s, rd_ks, 0);
        AL_FENCE;
    }
    if (X) {
#pragma unroll
        for (int l = 0; l < NL; ++l) P[l] = make_uint2(a[l], b[l]);
    }
}

// 8 waves = 256 queries per workgroup: a thread stages NS = two float4 per operand and tile instead of four, which is what lets
// the limbs of the next tile (24 registers on three limbs) sit beside 48 Q-limb, 64 accumulator and 48 fragment / probability
// registers without spilling (the 4-wave form needs 48 and spilled 14 registers into the loop); a 3072-query head is 12
// workgroups, 192 per attention -- as many CUs busy with 8 waves each as the 4-wave form keeps busy with 8 (two workgroups of 4).
__global__ __launch_bounds__(512) void attention_l3_pipe_kernel(const float *__restrict__ Q, int ldq, const float *__restrict__ K,
                                                                  int ldk, const float *__restrict__ Vt, int ldvt,
                                                                  float *__restrict__ O, int ldo, int Tq, int Tk, float scale_log2e,
                                                                  unsigned char *__restrict__ O_lt, int o_row0, int o_k8, AttnL3Batch ab) {
#pragma clang fp contract(off)
    constexpr int FMT = LT_BF16X3;
    typedef Limb<FMT> L;
    typedef L::frag frag;
    constexpr int NL = L::NL, OP = AL_OP<FMT>;
    constexpr int NS = 2;                           // float4 per thread, operand and tile: 1024 / (8 waves x 64)
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * OP];   // [K limbs | V^T limbs]
    frag qf[4][NL];
    const AttnL3Lane a = attn_l3_prologue<FMT, 8>(Q, ldq, K, Vt, ldvt, O, o_row0, Tq, scale_log2e, ab, qf);
    const int sr = a.sr, sq = a.sq;

    // staging: thread t takes quad t % 16 of rows t / 16 + 32 i (i = 0, 1); K row kk = sr + 32 i goes to position 32 i + pk(sr)
    // (bits 2 and 3 swapped)
    const int kofs = (sq >> 1) * AL_CS + ((sr & 0x13) | ((sr & 4) << 1) | ((sr & 8) >> 1)) * 16 + (sq & 1) * 8;   // + 512 i
    const int vofs = OP + (sq >> 1) * AL_CS + sr * 16 + (sq & 1) * 8;                                             // + 512 i
    const int fro = a.h * AL_CS + a.qc * 16;
    const unsigned char *kfr = smem + fro, *vfr = smem + OP + fro;   // fragment reads (attn_l3_frag)

    const int nt = (Tk + 63) / 64;
    float4 rk[NS], rv[NS];
    uint2 pk[NS][NL], pv[NS][NL];
    auto gload = [&](int t) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int key = min(t * 64 + sr + 32 * i, Tk - 1);
            rk[i] = *reinterpret_cast<const float4 *>(a.Kh + (long)key * ldk);
            rv[i] = *reinterpret_cast<const float4 *>(a.Vh + (long)(32 * i) * ldvt + t * 64);
        }
    };
    auto write_all = [&]() {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                *reinterpret_cast<uint2 *>(smem + kofs + i * 512 + l * AL_LT) = pk[i][l];
                *reinterpret_cast<uint2 *>(smem + vofs + i * 512 + l * AL_LT) = pv[i][l];
            }
        }
    };

    f32x16 o0, o1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { o0[i] = 0.f; o1[i] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;

    gload(0);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        L::split4(rk[i].x, rk[i].y, rk[i].z, rk[i].w, pk[i]);
        L::split4(rv[i].x, rv[i].y, rv[i].z, rv[i].w, pv[i]);
    }
    write_all();
    __syncthreads();
    if (nt > 1) gload(1);

    for (int t = 0; t < nt; ++t) {
        // ---- QK phase: S^T = K . Q^T with the split of the next tile's rows in the MFMA shadows
        f32x16 s0, s1;
#pragma unroll
        for (int i = 0; i < 16; ++i) { s0[i] = 0.f; s1[i] = 0.f; }
        frag k0[NL], k1[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) { k0[l] = attn_l3_frag<FMT>(kfr, l, 0, 0); k1[l] = attn_l3_frag<FMT>(kfr, l, 0, 1); }
        AL_FENCE;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            // group (ks, rt = 0) uses k0; k1 of this k-step is already on its way (read during the previous group).
            // k-steps 0 / 1 carry the split of the next tile's two K / two V^T float4 of this thread.
            const bool sp = ks < NS;
            attn_l3_group<FMT>(s0, k0, qf[ks], sp ? &rk[ks % NS] : nullptr, pk[ks % NS]);
            // group (ks, rt = 1) uses k1; k0 is dead: the next k-step's k0 is read into it
            if (ks < 3) {
                attn_l3_group<FMT>(s1, k1, qf[ks], sp ? &rv[ks % NS] : nullptr, pv[ks % NS], k0, kfr, ks + 1);
                // k1 is dead now: the next k-step's k1 (its reads land during the next group, which uses k0)
#pragma unroll
                for (int l = 0; l < NL; ++l) k1[l] = attn_l3_frag<FMT>(kfr, l, ks + 1, 1);
                AL_FENCE;
            } else {
                attn_l3_group<FMT>(s1, k1, qf[ks], nullptr, nullptr);
            }
        }
        // ---- softmax (fp32)
        float alpha;
        const float m_new = attn_l3_row_max(s0, s1, t, Tk, a.h, m_run, alpha);
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s0[r] = __builtin_amdgcn_exp2f(s0[r] - m_new);
            s1[r] = __builtin_amdgcn_exp2f(s1[r] - m_new);
            ps += s0[r] + s1[r];
        }
        l_run = l_run * alpha + ps;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }

        // ---- PV phase: O^T += V^T . P^T; the split of k-step + 1's probabilities in the shadows of k-step's MFMAs
        frag p[NL], v0[NL], v1[NL];
        {
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = s0[j];
            L::split8(x, p);
        }
#pragma unroll
        for (int l = 0; l < NL; ++l) { v0[l] = attn_l3_frag<FMT>(vfr, l, 0, 0); v1[l] = attn_l3_frag<FMT>(vfr, l, 0, 1); }
        AL_FENCE;
#pragma unroll
        for (int kstep = 0; kstep < 4; ++kstep) {
            lt_u32x4 n[NL];   // the next k-step's P limbs, built pair by pair
            float y[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) y[j] = (kstep + 1 < 2) ? s0[8 * ((kstep + 1) & 1) + j] : s1[8 * ((kstep + 1) & 1) + j];
            const bool more = kstep < 3;
#define AL_PAIR(i_)                                                                                      \
    do {                                                                                                \
        if (more) {                                                                                     \
            unsigned c[NL];                                                                              \
            float ya = y[2 * (i_)], yb = y[2 * (i_) + 1];                                                \
            AL_PIN2(ya, yb);                                                                             \
            L::split2(ya, yb, c);                                                                        \
            asm volatile("" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]));                                       \
            _Pragma("unroll") for (int l = 0; l < NL; ++l) n[l][i_] = c[l];                              \
        }                                                                                               \
    } while (0)
            // group (kstep, dt = 0): v0; during it v1 lands (read one group ago) -- NP MFMAs, two pair splits
#pragma unroll
            for (int s = 0; s < L::NP; ++s) {
                o0 = L::mfma(o0, v0[L::PROD[s][0]], p[L::PROD[s][1]]);
                if (s == 0) AL_PAIR(0);
                if (s == NL - 1) AL_PAIR(1);
                AL_FENCE;
            }
            // group (kstep, dt = 1): v1; v0 is dead: the next k-step's v0 is read into it
#pragma unroll
            for (int s = 0; s < L::NP; ++s) {
                o1 = L::mfma(o1, v1[L::PROD[s][0]], p[L::PROD[s][1]]);
                if (s == 0) AL_PAIR(2);
                if (s == NL - 1) AL_PAIR(3);
                if (more && s < NL) v0[s] = attn_l3_frag<FMT>(vfr, s, kstep + 1, 0);
                AL_FENCE;
            }
            if (more) {
#pragma unroll
                for (int l = 0; l < NL; ++l) v1[l] = attn_l3_frag<FMT>(vfr, l, kstep + 1, 1);
#pragma unroll
                for (int l = 0; l < NL; ++l) p[l] = __builtin_bit_cast(frag, n[l]);
                AL_FENCE;
            }
#undef AL_PAIR
        }
        if (t + 1 < nt) {
            __syncthreads();   // every wave has read this tile's fragments
            write_all();
            if (t + 2 < nt) gload(t + 2);
            __syncthreads();
        }
    }
    attn_l3_store(o0, o1, l_run, a, ldo, Tq, O_lt, o_k8, ab.o_fmt);
}
#undef AL_FENCE
#undef AL_PIN4
#undef AL_PIN2

}  // namespace sculpt

using namespace sculpt;

static int attention_l3_go(const float *Q, int ldq, const float *K, int ldk, const float *Vt, int ldvt, float *O, int ldo, void *O_lt,
                           int o_row0, int o_k8, int Tq, int Tk, int heads, float scale, sculpt_stream_t stream, int batch = 1,
                           AttnL3Batch ab = AttnL3Batch{0, 0, 0, 0, 0, 0}, int two_fp16_limbs = 0) {
    SC_REQUIRE(batch >= 1 && batch <= 65535, "attention_f32_l3: bad batch %d", batch);
    SC_REQUIRE(ab.o_fmt == LT_BF16X3 || ab.o_fmt == LT_F16X2, "attention_f32_l3: unknown limb format %d", ab.o_fmt);
    SC_REQUIRE(batch == 1 || (ab.q_bs % 4 == 0 && ab.k_bs % 4 == 0 && ab.vt_bs % 4 == 0 && ab.o_bs % 4 == 0 && ab.o_row_bs >= 0),
               "attention_f32_l3: batch strides must be multiples of 4 elements");
    SC_REQUIRE(Q && K && Vt && (O || O_lt), "attention_f32_l3: null argument");
    SC_REQUIRE(Tq >= 1 && Tk >= 1 && heads >= 1 && heads <= 65535, "attention_f32_l3: bad shape Tq=%d Tk=%d heads=%d", Tq, Tk, heads);
    SC_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0 && ldvt % 4 == 0 && ldo % 4 == 0, "attention_f32_l3: row strides must keep 16-byte alignment");
    SC_REQUIRE(ldvt >= ((Tk + 63) / 64) * 64, "attention_f32_l3: ldvt=%d must be >= round_up(Tk=%d, 64) (finite padding columns)", ldvt, Tk);
    SC_REQUIRE(scale > 0.f && scale == scale, "attention_f32_l3: scale must be positive");
    SC_REQUIRE(!O_lt || (o_row0 >= 0 && o_k8 >= heads * 8 && ((uintptr_t)O_lt & 15) == 0),
               "attention_f32_l3_limbs: the limb output needs o_row0 >= 0, >= heads * 64 columns and 16-byte alignment");
    unsigned char *olt = reinterpret_cast<unsigned char *>(O_lt);
    // the pipelined 8-wave form (256 queries per workgroup) where it keeps at least 2/3 of the CUs busy -- the backbone's 3072
    // queries x 16 heads = 192 workgroups --; otherwise (the image tokenizer: 1025 queries x 12 heads) the plain 4-wave form
    // SCULPT_ATTN_FORM tokens l3pipe / nol3pipe: always / never the pipelined form (A/B, tests; read per call)
    const int fpipe = form_has("SCULPT_ATTN_FORM", "l3pipe") ? 1 : (form_has("SCULPT_ATTN_FORM", "nol3pipe") ? 0 : -1);
    // (the two-limb arithmetic exists in the pipelined form only, and that form wins there even on the image tokenizer's 60
    // workgroups: 53 against 59 us on three limbs and 4 waves)
    const bool pipe = fpipe >= 0 ? fpipe != 0 : (two_fp16_limbs || (long)cdiv(Tq, 256) * heads * batch * 3 >= 2L * num_cus());
    // two fp16 limbs per operand (attention_l2.hip: half the matrix work) where the pipelined form runs; the small launches (the
    // image tokenizer's) stay on the three-limb 4-wave kernel
    const float scale_log2e = scale * 1.44269504088896340736f;
    if (pipe && two_fp16_limbs)
        attention_l2_pipe_launch(dim3(cdiv(Tq, 256), heads, batch), as_stream(stream), Q, ldq, K, ldk, Vt, ldvt, O, ldo, Tq, Tk,
                                 scale_log2e, olt, o_row0, o_k8, ab);
    else if (!pipe)
        hipLaunchKernelGGL(attention_l3_kernel, dim3(cdiv(Tq, 128), heads, batch), dim3(256), 0, as_stream(stream), Q, ldq, K, ldk, Vt,
                           ldvt, O, ldo, Tq, Tk, scale_log2e, olt, o_row0, o_k8, ab);
    else
        hipLaunchKernelGGL(attention_l3_pipe_kernel, dim3(cdiv(Tq, 256), heads, batch), dim3(512), 0, as_stream(stream), Q, ldq, K, ldk,
                           Vt, ldvt, O, ldo, Tq, Tk, scale_log2e, olt, o_row0, o_k8, ab);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sculpt_attention_f32_l3(const float *Q, int ldq, const float *K, int ldk, const float *Vt, int ldvt, float *O, int ldo,
                                       int Tq, int Tk, int heads, float scale, sculpt_stream_t stream) {
    SC_REQUIRE(O, "attention_f32_l3: null argument");
    return attention_l3_go(Q, ldq, K, ldk, Vt, ldvt, O, ldo, nullptr, 0, 0, Tq, Tk, heads, scale, stream);
}

extern "C" int sculpt_attention_f32_l3_limbs(const float *Q, int ldq, const float *K, int ldk, const float *Vt, int ldvt, void *O_lt,
                                             int format, int o_row0, int o_cols, int Tq, int Tk, int heads, float scale,
                                             int two_fp16_limbs, sculpt_stream_t stream) {
    SC_REQUIRE(O_lt && o_cols % 32 == 0, "attention_f32_l3_limbs: null output or o_cols=%d not a multiple of 32", o_cols);
    return attention_l3_go(Q, ldq, K, ldk, Vt, ldvt, nullptr, 0, O_lt, o_row0, o_cols / 8, Tq, Tk, heads, scale, stream, 1,
                           AttnL3Batch{0, 0, 0, 0, 0, format}, two_fp16_limbs);
}

/* `batch` attentions of one shape in ONE launch (grid z): entry b reads Q + b*q_bs, K + b*k_bs, Vt + b*vt_bs (element strides,
 * multiples of 4; vt_bs may be a column offset into one [heads*64][ldvt] array) and writes O + b*o_bs, or -- O_lt given, O null --
 * rows o_row0 + b*o_row_bs .. of the limb-tiled output. */
extern "C" int sculpt_attention_f32_l3_batched(const float *Q, int ldq, int64_t q_bs, const float *K, int ldk, int64_t k_bs,
                                               const float *Vt, int ldvt, int64_t vt_bs, float *O, int ldo, int64_t o_bs, void *O_lt,
                                               int format, int o_row0, int o_row_bs, int o_cols, int Tq, int Tk, int heads, int batch,
                                               float scale, int two_fp16_limbs, sculpt_stream_t stream) {
    SC_REQUIRE((O != nullptr) != (O_lt != nullptr), "attention_f32_l3_batched: exactly one of O / O_lt");
    SC_REQUIRE(!O_lt || o_cols % 32 == 0, "attention_f32_l3_batched: o_cols=%d not a multiple of 32", o_cols);
    return attention_l3_go(Q, ldq, K, ldk, Vt, ldvt, O, ldo, O_lt, o_row0, o_cols / 8, Tq, Tk, heads, scale, stream, batch,
                           AttnL3Batch{(long)q_bs, (long)k_bs, (long)vt_bs, (long)o_bs, o_row_bs, O_lt ? format : 0}, two_fp16_limbs);
}
