// The covered texels of a rasterised UV atlas as a list on the device, for gfx950 (MI355X): sculpt_bake_texel_list, the first
// half of the displacement bake.  The line search (sculpt_triplane_project_along,
// csrc/mesh_project.hip) then runs over the list, reads its length from device memory and scatters into the images: the host
// never learns the count, so nothing waits.
//
// Three launches, count -> scan -> emit, one texel per thread in row-major order:
//   * texel_count_kernel: the coverage of texel_position (csrc/bake_texel.h: tri in range, its three vertex rows in range) and
//     the number of covered texels of each 512-texel block (block_flag_count, csrc/block_scan.h);
//   * texel_scan_kernel: one workgroup turns the block counts into block offsets in place (block_scan_in_place) and stores the
//     total;
//   * texel_emit_kernel: the coverage again, a texel's rank inside its block (block_flag_rank) and with the block's offset its
//     row in the list.  No atomic decides a position: the list is torch.nonzero of the coverage, bit for bit and in its order.
//     Per listed texel the kernel also stores p0 (texel_position: sculpt_bake_interpolate's bits) and the direction
//     N = (N0 u + N1 v) + N2 w of the per-vertex normals at the face's corners (un-normalised, as csrc/tangent_frame.h
//     interpolates a frame; fp32 without contraction), the mask of every texel, and for a texel that is NOT covered the values
//     the line search will not write: height and residual +0, status -1, evals 0.
#include "bake_texel.h"
#include "block_scan.h"
#include "common.h"

namespace sculpt {

constexpr int TEXEL_BLOCK = 512, TEXEL_WAVES = TEXEL_BLOCK / 64;

__global__ __launch_bounds__(TEXEL_BLOCK) void texel_count_kernel(const float4 *__restrict__ rast, long N, const float *__restrict__ v_pos,
                                                                  long nv, const void *__restrict__ faces, int faces_i64, long nf,
                                                                  int *__restrict__ block_counts) {
    __shared__ unsigned s_w[TEXEL_WAVES];
    const long i = (long)blockIdx.x * TEXEL_BLOCK + threadIdx.x;
    const bool covered = i < N && texel_position(rast[i < N ? i : N - 1], v_pos, nv, faces, faces_i64, nf).covered;
    const unsigned c = block_flag_count<TEXEL_WAVES>(covered, s_w);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = (int)c;
}

__global__ __launch_bounds__(TEXEL_BLOCK) void texel_scan_kernel(int *__restrict__ block_counts, int nblocks, int *__restrict__ count) {
    __shared__ int s_w[TEXEL_WAVES];
    const int total = block_scan_in_place<TEXEL_WAVES>(block_counts, nblocks, s_w);
    if (threadIdx.x == 0) *count = total;
}

__global__ __launch_bounds__(TEXEL_BLOCK) void texel_emit_kernel(const float4 *__restrict__ rast, long N, const float *__restrict__ v_pos,
                                                                 long nv, const void *__restrict__ faces, int faces_i64, long nf,
                                                                 const float *__restrict__ normals, const int *__restrict__ block_offsets,
                                                                 int *__restrict__ list, float *__restrict__ out_p0,
                                                                 float *__restrict__ out_dir, uint8_t *__restrict__ mask,
                                                                 float *__restrict__ height, float *__restrict__ residual,
                                                                 int *__restrict__ status, int *__restrict__ evals) {
#pragma clang fp contract(off)
    __shared__ unsigned s_w[TEXEL_WAVES];
    const long i = (long)blockIdx.x * TEXEL_BLOCK + threadIdx.x;
    const bool live = i < N;
    const float4 r = rast[live ? i : N - 1];
    const Texel tx = texel_position(r, v_pos, nv, faces, faces_i64, nf);
    const bool covered = live && tx.covered;
    const unsigned rank = block_flag_rank<TEXEL_WAVES>(covered, s_w);
    if (!live) return;
    if (mask) mask[i] = covered ? 1 : 0;
    if (covered) {
        const long row = (long)block_offsets[blockIdx.x] + rank;   // < the number of covered texels <= N
        list[row] = (int)i;
        if (out_p0) out_p0[3 * row] = tx.x[0], out_p0[3 * row + 1] = tx.x[1], out_p0[3 * row + 2] = tx.x[2];
        if (out_dir) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                out_dir[3 * row + k] = (normals[3 * tx.i[0] + k] * r.x + normals[3 * tx.i[1] + k] * r.y) + normals[3 * tx.i[2] + k] * r.z;
        }
    } else {
        if (height) height[i] = 0.f;
        if (residual) residual[i] = 0.f;
        if (status) status[i] = -1;
        if (evals) evals[i] = 0;
    }
}

}  // namespace sculpt

using namespace sculpt;

extern "C" size_t sculpt_bake_texel_list_workspace_bytes(int res) {
    if (res < 1) return 0;
    return (size_t)cdiv((long)res * res, TEXEL_BLOCK) * sizeof(int);
}

extern "C" int sculpt_bake_texel_list(const float *v_pos, size_t nv, const void *faces, int faces_i64, size_t nf, const float *normals,
                                      const float *rast, int res, void *workspace, int *list, int *count, float *p0, float *directions,
                                      uint8_t *mask, float *height, float *residual, int *status, int *evals, sculpt_stream_t stream) {
    SC_REQUIRE(res >= 0 && res <= 46340, "bake_texel_list: res=%d (0 .. 46340: a texel index is an int32)", res);
    SC_REQUIRE(count, "bake_texel_list: null count");
    SC_REQUIRE(nv <= (size_t)1 << 40 && nf <= (size_t)1 << 40, "bake_texel_list: mesh too large");
    hipStream_t st = as_stream(stream);
    if (res == 0) {
        SC_HIP(hipMemsetAsync(count, 0, sizeof(int), st));
        return 0;
    }
    SC_REQUIRE(rast && list && workspace, "bake_texel_list: null rast, list or workspace");
    SC_REQUIRE(nf == 0 || (v_pos && faces && nv > 0), "bake_texel_list: null mesh");
    SC_REQUIRE(!directions || normals || nf == 0, "bake_texel_list: directions asked for without per-vertex normals");
    const long N = (long)res * res;
    const int nblocks = cdiv(N, TEXEL_BLOCK);
    int *block_counts = reinterpret_cast<int *>(workspace);
    const float4 *r4 = reinterpret_cast<const float4 *>(rast);
    hipLaunchKernelGGL(texel_count_kernel, dim3(nblocks), dim3(TEXEL_BLOCK), 0, st, r4, N, v_pos, (long)nv, faces, faces_i64, (long)nf,
                       block_counts);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(texel_scan_kernel, dim3(1), dim3(TEXEL_BLOCK), 0, st, block_counts, nblocks, count);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(texel_emit_kernel, dim3(nblocks), dim3(TEXEL_BLOCK), 0, st, r4, N, v_pos, (long)nv, faces, faces_i64, (long)nf,
                       normals, block_counts, list, p0, directions, mask, height, residual, status, evals);
    SC_LAUNCH_CHECK();
    return 0;
}
