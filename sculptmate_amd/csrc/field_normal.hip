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
// The steps above are field_eval_fwd (csrc/field_fwd.h), the one copy every forward-mode kernel calls; the prologue and the launch
// plan are csrc/field_kernel.h's.
#include "common.h"
#include "field_fwd.h"
#include "triplane_mlp.h"

namespace sculpt {

template <int C, bool AC>
__global__ __launch_bounds__(512) void density_grad_kernel(
    const float *__restrict__ planes, int H, int W, const float *__restrict__ blob, const float *__restrict__ pts, long N,
    float radius, float span, float *__restrict__ grad, float *__restrict__ normal, float *__restrict__ density, int a0_lds) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FieldCtx c = field_prologue<C>(smem, blob, a0_lds);
    const int p = c.p, kind = p & 3;
    const bool is_value = kind == 0;
    const long ntiles = (N + 7) / 8;

    for (long tile = (long)blockIdx.x * c.nwave + c.wave; tile < ntiles; tile += (long)gridDim.x * c.nwave) {
        long n = tile * 8 + (p >> 2);
        const bool valid = n < N;
        if (!valid) n = N - 1;
        const float s =
            field_eval_fwd<C, AC>(c, planes, H, W, radius, span, a0_lds, kind, pts[3 * n], pts[3 * n + 1], pts[3 * n + 2]);
        const float d = s + c.L.blast[0];
        // the quad's three tangents into the point's lane
        const float gx = quad_bcast<1>(s), gy = quad_bcast<2>(s), gz = quad_bcast<3>(s);
        if (valid && is_value && c.h == 0) {
            if (density) density[n] = d;
            if (grad) { grad[3 * n] = gx; grad[3 * n + 1] = gy; grad[3 * n + 2] = gz; }
            if (normal) {
                float nx, ny, nz;
                unit_normal_of(gx, gy, gz, nx, ny, nz);
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
    FieldPlan plan;
    if (const int e = field_plan("triplane_density_grad", C, planes_cl, mlp_packed, H, W, n_hidden_64, radius, plan, [&] {
            SC_REQUIRE(N >= 0, "triplane_density_grad: negative point count %lld", N);
            SC_REQUIRE((flags & ~(int)SCULPT_QUERY_ALIGN_CORNERS) == 0, "triplane_density_grad: unknown flags %d", flags);
            return 0;
        }))
        return e;
    if (N == 0) return 0;   // empty arrays have no address: nothing to refuse, nothing to launch
    SC_REQUIRE(grad || normal || density, "triplane_density_grad: no output asked for (grad, normal and density are all null)");
    SC_REQUIRE(points, "triplane_density_grad: null points");
    auto kern = (flags & (int)SCULPT_QUERY_ALIGN_CORNERS) ? density_grad_kernel<40, true> : density_grad_kernel<40, false>;
    int grid;
    if (const int e = field_grid(plan, kern, ((long)N + 7) / 8, grid)) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), plan.lds, as_stream(stream), planes_cl, H, W,
                       reinterpret_cast<const float *>(mlp_packed), points, (long)N, radius, plan.span, grad, normal, density,
                       plan.a0_lds);
    SC_LAUNCH_CHECK();
    return 0;
}
