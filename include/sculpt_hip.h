/*
 * sculpt_hip.h -- C ABI of libsculpt_hip.so, the MI355X (gfx950) implementation of the
 * TripoSR generation hot path of SculptMate.
 *
 * Every entry point replaces a piece of the reference's Python/torch hot path (file:line are
 * relative to the reference repository root):
 *
 *   sculpt_triplane_query        TriplaneNeRFRenderer.query_triplane + NeRFMLP.forward
 *                                  TripoSR/tsr/models/nerf_renderer.py:41-91
 *                                  TripoSR/tsr/models/network_utils.py:116-124
 *   sculpt_plane_features +
 *   sculpt_density_grid          TSR.extract_mesh's dense query over MarchingCubeHelper.grid_vertices
 *                                  TripoSR/tsr/system.py:171-183, TripoSR/tsr/models/isosurface.py:25-39
 *   sculpt_mc_*                  MarchingCubeHelper.forward -> skimage.measure.marching_cubes(vol, 0.0)
 *                                  TripoSR/tsr/models/isosurface.py:41-54
 *   sculpt_gemm_bf16 / sculpt_attention_bf16 / sculpt_layernorm / sculpt_groupnorm_tokens /
 *   sculpt_vit_* / sculpt_upsample_scatter
 *                                Transformer1D / BasicTransformerBlock / Attention / GEGLU,
 *                                  HF ViTModel, TriplaneUpsampleNetwork
 *                                  TripoSR/tsr/models/transformer/transformer_1d.py:179-219
 *                                  TripoSR/tsr/models/transformer/basic_transformer_block.py:149-206,291-315
 *                                  TripoSR/tsr/models/transformer/attention.py:569-653
 *                                  TripoSR/tsr/models/tokenizers/image.py:41-60
 *                                  TripoSR/tsr/models/network_utils.py:24-32
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch types.  All data pointers are DEVICE
 *     pointers (HBM) unless the parameter name ends in _host.
 *   - every function returns 0 on success, non-zero on error; the message is available from
 *     sculpt_last_error() (thread local).  Nothing is retained past the call.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Launch functions are
 *     asynchronous and graph-capturable unless stated otherwise.
 *   - there is NO CPU fallback: without a usable HIP device the launch functions fail.
 */
#ifndef SCULPT_HIP_H
#define SCULPT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: sculpt_attention_bf16 no longer takes scale == 0 for pre-scaled queries (sculpt_attention_bf16_prescaled); batched
 *    attention, host-side PLY face records; sculpt_gemm_f32 forwards to sculpt_gemm_f32_ex and takes its two preconditions
 *    (bias 16-byte aligned; without a bias at most 65 532 output columns, see there)
 * 3: the two-pass dense density grid (sculpt_density_grid_filtered, sculpt_density_filter_workspace_bytes,
 *    sculpt_density_filter_stats); added without a version change (new symbols only): sculpt_limbs_bytes, sculpt_limbs_split,
 *    sculpt_gemm_l3p, sculpt_layernorm_limbs, sculpt_attention_f32_l3_limbs, sculpt_mc_count_launch, sculpt_mc_count_read,
 *    sculpt_mc_emit_capped, sculpt_attention_f32_l3_batched, sculpt_mc_count_launch_signed,
 *    sculpt_density_filter_sign_offset
 * 4: the two-pass grid's guard: 12 statistics words instead of 8 (sculpt_density_filter_stats fills SCULPT_FILTER_STATS_WORDS),
 *    word 1 covers every re-evaluated point, the audit sample and the sign mismatches are new; the marching-cubes workspace
 *    is a record pool with a capacity (SCULPT_ERR_MC_WORKSPACE, sculpt_mc_workspace_bytes_for, sculpt_mc_count_launch_for,
 *    sculpt_mc_count_read_ex); added without a version change (new symbols only): sculpt_gemm_last_form,
 *    sculpt_attention_last_form */
#define SCULPT_ABI_VERSION 4

typedef void *sculpt_stream_t;

int sculpt_version(void);
/* sha256 (first 32 hex digits) of the HIP sources, headers and compile flags this library was built from
 * (sculptmate_amd/build.py: source_digest); "unknown" when built by hand without -DSCULPT_SOURCE_DIGEST. */
const char *sculpt_source_digest(void);
const char *sculpt_last_error(void);
/* number of visible HIP devices (0 if none); never fails */
int sculpt_device_count(void);
/* A HIP stream whose kernels run only on CUs [first_cu, first_cu + n_cus) of the current device (hipExtStreamCreateWithCUMask;
 * the driver stripes the CU numbering over the 8 XCDs, so a contiguous range takes the same share of every XCD): lets the
 * MFMA-bound density grid of image i and the latency-bound transformer of image i+1 run side by side on disjoint CUs
 * (tools/try_cumask.py).  Destroy with sculpt_stream_destroy. */
int sculpt_stream_create_cu_mask(int first_cu, int n_cus, sculpt_stream_t *stream_out);
int sculpt_stream_destroy(sculpt_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * NeRF decoder weights.  The reference MLP is Linear(3*C,64)+SiLU, NH x [Linear(64,64)+SiLU],
 * Linear(64,4)  (network_utils.py:48-79; C=40, NH=8 in TripoSR/checkpoints/config.yaml:23-28).
 * sculpt_mlp_pack re-orders the torch-layout weights (HOST pointers, W[l] is [out][in] row
 * major) into the lane order the MFMA kernels read; the caller uploads the packed blob.
 * ------------------------------------------------------------------------------------------ */
size_t sculpt_mlp_packed_bytes(int in_channels, int n_hidden_64);
int sculpt_mlp_pack(const float *const *W_host, const float *const *b_host, int n_layers,
                    const int *dims_host, void *packed_host, size_t packed_bytes);

/* query_triplane at arbitrary points.
 *   planes      f32 [3][C][H][W]   (scene code of one image, TSR.forward output layout)
 *   mlp_packed  blob from sculpt_mlp_pack (device copy); n_hidden_64 = the NH it was packed with
 *   points      f32 [N][3] in (-radius, radius)
 *   outputs (each may be NULL): density [N], features [N][3], density_act [N], color [N][3]
 *   density_act = exp(density + density_bias), color = sigmoid(features)  (nerf_renderer.py:82-87) */
int sculpt_triplane_query(const float *planes, int C, int H, int W, const void *mlp_packed,
                          int n_hidden_64, const float *points, int64_t N, float radius, float density_bias,
                          float *density, float *features, float *density_act, float *color,
                          sculpt_stream_t stream);

/* Same with sampling flags.  SCULPT_QUERY_ALIGN_CORNERS: grid_sample(align_corners=True), as
 * SF3D.query_triplane does (StableFast/sf3d/system.py:170-199) followed by one MaterialMLP head
 * (StableFast/sf3d/models/network.py:148-210) packed into the (density | features) 4-row output layer:
 * a 1-channel head in row 0 (density_act = exp(out + bias) == trunc_exp), a 3-channel head in rows 1..3
 * (color = sigmoid). */
#define SCULPT_QUERY_ALIGN_CORNERS 1u
/* SCULPT_QUERY_CHANNEL_LAST: `planes` is [3][H][W][C] (sculpt_planes_channel_last of the reference layout): one tap
 * is C contiguous floats, ~20x fewer cache lines per point than gathering from C separate channel planes. */
#define SCULPT_QUERY_CHANNEL_LAST 2u
int sculpt_planes_channel_last(const float *planes /* [3][C][H][W] */, int C, int H, int W, float *out /* [3][H][W][C] */,
                               sculpt_stream_t stream);
int sculpt_triplane_query_ex(const float *planes, int C, int H, int W, const void *mlp_packed,
                             int n_hidden_64, const float *points, int64_t N, float radius, float density_bias,
                             unsigned flags, float *density, float *features, float *density_act, float *color,
                             sculpt_stream_t stream);

/* Volume-render rays through a scene code (TriplaneNeRFRenderer._forward, nerf_renderer.py:93-152, with the box test of
 * utils.py:115-149), one launch; per sample the arithmetic of sculpt_triplane_query_ex(SCULPT_QUERY_CHANNEL_LAST).
 *   planes_cl   f32 [3][H][W][C]   (sculpt_planes_channel_last of the scene code)
 *   rays_o/d    f32 [n_rays][3]    world origins and directions (directions as the caller has them: not normalised here)
 *   t_vals      f32 [S + 1] device: torch.linspace(0, 1, S + 1), made on the host (its fp32 roundings are part of the contract)
 *   comp_rgb    f32 [n_rays][3]    sum_i w_i color_i + (1 - sum_i w_i); a ray that misses the box is white
 *   opacity     f32 [n_rays]       sum_i w_i (0 for a miss); may be NULL
 *   z_vals      f32 [n_rays][S]    sample depths, zero for a miss; may be NULL
 *   weights     f32 [n_rays][S]    w_i = alpha_i T_i, zero for a miss; may be NULL
 * A ray's result depends on that ray alone (not on n_rays, its position in the array or the launch geometry). */
int sculpt_render_rays(const float *planes_cl /* [3][H][W][C] */, int C, int H, int W,
                       const void *mlp_packed, int n_hidden_64,
                       const float *rays_o, const float *rays_d /* [n_rays][3] */, int64_t n_rays,
                       float radius, float density_bias,
                       const float *t_vals /* device, [S + 1] */, int S,
                       float *comp_rgb /* [n_rays][3] */,
                       float *opacity /* nullable [n_rays] */,
                       float *z_vals  /* nullable [n_rays][S] */,
                       float *weights /* nullable [n_rays][S] */,
                       sculpt_stream_t stream);

/* sculpt_render_rays with passes beside the colour: raw per-ray sums over the samples, with the weights w_i of the colour
 * picture, each exactly 0 for a miss.  Same arguments, same refusals; the three new outputs are nullable.
 *   depth_sum   f32 [n_rays]       sum_i w_i z_i (sequential in i, fp32, every operation rounded on its own); depth_sum / opacity
 *                                  is the expected distance along the ray, in units of |rays_d|
 *   normal_sum  f32 [n_rays][3]    sum_i w_i n_i, n_i = the `normal` of sculpt_triplane_density_grad at o + z_i d, bit for bit
 *                                  (-grad / |grad| of the raw density, 0 where the gradient is 0 or not finite); world space
 *   premul      f32 [n_rays][3]    sum_i w_i color_i: comp_rgb before the white background, comp_rgb = premul + (1 - opacity)
 * With all three NULL this is sculpt_render_rays: the same launch.  Without normal_sum, depth_sum and premul come from the
 * colour kernel's second form, at the colour kernel's price.  With normal_sum the call is one launch of the forward-mode
 * kernel (8 rays x {value, d/dx, d/dy, d/dz} per wave, about 4.5 x the colour kernel's time), which writes every output asked
 * for.  Either way comp_rgb, opacity, z_vals and weights have sculpt_render_rays' bits.  The forward-mode kernel stops
 * evaluating a tile of 8 rays once the transmittance of each is exactly 0 (every later weight is +0 for a finite field: no
 * result changes; SCULPT_RENDER_FORM=noskip walks every sample).  A ray's result depends on that ray alone. */
int sculpt_render_passes(const float *planes_cl /* [3][H][W][C] */, int C, int H, int W,
                         const void *mlp_packed, int n_hidden_64,
                         const float *rays_o, const float *rays_d /* [n_rays][3] */, int64_t n_rays,
                         float radius, float density_bias,
                         const float *t_vals /* device, [S + 1] */, int S,
                         float *comp_rgb /* [n_rays][3] */,
                         float *opacity /* nullable [n_rays] */,
                         float *z_vals  /* nullable [n_rays][S] */,
                         float *weights /* nullable [n_rays][S] */,
                         float *depth_sum  /* nullable [n_rays] */,
                         float *normal_sum /* nullable [n_rays][3] */,
                         float *premul     /* nullable [n_rays][3] */,
                         sculpt_stream_t stream);

/* Texture bake of a scene code: colour of every covered texel of a rasterised UV atlas (sculpt_bake_rasterize), one launch;
 * per covered texel the position (a*u + b*v) + c*w of sculpt_bake_interpolate (gathered through faces[tri] from the indexed
 * vertices) and the colour of sculpt_triplane_query_ex(SCULPT_QUERY_CHANNEL_LAST) at it, bit for bit; the density row of the
 * decoder is not evaluated and nothing per texel but the result is written.
 *   planes_cl   f32 [3][H][W][C]     (sculpt_planes_channel_last of the scene code)
 *   v_pos       f32 [nv][3], faces i32 or i64 [nf][3] (DEVICE)
 *   rast        f32 [res][res][4]    (u, v, w, tri) or (0, 0, 0, -1)
 *   color       f32 [res][res][3]    exactly 0 where the texel is not covered
 *   mask        u8  [res][res]       1 where covered; may be NULL
 * A texel whose tri is outside [0, nf), or whose vertex indices are outside [0, nv), counts as not covered and nothing is
 * read through such an index.  A texel's result depends on that texel alone (not on res, its place in the image or the
 * launch geometry).  res == 0 is a no-op. */
int sculpt_bake_scene_color(const float *planes_cl /* [3][H][W][C] */, int C, int H, int W,
                            const void *mlp_packed, int n_hidden_64,
                            const float *v_pos /* [nv][3] */, size_t nv,
                            const void *faces /* [nf][3] */, int faces_i64, size_t nf,
                            const float *rast /* [res][res][4] = (u, v, w, tri) or (0,0,0,-1) */, int res,
                            float radius,
                            float *color /* [res][res][3] */, uint8_t *mask /* nullable [res][res] */,
                            sculpt_stream_t stream);

/* Per-corner tangent frames of a UV-mapped triangle mesh, one thread per face, every operation rounded on its own:
 *   v_pos f32 [nv][3], faces i32 or i64 [nf][3], uvs f32 [3 nf][2] per face corner (origin bottom-left),
 *   corner_normals f32 [3 nf][3] unit normals per face corner (DEVICE)  ->  tangents f32 [3 nf][4] = (T.xyz, w)
 * Face: t = dP/du = (e1 dv2 - e2 dv1) / det, b = dP/dv = (e2 du1 - e1 du2) / det, det = du1 dv2 - du2 dv1.  Corner with normal
 * N: T = normalize(t - N (N.t)), w = +1 if cross(N, T).b >= 0, else -1 (a chart mirrored in the atlas gets -1).
 * Degenerate (det 0 or not finite, a vertex index outside [0, nv) -- nothing is read through it --, or t parallel to N):
 * T = normalize(cross(N, e_a)) with a the axis of N's smallest component in magnitude (the lowest on a tie), w = +1; (1, 0, 0, +1)
 * if N is 0 or not finite.  The order of operations is written down in csrc/bake_normal.hip.  nf == 0 is a no-op. */
int sculpt_corner_tangents(const float *v_pos /* [nv][3] */, size_t nv, const void *faces /* [nf][3] */, int faces_i64, size_t nf,
                           const float *uvs /* [3 nf][2] */, const float *corner_normals /* [3 nf][3] */,
                           float *tangents /* [3 nf][4] */, sculpt_stream_t stream);

/* Normal-map bake of a scene code: the unit normal of the density field at every covered texel of a rasterised UV atlas, one
 * launch.  Per covered texel the position of sculpt_bake_scene_color (the bits of sculpt_bake_interpolate) and the `normal` of
 * sculpt_triplane_density_grad (flags 0) at it, bit for bit: the world normal n.
 *   corner_normals, corner_tangents both NULL: object space, normal = n.
 *   both given (f32 [3 nf][3] and [3 nf][4], sculpt_corner_tangents): tangent space in the MikkTSpace / glTF convention of
 *     un-normalised interpolated frames.  With the texel's barycentrics (u, v, w) and its face's corner rows,
 *     N = (N0 u + N1 v) + N2 w, T likewise, B = s cross(N, T), s = the w of the face's first corner; the stored unit vector
 *     (x, y, z) is the one with normalize(x T + y B + z N) = n, i.e. normalize(nT gnn - nN gtn, nB, nN gtt - nT gtn) with
 *     gtt = T.T, gnn = N.N, gtn = T.N, nT = n.T, nN = n.N, nB = n.B.  The flat (0, 0, 1) is stored where gtt gnn - gtn^2 <= 0,
 *     a component is not finite or n is 0.  The order of operations is written down in csrc/bake_normal.hip.
 *   normal  f32 [res][res][3]  in [-1, 1], not encoded; exactly +0 where the texel is not covered
 *   mask    u8  [res][res]     1 where covered; may be NULL
 * Index guard and independence as for sculpt_bake_scene_color: a texel whose tri or vertex indices are out of range counts as
 * not covered, and a texel's result depends on that texel alone.  res == 0 is a no-op. */
int sculpt_bake_scene_normal(const float *planes_cl /* [3][H][W][C] */, int C, int H, int W,
                             const void *mlp_packed, int n_hidden_64,
                             const float *v_pos /* [nv][3] */, size_t nv,
                             const void *faces /* [nf][3] */, int faces_i64, size_t nf,
                             const float *rast /* [res][res][4] = (u, v, w, tri) or (0,0,0,-1) */, int res,
                             float radius,
                             const float *corner_normals /* nullable [3 nf][3] */, const float *corner_tangents /* nullable [3 nf][4] */,
                             float *normal /* [res][res][3] */, uint8_t *mask /* nullable [res][res] */,
                             sculpt_stream_t stream);

/* Gradient of the raw density (the decoder's output 0, before bias and exp) with respect to the query point, in world units,
 * and the outward unit normal of the density's iso-surface through the point: forward-mode differentiation of
 * sculpt_triplane_query_ex(SCULPT_QUERY_CHANNEL_LAST), one launch, 8 points x {value, d/dx, d/dy, d/dz} per MFMA tile.
 *   planes_cl   f32 [3][H][W][C]   (sculpt_planes_channel_last of the scene code)
 *   points      f32 [N][3]
 *   flags       0 or SCULPT_QUERY_ALIGN_CORNERS
 *   grad        f32 [N][3]   d density / d p; floor's one-sided derivative where a pixel coordinate is an integer (torch
 *                            autograd's); exactly 0 for a point outside all three planes
 *   normal      f32 [N][3]   -grad / |grad| (the density grows inwards); exactly (0,0,0) where |grad| is 0 or not finite
 *   density     f32 [N]      the `density` of sculpt_triplane_query_ex at the point, bit for bit
 * Each output may be NULL, not all three.  A point's result depends on that point alone (not on N, its place in the array or
 * the launch geometry).  Refused: C != 40, N < 0, unknown flags, all outputs NULL (with N > 0).  N == 0 is a no-op. */
int sculpt_triplane_density_grad(const float *planes_cl /* [3][H][W][C] */, int C, int H, int W,
                                 const void *mlp_packed, int n_hidden_64,
                                 const float *points /* [N][3] */, long long N, float radius, int flags /* QUERY_ALIGN_CORNERS */,
                                 float *grad /* [N][3] or null */, float *normal /* [N][3] or null */, float *density /* [N] or null */,
                                 sculpt_stream_t stream);

/* Dense density grid over the lattice slab ix in [x_begin,x_end), flat order ix*R*R + iy*R + iz
 * (isosurface.py:34-37), in two launches:
 *
 * 1. sculpt_plane_features: the lattice is separable, and the first MLP layer is linear in the three
 *    bilinear plane samples, so it is evaluated once per lattice PAIR and plane:
 *      FA[ix][iy] = W0[:, 0:C]   . sample(plane0; x=ix, y=iy) + b0
 *      FB[ix][iz] = W0[:, C:2C]  . sample(plane1; x=ix, z=iz)
 *      FC[iy][iz] = W0[:, 2C:3C] . sample(plane2; y=iy, z=iz)      (nerf_renderer.py:57-68)
 *    axis_coords[R]: coordinate in (-radius,radius) of lattice index i, computed by the host exactly
 *    as the reference does (linspace(0,1,R) then scale_tensor, isosurface.py:28-32, system.py:177-181).
 *    workspace: sculpt_density_grid_workspace_bytes(R, x_end-x_begin) bytes, holds FA|FB|FC.
 * 2. sculpt_density_grid: per point silu(FA+FB+FC) -> hidden layers (fp32 MFMA) -> density row of the
 *    last layer -> out = exp(density + density_bias) + out_add, f32 [(x_end-x_begin)*R*R].
 *    out_add = -threshold gives the volume the reference hands to marching cubes
 *    (system.py:184 + isosurface.py:45).
 * Linearity only regroups the fp32 sum of layer 0 (see DESIGN.md "fused sample+MLP kernel"). */
size_t sculpt_density_grid_workspace_bytes(int R, int nx);
int sculpt_plane_features(const float *planes, int C, int H, int W, const void *mlp_packed,
                          const float *axis_coords, int R, int x_begin, int x_end, float radius,
                          void *workspace, sculpt_stream_t stream);
/* The same tables with flags: SCULPT_QUERY_ALIGN_CORNERS = grid_sample(align_corners=True), SF3D's query (sf3d/system.py:185-195). */
int sculpt_plane_features_ex(const float *planes, int C, int H, int W, const void *mlp_packed,
                             const float *axis_coords, int R, int x_begin, int x_end, float radius, unsigned flags,
                             void *workspace, sculpt_stream_t stream);
int sculpt_density_grid(const void *mlp_packed, int n_hidden_64, int R, int x_begin, int x_end,
                        float density_bias, float out_add, const void *workspace, float *out,
                        sculpt_stream_t stream);
/* Same with flags (values 1 and 2 were the two-limb experiments SCULPT_DENSITY_BF16X3 / _FP16X3 of rounds 2-5: removed, refused).
 * SCULPT_DENSITY_BF16L3: fp32-equivalent mode on the 16-bit matrix pipe (what TSR.extract_meshes uses by default): both
 * operands split EXACTLY into three bf16 limbs (8 + 8 + 8 = 24 significant bits, fp32 exponent range),
 * W.x = W1.x3 + W3.x1 + W2.x2 + W1.x2 + W2.x1 + W1.x1 with every product exact and fp32 accumulation; the three dropped
 * products are below 2^-23 |W||x|.  No range limit, no fallback.  Replaces NeRFMLP's hidden Linear layers,
 * TripoSR/tsr/models/network_utils.py:116-124, inside nerf_renderer.py:82-87. */
#define SCULPT_DENSITY_BF16L3 4u
int sculpt_density_grid_ex(const void *mlp_packed, int n_hidden_64, int R, int x_begin, int x_end,
                           float density_bias, float out_add, const void *workspace, float *out, unsigned flags,
                           sculpt_stream_t stream);
/* The dense grid for marching cubes, filtered (csrc/density_filter.hip): marching cubes (isosurface.py:41-54) reads the magnitude
 * of the volume only at the end points of sign-changing lattice edges and at all corners of the cells whose sign pattern is
 * ambiguous (Lewiner's face / interior tests, centre vertex), and the sign everywhere else, so
 *   pass A evaluates every lattice point with ONE 16-bit product per hidden layer (bf16 operands, or IEEE half with
 *          SCULPT_FILTER_COARSE_FP16; fp32 accumulate) and marks the points with |log(density_act) - log(level)| < margin
 *          (level = -out_add > 0) or a non-finite coarse value,
 *   pass B re-evaluates the marked points with the SCULPT_DENSITY_BF16L3 arithmetic (bit for bit the values
 *          sculpt_density_grid_ex gives there): after it the sign of every lattice point is certain,
 *   pass C lists, from the signs, the values marching cubes reads (minus the marked points) and re-evaluates those.
 * out then holds the exact value wherever marching cubes reads one and a value of the right sign elsewhere, i.e. marching cubes
 * gives the mesh of the full evaluation bit for bit, PROVIDED no coarse error |log d~ - log d| reaches `margin`.  The caller
 * calibrates the margin: SCULPT_FILTER_MARK_ALL marks every point (margin and level unused), so that stats[1] is the largest
 * coarse error over the lattice.  At run time the call reports what it saw of the coarse error (the guard; the caller decides):
 * stats[1] the largest over ALL re-evaluated points, +inf when an UNMARKED point came out on the other side of the level than
 * the coarse pass had it (stats[10] counts those: each proves an error >= margin) or an exact value is a NaN; stats[8] the
 * largest over an audit sample of ~0.5 % of the points nothing else re-evaluates (unmarked, value not read by marching cubes;
 * pseudo-random, fixed per (R, x_begin, x_end)), appended to pass C.  A wrong sign that no mismatch reveals needs a whole
 * 6-connected component of the true inside or outside mis-signed at every one of its points (csrc/density_filter.hip).
 * flags must contain SCULPT_DENSITY_BF16L3; n_hidden_64 >= 1; R <= 1024.
 * filter_workspace: sculpt_density_filter_workspace_bytes(R, x_end - x_begin) bytes; its first SCULPT_FILTER_STATS_WORDS words are
 *   [0] points re-evaluated  [1] float bits of the largest coarse error seen (see above)  [2] points marked in pass A
 *   [3] non-finite coarse values (all marked)  [4] active cells  [5] lattice points  [6] list entries of pass B  [7] of pass C
 *   [8] float bits of the largest coarse error over the audit sample (+inf: an audited sign was wrong)  [9] audit points
 *   [10] unmarked points whose coarse sign was wrong  [11] marked points whose coarse sign pass B corrected
 * valid once the stream has passed this call (sculpt_density_filter_stats copies them to the host and waits). */
#define SCULPT_FILTER_STATS_WORDS 12
#define SCULPT_FILTER_COARSE_FP16 8u
#define SCULPT_FILTER_MARK_ALL 16u
/* run only the named passes (timing the passes one by one: A, then B, then C on the same filter_workspace); none = all three */
#define SCULPT_FILTER_PASS_A 32u
#define SCULPT_FILTER_PASS_B 64u
#define SCULPT_FILTER_PASS_C 128u
size_t sculpt_density_filter_workspace_bytes(int R, int nx);
int sculpt_density_grid_filtered(const void *mlp_packed, int n_hidden_64, int R, int x_begin, int x_end, float density_bias,
                                 float out_add, float margin, const void *workspace, void *filter_workspace, float *out,
                                 unsigned flags, sculpt_stream_t stream);
/* byte offset of the sign planes (uint32 [nx * R][ceil(R / 32)], bit = value > 0 of the final volume) inside the filter workspace */
size_t sculpt_density_filter_sign_offset(int R, int nx);
int sculpt_density_filter_stats(const void *filter_workspace, int32_t *stats /* host, SCULPT_FILTER_STATS_WORDS */, sculpt_stream_t stream);
/* Step 2 for a decoder head with a 3-channel output (SF3D's MaterialMLP heads evaluated on the marching-tetrahedra lattice,
 * sf3d/system.py:141-168 + network.py:148-210): density_act (nullable) = exp(row 0 + density_bias) + out_add as above,
 * features (nullable) f32 [(x_end-x_begin)*R*R][3] = rows 1..3 of the last layer, raw.  Exact-fp32 kernel only. */
int sculpt_grid_decode(const void *mlp_packed, int n_hidden_64, int R, int x_begin, int x_end, float density_bias,
                       float out_add, const void *workspace, float *density_act, float *features, sculpt_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Marching cubes (Lewiner), output identical to skimage.measure.marching_cubes(vol, level)
 * with default arguments, including vertex and face ORDER.
 *   vol f32 [n0][n1][n2] C order.  Two phases: count (waits for the counts, returns sizes),
 *   then emit into caller-allocated buffers.
 *   flags: SCULPT_MC_REFERENCE_ORDER  faces columns reordered [1,0,2] and stored as int64,
 *          verts multiplied by vert_scale (isosurface.py:52-53) then mapped v*a + b
 *          (scale_tensor, system.py:185-189) when SCULPT_MC_AFFINE is set.
 * Errors: SCULPT_ERR_MC_LEVEL (level outside data range -> skimage ValueError),
 *         SCULPT_ERR_MC_EMPTY (no surface -> skimage RuntimeError).
 * ------------------------------------------------------------------------------------------ */
#define SCULPT_MC_FACES_I64 1u
#define SCULPT_MC_REFERENCE_ORDER 2u
#define SCULPT_MC_USE_CLASSIC 4u
/* slab mode (512^3 split along axis 0): SLAB = do not fail on an empty slab;
 * SLAB_HALO_LOW = lattice plane 0 is the previous slab's last plane: its x/y-edge vertices are owned
 * there, faces reference them as -(1 + axis*n1*n2 + i1*n2 + i2) and are resolved after the gather
 * through the previous slab's top_plane_map (int32 [2][n1][n2], -1 = no vertex). */
#define SCULPT_MC_SLAB 8u
#define SCULPT_MC_SLAB_HALO_LOW 16u
/* sculpt_mc_count_launch_signed / sculpt_mc_count_read after it: the count phase took its "value > level" bits from caller-supplied
 * planes; no data range is collected -- an empty surface comes back as SCULPT_ERR_MC_EMPTY whether or not the level lies inside the
 * range (call sculpt_mc_count to tell skimage's two errors apart), minmax is (+FLT_MAX, -FLT_MAX) */
#define SCULPT_MC_SIGNED 32u
#define SCULPT_ERR_MC_LEVEL 11
#define SCULPT_ERR_MC_EMPTY 12
#define SCULPT_ERR_MC_NAN 13 /* the volume contains NaN (e.g. a 16-bit split density mode left its range) */
#define SCULPT_ERR_MC_WORKSPACE 14 /* more active cells than the workspace's pool is named for: repeat once with that many (below) */
#define SCULPT_ERR_MC_NO_COUNT 15 /* sculpt_mc_count_read: no count launch is pending for this workspace (see there) */

/* Workspace: per-row arrays + a record pool of 8 bytes per ACTIVE cell (a cell whose corner signs differ).
 * A pool is NAMED for a capacity of c records: max_active_cells of sculpt_mc_workspace_bytes_for / sculpt_mc_count_launch_for
 * (<= 0: the default, one active cell per 8 cells, at least 65 536; a closed surface at 256^3 has ~1 per 17), clamped to the
 * number of cells.  It occupies at most 2c records (up to 64 unevenly loaded parts of c records in all + a spill run of c).
 * sculpt_mc_workspace_bytes is the default: 39 MB at 256^3, 315 MB at 512^3.
 * Guarantee: a count phase with at most c active cells never runs out of pool -- in every count form (any level, classic
 * tables, sign planes, slab flags) and whatever the surface's spread.  A count phase with more active cells than that may run
 * out; it still returns the right totals, with SCULPT_ERR_MC_WORKSPACE and -- through sculpt_mc_count_read_ex -- the number of
 * active cells n.  The caller allocates sculpt_mc_workspace_bytes_for(.., n) and repeats the count ONCE with
 * sculpt_mc_count_launch_for(.., max_active_cells = n, ..): that count succeeds.  The error text names n and c (as
 * "rec_capacity" of the workspace).  (The emit phase after an overflow writes nothing.) */
size_t sculpt_mc_workspace_bytes(int n0, int n1, int n2);
size_t sculpt_mc_workspace_bytes_for(int n0, int n1, int n2, int64_t max_active_cells);
int sculpt_mc_count(const float *vol, int n0, int n1, int n2, double level, unsigned flags,
                    void *workspace, int64_t *n_verts_host, int64_t *n_faces_host,
                    float *minmax_host /* [2] data min,max or NULL */, sculpt_stream_t stream);
int sculpt_mc_emit(const float *vol, int n0, int n1, int n2, double level, unsigned flags,
                   void *workspace, float vert_div, float vert_mul, float vert_add,
                   int axis0_offset /* slab: global index of lattice plane 0 */,
                   float *verts, void *faces, int *top_plane_map /* or NULL */, sculpt_stream_t stream);
/* The same two phases without the host round trip between them (the stream otherwise idles while the host reads the counts,
 * allocates and launches: ~50 us of a 0.28 ms stage at 256^3):
 *   sculpt_mc_count_launch  the count phase, launched only: the totals stay in the workspace header;
 *   sculpt_mc_emit_capped   the emit phase into buffers of cap_verts vertices / cap_faces faces sized by the CALLER'S ESTIMATE
 *                           (e.g. the previous mesh + 25 %); the kernels read the totals on the device and write NOTHING when the
 *                           mesh does not fit either buffer;
 *   sculpt_mc_count_read    waits for the COUNTS and returns the totals with sculpt_mc_count's error semantics: when they exceed
 *                           the capacities the caller allocates exactly and calls sculpt_mc_emit.
 * sculpt_mc_count == launch + read + a stream synchronise; sculpt_mc_emit == emit_capped with unbounded capacities.
 * How the counts reach the host.  Every count launch (all sculpt_mc_count_launch* forms) queues, behind its last kernel, a copy of
 * the 64-byte header into a pinned host slot of the library and records an event; sculpt_mc_count_read / _read_ex wait for that
 * event (not for the stream) and read the slot.  The contract:
 *   - after sculpt_mc_count_read returns, the counts are final, and so is everything queued on the stream BEFORE the count launch
 *     (e.g. an asynchronous copy of sculpt_density_grid_filtered's statistics);
 *   - work queued on the stream AFTER the count launch -- sculpt_mc_emit_capped included -- may still be running: the caller's
 *     vertex and face buffers are ordered by the stream, as after any asynchronous launch;
 *   - a slot belongs to the (device, workspace pointer) of its launch until it is read: one read per launch.  A read without a
 *     pending launch for that workspace (never launched, read already) fails at once with SCULPT_ERR_MC_NO_COUNT; it never blocks;
 *   - a second count launch on the same workspace before the read REPLACES the pending one (the read returns the second's counts);
 *   - at most 8 count launches may be pending per device; a ninth takes the slot of the oldest, whose read then fails as above;
 *   - launch and read are made with the same current device; the `stream` argument of the read functions is unused (kept for
 *     the ABI);
 *   - the count launches are not graph-capturable (they record an event for the host).
 * The slots and events are created on first use and reused (no allocation on the warm path); calls may come from several host
 * threads (one mutex, never held across the wait). */
int sculpt_mc_count_launch(const float *vol, int n0, int n1, int n2, double level, unsigned flags, void *workspace,
                           sculpt_stream_t stream);
/* The count phase when the caller already holds the planes "vol > level" of the whole lattice -- sign_planes[(i0 * n1 + i1) *
 * words_per_row + i2 / 32] bit i2 % 32, bits past n2 zero: what sculpt_density_grid_filtered leaves in its workspace
 * (sculpt_density_filter_sign_offset) for level 0 -- : bricks of cells without a sign change never read the volume (most of it),
 * the others read their rows as before.  Same records, counts, vertices and faces as sculpt_mc_count_launch; pass
 * flags | SCULPT_MC_SIGNED to sculpt_mc_count_read.  Not for slab mode. */
int sculpt_mc_count_launch_signed(const float *vol, const uint32_t *sign_planes, int words_per_row, int n0, int n1, int n2,
                                  double level, unsigned flags, void *workspace, sculpt_stream_t stream);
int sculpt_mc_count_read(int n0, int n1, int n2, double level, unsigned flags, const void *workspace, int64_t *n_verts_host,
                         int64_t *n_faces_host, float *minmax_host /* [2] or NULL */, sculpt_stream_t stream);
/* The count phase into a workspace of sculpt_mc_workspace_bytes_for(n0, n1, n2, max_active_cells) bytes: sign_planes NULL (then
 * words_per_row is ignored) = sculpt_mc_count_launch, non-NULL with SCULPT_MC_SIGNED in flags = sculpt_mc_count_launch_signed.
 * sculpt_mc_count_read_ex: sculpt_mc_count_read + the number of active cells (what a SCULPT_ERR_MC_WORKSPACE caller asks for). */
int sculpt_mc_count_launch_for(const float *vol, const uint32_t *sign_planes /* or NULL */, int words_per_row, int n0, int n1, int n2,
                               double level, unsigned flags, int64_t max_active_cells, void *workspace, sculpt_stream_t stream);
int sculpt_mc_count_read_ex(int n0, int n1, int n2, double level, unsigned flags, const void *workspace, int64_t *n_verts_host,
                            int64_t *n_faces_host, float *minmax_host /* [2] or NULL */, int64_t *n_active_host /* or NULL */,
                            sculpt_stream_t stream);
int sculpt_mc_emit_capped(const float *vol, int n0, int n1, int n2, double level, unsigned flags, void *workspace, float vert_div,
                          float vert_mul, float vert_add, int axis0_offset, float *verts, int64_t cap_verts, void *faces,
                          int64_t cap_faces, int *top_plane_map /* or NULL */, sculpt_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Surface nets: the all-quad dual of marching cubes (csrc/surface_nets.hip; added without a version change: new symbols only).
 * One vertex INSIDE every cell the surface passes through, one quad across every sign-changing lattice edge whose four cells exist.
 * The rule, which tests/_snref.py restates in NumPy and the kernels meet bit for bit:
 *   vol      f32 [n0][n1][n2] C order on the device, every n >= 2, at most 2^30 points and n0 * n1 * ceil(n2 / 32) < 2^27 (1024^3
 *            fits; any other shape is refused with a message); level a double.
 *   inside   inside(p) = vol[p] > levelf, levelf the largest float <= level (marching cubes' predicate); a NaN is outside.
 *            sign_planes (or NULL): the caller's planes of that predicate -- sign_planes[(i0 * n1 + i1) * words_per_row + i2 / 32]
 *            bit i2 % 32, what sculpt_density_grid_filtered leaves behind for level 0; bits past n2 are ignored.  With them the
 *            count phase never reads the volume; the emit phase reads it at the corners of active cells only, where its sign
 *            must be the planes'.
 *   cells    cell (i0, i1, i2), 0 <= i_c <= n_c - 2, has the 8 points i + {0,1}^3; it is ACTIVE when its corners are neither all
 *            inside nor all outside.  One vertex per active cell, numbered in lexicographic order of (i0, i1, i2), i0 slowest.
 *   vertex   in fp64 from the fp32 values, no contraction, in this order: walk the cell's 12 edges -- the four along axis 0,
 *            then axis 1, then axis 2; within an axis the offsets on the two other axes go (0,0), (0,1), (1,0), (1,1), the lower
 *            axis first.  An edge with low corner offset lo (0 on its own axis), end values a (low) and b (high) and inside(a)
 *            != inside(b):  t = (level - a) / (b - a), a t that is not finite is 0.5;  s_c = s_c + (lo_c + (c == axis ? t : 0));
 *            n = n + 1.  Then p_c = i_c + s_c / n, rounded once to fp32: the LATTICE-UNIT position.  The returned vertex is
 *            marching cubes' map of it in fp32: o = p / vert_div, then rounded(o * vert_mul) + vert_add.
 *   quads    a lattice edge along axis a with low end p, p_a <= n_a - 2; u = (a + 1) % 3, v = (a + 2) % 3.  It is ELIGIBLE when
 *            inside differs at its ends and 1 <= p_u <= n_u - 2 and 1 <= p_v <= n_v - 2 (its four cells exist: a sign change on
 *            the box's boundary gives no quad, the surface is open there as marching cubes' is).  With c(du, dv) the vertex of
 *            the cell whose low corner is p + du e_u + dv e_v, the quad is [c(-1,-1), c(0,-1), c(0,0), c(-1,0)] when p is
 *            inside and that list reversed when p is outside: counter-clockwise seen from outside when inside is positive.
 *            Quads are ordered by the key (linear index of p) * 3 + a.
 *   faces    faces[2q], faces[2q + 1] split quad q = [q0, q1, q2, q3] along its shorter diagonal: d02, d13 = the fp64 squared
 *            lengths ((dx dx + dy dy) + dz dz) from the fp32 lattice-unit positions; d13 < d02: (q0,q1,q3), (q1,q2,q3),
 *            otherwise (q0,q1,q2), (q0,q2,q3).
 * A cell with an ambiguous sign pattern still gets ONE vertex: on a noisy field the mesh has non-manifold edges.
 * Two phases.  sculpt_surface_nets_count queues the masks and scans, copies the two totals into a pinned slot behind an event
 * (the way of sculpt_mc_count_launch / _read: it waits for that event only, never for the stream; not graph-capturable) and
 * returns them; no active cell: SCULPT_ERR_SN_EMPTY.  n_verts > 0 with n_quads == 0 is a valid result (a 2x2x2 volume).
 * sculpt_surface_nets_emit writes verts f32 [n_verts][3], quads [n_quads][4] (or NULL: not wanted) and faces [2 n_quads][3] (or
 * NULL) of int32, or of int64 under SCULPT_SN_INDEX_I64, into the caller's buffers; same vol, shape, level and workspace as
 * the count, which must not have been touched in between.  No atomics anywhere: ids are popcounts over bit masks plus scanned
 * prefixes, so the result does not depend on scheduling.
 * The workspace is DETERMINISTIC: sculpt_surface_nets_workspace_bytes is a function of the shape alone (bit masks -- six words per
 * 32 points -- plus two words per 8192 points; 12.6 MB at 256^3; 0 for a shape that is refused), 16-byte aligned.  There is no
 * record pool and no overflow protocol.
 * ------------------------------------------------------------------------------------------ */
#define SCULPT_SN_INDEX_I64 1u
#define SCULPT_ERR_SN_EMPTY 17 /* no cell has corners on both sides of the level */
size_t sculpt_surface_nets_workspace_bytes(int n0, int n1, int n2);
int sculpt_surface_nets_count(const float *vol, const uint32_t *sign_planes /* or NULL */, int words_per_row, int n0, int n1, int n2,
                              double level, unsigned flags, void *workspace, int64_t *n_verts_host, int64_t *n_quads_host,
                              sculpt_stream_t stream);
int sculpt_surface_nets_emit(const float *vol, int n0, int n1, int n2, double level, unsigned flags, void *workspace, float vert_div,
                             float vert_mul, float vert_add, float *verts, void *quads /* or NULL */, void *faces /* or NULL */,
                             sculpt_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Connected components of an indexed triangle mesh, and the mesh without its small ones (csrc/mesh_components.hip).
 *   faces   int32 or int64 (faces_i64 != 0) [n_faces][3], on the device, over n_vertices SHARED vertices (what sculpt_mc_emit
 *           writes): two faces are connected when they name a common vertex.  0 <= n_vertices, n_faces < 2^31.
 *   labels  labels[v] = the smallest vertex index of v's component: exact, and the same whatever the order of the faces or of
 *           the threads.  A vertex no face names is a component of its own with 0 faces.  A face with repeated indices connects
 *           less and still counts.  A face with an index outside [0, n_vertices) is never read through: the result is refused
 *           (SCULPT_ERR_MESH_COMPONENTS).  Every loop of the kernels has a step budget that cannot run out while the
 *           union-find's invariant (parent[x] <= x) holds; should one run out, the same error comes back instead of a spin.
 *   rule    which components sculpt_mesh_components_compact keeps:
 *           SCULPT_CC_KEEP_NONE       none asked for (labels and counts only: sculpt_mesh_components_report)
 *           SCULPT_CC_KEEP_LARGEST    the one with the most faces; of several with as many, the one with the smallest root
 *           SCULPT_CC_KEEP_MIN_FACES  those with at least min_faces (>= 1) faces
 *           SCULPT_CC_KEEP_FRACTION   those with (double)faces >= fraction * (double)largest face count, 0 < fraction < 1
 *           A component without faces is never kept.
 * Two phases, like marching cubes, with the counts' way to the host of sculpt_mc_count_launch / _read (a pinned slot and an event
 * per launch, keyed by the workspace pointer, at most 8 pending per device, not graph-capturable; the contract stated there):
 *   sculpt_mesh_components_launch   label + count + select + the scans' totals, queued on `stream`.  Refuses n_faces == 0 or
 *                                   n_vertices == 0: there is nothing to launch, the caller returns the empty result.
 *   sculpt_mesh_components_read     waits for the launch's event; counts_host[5] = {components, faces of the largest, root of
 *                                   the largest, kept vertices, kept faces} (the last two are 0 under SCULPT_CC_KEEP_NONE).
 *   sculpt_mesh_components_compact  the kept vertex rows and faces in their input order (the input with rows deleted), the faces
 *                                   re-indexed and in the input's integer type; vertex_index[i] / face_index[j] = the input row
 *                                   of output row i / j.  cap_vertices / cap_faces: rows of the output buffers (the counts read
 *                                   above); a row beyond them is not written.  vertices: f32 [n_vertices][3].
 *   sculpt_mesh_components_report   labels (or NULL) [n_vertices]; every root ascending [n_components], with the faces and the
 *                                   vertices of its component.
 *   sculpt_mesh_component_labels    label only, into the caller's array, and wait for the error word (synchronous).
 * The workspace (sculpt_mesh_components_workspace_bytes; 0 for sizes out of range) is 16 bytes per vertex + 4 bytes per 1024
 * vertices (twice) and per 1024 faces + under 2 KB of header and alignment; launch, compact and report of one mesh take the same one, untouched in between.
 * ------------------------------------------------------------------------------------------ */
#define SCULPT_CC_KEEP_NONE 0
#define SCULPT_CC_KEEP_LARGEST 1
#define SCULPT_CC_KEEP_MIN_FACES 2
#define SCULPT_CC_KEEP_FRACTION 3
#define SCULPT_ERR_MESH_COMPONENTS 16 /* an index out of range, a step budget spent, or a read without a pending launch */
size_t sculpt_mesh_components_workspace_bytes(int64_t n_vertices, int64_t n_faces);
int sculpt_mesh_components_launch(const void *faces, int faces_i64, int64_t n_faces, int64_t n_vertices, int rule, int64_t min_faces,
                                  double fraction, void *workspace, sculpt_stream_t stream);
int sculpt_mesh_components_read(const void *workspace, int64_t *counts_host /* [5] */);
int sculpt_mesh_components_compact(const float *vertices, const void *faces, int faces_i64, int64_t n_faces, int64_t n_vertices,
                                   void *workspace, float *out_vertices, int64_t cap_vertices, void *out_faces, int64_t cap_faces,
                                   int64_t *vertex_index, int64_t *face_index, sculpt_stream_t stream);
int sculpt_mesh_components_report(const void *workspace, int64_t n_vertices, int64_t n_faces, int64_t n_components,
                                  int32_t *labels /* or NULL */, int32_t *roots, int32_t *face_counts, int32_t *vertex_counts,
                                  sculpt_stream_t stream);
int sculpt_mesh_component_labels(const void *faces, int faces_i64, int64_t n_faces, int64_t n_vertices, int32_t *labels,
                                 void *workspace, sculpt_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Transformer primitives (bf16 storage, fp32 accumulate).  bf16 values are uint16_t bit patterns.
 * ------------------------------------------------------------------------------------------ */
#define SCULPT_EPI_NONE 0
#define SCULPT_EPI_GELU 1   /* out = gelu_erf(acc + bias) */
#define SCULPT_EPI_GEGLU 2  /* W holds [2*N][K]: out[:, n] = (acc_n + b_n) * gelu_erf(acc_{N+n} + b_{N+n}) */
#define SCULPT_EPI_RELU 3   /* out = max(acc + bias, 0)  (SF3D PixelShuffleUpsampleNetwork convs) */

/* out[M][N] = epi(A[M][K] . W[N][K]^T + bias[N]) (+ residual[M][N], fp32)
 *   A, W bf16 (K contiguous); bias fp32 or NULL; residual fp32 [M][ldr] or NULL;
 *   outputs (any subset, at least one): out_f32 [M][ldo] fp32, out_bf16 [M][ldo] bf16,
 *   out_bf16_t [N][ldt] bf16 = the transposed result (used to hand V^T to the attention kernel).
 *   n_split (0 or N = off): columns n < n_split go to out_f32/out_bf16 only, columns n >= n_split go to
 *   out_bf16_t only, at row n - n_split (one launch for a fused [Q|K|V] projection: Q,K token-major, V^T).
 *   lda/ldw/ldo/ldt are row strides in elements.  K % 64 == 0; N % 128 == 0 (GEGLU: W has 2N rows,
 *   N % 64 == 0); any M >= 1 (ragged last tile handled). */
int sculpt_gemm_bf16(const uint16_t *A, int lda, const uint16_t *W, int ldw, const float *bias,
                     const float *residual, int ldr, float *out_f32, uint16_t *out_bf16, int ldo,
                     uint16_t *out_bf16_t, int ldt, int n_split, int M, int N, int K, int epilogue,
                     sculpt_stream_t stream);
/* Same with n_store: only output columns n < n_store are written (N stays a multiple of 128, i.e. W and bias are padded;
 * n_store % 4 == 0): lets a layer with few output channels write straight into a narrow slice of a wider activation
 * buffer (`out` pointing at the slice's first column, ldo = the buffer's row stride). */
int sculpt_gemm_bf16_ex(const uint16_t *A, int lda, const uint16_t *W, int ldw, const float *bias,
                        const float *residual, int ldr, float *out_f32, uint16_t *out_bf16, int ldo,
                        uint16_t *out_bf16_t, int ldt, int n_split, int n_store, int M, int N, int K, int epilogue,
                        sculpt_stream_t stream);

/* The same GEMM with a LayerNorm folded in (nn.LayerNorm in front of every Linear of the two transformers:
 * basic_transformer_block.py:98,114,132 / HF ViT layernorm_before, layernorm_after).
 *   Producer side (ln->stats_out): besides out_f32 (and its bf16 copy out_bf16) the launch writes, per row, the (mean, M2 =
 *     sum of squared deviations) of every 64-column slice of the fp32 result: stats_out [N/64][stats_ld][2].
 *   Consumer side (ln->stats_in): A holds those UN-normalised rows x in bf16, W = W0 * diag(gamma) (gamma folded in),
 *     bias = bias0 + W0 . beta, colsum[n] = sum_k W[n][k]; the slice statistics are combined per row (parallel-variance
 *     formula) into (mean, rstd) and   out[m][n] = epi(rstd[m] * (acc[m][n] - mean[m] * colsum[n]) + bias[n])
 *     == epi(LayerNorm(x)[m] . W0[n] + bias0[n]) -- no LayerNorm launch, no normalised copy of x in HBM. */
typedef struct sculpt_ln_fold {
    const float *stats_in; /* [slots_in][stats_ld][2] (slice-major: the rows of one slice are contiguous) or NULL */
    int slots_in;          /* K / 64 */
    const float *colsum;   /* [N] (GEGLU: [2N]) */
    float eps;
    float *stats_out;      /* [N/64][stats_ld][2] or NULL */
    int stats_ld;          /* rows per slice plane of stats_in / stats_out, >= M */
    int rows_per_image;    /* 0, or the rows of ONE image when A stacks the token rows of several (a batched pass): the tile form
                            * is then the one a single image takes (on a taller grid), so that every output and statistic is
                            * accumulated in the single-image order -- the batched pass gives each image the bits of its own pass.
                            * The statistics pointers may all be NULL when only this hint is wanted.  (ABI 4) */
} sculpt_ln_fold_t;
int sculpt_gemm_bf16_ln(const uint16_t *A, int lda, const uint16_t *W, int ldw, const float *bias,
                        const float *residual, int ldr, float *out_f32, uint16_t *out_bf16, int ldo,
                        uint16_t *out_bf16_t, int ldt, int n_split, int n_store, int M, int N, int K, int epilogue,
                        const sculpt_ln_fold_t *ln /* or NULL */, sculpt_stream_t stream);
/* Which tile form the calling thread's last sculpt_gemm_bf16* / sculpt_conv3x3_bf16 launch took, e.g.
 *   "g128 epi=0 bw=64 nw=8 bm=192 ks=1 res=0 conv=0 gm=0 nmaj=0 stage=0 grid=16x16"   ("none" before the first launch)
 * g128 / g256: the kernel family (gemm_bf16_kernel / gemm256_kernel); epi: SCULPT_EPI_*; bw / bm: weight / activation rows per
 * workgroup; nw: waves; ks: k-split pairs; res: the residual form of the 256 family; conv: implicit 3x3 convolution; gm: rows of
 * the grouped tile order (0 = band order); nmaj: weight-tile-major bands; stage: staged bf16 stores; grid: workgroups x, y.
 * The launchers only fill a thread-local struct of ints; the text is formatted here, into a thread-local buffer that the next
 * call on the same thread overwrites.  For tests of the dispatch rules and for A/B tools; never fails. */
const char *sculpt_gemm_last_form(void);
/* Which kernel the calling thread's last sculpt_attention_bf16* launch started, e.g.
 *   "attn kernel=pipe nqb=6 pre=1 batch=3 grid=16x48"   ("none" before the first launch)
 * kernel: plain (attention_kernel) / pipe (attention_pipe_kernel); nqb: 32-query blocks per workgroup (4 / 6 / 8); pre: pre-scaled
 * queries; batch: entries of the launch; grid: workgroups x, y.  Filled and formatted like sculpt_gemm_last_form; never fails. */
const char *sculpt_attention_last_form(void);
/* (mean, M2) of every 64-column slice of x [rows][cols] fp32 -> stats [cols/64][stats_ld][2], and the bf16 copy of x: the
 * producer side of the fold for rows that do not come out of a GEMM (the ViT's embedding output). cols % 64 == 0. */
int sculpt_row_slice_stats(const float *x, int ldx, int rows, int cols, float *stats, int stats_ld, uint16_t *x_bf16, int ldb,
                           sculpt_stream_t stream);

/* fp32 "parity mode" of the same stack (exact-fp32 MFMA, ~5x slower; not timed by bench.py):
 *   out[m][n] = epi(alpha * A[m][:].W[n][:] + bias[n]) (+ residual); A, W, out fp32; K % 16 == 0; N % 4 == 0
 *   (w_rows = valid rows of W when N is padded; 0 = N); n_split / out_t as in sculpt_gemm_bf16.
 *   Preconditions since ABI 2 (both entries; a violation is refused with an error, never computed wrongly):
 *     - bias, when given, is 16-byte aligned (the epilogue reads it as float4; a view at a 4- or 8-byte offset must be copied);
 *     - without a bias the per-column vector comes from a 256 KiB zero page: N (2 N with the GEGLU epilogue) + 4 <= 65 536. */
int sculpt_gemm_f32(const float *A, int lda, const float *W, int ldw, const float *bias, const float *residual, int ldr,
                    float *out, int ldo, float *out_t, int ldt, int n_split, int w_rows, int M, int N, int K,
                    float alpha, int epilogue, sculpt_stream_t stream);
/* The same GEMM with a choice of arithmetic and a batch dimension (grid z):
 *   arithmetic SCULPT_F32_EXACT  = v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain (sculpt_gemm_f32);
 *              SCULPT_F32_BF16L3 = fp32 arithmetic on the bf16 matrix pipe: A and W are split EXACTLY into three bf16 limbs each
 *                                  while staged (x = x1 + x2 + x3, 24 significant bits, fp32 exponent range), the six limb products
 *                                  of order >= 2^-16 are exact in fp32 and accumulate in fp32 (csrc/gemm_l3.hip); K % 32 == 0.
 *                                  What TSR(precision="bf16l3") runs its Linears and per-head attention products on: the
 *                                  reference's fp32 Linears (TripoSR/tsr/models/transformer/attention.py:569-653,
 *                                  basic_transformer_block.py:291-315) to fp32 rounding.
 *   batch > 1: entry z reads A + z*a_bs, W + z*w_bs and writes out / out_t (+ reads residual) + z*o_bs (element strides,
 *              multiples of 4): the heads of one attention as ONE launch. */
#define SCULPT_F32_EXACT 0
#define SCULPT_F32_BF16L3 1
int sculpt_gemm_f32_ex(const float *A, int lda, const float *W, int ldw, const float *bias, const float *residual, int ldr,
                       float *out, int ldo, float *out_t, int ldt, int n_split, int w_rows, int M, int N, int K, float alpha,
                       int epilogue, int arithmetic, int batch, int64_t a_bs, int64_t w_bs, int64_t o_bs, sculpt_stream_t stream);
/* Fused attention of the fast parity mode: O = softmax(Q K^T * scale) V per head (head dim 64), fp32 in and out, both products
 * with three-limb bf16 operands and fp32 accumulation (SCULPT_F32_BF16L3 arithmetic), the softmax in fp32 registers
 * (csrc/attention_l3.hip; attention.py:629-631 in the reference's own fp32).  Q [Tq][ldq], K [Tk][ldk] with head h at columns
 * 64 h ..; Vt [heads*64][ldvt] = V transposed, ldvt >= round_up(Tk, 64), columns >= Tk finite; O [Tq][ldo]. */
int sculpt_attention_f32_l3(const float *Q, int ldq, const float *K, int ldk, const float *Vt, int ldvt, float *O, int ldo, int Tq,
                            int Tk, int heads, float scale, sculpt_stream_t stream);
/* "Limbs once" form of the SCULPT_F32_BF16L3 arithmetic (csrc/gemm_l3p.hip): the split of an fp32 value into 16-bit limbs is done
 * ONCE -- weights at load time, activations by the kernel that produces them -- instead of by every column tile of every launch.
 * A limb-tiled matrix X [R][K] (K % 32 == 0) with NL limbs per element is ceil(R / 32) * K * 64 * NL bytes (sculpt_limbs_bytes),
 * 16-byte aligned:
 *     byte offset of limb l (0 = leading) of X[r][k] = (((r / 32) * (K / 8) + k / 8) * NL + l) * 512 + (r % 32) * 16 + (k % 8) * 2
 * (32-row blocks x 8-k chunks x limb: one matrix-instruction fragment = 512 contiguous bytes, a 16-k step of a row block = NL KiB that
 * the GEMM copies into LDS by DMA).  Rows >= R of the last block: zeros from sculpt_limbs_split, unspecified from other producers
 * (they reach only outputs that are never stored).  Formats:
 *   SCULPT_LIMBS_BF16X3  three bf16 limbs, x = x1 + x2 + x3 exactly (24 significant bits, fp32 exponent range); six limb products per
 *                        multiply: the same products in the same order as sculpt_gemm_f32_ex(SCULPT_F32_BF16L3) -- bit-identical.
 *   SCULPT_LIMBS_F16X2   two fp16 limbs: 22 significant bits for |x| >= 2^-3, an absolute error <= 2^-25 below, |x| < 65504 (larger
 *                        values become inf and the result non-finite: the caller checks); three limb products per multiply, each
 *                        exact in fp32 -- half the matrix work.  A weight is stored times a power of two `scale` that puts its largest
 *                        magnitude in [2^14, 2^15) (sculpt_limbs_split's scale; exact) and the GEMM takes alpha = 1 / scale.
 *   sculpt_limbs_split: scale * fp32 [rows][K] (row stride ld, multiple of 4; src and dst 16-byte aligned) -> limb-tiled.
 *   sculpt_gemm_l3p:    out[m][n] = epi(alpha * A[m][:].W[n][:] + bias[n]) (+ residual), A [M][K] and W [N][K] limb-tiled in `format`.
 *                       N % 128 == 0 (GEGLU: N % 64 == 0 and W stored as 32-row blocks in the order value n..n+31, gate n..n+31,
 *                       value n+32.., gate n+32.. per 64 output columns).  Outputs: out / out_t / n_split / residual as
 *                       sculpt_gemm_f32, OR out_lt: the result itself as a limb-tiled [M][N] matrix in out_format (what the next
 *                       Linear reads; excludes the others).
 *   sculpt_layernorm_limbs:        sculpt_layernorm on fp32 rows with the normalised rows written limb-tiled ([rows][cols]; y_f32
 *                                  optional: the same rows in fp32 as well).
 *   sculpt_attention_f32_l3_limbs: sculpt_attention_f32_l3 with O written limb-tiled: query q of this call is row o_row0 + q of a
 *                                  limb-tiled matrix of o_cols (>= heads * 64, multiple of 32) columns, head h at columns 64 h .. */
#define SCULPT_LIMBS_BF16X3 0
#define SCULPT_LIMBS_F16X2 1
size_t sculpt_limbs_bytes(int rows, int K, int format);
int sculpt_layernorm_limbs(const float *x, int ldx, const float *gamma, const float *beta, float eps, void *y_lt, int format,
                           float *y_f32, int ldy, int rows, int cols, sculpt_stream_t stream);
int sculpt_attention_f32_l3_limbs(const float *Q, int ldq, const float *K, int ldk, const float *Vt, int ldvt, void *O_lt, int format,
                                  int o_row0, int o_cols, int Tq, int Tk, int heads, float scale, int two_fp16_limbs,
                                  sculpt_stream_t stream);
/* `batch` fused three-limb attentions of one shape in ONE launch (TSR.forward on a list of images in the tolerance mode): entry b
 * reads Q + b*q_bs, K + b*k_bs, Vt + b*vt_bs (element strides, multiples of 4; vt_bs may be a column offset into one
 * [heads*64][ldvt] array) and writes O + b*o_bs -- or, with O null and O_lt given, rows o_row0 + b*o_row_bs .. of the limb-tiled
 * output of o_cols columns in `format`.
 * two_fp16_limbs != 0 (both entries): both products on TWO fp16 limbs per operand (22 bits; csrc/attention_l2.hip) instead of three
 * bf16 limbs where the pipelined 256-query form runs (the small launches keep three limbs): half the matrix work, the arithmetic
 * of TSR(precision="fp16l2"); the operands of an attention -- scaled queries, keys, values, probabilities -- are O(1). */
int sculpt_attention_f32_l3_batched(const float *Q, int ldq, int64_t q_bs, const float *K, int ldk, int64_t k_bs, const float *Vt,
                                    int ldvt, int64_t vt_bs, float *O, int ldo, int64_t o_bs, void *O_lt, int format, int o_row0,
                                    int o_row_bs, int o_cols, int Tq, int Tk, int heads, int batch, float scale, int two_fp16_limbs,
                                    sculpt_stream_t stream);
int sculpt_limbs_split(const float *src, int ld, int rows, int K, float scale, int format, void *dst, sculpt_stream_t stream);
int sculpt_gemm_l3p(const void *A_lt, const void *W_lt, int format, float alpha, const float *bias, const float *residual, int ldr,
                    float *out, int ldo, float *out_t, int ldt, int n_split, void *out_lt, int out_format, int M, int N, int K,
                    int epilogue, sculpt_stream_t stream);
/* in-place softmax over the first `cols` columns of each row; columns [cols, pad_cols) are set to 0 */
int sculpt_softmax_rows_f32(float *x, int ld, int rows, int cols, int pad_cols, sculpt_stream_t stream);

/* softmax(Q K^T * scale) V per head, no mask (attention.py:629-631; HF ViTSelfAttention).
 *   Q [Tq][ldq], K [Tk][ldk] bf16 with head h at columns h*64 .. h*64+63;
 *   Vt [heads*64][ldvt] bf16 = V transposed (row = h*64 + d, column = key); ldvt >= round_up(Tk, 64)
 *   and the columns >= Tk must hold finite values (they are multiplied by exact zeros);
 *   O [Tq][ldo] bf16.  Head dim is 64.
 *   scale must be positive.  Row extents must stay below 2 GiB (round_up(Tk,128) * ldk * 2 B and 64 * ldvt * 2 B): the K / V
 *   tiles are fetched with 32-bit buffer offsets. */
int sculpt_attention_bf16(const uint16_t *Q, int ldq, const uint16_t *K, int ldk, const uint16_t *Vt,
                          int ldvt, uint16_t *O, int ldo, int Tq, int Tk, int heads, float scale,
                          sculpt_stream_t stream);
/* The same with queries that ALREADY carry softmax_scale * log2(e) (folded into the query projection before its bf16
 * rounding): O = softmax_2(Q K^T) V with 2^x in place of e^x; the kernel subtracts the running maximum inside the matrix
 * product and skips one VALU multiply-add per score (1.1-1.2x faster).  What the bf16 transformers use. */
int sculpt_attention_bf16_prescaled(const uint16_t *Q, int ldq, const uint16_t *K, int ldk, const uint16_t *Vt,
                                    int ldvt, uint16_t *O, int ldo, int Tq, int Tk, int heads, sculpt_stream_t stream);

/* `batch` independent attentions of the same shape in ONE launch (TSR.forward on a batch of images,
 * TripoSR/tsr/system.py:82-115: batch_size = rgb_cond.shape[0]; attention.py:629-631 with a leading batch dimension).
 * Entry b reads Q + b*q_bs, K + b*k_bs, Vt + b*vt_bs and writes O + b*o_bs (strides in ELEMENTS, multiples of 8; o_bs of 4):
 * token rows of the entries stacked below each other, V^T either side by side in one [heads*64][ldvt] array (vt_bs = a column
 * offset, (batch-1)*vt_bs + round_up(Tk,64) <= ldvt) or one array per entry (vt_bs >= heads*64*ldvt).  prescaled != 0: queries
 * carry softmax_scale * log2(e) (scale ignored), as sculpt_attention_bf16_prescaled; otherwise scale must be positive. */
int sculpt_attention_bf16_batched(const uint16_t *Q, int ldq, int64_t q_bs, const uint16_t *K, int ldk, int64_t k_bs,
                                  const uint16_t *Vt, int ldvt, int64_t vt_bs, uint16_t *O, int ldo, int64_t o_bs, int Tq, int Tk,
                                  int heads, int batch, int prescaled, float scale, sculpt_stream_t stream);

/* y = LayerNorm(x) * gamma + beta over the last dim (rows x cols), x fp32 or bf16, y bf16 */
int sculpt_layernorm(const float *x_f32, const uint16_t *x_bf16, int ldx, const float *gamma,
                     const float *beta, float eps, uint16_t *y, int ldy, float *y_f32, int rows, int cols,
                     sculpt_stream_t stream);

/* GroupNorm over x [C][T] fp32 (groups of C/G channels x T tokens, transformer_1d.py:183) written
 * transposed as tokens y [T][C] bf16 */
int sculpt_groupnorm_tokens(const float *x, int C, int T, int G, const float *gamma, const float *beta,
                            float eps, uint16_t *y, float *y_f32 /* either output may be NULL */,
                            float *stats_ws /* 2*G floats scratch */, sculpt_stream_t stream);

/* out[c][t] = x[t][c] + residual[c][t]  (proj_out permute + residual, transformer_1d.py:211-217) */
int sculpt_transpose_add(const float *x_tc, const float *residual_ct, float *out_ct, int T, int C,
                         sculpt_stream_t stream);

/* ImagePreprocessor resize (tsr/utils.py:82-88): F.interpolate(bilinear, align_corners=False, antialias=True)
 * on an HWC fp32 image; tmp = Hin*Wout*C floats of scratch. */
int sculpt_resize_aa_bilinear(const float *in_hwc, int Hin, int Win, int C, float *tmp, float *out_hwc, int Hout,
                              int Wout, sculpt_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The image front end on the device (preprocessing.preprocess_image_device; the host path it restates: preprocessing.py:73-127,
 * rembg/bg.py:149-238, rembg/sessions/base.py:44-69, rembg/sessions/u2net.py:34-44).  Images are tightly packed uint8 [H][W][C]
 * with sides in [1, 32768].  EXACTNESS: every entry point below is integer arithmetic or IEEE operations rounded one by one (the
 * file is compiled without floating-point contraction), and gives the bytes / floats the host library gives -- Pillow's
 * Image.resize(LANCZOS) and Image.composite, numpy's float64 / float32 expressions -- bit for bit.  Added without a version
 * change (new symbols only).
 *
 * Pillow's 8-bit LANCZOS resample is separable.  The tables of one axis, inSize -> outSize, are computed on the HOST (double
 * arithmetic and libm's sin, the very function the host library calls; no device memory is touched, no GPU is needed):
 *   sculpt_resample_lanczos_ksize   taps per output index, (int)ceil(3 max(inSize / outSize, 1)) * 2 + 1; 0 for sizes out of range
 *   sculpt_resample_lanczos_coeffs  bounds_host int32 [outSize][2] = (first input index, taps used), kk_host int32 [outSize][ksize]
 *                                   = the weights in 2^-22 units, rounded half away from zero, zero past the taps used
 * sculpt_resample_u8 takes them as DEVICE arrays: the horizontal pass first (into tmp, uint8 [Hin][Wout][C]), then the vertical
 * one; each is acc = 2^21 + sum pixel * k in int32, out = clamp(acc >> 22, 0, 255).  A pass whose size does not change is skipped
 * and its tables may be NULL (tmp is needed only when both run); C is 1, 3 or 4 and every channel is treated alike (no alpha
 * premultiplication: what Pillow does for L and RGB, not for RGBA). */
int sculpt_resample_lanczos_ksize(int in_size, int out_size);
int sculpt_resample_lanczos_coeffs(int in_size, int out_size, int ksize, int32_t *bounds_host, int32_t *kk_host);
int sculpt_resample_u8(const uint8_t *in_hwc, int Hin, int Win, int C, const int32_t *bounds_x, const int32_t *kk_x, int ksize_x,
                       const int32_t *bounds_y, const int32_t *kk_y, int ksize_y, uint8_t *tmp, uint8_t *out_hwc, int Hout, int Wout,
                       sculpt_stream_t stream);
/* U^2-Net's input from the resized picture (C = 3 or 4; a fourth channel is ignored): out_chw fp32 [3][H][W] =
 * (float)(((double)v / max - mean[c]) / std[c]) with max the maximum over the three channels of the whole image, taken on the device;
 * three fp64 operations and one rounding to fp32, as numpy evaluates normalize().  ws: 4 int32 of device scratch. */
int sculpt_u2net_input(const uint8_t *img_hwc, int H, int W, int C, const double *mean3_host, const double *std3_host, int32_t *ws,
                       float *out_chw, sculpt_stream_t stream);
/* The 8-bit mask of the network's output d0 (fp32, n elements): mask = (uint8)(((d - mi) / (ma - mi)) * 255) with mi, ma the
 * minimum and maximum of d0 taken on the device, every fp32 operation rounded on its own, truncating conversion.  ma == mi (a
 * constant d0) gives 0 everywhere -- the host's result there is numpy's undefined cast of NaN.  ws: 4 uint32 of device scratch. */
int sculpt_u2net_mask(const float *d0, int64_t n, uint32_t *ws, uint8_t *mask, sculpt_stream_t stream);
/* The cut-out Image.composite(img, transparent, mask) is, per byte, md255(v, M) = (t = v * M + 128, ((t >> 8) + t) >> 8), with
 * alpha 255 for C = 3.  sculpt_cutout_bbox: bbox_host[4] = (ymin, ymax, xmin, xmax), both ends INCLUSIVE, of the pixels whose
 * cut-out alpha md255(A, M) is non-zero; (H, -1, W, -1) when there is none.  img_hwc may be NULL for C = 3.  This is the front
 * end's only readback: the four integers (ws: 4 int32 of device scratch) are copied into a pinned slot of the library behind the
 * kernel, an event is recorded behind the copy, and the call waits for that event -- not for the stream -- as
 * sculpt_mc_count_read does.  Not graph-capturable; calls may come from several host threads. */
int sculpt_cutout_bbox(const uint8_t *img_hwc, const uint8_t *mask, int H, int W, int C, int32_t *ws, int32_t *bbox_host,
                       sculpt_stream_t stream);
/* Cut-out, frame and grey composite as one gather: out [S][S][grey ? 3 : 4]; pixel (oy, ox) is the cut-out's pixel
 * (y0 + oy - top, x0 + ox - left) where that lies in the box [y0, y0 + h) x [x0, x0 + w), transparent black elsewhere.
 * grey = 0: RGBA.  grey != 0: x = v / 255, a = alpha / 255, rgb = x * a + (1 - a) * 0.5, out = (uint8)(rgb * 255) in fp32, every
 * operation rounded on its own and no fused multiply-add (preprocessing.py:112-116). */
int sculpt_cutout_frame(const uint8_t *img_hwc, const uint8_t *mask, int H, int W, int C, int y0, int x0, int h, int w, int top,
                        int left, int S, int grey, uint8_t *out, sculpt_stream_t stream);
/* out = (float)v / 255, a rounded fp32 division: what ImagePreprocessor's conversion gives for a uint8 image */
int sculpt_u8_to_unit_f32(const uint8_t *in, int64_t n, float *out, sculpt_stream_t stream);

/* ViT front end (tokenizers/image.py:48 + HF ViTEmbeddings; DINOv2: sf3d/models/tokenizers/image.py:86 +
 * dinov2.py:176-210): normalise (x-mean)/std and cut the [S][S][3] fp32 image into patch rows
 * [floor(S/P)^2][ld] (the stride-P patch convolution as a GEMM; trailing S - floor(S/P)*P pixels ignored like the
 * convolution does); columns 3*P*P..ld-1 are written as zero (K padding; ld <= 0 means 3*P*P) */
int sculpt_vit_patchify(const float *image_hwc, int S, int P, const float *mean3_host, const float *std3_host,
                        uint16_t *patches, float *patches_f32 /* either may be NULL */, int ld, sculpt_stream_t stream);
/* tokens[0] = cls + pos[0]; tokens[1+i] = patch_out[i] + pos[1+i]  (fp32 residual stream) */
int sculpt_vit_assemble(const float *patch_out, const float *cls, const float *pos, float *tokens,
                        int n_patches, int hidden, sculpt_stream_t stream);
/* sculpt_vit_assemble and sculpt_row_slice_stats of its n_patches + 1 rows in one launch: tokens [rows][ldt] fp32, their bf16 copy
 * [rows][ldb] (may be NULL) and stats [hidden/64][stats_ld][2] -- the same bits as the two calls. hidden % 64 == 0; every array
 * 16-byte aligned. */
int sculpt_vit_assemble_stats(const float *patch_out, const float *cls, const float *pos, float *tokens, int ldt, int n_patches,
                              int hidden, float *stats, int stats_ld, uint16_t *tokens_bf16, int ldb, sculpt_stream_t stream);

/* ConvTranspose2d(k=2,s=2) epilogue: g [3*S*S][ldg] fp32 (GEMM output, column = co*4 + dy*2 + dx)
 * + bias[Co] -> planes [3][Co][2S][2S]  (network_utils.py:20-32) */
int sculpt_upsample_scatter(const float *g, int ldg, const float *bias, float *planes, int S, int Co,
                            sculpt_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * UV-space texture baker (StableFast "next" row).  Replaces the exports of
 * StableFast/sf3d/texture_baker/texture_baker.dll (ABI declared at baker.py:31-57, 91-118; semantics
 * restated in common.py:104-142, 214-229): pixel (x,y) samples (x/res, 1 - y/res); rast = (u,v,w,tri) or
 * (0,0,0,-1); where several triangles cover a sample the LOWEST index wins.
 * ------------------------------------------------------------------------------------------ */
size_t sculpt_bake_workspace_bytes(int res);
/* uv f32 [nv][2], idx i32 [nf][3] (DEVICE), out f32 [res][res][4] */
int sculpt_bake_rasterize(const float *uv, size_t nv, const int *idx, size_t nf, int res, void *workspace,
                          float *out, sculpt_stream_t stream);
/* attr f32 [nv][3], rast f32 [res][res][4] (DEVICE) -> out f32 [res][res][3] */
int sculpt_bake_interpolate(const float *attr, size_t nv, const int *idx, size_t nf, const float *rast, int res,
                            float *out, sculpt_stream_t stream);
/* The DLL's own entry points (HOST pointers, same names/signatures as baker.py declares): */
void rasterize_cpu(const float *uv, size_t nv, const int *idx, size_t nf, long long res, float *out);
void interpolate_cpu(const float *attr, size_t nv, const int *idx, size_t nf, const float *rast, long long res,
                     float *out);

/* StableFast-3D networks (BASELINE config 4).
 *
 * PixelShuffleUpsampleNetwork (StableFast/sf3d/models/network.py:29-75): each 3x3/pad-1 Conv2d is
 *   sculpt_im2col3x3 (channel-last activations [n][S*S][C] -> rows [n*S*S][9*C], k = (ky*3+kx)*C + c,
 *   elements of 2 (bf16) or 4 (f32) bytes) followed by sculpt_gemm_bf16 with W reordered to [Cout][ky][kx][Cin]
 *   (SCULPT_EPI_RELU for all but the last); sculpt_pixel_shuffle = nn.PixelShuffle(r) of the last GEMM's fp32
 *   output [n*S*S][ldg] (column co*r*r + dy*r + dx) into planes [n][Co][S*r][S*r]. */
int sculpt_im2col3x3(const void *in, int n_planes, int S, int C, int elem_bytes, void *out, sculpt_stream_t stream);
int sculpt_pixel_shuffle(const float *g, int ldg, float *planes, int n_planes, int S, int Co, int r,
                         sculpt_stream_t stream);

/* F.normalize(x, dim=-1, p=2, eps) on n rows of 3 (the "normalize_channel_last" head activation, network.py:129-130;
 * may run in place).  A finite row whose squared norm overflows fp32 (|x| >= 2^64) is still normalised to unit length, as the
 * operation defines it (an fp32 evaluation of the formula would divide by inf and return 0). */
int sculpt_normalize_rows3(const float *x, int64_t n, float eps, float *y, sculpt_stream_t stream);

/* Texture bake, material composition per texel (StableFast/sf3d/system.py:375-440): all inputs are [res*res][3]
 * texel images except rast [res*res][4] (texels with rast[..][3] < 0 are outside every chart and stay 0):
 * albedo = color; bump = clamp(0.5*(pn.t, pn.b, clip(pn.n, 0.3, 1)) + 0.5, 0, 1) with n, t the normalised interpolated
 * normal / tangent, b = normalize(cross(t, n)), pn = normalize(perturb_normal).  bump may be NULL (albedo only). */
int sculpt_bake_material(const float *rast, int res, const float *color, const float *perturb_normal, const float *nrm,
                         const float *tng, float *albedo, float *bump, sculpt_stream_t stream);

/* Stand-in UV layout (NOT the reference's box-projection atlas, which ends in uv_unwrapper.dll): triangle f is drawn
 * isometrically inside cell (f % cols, f / cols) of a cols x rows grid with relative padding; uv f32 [3*nf][2] in
 * face-corner order (what Mesh.unwrap_uv's `uv[indices]` produces, mesh.py:236-262). */
int sculpt_uv_cell_atlas(const float *v_pos, const void *faces, int faces_i64, int64_t nf, int cols, int rows, float padding,
                         float *uv, sculpt_stream_t stream);

/* MarchingTetrahedraHelper (StableFast/sf3d/models/isosurface.py:108-229).
 *   sculpt_mtet_deform: out = grid_vertices + scale * tanh(offsets), scale = (1-0)/resolution (:108-115, 211-216).
 *   Static per-grid tables (host, once): tets i32 [Nt][4]; edges i32 [Ne][2] = the lexicographically sorted unique
 *   undirected edges (a < b) of the grid (== the reference's all_edges, :117-131); tet_edges i32 [Nt][6] = edge
 *   id of each tet's edges in base_tet_edges order (0-1, 0-2, 0-3, 1-2, 1-3, 2-3; :64-69).
 *   sculpt_mtet_count: scans -> number of vertices (sign-changing edges, sdf > 0 is "inside", :143) and faces; keeps
 *   offsets in `workspace` (sculpt_mtet_workspace_bytes).  sculpt_mtet_emit: vertices f32 [Nv][3] =
 *   (pos_a * (-s_b/(s_a-s_b)) + pos_b * (s_a/(s_a-s_b))) * vert_mul + vert_add in the reference's vertex order
 *   (crossing edges sorted), faces i64 [Nf][3] in the reference's order (one-triangle tets, then two-triangle tets).
 *   Bit-identical to the reference given the same pos/sdf. */
int sculpt_mtet_deform(const float *grid_vertices, const float *offsets, int64_t n_vertices, float scale, float *out,
                       sculpt_stream_t stream);
size_t sculpt_mtet_workspace_bytes(int64_t n_edges, int64_t n_tets);
int sculpt_mtet_count(const float *sdf, const int32_t *tets, int64_t n_tets, const int32_t *edges, int64_t n_edges,
                      void *workspace, int64_t *n_verts_host, int64_t *n_faces_host, sculpt_stream_t stream);
int sculpt_mtet_emit(const float *pos, const float *sdf, const int32_t *tets, int64_t n_tets, const int32_t *edges,
                     int64_t n_edges, const int32_t *tet_edges, void *workspace, float vert_mul, float vert_add,
                     float *verts, int64_t *faces, sculpt_stream_t stream);

/* Channel-last bf16 conv-net building blocks (U^2-Net background removal; the reference runs it
 * as an opaque ONNX graph: rembg/sessions/u2net.py:16-46).  Activations are [H*W][ld] bf16, `in`/`out` point at the first
 * channel of a slice, C = real channels (multiple of 8).
 *   sculpt_im2col3x3_dilated: rows [H*W][9*C_pad], k = (ky*3+kx)*C_pad + c, taps at (y+(ky-1)*d, x+(kx-1)*d), zero outside
 *     the image and for c >= C -- followed by sculpt_gemm_bf16_ex = Conv2d(3x3, padding=d, dilation=d) (+ folded
 *     BatchNorm, ReLU epilogue).
 *   sculpt_maxpool2x2_ceil = nn.MaxPool2d(2, stride=2, ceil_mode=True); sculpt_upsample_bilinear_* =
 *     F.interpolate(mode="bilinear", align_corners=False) to (H, W); sculpt_add_bf16 = elementwise sum of two slices;
 *   sculpt_fuse_sigmoid: out[i] = sigmoid(sum_k w[k]*maps[k][i] + bias) (the 1x1 fusion of the six side outputs). */
int sculpt_im2col3x3_dilated(const uint16_t *in, int ld_in, int H, int W, int C, int C_pad, int dilation, uint16_t *out,
                             sculpt_stream_t stream);
/* The same convolution WITHOUT materialising the im2col rows (implicit GEMM): the activation tile of K-step
 * (tap, 64-channel chunk) is fetched by LDS-DMA straight from the shifted pixels of the channel-last input (a zero page for
 * taps outside the image).  in: [n_images][H*W][ld_in] with at least C_pad readable channels from `in` in every pixel row
 * (channels beyond the real ones must be finite; their weights are zero); Wt bf16 [N][9*C_pad], k = (ky*3+kx)*C_pad + c;
 * outputs as sculpt_gemm_bf16_ex (fp32 and/or bf16, row stride ldo, columns < n_store); epilogue NONE or RELU. */
int sculpt_conv3x3_bf16(const uint16_t *in, int ld_in, int n_images, int H, int W, int C_pad, int dilation,
                        const uint16_t *Wt, const float *bias, float *out_f32, uint16_t *out_bf16, int ldo, int n_store,
                        int N, int epilogue, sculpt_stream_t stream);
int sculpt_maxpool2x2_ceil(const uint16_t *in, int ld_in, int H, int W, int C, uint16_t *out, int ld_out, sculpt_stream_t stream);
int sculpt_upsample_bilinear_bf16(const uint16_t *in, int ld_in, int h, int w, int C, uint16_t *out, int ld_out, int H, int W,
                                  sculpt_stream_t stream);
int sculpt_upsample_bilinear_f32(const float *in, int ld_in, int h, int w, float *out, int H, int W, sculpt_stream_t stream);
int sculpt_add_bf16(const uint16_t *a, int lda, const uint16_t *b, int ldb, uint16_t *out, int ldo, int64_t rows, int C,
                    sculpt_stream_t stream);
int sculpt_fuse_sigmoid(const float *maps, int n_maps, int64_t n, const float *w, float bias, float *out, sculpt_stream_t stream);

/* StableFast-3D estimators (SURVEY.md 8b "SF3D boundary": run_image returns roughness / metallic):
 *   sculpt_resize_bilinear_hwc: F.interpolate(bilinear, align_corners=False, no antialias) of an fp32 [Hin][Win][C] image,
 *     each source pixel first multiplied by mul_hw[Hin][Win] when given -- ClipBasedHeadEstimator's input
 *     rgb_cond * mask_cond resized to 224 (sf3d/system.py:326-329, image_estimator/clip_based_estimator.py:95-100);
 *   sculpt_im2col3x3_strided: rows of a 3x3 / padding 0 / stride s convolution over n_groups channel-last maps
 *     [n_groups][S*S][C] treated as ONE image with n_groups*C channels (channel = g*C + c, the reshape at
 *     global_estimator/multi_head_estimator.py:90-94): out [So*So][9*n_groups*C], k = (ky*3+kx)*n_groups*C + g*C + c,
 *     So = (S-3)/s + 1; elements of 2 (bf16) or 4 (f32) bytes, C*elem_bytes a multiple of 16;
 *   sculpt_col_reduce_f32: out[c] = max (mean = 0) or mean (mean != 0) over the rows of x [rows][ld]
 *     (x.amax / x.mean over the pixels, multi_head_estimator.py:96-101); as amax, a column holding a NaN gives NaN and an
 *     all -inf column gives -inf; rows >= 1 (an empty reduction is refused). */
int sculpt_resize_bilinear_hwc(const float *in_hwc, const float *mul_hw /* may be NULL */, int Hin, int Win, int C, float *out_hwc,
                               int Hout, int Wout, sculpt_stream_t stream);
int sculpt_im2col3x3_strided(const void *in, int n_groups, int S, int C, int elem_bytes, int stride, void *out, sculpt_stream_t stream);
int sculpt_col_reduce_f32(const float *x, int ld, int rows, int cols, int mean, float *out, sculpt_stream_t stream);

/* Box-projection UV unwrapping (StableFast/sf3d/uv_unwrapper/unwrap.py:625-697), one entry point per
 * stage; the host side (sculptmate_amd/sf3d/unwrap.py) mirrors Unwrapper.forward.  `stats`: device scratch of
 * sculpt_uv_stats_words() 32-bit words, initialised by sculpt_uv_box_project and carried through the later stages of the
 * same mesh.  faces: int32 or int64 [nf][3] (faces_i64).
 *   sculpt_uv_moments         sums9 (device doubles) = sum of x, y, z, xx, xy, xz, yy, yz, zz over the vertices: the statistics
 *                             behind _align_mesh_with_main_axis (:546-623; exact principal axes instead of the reference's
 *                             randomised torch.pca_lowrank); workspace: sculpt_uv_moments_workspace_bytes() device bytes,
 *                             the sums are added in a fixed order (reproducible to the bit)
 *   sculpt_uv_box_project     rot_pos / rot_nrm = rot (row-major 3x3, host) applied to every vertex; face_uv [nf][3][2] and
 *                             chart [nf] in 0..5 = _box_assign_vertex_to_cube_face (:16-122)
 *   sculpt_uv_chart_tangents  vertex_tangents4 [nv][4] (xyz = _calculate_tangents, :239-305, w = corner count); sums42 (device
 *                             doubles) [6][7] = per chart the sum over its corners of the vertex tangent (3), of the expected
 *                             tangent (3; with the reference's F.normalize(x, -1) scaling, :326-341) and the corner count;
 *                             workspace: sculpt_uv_chart_tangents_workspace_bytes(nv) device bytes.  Reproducible to the bit:
 *                             fixed-point vertex sums, chart sums added in a fixed order
 *   sculpt_uv_rotate_charts   face_uv rotated per chart by the angle (cos, sin given per chart) about the chart centre and
 *                             stretched to [0, 1] by the chart's joint min / max (:357-381), in place
 *   sculpt_uv_assign_atlas    assigned [nf]: chart c stays c, moves to the overlap slice c + 6, or to 12 ("remaining") -- the
 *                             contract of assign_faces_uv_to_atlas_index in uv_unwrapper.dll (:124-175), own algorithm
 *                             (UV-space z-buffer of res x res pixels per chart, zbuf = 6*res*res uint64 scratch)
 *   sculpt_uv_place           out_uv [nf][3][2] atlas coordinates (:177-237, 383-527); block_scratch: ceil(nf/256) ints */
size_t sculpt_uv_stats_words(void);
size_t sculpt_uv_moments_workspace_bytes(void);
int sculpt_uv_moments(const float *v_pos, size_t nv, double *sums9, void *workspace, sculpt_stream_t stream);
int sculpt_uv_box_project(const float *v_pos, const float *v_nrm, size_t nv, const void *faces, int faces_i64, size_t nf,
                          const float *rot9_host, float *rot_pos, float *rot_nrm, float *face_uv, int *chart, unsigned *stats,
                          sculpt_stream_t stream);
size_t sculpt_uv_chart_tangents_workspace_bytes(size_t nv);
int sculpt_uv_chart_tangents(const float *rot_pos, const float *rot_nrm, size_t nv, const void *faces, int faces_i64, size_t nf,
                             const float *face_uv, const int *chart, float *vertex_tangents4, double *sums42, void *workspace,
                             sculpt_stream_t stream);
int sculpt_uv_rotate_charts(float *face_uv, const int *chart, size_t nf, const float *cos6_host, const float *sin6_host, unsigned *stats,
                            sculpt_stream_t stream);
int sculpt_uv_assign_atlas(const float *rot_pos, const void *faces, int faces_i64, size_t nf, const float *face_uv, const int *chart,
                           int res, unsigned long long *zbuf, int *assigned, sculpt_stream_t stream);
int sculpt_uv_place(const float *face_uv, const int *assigned, size_t nf, double island_padding, unsigned *stats, int *block_scratch,
                    float *out_uv, sculpt_stream_t stream);
/* The DLL's own entry point (HOST pointers, same name / signature as unwrap.py:147-154 declares for uv_unwrapper.dll):
 * vertices [nv][3] (already rotated into the principal frame), indices int64 [nf][3], face_uv [nf][3][2], face_index int64 [nf]
 * in 0..5 -> out int64 [nf] in {c, c + 6, 12} */
void assign_faces_uv_to_atlas_index(const float *vertices, size_t nv, const long long *indices, size_t nf, const float *face_uv,
                                    const long long *face_index, long long *out);

/* StableFast geometry tail:
 *   dilate_fill (sf3d/models/utils.py:96-133): img f32 [3][H][W], mask f32 [H][W]; scratch 8*H*W floats
 *   vertex normals / tangents (sf3d/models/mesh.py:66-139): area-weighted face normal / UV tangent splat
 *   as order-independent fixed-point sums (reproducible to the bit), normalise, Gram-Schmidt; workspace:
 *   sculpt_vertex_accumulate_workspace_bytes(nv) device bytes. */
int sculpt_dilate_fill(const float *img, const float *mask, int H, int W, int iterations, float *scratch, float *out,
                       sculpt_stream_t stream);
size_t sculpt_vertex_accumulate_workspace_bytes(size_t nv);
int sculpt_vertex_normals(const float *v_pos, size_t nv, const void *faces, int faces_i64, size_t nf, void *workspace, float *out,
                          sculpt_stream_t stream);
int sculpt_vertex_tangents(const float *v_pos, const float *v_tex, const float *v_nrm, size_t nv, const void *faces,
                           int faces_i64, size_t nf, void *workspace, float *out, sculpt_stream_t stream);

/* fp32 -> bf16 (round to nearest even), n elements */
int sculpt_cast_bf16(const float *x, uint16_t *y, int64_t n, sculpt_stream_t stream);

/* Triangle remeshing of the SF3D output mesh: the three gpytoolbox calls of Mesh.triangle_remesh
 * (StableFast/sf3d/models/mesh.py:175-237), on the HOST like the reference's (HOST pointers; no GPU work, no stream).
 *   sculpt_mesh_subdivide      = gpytoolbox.subdivide(v, f, iters=...)      midpoint 1 -> 4 subdivision       (mesh.py:187-191)
 *   sculpt_mesh_decimate       = gpytoolbox.decimate(v, f, face_ratio=...)  shortest-edge collapse to the midpoint with the
 *                                link condition, until <= target_faces faces remain (libigl's default)        (mesh.py:195-199)
 *   sculpt_mesh_remesh_botsch  = gpytoolbox.remesh_botsch(v, f, i, h)       Botsch-Kobbelt isotropic remeshing: split > 4/3 h,
 *                                collapse < 4/5 h, valence flips, tangential relaxation, projection onto the input surface
 *                                (project != 0); h <= 0 = mean edge length of the input; boundary vertices stay  (mesh.py:225-230)
 * V f64 [nv][3], F int32 [nf][3].  The result is an opaque object (its size is not known beforehand): read the counts, copy
 * it out with sculpt_mesh_read (V f64 [num_vertices][3], F int32 [num_faces][3]) and release it with sculpt_mesh_free.
 * gpytoolbox / libigl are absent from the reference tree and the build image: PARITY UNPINNED (csrc/remesh_host.h). */
typedef struct sculpt_host_mesh sculpt_host_mesh_t;
int sculpt_mesh_subdivide(const double *V, size_t nv, const int32_t *F, size_t nf, int iters, sculpt_host_mesh_t **out);
int sculpt_mesh_decimate(const double *V, size_t nv, const int32_t *F, size_t nf, size_t target_faces,
                         sculpt_host_mesh_t **out);
int sculpt_mesh_remesh_botsch(const double *V, size_t nv, const int32_t *F, size_t nf, int iters, double h, int project,
                              sculpt_host_mesh_t **out);
size_t sculpt_mesh_num_vertices(const sculpt_host_mesh_t *m);
size_t sculpt_mesh_num_faces(const sculpt_host_mesh_t *m);
int sculpt_mesh_read(const sculpt_host_mesh_t *m, double *V, int32_t *F);
void sculpt_mesh_free(sculpt_host_mesh_t *m);

/* Triangle remeshing ON THE DEVICE (csrc/remesh_device.hip; driven by sculptmate_amd/sf3d/remesh_device.py, which does the
 * sorts and prefix sums): the same three operations as sculpt_mesh_* above, with the mesh in HBM.  Positions fp32 [nv][3], faces
 * int32 [nf][3]; DEVICE pointers except where a name ends in _host; every call is asynchronous on `stream`.
 * Every pass rebuilds its topology from the faces:
 *   sculpt_rmd_halfedge_keys   keys[3 f + k] = (min << 32 | max) of half-edge F[f][k] -> F[f][(k + 1) % 3]
 *   (caller: stable sort of the keys -> skeys, sperm)
 *   sculpt_rmd_edge_heads      head[i] = 1 where a run of equal sorted keys starts      (caller: inclusive prefix sum -> eid_incl)
 *   sculpt_rmd_edge_fill       she[i] = sperm[i], fe[half-edge] = edge, es[edge] = first sorted index (es[ne] = 3 nf)
 *   (caller: stable sort of the corners by vertex -> vfc, vfs = CSR offsets [nv + 1])
 *   sculpt_rmd_high_valence    flags[u] = 1 (caller zeroes it) where u has more than 64 distinct neighbours
 *   sculpt_rmd_boundary        bnd[u] = 1 where an edge at u does not have exactly two faces; the caller fills bnd beforehand with
 *                              the flags it carries: for the first pass over an input, its high-valence flags; after that, the
 *                              previous pass's bnd (0 for vertices a split added), with bnd[kept] |= bnd[removed] after a
 *                              decimation collapse.  High-valence rule, the host's (remesh_host.h: Mesh::build scans once, the
 *                              operations keep the flags): a vertex with more than 64 distinct neighbours in the INPUT is a
 *                              feature like a boundary vertex for the whole call, whatever its valence becomes -- the
 *                              Botsch-Kobbelt pass never moves or removes it (an interior neighbour may collapse into it), the
 *                              link condition treats it as a boundary vertex, and its flip valence is faces + 1 with target 4.
 *                              No operation is refused for the size of a fan.
 * Local operations claim their footprint with a 64-bit atomicMin of (priority << 32 | edge id) on claim[nv] (caller fills it
 * with ~0); a candidate applies only when it holds every vertex of its footprint, so a round is deterministic.
 *   sculpt_rmd_collapse_*      mode 0 = decimate (any edge, midpoint, link condition), 1 = Botsch-Kobbelt (edges < low, boundary
 *                              vertices stay, no new edge > high, no face turns over); footprint: every vertex of every face around
 *                              both ends; priority: edge length.  select: win[e] = faces removed (0: lost); apply: dead faces get
 *                              face_alive = 0 (caller fills 1), F and P change in place.
 *   sculpt_rmd_flip_*          valence flips (target 6, 4 on the boundary) with the crease (cos >= 0.5) and fold guards; footprint
 *                              {u, v, a, b}; win[e] = 1 for an applied flip.
 *   sculpt_rmd_split_*         mark edges longer than `high` (one or two faces), count the children of every face (1..4), then emit
 *                              the new vertices at P[nv + mark_incl[e] - 1] and the children at Fo[off_incl[f] - count ..]; nothing
 *                              is written at or beyond vcap vertices / fcap faces: the caller compares the totals with the
 *                              capacities and emits again into larger buffers if they did not fit.
 *   sculpt_rmd_grid_*          uniform grid over the projection surface GP / GF: params_host = {lo x, y, z, cell, nx, ny, nz};
 *                              count the cells of every face, then write (cell, face) pairs (caller: stable sort by cell, CSR)
 *   sculpt_rmd_relax           tangential relaxation (Jacobi) + projection onto the grid's surface in fp64, the centroid over the
 *                              distinct neighbours; then every vertex of a face that turned over takes its move back, repeated
 *                              until no face is turned over (one readback per pass: this call synchronizes `stream`);
 *                              Q [nv][3] out, undo: 4-byte aligned scratch of SCULPT_RMD_UNDO_BYTES(nv) bytes
 *   sculpt_rmd_compact_faces, _mark_used, _compact_vertices: keep live faces / referenced vertices in index order
 *   sculpt_rmd_first_halfedge, _subdivide: midpoint subdivision, new vertices in order of first appearance (like the host's)
 *   sculpt_rmd_validate        status bit 0: face index out of range, 1: repeated index in a face, 2: non-finite position
 *   sculpt_rmd_halfedge_lengths per face: the sum of its three side lengths (fp64)
 * Quadric-error simplification (csrc/mesh_simplify.hip; sf3d/remesh_device.py simplify_device, ops.mesh_simplify), on the same
 * topology and rounds; compiled without floating-point contraction, so every value below is a fixed sequence of IEEE fp64
 * operations (restated in tests/_qemref.py):
 *   sculpt_rmd_qem_quadrics    Q[u][10] fp64 = {aa ab ac ad bb bc bd cc cd dd} summed, in the order of u's CSR corners, over the
 *                              plane (unit normal n, d = -n . p0) of every face around u; a face whose cross product has zero or
 *                              non-finite length contributes nothing.  Once per call: vertices keep their indices, apply keeps Q.
 *   sculpt_rmd_qem_cost        per edge with one or two faces, q = Q[u] + Q[v] (u < v; u goes, v stays): no candidate when
 *                              bnd[u] != bnd[v]; target = the minimiser of the error (the reference's three determinants) unless
 *                              both ends are flagged, det == 0 or the point rounded to fp32 is not finite -- then whichever of
 *                              p_u, p_v, the fp32 midpoint has the least error (ties in that order).  target[e][3] fp32 is the
 *                              point rounded once; cost = the error AT target, clamped at 0 (a non-finite error: no candidate).
 *                              The link condition as in mode 0;
 *                              fold-over: for every face of the two fans that survives and has a normal now, the unit edges
 *                              d1, d2 from the target to its other corners must exist with |d1 . d2| <= 0.999 and
 *                              normalize(d1 x d2) . (current unit normal) >= 0.2.  cand[e] = (fp32 bits of cost) << 32 | e, or ~0
 *                              (then target[e] = 0).  Claims nothing.
 *   sculpt_rmd_qem_claim       candidates with cand[e] <= *cap (a DEVICE scalar: the round's k-th smallest key) claim the footprint
 *                              of mode 0 on claim[nv]; then sculpt_rmd_collapse_select(mode 0) names the winners
 *   sculpt_rmd_qem_apply       like sculpt_rmd_collapse_apply, with P[v] = target[e] and Q[v] += Q[u] */
typedef struct sculpt_rmd_topo {
    const int32_t *F;      /* [nf][3] */
    const int64_t *skeys;  /* [3 nf] half-edge keys, sorted */
    const int32_t *she;    /* [3 nf] half-edge ids in sorted order */
    const int32_t *es;     /* [ne + 1] first sorted index of every edge */
    const int32_t *fe;     /* [3 nf] edge of every half-edge */
    const int32_t *vfs;    /* [nv + 1] vertex -> corner offsets */
    const int32_t *vfc;    /* [3 nf] corners (3 f + k) by vertex, in corner order */
    const uint8_t *bnd;    /* [nv] */
    int64_t nf, nv, ne;
} sculpt_rmd_topo_t;
int sculpt_rmd_halfedge_keys(const int32_t *F, int64_t nf, int64_t *keys, sculpt_stream_t stream);
int sculpt_rmd_edge_heads(const int64_t *skeys, int64_t nh, int32_t *head, sculpt_stream_t stream);
int sculpt_rmd_edge_fill(const int64_t *sperm, const int32_t *eid_incl, int64_t nh, int32_t *she, int32_t *fe, int32_t *es,
                         sculpt_stream_t stream);
int sculpt_rmd_high_valence(const sculpt_rmd_topo_t *topo, uint8_t *flags, sculpt_stream_t stream);
int sculpt_rmd_boundary(const sculpt_rmd_topo_t *topo, uint8_t *bnd, sculpt_stream_t stream);
#define SCULPT_RMD_UNDO_BYTES(nv) ((((int64_t)(nv) + 3) & ~(int64_t)3) + 4) /* a flag per vertex, then the pass's int32 "grew" */
int sculpt_rmd_collapse_propose(const sculpt_rmd_topo_t *topo, const float *P, int mode, double low, double high,
                                unsigned long long *claim, unsigned long long *cand, sculpt_stream_t stream);
int sculpt_rmd_collapse_select(const sculpt_rmd_topo_t *topo, const float *P, int mode, const unsigned long long *claim,
                               const unsigned long long *cand, int32_t *win, sculpt_stream_t stream);
int sculpt_rmd_collapse_apply(const sculpt_rmd_topo_t *topo, float *P, int32_t *F, int mode, const int32_t *win, uint8_t *face_alive,
                              sculpt_stream_t stream);
int sculpt_rmd_flip_propose(const sculpt_rmd_topo_t *topo, const float *P, unsigned long long *claim, unsigned long long *cand,
                            sculpt_stream_t stream);
int sculpt_rmd_flip_apply(const sculpt_rmd_topo_t *topo, const float *P, const unsigned long long *claim,
                          const unsigned long long *cand, int32_t *F, int32_t *win, sculpt_stream_t stream);
int sculpt_rmd_split_mark(const sculpt_rmd_topo_t *topo, const float *P, double high, int32_t *mark, sculpt_stream_t stream);
int sculpt_rmd_split_count(const sculpt_rmd_topo_t *topo, const int32_t *mark, int32_t *cnt, sculpt_stream_t stream);
int sculpt_rmd_split_emit(const sculpt_rmd_topo_t *topo, float *P, int64_t vcap, const int32_t *mark, const int32_t *mark_incl,
                          const int32_t *off_incl, int64_t fcap, int32_t *Fo, sculpt_stream_t stream);
int sculpt_rmd_grid_count(const float *GP, const int32_t *GF, int64_t gnf, const double *params_host, int32_t *cnt,
                          sculpt_stream_t stream);
int sculpt_rmd_grid_fill(const float *GP, const int32_t *GF, int64_t gnf, const double *params_host, const int32_t *off_incl,
                         int32_t *cell, int32_t *face, sculpt_stream_t stream);
int sculpt_rmd_relax(const sculpt_rmd_topo_t *topo, const float *P, const float *GP, const int32_t *GF, int64_t gnf,
                     const int32_t *items, const int32_t *start, const double *params_host, int project, float *Q, uint8_t *undo,
                     sculpt_stream_t stream);
int sculpt_rmd_compact_faces(const int32_t *F, const uint8_t *alive, const int32_t *incl, int64_t nf, int32_t *Fo,
                             sculpt_stream_t stream);
int sculpt_rmd_mark_used(const int32_t *F, int64_t nf, int32_t *used, sculpt_stream_t stream);
int sculpt_rmd_compact_vertices(const float *P, const int32_t *used, const int32_t *incl, int64_t nv, float *Po, int32_t *F, int64_t nf,
                                sculpt_stream_t stream);
int sculpt_rmd_first_halfedge(const sculpt_rmd_topo_t *topo, int32_t *first, sculpt_stream_t stream);
int sculpt_rmd_subdivide(const sculpt_rmd_topo_t *topo, const float *P, const int32_t *rank_incl, float *Po, int32_t *Fo,
                         sculpt_stream_t stream);
int sculpt_rmd_validate(const float *P, int64_t nv, const int32_t *F, int64_t nf, int32_t *status, sculpt_stream_t stream);
int sculpt_rmd_halfedge_lengths(const float *P, const int32_t *F, int64_t nf, double *len, sculpt_stream_t stream);
int sculpt_rmd_qem_quadrics(const sculpt_rmd_topo_t *topo, const float *P, double *Q, sculpt_stream_t stream);
int sculpt_rmd_qem_cost(const sculpt_rmd_topo_t *topo, const float *P, const double *Q, unsigned long long *cand, float *target,
                        sculpt_stream_t stream);
int sculpt_rmd_qem_claim(const sculpt_rmd_topo_t *topo, const unsigned long long *cand, const unsigned long long *cap,
                         unsigned long long *claim, sculpt_stream_t stream);
int sculpt_rmd_qem_apply(const sculpt_rmd_topo_t *topo, float *P, int32_t *F, double *Q, const float *target, const int32_t *win,
                         uint8_t *face_alive, sculpt_stream_t stream);

/* Mesh smoothing ON THE DEVICE: Taubin's lambda|mu filter (csrc/mesh_smooth.hip; sf3d/remesh_device.py smooth_device,
 * ops.mesh_smooth).  The faces do not change; the positions do.  DEVICE pointers, asynchronous on `stream`, no host wait.
 * Compiled without floating-point contraction: every position is a fixed sequence of IEEE fp32 operations (restated in
 * tests/_smoothref.py).  The neighbour table is built once per call from a topology (sculpt_rmd_topo_t):
 *   sculpt_smooth_edge_keys    keys[2 e] = (u << 32 | v), keys[2 e + 1] = (v << 32 | u) for every edge e = {u, v} of the topology;
 *                              keys [2 ne].  (caller: sort the keys -- they are distinct, so the order is unique -- and
 *                              start[u] = the first sorted index with key >= u << 32, [nv + 1])
 *   sculpt_smooth_neighbours   nb[i] = the low 32 bits of skeys[i]: row u of the CSR (start, nb) holds the distinct neighbours
 *                              of u in ascending order
 *   sculpt_smooth_taubin       `iterations` (1 .. 1000) times: a half-step with factor (float)lam, then one with (float)mu;
 *                              mu == 0: the first alone (plain Laplacian).  0 < lam <= 1; mu == 0 or -1 <= mu < -lam.
 *                              A half-step, per vertex u of degree deg = start[u + 1] - start[u], p -> q:
 *                                  s = p[nb[start[u]]], then s = s + p[nb[j]] for the rest of the row in order
 *                                  q = p + k * (s / (float)deg - p)      (a division, a subtraction, a product, a sum)
 *                              and q = p where fixed[u] != 0 or deg == 0.  fixed [nv]: sculpt_rmd_boundary on zeroes (an edge at
 *                              u without exactly two faces).  P [nv][3] in, out [nv][3] (may be P); work_a, work_b: two
 *                              distinct 16-byte aligned buffers of nv * 4 floats (positions as x y z - rows, read and written
 *                              in turn).  nb holds n_nb entries, each in [0, nv): the caller's table is trusted, like F.
 * Null, misaligned or out-of-range arguments are refused with an error code and a message; nv == 0 launches nothing. */
int sculpt_smooth_edge_keys(const sculpt_rmd_topo_t *topo, int64_t *keys, sculpt_stream_t stream);
int sculpt_smooth_neighbours(const int64_t *skeys, int64_t n, int32_t *nb, sculpt_stream_t stream);
int sculpt_smooth_taubin(const int32_t *start, const int32_t *nb, const uint8_t *fixed, int64_t nv, int64_t n_nb, const float *P,
                         int iterations, double lam, double mu, float *work_a, float *work_b, float *out, sculpt_stream_t stream);

/* Loop subdivision ON THE DEVICE, one level per pair of calls (csrc/mesh_subdivide.hip; sf3d/remesh_device.py
 * loop_subdivide_device, ops.mesh_subdivide).  DEVICE pointers, asynchronous on `stream`, no host wait.
 * Added without a version change (new symbols only).  Compiled without floating-point contraction and restated bit for bit in
 * tests/_loopref.py.  The faces and the numbering are sculpt_rmd_subdivide's: new vertex nv + rank_incl[h] - 1 for the edge
 * whose first half-edge is h (rank_incl: the inclusive prefix sum of sculpt_rmd_first_halfedge), face (a, b, c) -> (a, ab, ca),
 * (b, bc, ab), (c, ca, bc), (ab, bc, ca) at rows 4 f .. 4 f + 3.  An edge is classified by its face count es[e + 1] - es[e]
 * alone -- 2: interior, 1: border, 3 or more: non-manifold; topo->bnd is not read.
 *   sculpt_subdiv_classify   cls [nv][4] int32 (16-byte aligned; zeroed here, then integer atomics only: one possible result) =
 *                            {border edges at u, 1 + the largest other end of one, nv - the smallest, 1 if a non-manifold edge
 *                            touches u}; rows [nv][4] floats (16-byte aligned) = the positions P [nv][3] as x y z - rows.
 *   sculpt_subdiv_loop       Po [nv + ne][3], Fo [4 nf][3] and, with A [nv][channels] (1 <= channels <= 8; A and Ao both or
 *                            neither), Ao [nv + ne][channels].  Per component in fp64 from the fp32 values, exactly these
 *                            operations, rounded once to fp32:
 *                              odd vertex of edge {u, v}: interior, a and b the third vertices of its two faces:
 *                                    0.375 * (P[u] + P[v]) + 0.125 * (P[a] + P[b]);   otherwise 0.5 * (P[u] + P[v])
 *                              even vertex u with fan n = vfs[u + 1] - vfs[u]:
 *                                n == 0, a non-manifold edge at u, or border edges at u neither 0 nor 2 (a corner): its bits;
 *                                two border edges with other ends a, b (a crease): 0.75 * P[u] + 0.125 * (P[a] + P[b]);
 *                                otherwise beta = n == 3 ? 0.1875 : 3.0 / (8.0 * n) (Warren), S = the sum left to right, over
 *                                the corners 3 f + k of u's fan in vfc order, of P[F[3 f + (k + 1) % 3]] and then
 *                                P[F[3 f + (k + 2) % 3]], starting as the first term (every neighbour enters twice):
 *                                    (1.0 - n * beta) * P[u] + (0.5 * beta) * S
 *                            The attributes go through the same masks.  The outputs must not alias the inputs.
 * A null topology or array, a misaligned buffer, channels out of range and counts whose level would leave int32 (nv + ne,
 * 12 nf) are refused with an error code and a message; nf == 0 launches nothing (the caller returns copies). */
int sculpt_subdiv_classify(const sculpt_rmd_topo_t *topo, const float *P, int32_t *cls, float *rows, sculpt_stream_t stream);
int sculpt_subdiv_loop(const sculpt_rmd_topo_t *topo, const int32_t *cls, const float *rows, const int32_t *rank_incl, const float *A,
                       int channels, float *Po, int32_t *Fo, float *Ao, sculpt_stream_t stream);

/* Catmull-Clark subdivision ON THE DEVICE, one level per pair of calls, triangles or quads in and all quads out
 * (csrc/mesh_catmull.hip; sf3d/remesh_device.py catmull_clark_device, ops.mesh_catmull_clark).  DEVICE
 * pointers, asynchronous on `stream`, no host wait.  Added without a version change (new symbols only).  Compiled without
 * floating-point contraction and restated bit for bit in tests/_catmullref.py.
 * THE RULE.  P fp32 [nv][3], F int32 [nf][k], k = 3 or 4, uniform per call.  Half-edge h = k f + c runs F[f][c] ->
 * F[f][(c + 1) % k].  An edge is the unordered pair of its ends; edge e (0-based) is its rank by first appearance over
 * h = 0, 1, ...; with two faces it is interior, with one a border edge, with three or more non-manifold; its faces are listed in
 * half-edge order.  Every component below is computed in fp64 from the fp32 values with exactly the operations written, left
 * to right, without contraction, and rounded once to fp32; where a face point appears inside another rule it is the unrounded
 * fp64 value of the same operations.
 *   numbering    old vertices keep 0 .. nv - 1; the face point of f is nv + f; the edge point of e is nv + nf + e.
 *                nv' = nv + nf + ne, nq' = k nf.
 *   quads        corner c of face f becomes row k f + c =
 *                    (F[f][c], edge point of half-edge (f, c), nv + f, edge point of half-edge (f, (c - 1) % k));
 *                orientation is kept.
 *   face point   Fp(f) = (((P[c0] + P[c1]) + P[c2]) [+ P[c3]]) / (double)k
 *   edge point   of {u, v}: interior, faces f0, f1:  0.25 * ((P[u] + P[v]) + (Fp(f0) + Fp(f1)));
 *                border or non-manifold:             0.5 * (P[u] + P[v])
 *   old vertex   u with n corners in the faces (its fan, in ascending corner index k f + c):
 *                  n == 0, a non-manifold edge at u, or border edges at u neither 0 nor 2 (a corner): its bits;
 *                  two border edges with other ends a < b (a crease): 0.75 * P[u] + 0.125 * (P[a] + P[b]);
 *                  otherwise, m = (double)n:  ((m - 2.0) * P[u] + (0.5 * SN + SQ) / m) / m, where SN is the sum over the
 *                  fan in order of P[F[f][(c + 1) % k]] and then P[F[f][(c - 1) % k]] of each corner (f, c), starting as the
 *                  first term (every neighbour enters twice: no dependence on orientation), and SQ the sum over the fan of
 *                  Fp(f), starting as the first term.  Any valence follows these rules.
 *   attributes   [nv][channels], 1 <= channels <= 8, go through the same masks.
 *   triangles    rows 2 q, 2 q + 1 split quad q = (q0, q1, q2, q3) along its shorter diagonal, sculpt_surface_nets_emit's
 *                split on the REFINED fp32 positions: d02 = |P'[q0] - P'[q2]|^2, d13 = |P'[q1] - P'[q3]|^2 in fp64 as
 *                (dx dx + dy dy) + dz dz; d13 < d02: (q0, q1, q3), (q1, q2, q3); otherwise (a tie included): (q0, q1, q2),
 *                (q0, q2, q3).
 * THE CALLS.  The topology is the triangle passes' (sorted half-edge keys, vertex -> corner CSR) for k corners; the caller
 * sorts and scans as for sculpt_rmd_topo_t, and sculpt_rmd_edge_heads / sculpt_rmd_edge_fill serve any k (they take nh = k nf).
 *   sculpt_catmull_validate        status bit 0: face index out of range, 1: repeated index in a face, 2: non-finite position
 *   sculpt_catmull_halfedge_keys   keys [k nf]: (min << 32 | max) of every half-edge's ends
 *   sculpt_catmull_first_halfedge  first [k nf] = 1 where h is the lowest half-edge of its edge (rank_incl: its inclusive
 *                                  prefix sum; the edge whose first half-edge is h has rank rank_incl[h] - 1)
 *   sculpt_catmull_classify        cls [nv][4] int32 and rows [nv][4] floats, as sculpt_subdiv_classify writes them
 *   sculpt_catmull_refine          ONE launch: Po [nv + nf + ne][3], Qo [k nf][4], To [2 k nf][3] and, with A [nv][channels]
 *                                  (A and Ao both or neither), Ao [nv + nf + ne][channels].  The outputs must not alias the inputs.
 * A null topology or array, a misaligned buffer, k other than 3 or 4, channels out of range and counts whose level would leave
 * int32 (nv + nf + ne, 4 k nf) are refused with an error code and a message; nf == 0 launches nothing (the caller returns copies). */
typedef struct sculpt_catmull_topo {
    const int32_t *F;      /* [nf][k] */
    const int64_t *skeys;  /* [k nf] half-edge keys, sorted */
    const int32_t *she;    /* [k nf] half-edge ids in sorted order */
    const int32_t *es;     /* [ne + 1] first sorted index of every edge (in sorted-key order) */
    const int32_t *fe;     /* [k nf] edge of every half-edge */
    const int32_t *vfs;    /* [nv + 1] vertex -> corner offsets */
    const int32_t *vfc;    /* [k nf] corners (k f + c) by vertex, in corner order */
    int64_t nf, nv, ne;
    int32_t k;
} sculpt_catmull_topo_t;
int sculpt_catmull_validate(const float *P, int64_t nv, const int32_t *F, int64_t nf, int k, int32_t *status, sculpt_stream_t stream);
int sculpt_catmull_halfedge_keys(const int32_t *F, int64_t nf, int k, int64_t *keys, sculpt_stream_t stream);
int sculpt_catmull_first_halfedge(const sculpt_catmull_topo_t *topo, int32_t *first, sculpt_stream_t stream);
int sculpt_catmull_classify(const sculpt_catmull_topo_t *topo, const float *P, int32_t *cls, float *rows, sculpt_stream_t stream);
int sculpt_catmull_refine(const sculpt_catmull_topo_t *topo, const int32_t *cls, const float *rows, const int32_t *rank_incl,
                          const float *A, int channels, float *Po, int32_t *Qo, int32_t *To, float *Ao, sculpt_stream_t stream);

/* Distance between triangle surfaces ON THE DEVICE (csrc/mesh_distance.hip; ops.mesh_closest_points, ops.mesh_sample_surface,
 * ops.mesh_distance).  DEVICE pointers (params_host excepted), asynchronous on `stream`, no host wait.
 * Compiled without floating-point contraction and restated bit for bit in tests/_distref.py.  Added without a version change
 * (new symbols only).  The grid is the remesher's (sculpt_rmd_grid_count / sculpt_rmd_grid_fill, params_host = {lo x, y, z,
 * cell, nx, ny, nz}, items / start the CSR of faces per cell); GP [nv][3], GF [gnf][3] with every index in range (trusted).
 *   sculpt_surface_closest   per query Q[i] (fp32, widened to fp64): the lexicographic minimum of (d2_f, f) over ALL faces whose
 *                            d2_f is not NaN, d2_f = |q_f - p|^2 summed (x x + y y) + z z, q_f = Ericson's closest point of face
 *                            f.  d2 [n] f64, face [n] int32, closest [n][3] = q_face rounded once to fp32.  No face, or only
 *                            NaN: +inf, -1, the query.  A non-finite query: NaN, -1, the query.  amax: a bound on |coordinate|
 *                            of every vertex the faces name (it scales the guard of the walk's stopping test).
 *                            order == records == NULL: the plain form, one thread per query in input order.  Otherwise the
 *                            sorted form: order [n] = the permutation that sorts the keys of sculpt_surface_cells (int64),
 *                            records = sculpt_surface_pack's.  Both forms give the same bits on every input.
 *   sculpt_surface_cells     key [n] int32: the linear index of the query's clamped grid cell; nx ny nz for a non-finite query
 *   sculpt_surface_pack      records [gnf][16] floats, 16-byte aligned: box min, box max, a, b, c, one pad
 *   sculpt_surface_weights   area2 [nf] f64 = |cross(b - a, c - a)|; *max_bits = the bits of its maximum; w [nf] int64 =
 *                            llrint(ldexp(area2, B - e)), e the frexp exponent of the maximum, B = min(40, 62 - bit_length(nf))
 *   sculpt_surface_sample    n samples from cdf [nf] int64, the inclusive prefix sum of w with cdf[nf - 1] > 0: sample i takes
 *                            words 3i .. 3i + 2 of splitmix64(seed): face = the first f with cdf[f] > mulhi64(r0, W); u, v =
 *                            (r >> 40) 2^-24, reflected when u + v > 1; points [n][3] = (a + u (b - a)) + v (c - a) in fp32,
 *                            face [n] int32, uv [n][2]
 * Null, misaligned or out-of-range arguments are refused with an error code and a message; n == 0 launches nothing. */
int sculpt_surface_closest(const float *Q, int64_t n, const int64_t *order, const float *GP, const int32_t *GF, int64_t gnf,
                           const float *records, const int32_t *items, const int32_t *start, const double *params_host, double amax,
                           double *d2, int32_t *face, float *closest, sculpt_stream_t stream);
int sculpt_surface_cells(const float *Q, int64_t n, const double *params_host, int32_t *key, sculpt_stream_t stream);
int sculpt_surface_pack(const float *GP, const int32_t *GF, int64_t gnf, float *records, sculpt_stream_t stream);
int sculpt_surface_weights(const float *P, const int32_t *F, int64_t nf, double *area2, unsigned long long *max_bits, int64_t *w,
                           sculpt_stream_t stream);
int sculpt_surface_sample(const float *P, const int32_t *F, int64_t nf, const int64_t *cdf, int64_t n, unsigned long long seed,
                          float *points, int32_t *face, float *uv, sculpt_stream_t stream);

/* Inside / outside of a triangle surface (csrc/mesh_winding.hip; ops.mesh_winding, ops.mesh_contains, ops.mesh_signed_distance,
 * ops.mesh_sdf_grid, ops.mesh_voxel_remesh).  Compiled without floating-point contraction and restated bit
 * for bit in tests/_windref.py.  Added without a version change (new symbols only).  The mesh, the grid, the records and the order
 * are those of sculpt_surface_closest.
 *   sculpt_surface_winding          w [n][3] int32: per query Q[i] and axis a, the sum over ALL faces of the signed crossings of
 *                                   the ray from Q[i] along +a under the watertight rule at the top of csrc/mesh_winding.hip
 *                                   (box clause, edge signs with a symbolic tie-break, strictly ahead).  A non-finite query:
 *                                   INT32_MIN three times.  No faces: zeros.  order == records == NULL: the plain form, one
 *                                   thread per query in input order; otherwise the sorted form.  The same integers either way.
 *   sculpt_surface_winding_lattice  the same at the points (i0, i1, i2) of a lattice, x_k = (float)(lo_host[k] + i_k h) with the
 *                                   product and the sum in fp64: planes uint32 [n0 n1][ceil(n2 / 32)], bit i2 % 32 of word
 *                                   i2 / 32 = at least two of the three counts are nonzero, bits past n2 zero (what
 *                                   sculpt_mc_count_launch_for takes as sign planes); counts int32 [n0][n1][n2][3], always
 *                                   written (one launch per axis shares each lattice line's walk; the vote reads them).
 *                                   records are always needed with gnf > 0.  Each side 1 .. 1024.
 *   sculpt_lattice_active_corners   the lattice points that are a corner of a cell whose 8 bits are not all equal, as ascending
 *                                   linear indices (i0 n1 + i1) n2 + i2.  Two calls with the same offsets int32
 *                                   [sculpt_lattice_active_blocks(n0, n1, n2) + 1]: list == NULL counts and scans (the last word
 *                                   of offsets is the number of active points, for the caller to read back), list != NULL emits
 *                                   at most `capacity` indices.
 *   sculpt_sdf_fill                 vol f32 [n0][n1][n2]: +band / -band at every point by its bit; at listed point list[j] with
 *                                   squared distance d2[j] (f64): d = (float)fmin(sqrt(d2[j]), band); bit set: d if d > 0 else
 *                                   2^-126; bit clear: -d.  So (vol > 0) == bit at every lattice point.
 * Null, misaligned or out-of-range arguments are refused with an error code and a message; n == 0 launches nothing. */
int sculpt_surface_winding(const float *Q, int64_t n, const int64_t *order, const float *GP, const int32_t *GF, int64_t gnf,
                           const float *records, const int32_t *items, const int32_t *start, const double *params_host, int32_t *w,
                           sculpt_stream_t stream);
int sculpt_surface_winding_lattice(const double *lo_host, double h, int n0, int n1, int n2, const float *GP, const int32_t *GF,
                                   int64_t gnf, const float *records, const int32_t *items, const int32_t *start,
                                   const double *params_host, uint32_t *planes, int32_t *counts, sculpt_stream_t stream);
int64_t sculpt_lattice_active_blocks(int n0, int n1, int n2);
int sculpt_lattice_active_corners(const uint32_t *planes, int n0, int n1, int n2, int32_t *offsets, int32_t *list, int64_t capacity,
                                  sculpt_stream_t stream);
int sculpt_sdf_fill(float *vol, const uint32_t *planes, int n0, int n1, int n2, const int32_t *list, const double *d2, int64_t n,
                    double band, sculpt_stream_t stream);

/* The mesh report (csrc/mesh_report.hip; ops.mesh_report, ops.mesh_self_intersections).  Compiled without
 * floating-point contraction and restated in tests/_reportref.py.  Added without a version change (new symbols only).
 *   sculpt_mesh_edge_census     counts int64 [8] on the device, over the undirected sorted half-edge keys of `topo`: [0] edges,
 *                               [1] border edges (1 half-edge), [2] non-manifold edges (>= 3), [3] inconsistently wound edges
 *                               (exactly 2 half-edges that start at the same vertex), [4] vertices named by at least one face,
 *                               [5 .. 7] zero.  A face with a repeated index contributes its half-edges like any other,
 *                               self-loops included.  Integer atomics, one per workgroup and figure: exact in any order.
 *   sculpt_mesh_face_measures   per face with corners a, b, c (fp32 widened to fp64): area2 [nf] f64 = |cross(b - a, c - a)|
 *                               (sculpt_surface_weights' value, bit for bit), vol6 [nf] f64 = (a0 (b1 c2 - b2 c1) - a1 (b0 c2 -
 *                               b2 c0)) + a2 (b0 c1 - b1 c0); *n_degenerate (int64 on the device, zeroed by the call) = the faces
 *                               that repeat an index or have area2 == 0.
 *   sculpt_surface_self_count   the pairs of faces i < j that intersect under the rule at the top of csrc/mesh_report.hip:
 *                               orient(a, b, c, d) of four vertex indices is 0 when two are equal and else the sign of the fp64
 *                               determinant (u0 (v1 w2 - v2 w1) - u1 (v0 w2 - v2 w0)) + u2 (v0 w1 - v1 w0) of u, v, w = P[b], P[c],
 *                               P[d] - P[a]; a segment (p, q) meets a triangle (a, b, c) when orient(a, b, c, p) orient(a, b, c,
 *                               q) < 0 and orient(p, q, a, b), orient(p, q, b, c), orient(p, q, c, a) are all >= 0 or all <= 0 and
 *                               not all zero; faces intersect when their fp32 boxes overlap (closed) and an edge of one meets
 *                               the other.  n [gnf] int32 = the number of j > i that intersect i; flag [gnf] uint8, zeroed by
 *                               the CALLER, gets 1 at both faces of every pair.  The mesh, the grid and the records are those
 *                               of sculpt_surface_closest; the grid only skips pairs, and a pair is tested once, in the first
 *                               cell its two boxes share.  order == records == NULL: the plain form, one thread per face in
 *                               input order; otherwise order int64 [gnf] is a permutation of the faces (by first cell) and the
 *                               boxes come from the records.  The same integers either way.
 *   sculpt_surface_self_emit    the same walk; offsets int64 [gnf + 1] = the exclusive scan of n with the total last; writes
 *                               keys[offsets[i] ..] = i << 32 | j, never at or past min(offsets[i + 1], capacity).  The order of
 *                               one face's keys is unspecified: the caller sorts.
 * Null, misaligned or out-of-range arguments are refused with an error code and a message; no faces launches nothing. */
int sculpt_mesh_edge_census(const sculpt_rmd_topo_t *topo, int64_t *counts, sculpt_stream_t stream);
int sculpt_mesh_face_measures(const float *P, const int32_t *F, int64_t nf, double *area2, double *vol6, int64_t *n_degenerate,
                              sculpt_stream_t stream);
int sculpt_surface_self_count(const float *GP, const int32_t *GF, int64_t gnf, const int64_t *order, const float *records,
                              const int32_t *items, const int32_t *start, const double *params_host, int32_t *n, uint8_t *flag,
                              sculpt_stream_t stream);
int sculpt_surface_self_emit(const float *GP, const int32_t *GF, int64_t gnf, const int64_t *order, const float *records,
                             const int32_t *items, const int32_t *start, const double *params_host, const int64_t *offsets,
                             int64_t *keys, int64_t capacity, sculpt_stream_t stream);

/* Fill holes (csrc/mesh_holes.hip; ops.mesh_border_loops, ops.mesh_fill_holes).  The rule stands at the top
 * of csrc/mesh_holes.hip and is restated in tests/_holesref.py.  Compiled without floating-point contraction; everything up to the
 * centroids is integers.  Added without a version change (new symbols only).  All arrays are on the device; nb is the number of
 * border half-edges (the caller reads it from the scan of `flag`), and a "list index" is a position in their ascending list.
 *   sculpt_mesh_border_mark      flag int32 [3 nf] = 1 at the one half-edge of every edge that has exactly one; vout, vin int32 [nv]
 *                                = how many of them start / end at the vertex; start_of int32 [nv] = the smallest of them that
 *                                starts there.  All four are initialised by the call.
 *   sculpt_mesh_border_next      incl = the inclusive scan of flag.  list int32 [nb] = the border half-edges, ascending;
 *                                next int32 [nb] = the list index of next(h), -1 for a blocked half-edge (an end with out != 1 or
 *                                in != 1); counts int64 [8], zeroed by the call: [0] = the pinched vertices.
 *   sculpt_mesh_border_label     pointer doubling over the two state buffers (int64 [nb] each), ceil(log2(nb)) + 1 rounds, each
 *                                reading one buffer and writing the other: leader int32 [nb] = the list index of the smallest
 *                                half-edge of the element's cycle, -1 when its chain reaches a blocked one; length int32 [nb],
 *                                zeroed by the call, = the cycle's length at its leader.
 *   sculpt_mesh_border_decide    max_edges == 0: every loop, else loops of at most max_edges >= 3 edges; in any case at most
 *                                2^22 - 1.  emits, centre, heads int32 [nb] = 1 where the element emits a face / leads a filled
 *                                loop of at least 4 edges / leads a loop; counts [1 .. 7] += loops, open half-edges, filled loops,
 *                                filled edges, skipped loops, new vertices, new faces.
 *   sculpt_mesh_border_loops     label int32 [nb] = the leader as a half-edge, -1 when open; leaders, lengths int32 [n_loops] in
 *                                ascending leader order (heads_incl = the inclusive scan of heads).
 *   sculpt_mesh_holes_centroids  rows Pn [n_new][3] (and An [n_new][channels], channels <= 8) = per filled loop of at least 4 edges,
 *                                in ascending leader order, the mean over the starts of its half-edges: two order-independent
 *                                passes (csrc/fixsum.h) over mag uint32 and acc int64 [n_new (3 + channels)], zeroed by the call,
 *                                then (float)(ldexp((double)acc, e - 40) / (double)n).  centre_incl = the inclusive scan of centre.
 *   sculpt_mesh_holes_emit       Fn int32 [n_faces][3], rows in ascending order of the emitting half-edge h = (a -> b): (b, a,
 *                                nv + the loop's centroid row), or for a loop of 3 (b, a, end(next(h))) from the leader alone.
 * Null or out-of-range arguments are refused with an error code and a message; no faces or nb == 0 launches nothing. */
int sculpt_mesh_border_mark(const sculpt_rmd_topo_t *topo, int32_t *flag, int32_t *vout, int32_t *vin, int32_t *start_of,
                            sculpt_stream_t stream);
int sculpt_mesh_border_next(const sculpt_rmd_topo_t *topo, const int32_t *flag, const int32_t *incl, int64_t nb, const int32_t *vout,
                            const int32_t *vin, const int32_t *start_of, int32_t *list, int32_t *next, int64_t *counts,
                            sculpt_stream_t stream);
int sculpt_mesh_border_label(const int32_t *next, int64_t nb, int64_t *state_a, int64_t *state_b, int32_t *leader, int32_t *length,
                             sculpt_stream_t stream);
int sculpt_mesh_border_decide(const int32_t *leader, const int32_t *length, int64_t nb, int64_t max_edges, int32_t *emits, int32_t *centre,
                              int32_t *heads, int64_t *counts, sculpt_stream_t stream);
int sculpt_mesh_border_loops(const int32_t *list, const int32_t *leader, const int32_t *length, const int32_t *heads_incl, int64_t nb,
                             int64_t n_loops, int32_t *label, int32_t *leaders, int32_t *lengths, sculpt_stream_t stream);
int sculpt_mesh_holes_centroids(const sculpt_rmd_topo_t *topo, const float *P, const float *A, int channels, const int32_t *list,
                                const int32_t *leader, const int32_t *length, const int32_t *centre, const int32_t *centre_incl, int64_t nb,
                                int64_t n_new, uint32_t *mag, int64_t *acc, float *Pn, float *An, sculpt_stream_t stream);
int sculpt_mesh_holes_emit(const sculpt_rmd_topo_t *topo, const int32_t *list, const int32_t *next, const int32_t *leader,
                           const int32_t *length, const int32_t *emits, const int32_t *emits_incl, const int32_t *centre,
                           const int32_t *centre_incl, int64_t nb, int64_t n_new, int64_t n_faces, int32_t *Fn, sculpt_stream_t stream);

/* Rays against a triangle surface (csrc/mesh_ray.hip; ops.mesh_ray_cast, ops.mesh_occlusion).  Compiled
 * without floating-point contraction and restated bit for bit in tests/_rayref.py.  Added without a version change (new symbols
 * only).  The grid, the records, the order and amax are those of sculpt_surface_closest; the grid must cover the surface: lo is
 * the least coordinate of the vertices the faces name, and lo + n cell is not below their greatest one on an axis with n < 1024.
 *   sculpt_surface_ray_cast   per ray (O[i], D[i]) (fp32, widened to fp64) over tmin <= t <= tmax (0 <= tmin <= tmax, tmax may
 *                             be +inf): the lexicographic minimum of (t_f, f) over ALL faces that the two-sided per-face rule
 *                             at the top of csrc/mesh_ray.hip reports hit (Moeller-Trumbore in fp64 with a relative
 *                             determinant test, then the box clause: the hit point lies within E = 2^-40 max(|o|_inf, amax) of
 *                             the face's bounding box).  t [n] f64, face [n] int32, uv [n][2] = (u, v) of the winner rounded
 *                             once.  No hit, or a zero direction: +inf, -1, 0.  A non-finite origin or direction: NaN, -1, 0.
 *                             order == records == NULL: the plain form, one thread per ray in input order; otherwise the sorted
 *                             form (order [n] sorts the keys of sculpt_surface_cells of the origins).  The same bits either way.
 *   sculpt_surface_occlusion  ao [n] f32 of the points P [n][3] with normals N [n][3] under the k directions dirs [k][3] shared
 *                             by all points, 1 <= k <= 1024, in fp32 without contraction: w_j = (n.x d.x + n.y d.y) + n.z d.z;
 *                             direction j takes part iff w_j > 0; its ray runs from p + offset n (the product rounded, then the
 *                             sum) along dirs[j] over [0, max_distance] and is occluded iff sculpt_surface_ray_cast would
 *                             report a face; ao = (sum of w_j of the rays that hit nothing) / (sum of all w_j), both summed in
 *                             the order of j; 1 when no direction takes part; NaN for a non-finite p or n.  records as above
 *                             (always needed with gnf > 0); order [n] or NULL (the points in input order).
 * Null, misaligned or out-of-range arguments are refused with an error code and a message; n == 0 launches nothing. */
int sculpt_surface_ray_cast(const float *O, const float *D, int64_t n, const int64_t *order, const float *GP, const int32_t *GF,
                            int64_t gnf, const float *records, const int32_t *items, const int32_t *start, const double *params_host,
                            double amax, double tmin, double tmax, double *t, int32_t *face, float *uv, sculpt_stream_t stream);
int sculpt_surface_occlusion(const float *P, const float *N, int64_t n, const int64_t *order, const float *dirs, int k, float offset,
                             float max_distance, const float *GP, const int32_t *GF, int64_t gnf, const float *records,
                             const int32_t *items, const int32_t *start, const double *params_host, double amax, float *ao,
                             sculpt_stream_t stream);

/* Wall thickness -- the shape diameter -- of points against the surface of the grid (csrc/mesh_ray.hip "thickness";
 * ops.mesh_thickness, Mesh.thickness, TSR.bake_thickness_map), in one launch.  Added without a version
 * change (a new symbol only).  The grid arguments, records, order and amax are those of sculpt_surface_occlusion.  Per point
 * P[i] with normal N[i], under the cone set cone_dirs [k][3] of unit vectors about +z shared by all points, 1 <= k <= 1024; steps
 * 1 - 3 and 5 - 6 in fp32 without contraction, every operation rounded on its own:
 *   1  m = unit(n): s = (n.x n.x + n.y n.y) + n.z n.z, len = sqrt(s) correctly rounded, n / len per component; it applies only
 *      when 0 < len < inf
 *   2  the frame: sg = copysign(1, m.z), a = -1 / (sg + m.z), b = (m.x m.y) a, T = (1 + (sg (m.x m.x)) a, sg b, -(sg m.x)),
 *      B = (b, sg + (m.y m.y) a, -m.y)
 *   3  o = p - offset m per component (the product rounded, then the difference)
 *   4  per direction j in order: d = (C_j.x T + C_j.y B) - C_j.z m per component; (t, f) = what sculpt_surface_ray_cast reports for
 *      (o, d) over [0, max_distance]; the hit is valid iff a face was hit and, with g = cross(b - a, c - a) of its corners in fp64,
 *      dot(g, d) outward > 0 strictly (the ray leaves through the back of the face); any other ray contributes nothing
 *   5  valid rays only: dist = fp32(t), w = C_j.z, sw += w, swt += w dist (the product rounded, then the sum), thin = min(thin, dist)
 *   6  thickness [n] f32 = swt / sw when a ray was valid, else +inf; thinnest [n] f32 = thin (+inf when none); valid [n] int32 the
 *      number of valid rays
 * A non-finite p or n: NaN, NaN, 0.  A normal to which unit does not apply (zero, overflowing): +inf, +inf, 0, nothing is cast; a
 * surface without faces: the same.  outward is +1 (faces wind counter-clockwise seen from outside) or -1; offset finite,
 * max_distance >= 0 (+inf allowed).  Null, misaligned or out-of-range arguments are refused with an error code and a message;
 * n == 0 launches nothing. */
int sculpt_surface_thickness(const float *P, const float *N, int64_t n, const int64_t *order, const float *cone_dirs, int k, float offset,
                             float max_distance, double outward, const float *GP, const int32_t *GF, int64_t gnf, const float *records,
                             const int32_t *items, const int32_t *start, const double *params_host, double amax, float *thickness,
                             float *thinnest, int32_t *valid, sculpt_stream_t stream);

/* Discrete curvature ON THE DEVICE after Meyer, Desbrun, Schroeder, Barr 2003: the integrated mean and Gaussian curvature per
 * vertex (csrc/mesh_curvature.hip; sf3d/remesh_device.py curvature_device, ops.mesh_curvature, Mesh.curvature,
 * TSR.bake_curvature_map).  DEVICE pointers, asynchronous on `stream`, no host wait.  Added without a
 * version change (new symbols only).  Compiled without floating-point contraction: all arithmetic is fp64 on the fp32 positions in
 * a fixed order (restated in tests/_curvref.py; everything but atan2 to the bit).
 *   sculpt_curvature_terms   per vertex u of the topology (its bnd: sculpt_rmd_boundary on zeroes), the corners of u in vfc order.
 *                            Corner of face (i, j, k) in the face's cyclic order seen from i = u:
 *                                e1 = pj - pi, e2 = pk - pi, g = e1 x e2, a2 = sqrt(g . g); unless 0 < a2 < inf it adds nothing
 *                                di = e1 . e2, dj = (pi - pj) . (pk - pj), dk = (pi - pk) . (pj - pk), cot_j = dj / a2, cot_k = dk / a2
 *                                theta = atan2(a2, di)
 *                                a = ((e1 . e1) cot_k + (e2 . e2) cot_j) / 8 when none of di, dj, dk is < 0 (a right angle is
 *                                    Voronoi), else a2 / 4 when di < 0, else a2 / 8                         (the mixed area)
 *                                A = A + a, Th = Th + theta, Kv = Kv + (cot_k (pi - pj) + cot_j (pi - pk)), N = N + g
 *                            valid [nv] u8 = bnd[u] == 0 and a face names u and A > 0.  area [nv] f64 = A, deficit [nv] f64 =
 *                            6.283185307179586 - Th, hint [nv] f64 = ((outward sign(Kv . N)) sqrt(Kv . Kv)) / 4, the integrated
 *                            mean curvature H A, positive on a convex surface whose faces wind outward (outward = +1; -1 for the
 *                            other winding); an invalid vertex writes zeros.  A pinched vertex whose edges all have two faces
 *                            is valid and gets the deficit of its whole angle sum.  P [nv][3]; work: 16-byte aligned, nv * 4
 *                            floats (positions as x y z - rows).  The faces are trusted to be in range (sculpt_rmd_validate).
 *   sculpt_curvature_ring    `rounds` (0 .. 8) times X'_u = X_u + the sum of X_v over the valid v of row u of the neighbour
 *                            table (start, nb: sculpt_smooth_neighbours), in row order, for the channels hint, deficit and
 *                            area; an invalid u stays zero.  In and out arrays [nv] f64 (out may be in); work_a, work_b: two
 *                            distinct 32-byte aligned buffers of nv * 4 doubles.  nb holds n_nb entries, each in [0, nv):
 *                            the caller's table is trusted, like F.
 *   sculpt_curvature_finish  mean [nv] f32 = (float)(hint / area), gauss [nv] f32 = (float)(deficit / area), NaN where invalid.
 * Null, misaligned or out-of-range arguments are refused with an error code and a message; nv == 0 launches nothing. */
int sculpt_curvature_terms(const sculpt_rmd_topo_t *topo, const float *P, double outward, float *work, double *area, double *deficit,
                           double *hint, uint8_t *valid, sculpt_stream_t stream);
int sculpt_curvature_ring(const int32_t *start, const int32_t *nb, const uint8_t *valid, int64_t nv, int64_t n_nb, int rounds,
                          const double *area, const double *deficit, const double *hint, double *work_a, double *work_b,
                          double *area_out, double *deficit_out, double *hint_out, sculpt_stream_t stream);
int sculpt_curvature_finish(const double *area, const double *deficit, const double *hint, const uint8_t *valid, int64_t nv, float *mean,
                            float *gauss, sculpt_stream_t stream);

/* A value per vertex read at points on a surface (csrc/mesh_curvature.hip; ops.surface_attribute_at): what lets an atlas bake
 * read a high-poly mesh's per-vertex field at its snapped texels.  points [m][3], face [m] (the face each point lies on), P
 * [nv][3], F [nf][3], values [nv][channels] f32, 1 <= channels <= 8 -> out [m][channels] f32.  Per point q on face (a, b, c), in
 * fp64 without contraction: g = (pb - pa) x (pc - pa); w0 = clamp(((pb - q) x (pc - q)) . g / (g . g)),
 * w1 = clamp(((pc - q) x (pa - q)) . g / (g . g)), w2 = clamp((1 - w0) - w1), clamp to [0, 1] by comparisons (a NaN stays).  Per
 * channel s = 0 and s = s + w_k v_k over the corners in order whose value is no NaN, ws the sum of their weights likewise:
 * (float)s when all three count, (float)(s / ws) when one or two do (one border vertex does not blank a texel), NaN when none
 * does.  face < 0 or >= nf, or a corner outside [0, nv): NaN.  m == 0 launches nothing. */
int sculpt_surface_attribute_at(const float *points, const int32_t *face, int64_t m, const float *P, const int32_t *F, int64_t nf,
                                int64_t nv, const float *values, int channels, float *out, sculpt_stream_t stream);

/* Ambient-occlusion bake over a rasterised atlas (csrc/mesh_ray.hip; ops.bake_occlusion, TSR.bake_occlusion_map; DESIGN.md section
 * 3.3h): sculpt_surface_occlusion at every covered texel of the atlas of a LOW mesh (v_pos [nv][3], faces [nf][3] int32 or int64,
 * per-vertex normals v_nrm [nv][3]) against the surface S of the grid (GP, GF, gnf, records, items, start, params_host, amax: as
 * for sculpt_surface_occlusion; records always needed with gnf > 0), in one launch.  Added without a version change (a new symbol
 * only).  Per texel of rast f32 [res][res][4] = (u, v, w, tri), in fp32 without contraction unless said otherwise:
 *   1  not covered (tri negative, NaN, >= nf, or a vertex index outside [0, nv): nothing is read through it): ao = 0, mask = 0
 *   2  p and n: the bits of sculpt_bake_interpolate applied to v_pos and to v_nrm, (a0 u + a1 v) + a2 w per component
 *   3  a non-finite p or n: ao = NaN, mask = 1
 *   4  cage > 0: c = cage n, o = p + c, d = -c; the closest hit (t, f) of sculpt_surface_ray_cast's rule over 0 <= t <= 2.  A hit:
 *      q = fp32(o + t d) (fp64 product and sum, one rounding to fp32); g = cross(b - a, c - a) of f's corners in fp64, negated
 *      when dot(g, n) < 0; m = fp32(g / sqrt(dot(g, g))) when that length is positive and finite, else n.  No hit, or
 *      cage == 0: (q, m) = (p, n)
 *   5  ao = sculpt_surface_occlusion's value at q with normal m under dirs [k][3], offset and max_distance; mask = 1
 * ao f32 [res][res], mask u8 [res][res].  1 <= k <= 1024, cage >= 0 and finite, offset finite, max_distance >= 0, res <= 32768.
 * Null, misaligned (rast and records: 16 bytes) or out-of-range arguments are refused with an error code and a message;
 * res == 0 launches nothing. */
int sculpt_bake_occlusion(const float *rast, int res, const float *v_pos, size_t nv, const void *faces, int faces_i64, size_t nf,
                          const float *v_nrm, const float *dirs, int k, float offset, float max_distance, float cage, const float *GP,
                          const int32_t *GF, int64_t gnf, const float *records, const int32_t *items, const int32_t *start,
                          const double *params_host, double amax, float *ao, uint8_t *mask, sculpt_stream_t stream);

/* Ray-cast views of a mesh with its attributes and baked maps (csrc/mesh_ray.hip; ops.mesh_render, Mesh.render, TSR.render_mesh;
 * DESIGN.md section 3.3i): every ray of rays_o / rays_d f32 [n_images][height][width][3] followed to its closest hit by
 * sculpt_surface_ray_cast's rule over [0, +inf] and the hit shaded, in one launch.  Added without a version change (a new symbol and
 * two structs only).  The grid arguments are those of sculpt_surface_occlusion (records always needed with gnf > 0).  The per-ray
 * rule -- weights, map lookup, albedo, geometric and shading normal, occlusion, the value and the background of every pass -- is
 * the header comment "the mesh render" of csrc/mesh_ray.hip.
 * material: DEVICE pointers, each null when the mesh has none.  uvs [3 gnf][2] per corner; texture [res][res][3], normal_map
 * [res][res][3], occlusion_map [res][res] (row 0 at the top; each needs uvs and its side in 1 .. 32768); corner_normals [3 gnf][3]
 * and corner_tangents [3 gnf][4] (both or neither; given: the normal map is in tangent space, else in object space);
 * vertex_colors [nv][vertex_color_channels] (3 or 4), vertex_normals [nv][3], vertex_occlusion [nv].  The caller vouches for the row
 * counts; map indices are clamped by the rule.
 * out: DEVICE pointers of the pictures to write, null for a pass that is not wanted (at least one is): color, shaded, normal
 * f32 [n][3]; rgba f32 [n][4]; opacity, depth, occlusion f32 [n]; face int32 [n]; n = n_images height width.
 * light: HOST pointer to the unit direction towards the light, or null for a headlight (-d / |d| per ray).  outward: the sign the
 * geometric normal is multiplied by.  height == 1 takes the rays as one row per image.  Null, misaligned (records: 16 bytes) or
 * out-of-range arguments are refused with an error code and a message; no rays launches nothing. */
typedef struct sculpt_render_material {
    const float *uvs, *texture, *normal_map, *corner_normals, *corner_tangents, *occlusion_map, *vertex_colors, *vertex_normals,
        *vertex_occlusion;
    int texture_res, normal_map_res, occlusion_map_res, vertex_color_channels;
} sculpt_render_material;
typedef struct sculpt_render_outputs {
    float *color, *shaded, *opacity, *rgba, *depth, *normal, *occlusion;
    int32_t *face;
} sculpt_render_outputs;
int sculpt_surface_render(const float *rays_o, const float *rays_d, int64_t n_images, int64_t height, int64_t width, const float *GP,
                          const int32_t *GF, int64_t gnf, const float *records, const int32_t *items, const int32_t *start,
                          const double *params_host, double amax, const sculpt_render_material *material, float ambient,
                          const float *light, double outward, const sculpt_render_outputs *out, sculpt_stream_t stream);

/* Mesh vertices onto the iso-surface of the density field (csrc/mesh_project.hip; ops.project_to_isosurface, ops.mesh_unfold,
 * ops.mesh_project).  DEVICE pointers, asynchronous on `stream`, no host wait.  Added without a version
 * change (new symbols only).
 *
 * sculpt_triplane_project: per point a Newton iteration along the gradient of the raw density d (the value and gradient of
 * sculpt_triplane_density_grad, the same bits) towards d(p) = target, in one launch: 8 points x {value, d/dx, d/dy, d/dz} per
 * MFMA tile, the state of the iteration in registers, every point stopping on its own.  fp32, the step without contraction:
 *   an axis a with |p0_a| >= radius is FROZEN: it keeps p0_a bit for bit and its gradient component is taken as 0
 *   1  (d, g) at p = p0, r = d - target; r not finite: status 3, the result is p0.  best = (p0, r)
 *   2  for k < max_steps:  |r| <= res_tol: status 0, stop
 *                          g2 = (gx gx + gy gy) + gz gz on the masked gradient; not > 0 or not finite: status 3, stop
 *                          s = r / g2; q_a = p_a - s g_a; q_a < -radius -> -radius, q_a > radius -> radius; frozen axes restored
 *                          (dx dx + dy dy) + dz dz of q - p0 above max_dist max_dist: status 2, stop
 *                          (d, g) at q, r_q = d - target; not finite: status 3, stop
 *                          p, r, g = q, r_q, g_q; |r| < |best.r|: best = (p, r)
 *   3  out of steps: status 0 if |r| <= res_tol, else 1
 *   points        f32 [N][3]
 *   out_points    f32 [N][3]   best.p (may not alias points)
 *   out_residual  f32 [N]      best.r = d(best.p) - target, nullable
 *   out_status    i32 [N]      0 converged, 1 out of steps, 2 left the trust region, 3 no usable value or gradient; nullable
 *   out_evals     i32 [N]      evaluations the point used, 1 .. max_steps + 1; nullable
 * A point's outputs depend on that point alone.  Refused: what sculpt_triplane_density_grad refuses, max_steps outside 0 .. 64,
 * max_dist or res_tol not positive and finite, a NaN target, a null out_points (with N > 0).  N == 0 is a no-op.
 *
 * sculpt_mesh_unfold: the fold guard.  P0 [Nv][3] the positions before the projection, P [Nv][3] after it (updated in place),
 * faces int64 [Nf][3].  With n0 = (b - a) x (c - a) on P0 and n1 the same on P, a face is INVERTED when n0.n0 > 0 and
 * n0.n1 <= 0 (dots as (x x + y y) + z z, fp32 without contraction; a face with an index outside [0, Nv) is skipped).  `rounds`
 * (0 .. 16) times: every vertex of an inverted face takes its P0 row back.  Then the faces still inverted are counted.
 *   mark_ws  i32 [Nv] workspace (cleared here; 0 untouched, 1 to revert, 2 reverted); may be null with rounds == 0
 *   stats    i32 [2]  (cleared here) vertices reverted, faces still inverted
 * Nv == 0 or Nf == 0 clears stats and launches nothing else.
 * Measured on one MI355X (tools/time_project.py, the 907 205 vertices / 1 680 874 faces of a 256^3 mesh, max_steps 8, warm
 * medians): sculpt_triplane_project 9.17 ms at 2.13 evaluations per vertex (one evaluation of all vertices: 3.06 ms);
 * sculpt_mesh_unfold with 4 rounds 0.24 ms. */
int sculpt_triplane_project(const float *planes_cl /* [3][H][W][C] */, int C, int H, int W, const void *mlp_packed, int n_hidden_64,
                            const float *points /* [N][3] */, long long N, float radius, int flags /* QUERY_ALIGN_CORNERS */,
                            float target, int max_steps, float max_dist, float res_tol, float *out_points /* [N][3] */,
                            float *out_residual /* [N] or null */, int *out_status /* [N] or null */, int *out_evals /* [N] or null */,
                            sculpt_stream_t stream);
int sculpt_mesh_unfold(const float *P0, float *P, const int64_t *faces, int64_t Nv, int64_t Nf, int rounds, int *mark_ws, int *stats,
                       sculpt_stream_t stream);

/* Bake at the surface (csrc/bake_surface.hip; ops.bake_scene_surface): every covered texel of a rasterised
 * UV atlas is first projected from its point on the low-poly face onto the iso-surface d(p) = target of the raw density, and the
 * field's unit normal is read THERE; one launch.  DEVICE pointers, asynchronous on `stream`, no host wait.  Added without a
 * version change (a new symbol only).  Arguments: those of sculpt_bake_scene_normal, then target, max_steps, max_dist, res_tol
 * of sculpt_triplane_project (flags 0).  Per covered texel (the index guard of sculpt_bake_scene_color):
 *   p0 = the texel's position, the bits of sculpt_bake_interpolate;
 *   (point, residual, status, evals) = what sculpt_triplane_project returns for p0 under the same parameters, bit for bit
 *     (the numbered rule above: frozen axes, trust region, best iterate, statuses 0 .. 3);
 *   normal, no frame = the `normal` of sculpt_triplane_density_grad (flags 0) at `point`, bit for bit: the raw gradient of the
 *     evaluation that made `point` the best iterate is kept, no further evaluation is run;
 *   normal, frame given = that world normal through the tangent-space transform of sculpt_bake_scene_normal at the texel's own
 *     barycentrics (the low-poly face and its interpolated frame do not move).
 *   max_steps == 0: point = p0 and normal = sculpt_bake_scene_normal's output, bit for bit, in both spaces.
 * Outputs, each nullable:
 *   point     f32 [res][res][3]     normal  f32 [res][res][3]  in [-1, 1], not encoded
 *   residual  f32 [res][res]        status  i32 [res][res]     evals  i32 [res][res]     mask  u8 [res][res]
 * A texel that is not covered gets point, normal and residual exactly +0, status -1, evals 0, mask 0.  A texel's outputs depend
 * on that texel alone.  Refused: what sculpt_bake_scene_normal refuses (but every output may be null), max_steps outside 0 .. 64,
 * max_dist or res_tol not positive and finite, a NaN target.  res == 0 is a no-op. */
int sculpt_bake_scene_surface(const float *planes_cl /* [3][H][W][C] */, int C, int H, int W, const void *mlp_packed, int n_hidden_64,
                              const float *v_pos /* [nv][3] */, size_t nv, const void *faces /* [nf][3] */, int faces_i64, size_t nf,
                              const float *rast /* [res][res][4] = (u, v, w, tri) or (0,0,0,-1) */, int res, float radius,
                              const float *corner_normals /* nullable [3 nf][3] */, const float *corner_tangents /* nullable [3 nf][4] */,
                              float target, int max_steps, float max_dist, float res_tol, float *point, float *normal, float *residual,
                              int *status, int *evals, uint8_t *mask, sculpt_stream_t stream);

/* Displacement bake (csrc/mesh_project.hip, csrc/bake_displacement.hip; ops.project_along, ops.bake_texel_list,
 * ops.bake_displacement).  DEVICE pointers, asynchronous on `stream`, no host wait.  Added without a
 * version change (new symbols only).
 *
 * sculpt_triplane_project_along: per point a safeguarded Newton search for d(p0 + s n) = target along the line through p0 with
 * the unit direction n = N / sqrt(N.N), in sculpt_triplane_project's tile (the value and gradient of
 * sculpt_triplane_density_grad, the same bits).  fp32, the rule without contraction:
 *   0  N.N = (x x + y y) + z z not finite or not > 0: status 3, height +0, residual +0, evals 0.  s = +0, no bracket
 *   for k = 0 .. max_steps:
 *   1  q_a = p0_a + s n_a; (d, g) at q; r = d - target
 *   2  r not finite: status 3, stop (at k == 0 the best iterate is (0, r))
 *   3  k == 0 or |r| < |best.r|: best = (s, r)
 *   4  |r| <= res_tol: status 0, stop.  k == max_steps: status 1, stop
 *   5  r < 0: a = s.  r > 0: b = s
 *   6  gn = (gx nx + gy ny) + gz nz; c = s - r / gn; c < -max_dist -> -max_dist, then c > max_dist -> max_dist (comparisons)
 *   7  a and b both set and c not strictly inside (min(a, b), max(a, b)): c = 0.5 (a + b)
 *   8  c not finite: status 3, stop.  c == s: status 2, stop
 *   9  any |p0_a + c n_a| > radius: status 2, stop
 *   10 s = c
 *   points, directions  f32 [N][3]
 *   count        device int32 or null: the number of points is min(max(*count, 0), N), read on the device; rows past it are
 *                neither read nor written
 *   scatter      int32 [N] or null: result i is stored at row scatter[i] (a row outside 0 .. out_rows is dropped) instead of i
 *   out_rows     the rows of the outputs; must be N without a scatter list
 *   out_height   f32  best.s: signed, world units, positive along n        out_residual  f32  best.r, nullable
 *   out_status   i32  0 converged, 1 out of steps, 2 left the trust region (|s| <= max_dist and the box), 3 no usable value,
 *                gradient or direction; nullable                           out_evals     i32  0 .. max_steps + 1, nullable
 * A point's outputs depend on that point alone.  Refused: what sculpt_triplane_project refuses.  N == 0 is a no-op.
 *
 * sculpt_bake_texel_list: the covered texels of rast (tri >= 0 and the index guard of sculpt_bake_scene_color) as flat indices
 * in row-major order -- torch.nonzero of the coverage, by per-block counts and scans, no atomics -- and their number in *count.
 *   workspace   sculpt_bake_texel_list_workspace_bytes(res) bytes
 *   list        i32 [res res]   rows 0 .. *count - 1 are written
 *   p0          f32 [res res][3], nullable: per listed texel its position, the bits of sculpt_bake_interpolate
 *   directions  f32 [res res][3], nullable (needs normals f32 [nv][3]): per listed texel (N0 u + N1 v) + N2 w of the per-vertex
 *               normals at the face's corners, un-normalised, fp32 without contraction
 *   mask        u8 [res][res], nullable: 1 covered, 0 not
 *   height, residual f32, status, evals i32 [res][res], each nullable: written for texels that are NOT covered only, with what
 *               sculpt_triplane_project_along (scatter = list, count = count) leaves out: +0, +0, -1, 0
 * res == 0 stores *count = 0 and launches nothing else. */
size_t sculpt_bake_texel_list_workspace_bytes(int res);
int sculpt_bake_texel_list(const float *v_pos /* [nv][3] */, size_t nv, const void *faces /* [nf][3] */, int faces_i64, size_t nf,
                           const float *normals /* nullable [nv][3] */, const float *rast /* [res][res][4] */, int res, void *workspace,
                           int *list, int *count, float *p0, float *directions, uint8_t *mask, float *height, float *residual,
                           int *status, int *evals, sculpt_stream_t stream);
int sculpt_triplane_project_along(const float *planes_cl /* [3][H][W][C] */, int C, int H, int W, const void *mlp_packed,
                                  int n_hidden_64, const float *points /* [N][3] */, const float *directions /* [N][3] */, long long N,
                                  const int *count /* device, nullable */, float radius, int flags /* QUERY_ALIGN_CORNERS */, float target,
                                  int max_steps, float max_dist, float res_tol, const int *scatter /* [N] or null */, long long out_rows,
                                  float *out_height, float *out_residual /* or null */, int *out_status /* or null */,
                                  int *out_evals /* or null */, sculpt_stream_t stream);

/* UV CHART ATLAS ON THE DEVICE (csrc/uv_charts.hip; sf3d/unwrap.py ChartUnwrapper; restated in tests/_chartref.py): charts that
 * are connected pieces of surface, shelf-packed.  DEVICE pointers, asynchronous on `stream`.  Compiled without floating-point
 * contraction; every fp64 operation below is one IEEE operation on the fp32 inputs widened exactly.  Integer atomics only: two
 * calls give the same bits.  P f32 [nv][3] finite, F int32 [nf][3] in range (the caller validates: sculpt_rmd_validate).
 * THE RULE, per round (the caller repeats 2 .. 6 until a round evicts nothing, at most 8 rounds; layer starts at 0):
 * 1 DIRECTION  a, b, c = the face's corners.  n = cross(b - a, c - a) in fp64 (differences, then products, then one subtraction
 *              per component: n_x = u_y v_z - u_z v_y, n_y = u_z v_x - u_x v_z, n_z = u_x v_y - u_y v_x).  k = the axis of the
 *              largest |n_k|, ties to the lowest k; d = 2 k + (n_k < 0).  Per corner (p, q) = (v[(k + 1) % 3], v[(k + 2) % 3]),
 *              swapped when n_k < 0: fp32 bits, unchanged.  n = 0 gives d = 0.  A non-degenerate face has positive area in (p, q).
 * 2 CHARTS     The half-edges 3 f + j (F[f][j] -> F[f][(j + 1) % 3]) sorted by their undirected key (min << 32 | max), as the
 *              remesh passes sort them (sculpt_rmd_halfedge_keys, a stable sort).  Two faces are joined when their key occurs
 *              exactly twice, the two half-edges start at different vertices (opposite directions), the faces differ, have the
 *              same d, the same layer, and that layer is < max_layers (a face at max_layers is a "single": never joined).
 *              Lock-free union-find over the faces (the scheme of csrc/mesh_components.hip): label[f] = the smallest face index
 *              of f's chart, exact.  chart[f] = the rank of label[f] among the roots in ascending order; n_charts = the roots.
 * 3 RECTANGLES per chart the fp32 minimum and maximum of p and of q over its corners (atomicMin / atomicMax on the ordered-float
 *              key of csrc/block_scan.h: -0 orders below +0) -> rect = (pmin, pmax, qmin, qmax).  w = (double)pmax - (double)pmin,
 *              h likewise.  h > w: the chart is TURNED, (p', q') = (q - qmin, pmax - p) and (w, h) swap; else (p - pmin, q - qmin).
 *              extent = (w, h) after the turn, w >= h.  sort_key = -(the int64 bits of h); slots >= n_charts get INT64_MAX, rect 0.
 *              (caller: order = the stable ascending argsort of sort_key: h descending, chart ids ascending among equals.)
 * 4 PACK       g = the gutter in UV units (the caller passes island_padding / 8).  Q(s, e) = (int64)ceil((s * e + g) * 2^20).
 *              At scale s, in sorted order j: Wq = Q(s, w), Hq = Q(s, h); cum[j] = the sum of Wq before j.  A row that starts at
 *              `start` holds the charts j >= start with cum[j + 1] - cum[start] <= 2^20; its height is Hq[start]; rows stack from
 *              y = 0.  s is FEASIBLE when every Wq <= 2^20 and the row heights sum to <= 2^20.  Search: w_max = m 2^e (0.5 <= m
 *              < 1, frexp) gives s0 = 2^(1 - e) (so 1 <= s0 w_max < 2); w_max = 0 gives s0 = 1.  s = s0, halved while infeasible
 *              (more than 80 halvings: error, the atlas cannot hold that many gutters).  If s0 itself was feasible it is taken.
 *              Otherwise t = 2 s, then up to 11 times t = t * 0.9375, taking the first feasible t; if none, s.  cell[c] = (x, y)
 *              of chart c's cell in units of 2^-20: x = cum[j] - cum[start of its row], y = the row's y.  One workgroup: the
 *              scans run over its 1024 threads, the row walk is one thread with a binary search in cum per row.
 * 5 PLACE      per corner u = fp32((x 2^-20 + 0.5 g) + s p'), v = fp32((y 2^-20 + 0.5 g) + s q'), p' and q' the fp64 differences
 *              of 3.  Corners of one chart that share a vertex get the same bits.
 * 6 CONFLICTS  rast_low = sculpt_bake_rasterize of uv with the faces in order, rast_high = with the face list reversed (triangle
 *              t' there is face nf - 1 - t').  At every texel both cover with different faces lo < hi, the sample point is the
 *              rasteriser's: px = fp32(x) / fp32(res), py = 1 - fp32(y) / fp32(res) in fp32.  In fp64, for a face with UV corners
 *              A, B, C: e0 = (Bx - Ax)(py - Ay) - (By - Ay)(px - Ax), e1 and e2 likewise from (B, C) and (C, A); the sample is
 *              STRICTLY inside when all three are > 0 or all three < 0.  Strictly inside both: evicted[hi] = 1,
 *              chart_conflict[chart[lo]] = chart_conflict[chart[hi]] = 1.  sculpt_uv_chart_evict then, mode 0: layer[f] += 1
 *              where evicted[f]; mode 1 (the caller's 8th round): layer[f] = max_layers for every face of a chart with
 *              chart_conflict set, and nothing else; mode 2: layers untouched.  All modes count the evicted faces.
 * The workspace (sculpt_uv_chart_workspace_bytes, 0 for nf out of [0, 2^24): the rasteriser carries face ids in fp32) starts
 * with eight int64 words the caller may copy to the host after any call: n_charts, evicted faces, error bits (1: a union-find
 * walk left its step budget, 2: no feasible scale), rows, scale evaluations, the scale (fp64 bits), conflicting texels, 0.
 * sculpt_uv_chart_label starts a round: it clears those words.  Arrays: direction, layer, label, chart, evicted,
 * chart_conflict int32 [nf]; pq f32 [nf][3][2]; rect f32 [nf][4]; extent f64 [nf][2]; sort_key, order int64 [nf];
 * cell int64 [nf][2]; uv f32 [3 nf][2].  nf == 0 launches nothing.  Null arguments are refused with an error code. */
size_t sculpt_uv_chart_workspace_bytes(int64_t n_faces);
int sculpt_uv_chart_directions(const float *P, int64_t nv, const int32_t *F, int64_t nf, int32_t *direction, float *pq,
                               sculpt_stream_t stream);
int sculpt_uv_chart_label(const int64_t *skeys /* [3 nf] sorted */, const int64_t *sperm /* [3 nf] half-edge ids in that order */,
                          const int32_t *F, int64_t nf, const int32_t *direction, const int32_t *layer, int max_layers, int32_t *label,
                          void *workspace, sculpt_stream_t stream);
int sculpt_uv_chart_rects(const float *pq, const int32_t *label, int64_t nf, int32_t *chart, float *rect, double *extent,
                          int64_t *sort_key, void *workspace, sculpt_stream_t stream);
int sculpt_uv_chart_pack(const int64_t *order, const double *extent, int64_t nf, double gutter, int64_t *cell, void *workspace,
                         sculpt_stream_t stream);
int sculpt_uv_chart_place(const float *pq, const int32_t *chart, const float *rect, const int64_t *cell, int64_t nf, double gutter,
                          const void *workspace, float *uv, sculpt_stream_t stream);
int sculpt_uv_chart_conflicts(const float *rast_low /* [res][res][4] */, const float *rast_high, int res, const float *uv,
                              const int32_t *chart, int64_t nf, int32_t *evicted, int32_t *chart_conflict, void *workspace,
                              sculpt_stream_t stream);
int sculpt_uv_chart_evict(const int32_t *evicted, const int32_t *chart_conflict, const int32_t *chart, int64_t nf, int max_layers,
                          int mode, int32_t *layer, void *workspace, sculpt_stream_t stream);

/* Mesh hand-off, HOST side (no GPU work): the face block of a binary little-endian PLY file -- per face `uchar 3` followed by
 * three int32 -- from the int64 faces TSR.run returns (the reference's `t_pos_idx.cpu().numpy()`, TripoSR/tsr/system.py:200).
 * faces_host int64 [n][3] -> records_host uint8 [n][13].  Thread-safe; callers split n over threads (sculptmate_amd/meshio.py). */
int sculpt_ply_face_records(const int64_t *faces_host, size_t n, uint8_t *records_host);

#ifdef __cplusplus
}
#endif
#endif /* SCULPT_HIP_H */
