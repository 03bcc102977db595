"""TSR -- the TripoSR system behind SculptMate's "lean" generator, MI355X-native.

Mirrors the surface of /root/reference/TripoSR/tsr/system.py::TSR that the add-on uses
(SURVEY.md section 8b): from_pretrained, renderer.set_chunk_size, to(device), __call__/forward,
extract_mesh, plus a headless run() that returns meshes.  All arithmetic of the hot path runs in
libsculpt_hip.so (hand-written HIP, gfx950); torch only owns HBM buffers and streams.

Pipeline per image (reference file:line):
  ImagePreprocessor (host)                          tsr/utils.py:62-112
  DINOSingleImageTokenizer = ViT-B/16, 1025 tokens  tsr/models/tokenizers/image.py:41-60
  Triplane1DTokenizer tokens [1024, 3072]           tsr/models/tokenizers/triplane.py:29-45
  Transformer1D, 16 blocks                          tsr/models/transformer/transformer_1d.py:179-219
  TriplaneUpsampleNetwork -> scene code [3,40,64,64] tsr/models/network_utils.py:24-32
  extract_mesh: density grid -> marching cubes      tsr/system.py:171-200
  render: spherical cameras -> ray kernel           tsr/utils.py:339-397, tsr/models/nerf_renderer.py:93-172
"""
import math
import os
from typing import List, Optional

import numpy as np
import torch

from .. import _lib, ops
from ..engine import KernelEngine, prepare_ln_linear
from .posemb import interpolate_pos_embedding
from .cameras import get_spherical_cameras
from . import passes as render_pass_rules
from .mesh import TENSOR_FIELDS, Mesh, PendingMesh, _PinnedLease, _PinnedPool, _host, _mesh_pass_to_pil  # noqa: F401
from .utils import ImagePreprocessor

BF16 = torch.bfloat16
LOG2E = 1.4426950408889634

from .spec import DEFAULT_CFG, IMAGE_MEAN, IMAGE_STD, param_spec  # noqa: E402,F401


_MC_SIGN_PLANES = not _lib.form_has("SCULPT_MC_FORM", "noplanes")   # A/B: the plain count phase over the whole volume


class PendingTokens:
    """The image tokens of one image, being computed on the tokenizer stream (TSR.tokens_async)."""

    __slots__ = ("ctx", "ready", "_slot", "image")

    def __init__(self, ctx, ready, slot, image=None):
        self.ctx, self.ready, self._slot, self.image = ctx, ready, slot, image


class MarchingCubeHelper:
    """tsr/models/isosurface.py:17-54 on the GPU (sculpt_mc_*)."""

    points_range = (0, 1)

    def __init__(self, resolution: int):
        self.resolution = resolution
        self._grid_vertices = None

    @property
    def grid_vertices(self) -> torch.Tensor:
        """[R^3, 3] lattice in [0,1] (isosurface.py:25-39).  Only built if somebody asks for it: the
        dense query generates positions from the separable axis table instead (no 201 MB tensor)."""
        if self._grid_vertices is None:
            R = self.resolution
            x = torch.linspace(*self.points_range, R)
            x, y, z = torch.meshgrid(x, x, x, indexing="ij")
            self._grid_vertices = torch.cat([x.reshape(-1, 1), y.reshape(-1, 1), z.reshape(-1, 1)], dim=-1)
        return self._grid_vertices

    def __call__(self, level: torch.Tensor):
        """level = -(density - threshold) as the reference passes it; returns (v_pos in [0,1], faces int64)."""
        R = self.resolution
        vol = (-level).reshape(R, R, R).contiguous()
        return ops.marching_cubes(vol, 0.0, reference_order=True, vert_div=R - 1.0, vert_mul=1.0, vert_add=0.0)


class TriplaneNeRFRenderer:
    """tsr/models/nerf_renderer.py:17-172: the point query of the mesh path and the volume renderer, each one fused launch
    (sculpt_triplane_query_ex, sculpt_render_rays)."""

    def __init__(self, cfg):
        self.cfg = type("Cfg", (), dict(cfg))()
        assert cfg.get("feature_reduction", "concat") == "concat"
        assert cfg.get("density_activation", "exp") == "exp"
        assert cfg.get("color_activation", "sigmoid") == "sigmoid"
        self.num_samples_per_ray = int(cfg.get("num_samples_per_ray", 128))
        self.randomized = bool(cfg.get("randomized", False))
        self.chunk_size = 0

    def set_chunk_size(self, chunk_size: int):
        assert chunk_size >= 0, "chunk_size must be a non-negative integer (0 for no chunking)."
        self.chunk_size = chunk_size  # kept for API parity; the fused kernel needs no chunking

    def query_triplane(self, decoder, positions, triplane):
        triplane = triplane.contiguous()
        if positions.numel() >= 3 * 4096:  # many points (vertex colours): channel-last taps, ~20x fewer cache lines
            triplane = ops.ChannelLastPlanes(triplane)
        return ops.triplane_query(triplane, decoder, positions, radius=self.cfg.radius,
                                  density_bias=self.cfg.density_bias)

    def query_normals(self, decoder, positions, triplane):
        """Outward unit normals of the density field at `positions` [..., 3]: -grad / |grad| of the raw density that
        query_triplane returns (ops.field_normals); exactly 0 where the gradient is 0.  triplane: [3, C, H, W] or an
        ops.ChannelLastPlanes."""
        if not isinstance(triplane, ops.ChannelLastPlanes):
            triplane = triplane.contiguous()
        return ops.field_normals(triplane, decoder, positions, radius=self.cfg.radius)["normal"]

    def _forward(self, decoder, triplane, rays_o, rays_d):
        if self.randomized:
            raise NotImplementedError("TriplaneNeRFRenderer: randomized=True (jittered samples, a training option) is not "
                                      "implemented; the ray kernel places samples at the interval midpoints")
        dev = triplane.data.device if isinstance(triplane, ops.ChannelLastPlanes) else triplane.device
        rgb, _ = ops.render_rays(triplane, decoder, rays_o.to(dev), rays_d.to(dev), radius=self.cfg.radius,
                                 density_bias=self.cfg.density_bias, n_samples=self.num_samples_per_ray)
        return rgb

    def forward(self, decoder, triplane, rays_o, rays_d):
        """nerf_renderer.py:154-172 -> comp_rgb with the rays' leading shape.  triplane: [3, C, H, W] (or an
        ops.ChannelLastPlanes) with rays [..., 3] for one scene; [B, 3, C, H, W] with rays [B, ..., 3] for a stack."""
        if isinstance(triplane, ops.ChannelLastPlanes) or triplane.ndim == 4:
            return self._forward(decoder, triplane, rays_o, rays_d)
        return torch.stack([self._forward(decoder, triplane[i], rays_o[i], rays_d[i]) for i in range(triplane.shape[0])], dim=0)

    __call__ = forward

    def render_passes(self, decoder, triplane, rays_o, rays_d, passes=("color", "opacity", "depth", "normal")):
        """forward with passes beside the colour picture -> {pass: tensor with the rays' leading shape} for the passes of
        tsr/passes.py ("color" [..., 3] is forward's picture bit for bit, "opacity" [...], "rgba" [..., 4] premultiplied, "depth"
        [...], "normal" [..., 3] in world space).  One launch per scene (ops.render_passes): the ray kernel, or, only when "normal"
        is asked for, its forward-mode form.  triplane and rays as in forward."""
        if self.randomized:
            raise NotImplementedError("TriplaneNeRFRenderer: randomized=True (jittered samples, a training option) is not "
                                      "implemented; the ray kernel places samples at the interval midpoints")
        passes = render_pass_rules.check_passes(passes)
        if not (isinstance(triplane, ops.ChannelLastPlanes) or triplane.ndim == 4):
            each = [self.render_passes(decoder, triplane[i], rays_o[i], rays_d[i], passes) for i in range(triplane.shape[0])]
            return {p: torch.stack([e[p] for e in each], dim=0) for p in passes}
        dev = triplane.data.device if isinstance(triplane, ops.ChannelLastPlanes) else triplane.device
        rgb, extras = ops.render_passes(triplane, decoder, rays_o.to(dev), rays_d.to(dev), radius=self.cfg.radius,
                                        density_bias=self.cfg.density_bias, n_samples=self.num_samples_per_ray,
                                        want=render_pass_rules.wanted(passes))
        return render_pass_rules.finish(passes, rgb, extras)


def _atlas_resolution(resolution, mesh, caller, maps):
    """The resolution of a bake over `mesh`'s atlas: the one given; else, on a mesh that has uvs, the size of the first of
    `maps` it carries; else 2048.  Below 1: ValueError in the caller's name."""
    if resolution is None:
        sized = [getattr(mesh, name) for name in maps if mesh.uvs is not None and getattr(mesh, name) is not None]
        resolution = sized[0].shape[0] if sized else 2048
    res = int(resolution)
    if res < 1:
        raise ValueError("TSR.%s: resolution must be positive" % caller)
    return res


def _bf(x, dev):
    return torch.as_tensor(x).to(device=dev, dtype=BF16).contiguous()


def _f32(x, dev):
    return torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()


class TSR(KernelEngine):
    def __init__(self, cfg=None, pos_embed_mode="scale_factor", precision="bf16", decoder_precision="bf16l3", decoder_filter=True):
        """precision: "bf16" (BASELINE config 2: bf16 storage, fp32 accumulate -- what bench.py times),
        "fp32" (parity mode: the whole transformer on the exact-fp32 matrix pipe, like the fp32 reference), or
        "bf16l3" (the fast parity mode: fp32 storage, norms and softmax as in "fp32", every matrix product on the bf16 matrix pipe
        with both operands split exactly into three bf16 limbs and fp32 accumulation -- fp32-equivalent, csrc/gemm_l3.hip), or
        "fp16l2" ("bf16l3" with the Linears of the two transformers on TWO fp16 limbs per operand, 22 significant bits, three
        products per multiply: fp32-equivalent on this model -- scene code 1e-6 from the fp32 reference like "fp32" itself -- at
        two thirds of the time; an activation beyond 65504 in magnitude makes the scene code non-finite: forward() then repeats the
        call on a "bf16l3" twin of the model and counts it in range_fallbacks).
        decoder_precision: how the 64x64 hidden layers of the dense density query (extract_mesh's 256^3 grid) are evaluated.
          "bf16l3" (default): fp32-equivalent -- both operands split EXACTLY into three bf16 limbs (24 significant bits, fp32
                   exponent range), six exact products per weight on the bf16 matrix pipe, fp32 accumulation; no range
                   limit and no fallback; measured error against the CPU oracle = the fp32 kernel's own.
          "fp32":  the exact-fp32 MFMA kernel (a k-ordered fmaf chain, 1.5x slower): the parity mode.
        decoder_filter (default True; applies to decoder_precision "bf16l3"): extract_mesh evaluates the dense grid in two passes
          (csrc/density_filter.hip) -- every lattice point with one 16-bit product per hidden layer, then the three-limb arithmetic at
          all corners of every cell that can be active -- which gives the mesh of the full evaluation bit for bit as long as no coarse
          error reaches the calibrated margin (8 x the largest error measured on a 64^3 probe of the first scene code); every call is
          guarded by the largest coarse error seen at the re-evaluated points and redone in full when that exceeds a third of the
          margin (filter_info counts both).  False: every lattice point with the three-limb arithmetic."""
        if precision not in ("bf16", "fp32", "bf16l3", "fp16l2"):
            raise ValueError("precision must be 'bf16', 'fp32', 'bf16l3' or 'fp16l2'")
        if decoder_precision not in ("fp32", "bf16l3"):
            raise ValueError("decoder_precision must be 'bf16l3' or 'fp32'")
        self.decoder_precision = decoder_precision
        self.decoder_filter = bool(decoder_filter)
        # state of the two-pass density grid: margin (None = not calibrated yet), coarse operand type, counters
        self.filter_info = {"margin": None, "coarse": "fp16", "usable": True, "calibrations": 0, "filtered": 0, "fallbacks": 0,
                            "last": None}
        self.cfg = cfg or DEFAULT_CFG
        self.pos_embed_mode = pos_embed_mode
        self.precision = precision
        self.l3p = False   # set by _prepare: the three-limb mode with operands split once (engine.py)
        self.range_fallbacks = 0   # fp16l2: forward() calls redone on three bf16 limbs because an activation left the fp16 range
        self._range_twin = None    # the "bf16l3" model those calls run on (built on first need from the current weights)
        self.adt = BF16 if precision == "bf16" else torch.float32  # activation / weight storage type
        self._spec = param_spec(self.cfg)
        self._sd = None
        self.device = None
        self.renderer = TriplaneNeRFRenderer(self.cfg["renderer"])
        self.image_processor = ImagePreprocessor()
        self.isosurface_helper = None
        self.decoder = None  # ops.PackedMLP after to(device)
        self.mesh_sink = None  # callable(verts, faces, colors, name); default: bpy if importable
        self.textured_mesh_sink = None  # callable(verts, faces, uvs, image, name) for baked meshes; default: bpy if importable
        self._unwrapper = None  # the cached BoxProjectionUnwrapper of bake_texture
        self.atlas = "box"  # "box" | "charts": which unwrapper _atlas makes when none is passed (see the class-level default)
        # None | "tangent" | "object": when set, extract_meshes adds a normal map (bake_normal_map) to every mesh it bakes a
        # texture for, at the texture's resolution, and extract_mesh hands it to the textured sink
        self.normal_map = None
        # None | what ops.occlusion_rule accepts (True, k, (k, max_distance)): when set, extract_meshes adds an ambient-occlusion
        # map (bake_occlusion_map) to every mesh it bakes a texture for, over the texture's atlas at its resolution, against the
        # mesh as it entered simplify (when simplify is given; else against itself).  _reshaped leaves that mesh in
        # _occlusion_source for _textured, which takes it out again.
        self.occlusion_map = None
        self._occlusion_source = None
        # forward(): images per transformer pass.  1 (default): image by image.  > 1: the reference's batched pass
        # (system.py:82-115) over stacked token rows; in the bf16 mode it gives each image the bits of its single-image pass
        # (every GEMM keeps the single-image tile form: encode_images), which is why run() batches by default there
        self.max_batch = 1
        # A stacked pass keeps the tile forms of the single-image pass (True: each image gets the scene code of its own pass bit for
        # bit; bf16 mode) or takes the forms that are fastest for the stacked rows (False: round 4-5 behaviour -- 0.7 ms per image
        # faster at four images, scene codes 2.7e-3 from the single-image ones: bf16 roundings flip in the LayerNorm statistics)
        self.batch_exact = True
        self._w = None
        self._head0 = None   # _backbone_head_cached
        self._pos_cache = {}
        self._buf = {}

    # ------------------------------------------------------------------ loading
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, config_name: str, weight_name: str, **model_kwargs):
        """system.py:51-66.  config.yaml is read with PyYAML (the ${tokenizer.num_channels}
        interpolation is resolved by hand); ViT hyper-parameters come from checkpoints/config.json.
        model_kwargs (beyond the reference's signature): TSR's own keyword arguments -- precision="bf16" | "bf16l3" | "fp32",
        decoder_precision, decoder_filter, pos_embed_mode."""
        if not os.path.isdir(pretrained_model_name_or_path):
            raise FileNotFoundError("Checkpoint directory given doesnt exist")
        cfg = load_config(os.path.join(pretrained_model_name_or_path, config_name),
                          os.path.join(pretrained_model_name_or_path, "config.json"))
        model = cls(cfg, **model_kwargs)
        ckpt = torch.load(os.path.join(pretrained_model_name_or_path, weight_name), map_location="cpu")
        model.load_state_dict(ckpt)
        return model

    def state_dict(self):
        return dict(self._sd or {})

    def load_state_dict(self, sd, strict=True):
        sd = {k: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k, v in sd.items()}
        missing = [k for k in self._spec if k not in sd]
        unexpected = [k for k in sd if k not in self._spec]
        if strict and (missing or unexpected):
            raise RuntimeError("Error(s) in loading state_dict for TSR: missing %s unexpected %s"
                               % (missing[:5], unexpected[:5]))
        for k, shp in self._spec.items():
            if k in sd and tuple(sd[k].shape) != tuple(shp):
                raise RuntimeError("size mismatch for %s: %s vs %s" % (k, tuple(sd[k].shape), shp))
        self._sd = {k: sd[k].detach().to(torch.float32) for k in self._spec if k in sd}
        # state derived from the previous weights: the fp16l2 range twin, the two-pass grid's calibration
        self._range_twin = None
        self.filter_info.update(margin=None, usable=True, last=None)
        if self.device is not None:
            self._prepare(self.device)
        return self

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.SculptError("TSR runs on an MI355X only (device %s requested; there is no CPU fallback)" % device)
        self.device = device
        if self._sd is not None:
            self._prepare(device)
        return self

    # ------------------------------------------------------------------ weight preparation
    def _prepare(self, dev):
        sd, cfg = self._sd, self.cfg
        wt = _bf if self.precision == "bf16" else _f32  # GEMM weight storage
        # "limbs once" (engine.py): in the three-limb mode the Linears of the two transformers keep their weights split
        # (the attention must be the fused kernel: the three-launch composition has no limb output)
        # A/B forms (tests): SCULPT_ATTN_FORM=l3unfused = the three-launch composition of the limb attention; SCULPT_L3_TILE=split =
        # every GEMM splits its operands while staging (the form before limbs-once)
        fused_attn = not _lib.form_has("SCULPT_ATTN_FORM", "l3unfused")
        self.l3p = self.precision == "fp16l2" or (self.precision == "bf16l3" and not _lib.form_has("SCULPT_L3_TILE", "split") and fused_attn)
        if self.l3p:
            # sculpt_gemm_l3p's tiles: N % 128 == 0 (N % 64 per GEGLU half), K % 32 == 0 for every Linear kept as limbs.  A model
            # with other widths runs "bf16l3" on the splitting GEMM (csrc/gemm_l3.hip: N % 4), as it did before limbs-once.
            vv, bb = cfg["image_tokenizer"], cfg["backbone"]
            Hh, Ii = vv["hidden_size"], vv["intermediate_size"]
            Dd = bb["num_attention_heads"] * bb["attention_head_dim"]
            bad = [n for n, ok in (("image_tokenizer.hidden_size", Hh % 128 == 0), ("image_tokenizer.intermediate_size", Ii % 128 == 0),
                                   ("backbone width", Dd % 128 == 0), ("backbone.cross_attention_dim", bb["cross_attention_dim"] % 32 == 0))
                   if not ok]
            if self.precision == "fp16l2":
                if bad or not fused_attn:
                    raise ValueError("precision='fp16l2' needs Linear widths the limb GEMM tiles (multiples of 128; cross-attention "
                                     "width a multiple of 32) and the fused limb attention (SCULPT_L3_ATTN_FUSED unset): "
                                     + (", ".join(bad) or "SCULPT_ATTN_FORM=l3unfused"))
            elif bad:
                self.l3p = False
        self.limb_format = "f16x2" if self.precision == "fp16l2" else "bf16x3"
        fmt = self.limb_format
        wh = (lambda x, d, geglu=False: ops.Limbs.of(_f32(ops.geglu_row_blocks(torch.as_tensor(x)) if geglu else x, d), fmt=fmt,
                                                     weight=True)) if self.l3p else (lambda x, d, geglu=False: wt(x, d))
        v, b = cfg["image_tokenizer"], cfg["backbone"]
        H = v["hidden_size"]
        w = {}
        p = "image_tokenizer.model."
        w["patch_w"] = wt(sd[p + "embeddings.patch_embeddings.projection.weight"].reshape(H, -1), dev)
        w["patch_b"] = _f32(sd[p + "embeddings.patch_embeddings.projection.bias"], dev)
        w["cls"] = _f32(sd[p + "embeddings.cls_token"].reshape(H), dev)
        fold = self.precision == "bf16"

        def ln_linear(L, key, W, bias, gamma, beta, q_rows=0, q_scale=1.0, geglu=False):
            """A Linear fed by a LayerNorm (engine.prepare_ln_linear): folded into the GEMM in bf16 mode."""
            prepare_ln_linear(L, key, W, bias, gamma, beta, fold, lambda x: wh(x, dev, geglu), lambda x: _f32(x, dev), q_rows, q_scale)

        w["vit"] = []
        for i in range(v["num_hidden_layers"]):
            q = p + "encoder.layer.%d." % i
            L = {}
            ln_linear(L, "qkv_w", torch.cat([sd[q + "attention.attention.%s.weight" % n] for n in ("query", "key", "value")], 0),
                      torch.cat([sd[q + "attention.attention.%s.bias" % n] for n in ("query", "key", "value")], 0),
                      sd[q + "layernorm_before.weight"], sd[q + "layernorm_before.bias"], q_rows=H,
                      q_scale=LOG2E / math.sqrt(H // v["num_attention_heads"]))
            L["o_w"], L["o_b"] = wh(sd[q + "attention.output.dense.weight"], dev), _f32(sd[q + "attention.output.dense.bias"], dev)
            ln_linear(L, "f1_w", sd[q + "intermediate.dense.weight"], sd[q + "intermediate.dense.bias"],
                      sd[q + "layernorm_after.weight"], sd[q + "layernorm_after.bias"])
            L["f2_w"], L["f2_b"] = wh(sd[q + "output.dense.weight"], dev), _f32(sd[q + "output.dense.bias"], dev)
            w["vit"].append(L)
        w["vit_ln_w"], w["vit_ln_b"] = _f32(sd[p + "layernorm.weight"], dev), _f32(sd[p + "layernorm.bias"], dev)

        t = cfg["tokenizer"]
        C, S = t["num_channels"], t["plane_size"]
        emb = sd["tokenizer.embeddings"]  # [3, C, S, S]
        emb_ct = emb.permute(1, 0, 2, 3).reshape(C, 3 * S * S).contiguous()  # "Np Ct Hp Wp -> Ct (Np Hp Wp)"
        w["emb_ct"] = _f32(emb_ct, dev)
        w["emb_tc"] = _f32(emb_ct.t().contiguous(), dev)  # residual in token-major layout
        w["gn_w"], w["gn_b"] = _f32(sd["backbone.norm.weight"], dev), _f32(sd["backbone.norm.bias"], dev)
        w["pin_w"], w["pin_b"] = wt(sd["backbone.proj_in.weight"], dev), _f32(sd["backbone.proj_in.bias"], dev)
        w["pout_w"], w["pout_b"] = wt(sd["backbone.proj_out.weight"], dev), _f32(sd["backbone.proj_out.bias"], dev)
        w["blocks"] = []
        for i in range(b["num_layers"]):
            q = "backbone.transformer_blocks.%d." % i
            L = {}
            Db, qs = b["num_attention_heads"] * b["attention_head_dim"], LOG2E / math.sqrt(b["attention_head_dim"])
            ln_linear(L, "sa_qkv", torch.cat([sd[q + "attn1.to_q.weight"], sd[q + "attn1.to_k.weight"], sd[q + "attn1.to_v.weight"]], 0),
                      None, sd[q + "norm1.weight"], sd[q + "norm1.bias"], q_rows=Db, q_scale=qs)
            L["sa_o"], L["sa_ob"] = wh(sd[q + "attn1.to_out.0.weight"], dev), _f32(sd[q + "attn1.to_out.0.bias"], dev)
            ln_linear(L, "ca_q", sd[q + "attn2.to_q.weight"], None, sd[q + "norm2.weight"], sd[q + "norm2.bias"], q_rows=Db, q_scale=qs)
            L["_ca_k"], L["_ca_v"] = sd[q + "attn2.to_k.weight"], sd[q + "attn2.to_v.weight"]
            L["ca_o"], L["ca_ob"] = wh(sd[q + "attn2.to_out.0.weight"], dev), _f32(sd[q + "attn2.to_out.0.bias"], dev)
            ln_linear(L, "ff1", sd[q + "ff.net.0.proj.weight"], sd[q + "ff.net.0.proj.bias"], sd[q + "norm3.weight"], sd[q + "norm3.bias"],
                      geglu=True)
            L["ff2"], L["ff2_b"] = wh(sd[q + "ff.net.2.weight"], dev), _f32(sd[q + "ff.net.2.bias"], dev)
            w["blocks"].append(L)
        # the cross-attention K/V projections of ALL layers depend only on the image tokens: one GEMM
        # [Tc, 768] x [L*2*D, 768]^T per image, rows ordered [K of layer 0..L-1 | V of layer 0..L-1]
        w["ca_kv_all"] = wh(torch.cat([L.pop("_ca_k") for L in w["blocks"]] + [L.pop("_ca_v") for L in w["blocks"]], 0), dev)
        # ConvTranspose2d(k2,s2) as a GEMM: rows (co,dy,dx), K = Cin; rows padded to a multiple of 128
        up = sd["post_processor.upsample.weight"]  # [Cin, Co, 2, 2]
        Co = up.shape[1]
        rows = up.permute(1, 2, 3, 0).reshape(4 * Co, up.shape[0])
        npad = ((4 * Co + 127) // 128) * 128
        upw = torch.zeros(npad, up.shape[0])
        upw[: 4 * Co] = rows
        w["up_w"], w["up_b"] = wt(upw, dev), _f32(sd["post_processor.upsample.bias"], dev)
        self._w = w
        d = cfg["decoder"]
        n = d["n_hidden_layers"] + 1
        self.decoder = ops.PackedMLP([sd["decoder.layers.%d.weight" % (2 * i)] for i in range(n)],
                                     [sd["decoder.layers.%d.bias" % (2 * i)] for i in range(n)], dev)
        self._pos_cache = {}
        self._buf = {}
        self._head0 = None   # the cached head of the backbone belongs to the weights (and the precision / limb format) just replaced

    def _pos(self, n_side, dev):
        if n_side not in self._pos_cache:
            pe = self._sd["image_tokenizer.model.embeddings.position_embeddings"].numpy()
            self._pos_cache[n_side] = _f32(interpolate_pos_embedding(pe, n_side, self.pos_embed_mode), dev)
        return self._pos_cache[n_side]

    # ------------------------------------------------------------------ forward
    @staticmethod
    def _token_stride(T, B):
        """Rows from one image's tokens to the next in a stacked batch: T itself for one image, else T rounded up to 8 so that
        every image's rows (and its V^T columns) start 16-byte aligned; the pad rows carry finite values nobody reads."""
        return T if B == 1 else ((T + 7) // 8) * 8

    def image_tokens(self, image_hwc):
        """DINOSingleImageTokenizer.forward (tokenizers/image.py:41-60) for one [S,S,3] fp32 device image, or for a LIST of B
        such images in one pass (the reference's batch dimension, system.py:82-99): every Linear is one launch over the stacked
        token rows, the attention one launch over B x heads -> (ctx bf16 [rows, H] for cross attention, ctx fp32 [rows, H]);
        image b's T tokens are rows b*Ts .. b*Ts+T-1, Ts = _token_stride(T, B)."""
        imgs = list(image_hwc) if isinstance(image_hwc, (list, tuple)) else [image_hwc]
        B = len(imgs)
        v, w = self.cfg["image_tokenizer"], self._w
        H, P, nh = v["hidden_size"], v["patch_size"], v["num_attention_heads"]
        S = imgs[0].shape[0]
        if any(tuple(im.shape) != tuple(imgs[0].shape) for im in imgs):
            raise ValueError("TSR.image_tokens: the images of a batch must have one size")
        n_side = S // P
        npatch = n_side * n_side
        T = npatch + 1
        Ts = self._token_stride(T, B)
        M = B * Ts
        ldt = ((((B - 1) * Ts + ((T + 63) // 64) * 64) + 63) // 64) * 64   # V^T columns: image b at column b*Ts
        patches = self._b("patches", (B * npatch, 3 * P * P), self.adt)
        for b, im in enumerate(imgs):
            ops.vit_patchify(im, P, IMAGE_MEAN, IMAGE_STD, patches[b * npatch:(b + 1) * npatch])
        pout = self._b("patch_out", (B * npatch, H), torch.float32)
        self._gemm(patches, w["patch_w"], bias=w["patch_b"], out_f32=pout)
        h = self._b("vit_h", (M, H), torch.float32, zero=True)
        pos = self._pos(n_side, imgs[0].device)
        st = self._stream_state("vit", h)     # the residual stream + its bf16 copy + slice statistics (LayerNorm fold)
        if B == 1 and self.precision == "bf16":   # one image: the rows, their bf16 copy and statistics in one launch (the same bits)
            ops.vit_assemble_stats(pout, w["cls"], pos, h, st["stats"], st["hb"])
        else:
            for b in range(B):
                ops.vit_assemble(pout[b * npatch:(b + 1) * npatch], w["cls"], pos, h[b * Ts:b * Ts + T])
                if Ts > T:   # the pad rows of the stacked stream take part in every Linear: start them from zero on every call, or
                    h[b * Ts + T:(b + 1) * Ts].zero_()   # they drift without bound in a long-running process
            self._stats_of(st)                # rows that do not come out of a GEMM: one small kernel
        qk = self._b("vit_qk", (M, 2 * H), self.adt)
        vt = self._b("vit_vt", (H, ldt), self.adt, zero=True)
        if self.l3p:   # read only by the next Linear: written as limbs by their producers
            att, ff = self._lt("vit_att", M, H), self._lt("vit_ff", M, v["intermediate_size"])
        else:
            att = self._b("vit_att", (M, H), self.adt, zero=True)
            ff = self._b("vit_ff", (M, v["intermediate_size"]), self.adt)
        eps = v["layer_norm_eps"]
        for L in w["vit"]:
            self._ln_gemm(st, L, "qkv_w", eps, out_bf16=qk, out_t=vt, n_split=2 * H)  # Q|K token-major, V^T
            self._attn(qk[:, :H], qk[:, H:], vt, att, T, T, nh, self._attn_scale(1.0 / math.sqrt(H // nh)),
                       B, Ts * 2 * H, Ts * 2 * H, Ts, Ts * H)
            self._res_gemm(st, att, L["o_w"], L["o_b"])
            self._ln_gemm(st, L, "f1_w", eps, out_bf16=ff, epilogue=_lib.EPI_GELU)
            self._res_gemm(st, ff, L["f2_w"], L["f2_b"])
        ctx32 = self._b("ctx32", (M, H), torch.float32)
        if self.precision == "bf16":
            ctx = self._b("ctx", (M, H), BF16)
            ops.layernorm(h, w["vit_ln_w"], w["vit_ln_b"], eps, y=ctx, y_f32=ctx32)
        elif self.l3p:   # the cross-attention K / V projection reads the tokens as limbs
            ctx = self._lt("ctx", M, H)
            ops.layernorm(h, w["vit_ln_w"], w["vit_ln_b"], eps, y_lt=ctx, y_f32=ctx32)
        else:
            ops.layernorm(h, w["vit_ln_w"], w["vit_ln_b"], eps, y_f32=ctx32)
            ctx = ctx32
        return ctx, ctx32

    def _attn_scale(self, scale):
        """bf16 mode: the query projections carry scale * log2(e) (ln_linear q_scale) -> sculpt_attention_bf16_prescaled (scale None)."""
        return None if self.precision == "bf16" else scale

    def _self_attention(self, st, L, batch=1):
        """h += attn1(LN1(h)) of one BasicTransformerBlock (basic_transformer_block.py:149-167); h holds `batch` images' tokens
        stacked (attention.py:629-631 with its leading batch dimension)."""
        b = self.cfg["backbone"]
        nh, hd = b["num_attention_heads"], b["attention_head_dim"]
        D, M = nh * hd, st["h"].shape[0]
        T = M // batch
        # V^T columns: entry b is read at column b * T for round64(T) columns (the same formula as ldc / ldt below: ADVICE r4)
        Mp = ((((batch - 1) * T + ((T + 63) // 64) * 64) + 63) // 64) * 64
        qk = self._b("bb_qk", (M, 2 * D), self.adt)
        vt = self._b("bb_vt", (D, Mp), self.adt, zero=True)
        att = self._lt("bb_att", M, D) if self.l3p else self._b("bb_att", (M, D), self.adt)
        self._ln_gemm(st, L, "sa_qkv", 1e-5, out_bf16=qk, out_t=vt, n_split=2 * D)  # one launch: Q|K token-major, V^T
        self._attn(qk[:, :D], qk[:, D:], vt, att, T, T, nh, self._attn_scale(1.0 / math.sqrt(hd)),
                   batch, T * 2 * D, T * 2 * D, T, T * D)
        self._res_gemm(st, att, L["sa_o"], L["sa_ob"])

    def _run_blocks(self, st, ctx: torch.Tensor, first_self_attention_done: bool = False, batch: int = 1, ctx_tokens=None, head=None):
        """All BasicTransformerBlocks on the fp32 residual stream h [batch*T, D] (updated in place).  ctx [rows, cross_dim]: the
        image tokens, image b's ctx_tokens rows starting at row b * (rows // batch) (image_tokens' stacking).
        head (_backbone_head_cached()): block 0 starts at its cross-attention, from the cached queries; its residual GEMM reads the
        cached stream and writes st's (one image), or st already holds copies of it (a stacked pass: _broadcast_state)."""
        b, w = self.cfg["backbone"], self._w
        nh, hd = b["num_attention_heads"], b["attention_head_dim"]
        D = nh * hd
        if self.l3p and not isinstance(ctx, ops.Limbs):   # tokens handed over as a plain fp32 matrix (backbone_tokens): split here
            ctx = ops.Limbs.of(ctx.to(torch.float32).contiguous(), fmt=self.limb_format)
        M, Mc = st["h"].shape[0], (ctx.rows if isinstance(ctx, ops.Limbs) else ctx.shape[0])
        T, Ts = M // batch, Mc // batch
        Tc = Ts if ctx_tokens is None else ctx_tokens
        ldc = ((((batch - 1) * Ts + ((Tc + 63) // 64) * 64) + 63) // 64) * 64
        q = self._b("bb_q", (M, D), self.adt)
        nL = len(w["blocks"])
        ck_all = self._b("bb_ck", (Mc, nL * D), self.adt)
        cvt_all = self._b("bb_cvt", (nL * D, ldc), self.adt, zero=True)
        self._gemm(ctx, w["ca_kv_all"], out_bf16=ck_all, out_t=cvt_all, n_split=nL * D, M=Mc)
        if self.l3p:
            att, ff = self._lt("bb_att", M, D), self._lt("bb_ff", M, 4 * D)
        else:
            att = self._b("bb_att", (M, D), self.adt)
            ff = self._b("bb_ff", (M, 4 * D), self.adt)
        scale = self._attn_scale(1.0 / math.sqrt(hd))
        for li, L in enumerate(w["blocks"]):
            ck, cvt = ck_all[:, li * D:(li + 1) * D], cvt_all[li * D:(li + 1) * D]
            if li == 0 and head is not None:
                if batch == 1:
                    self._attn(head["q0"], ck, cvt, att, T, Tc, nh, scale)
                    self._res_gemm(st, att, L["ca_o"], L["ca_ob"], residual=head["h0"])   # out of place: the cache is never written
                else:
                    q.view(batch, T, D).copy_(head["q0"][None])
                    self._attn(q, ck, cvt, att, T, Tc, nh, scale, batch, T * D, Ts * nL * D, Ts, T * D)
                    self._res_gemm(st, att, L["ca_o"], L["ca_ob"])
            else:
                if li > 0 or not first_self_attention_done:
                    self._self_attention(st, L, batch)
                self._ln_gemm(st, L, "ca_q", 1e-5, out_bf16=q)
                self._attn(q, ck, cvt, att, T, Tc, nh, scale, batch, T * D, Ts * nL * D, Ts, T * D)
                self._res_gemm(st, att, L["ca_o"], L["ca_ob"])
            self._ln_gemm(st, L, "ff1", 1e-5, out_bf16=ff, epilogue=_lib.EPI_GEGLU)
            self._res_gemm(st, ff, L["ff2"], L["ff2_b"])
        return st

    def _backbone_head(self):
        """The part of Transformer1D.forward that does not depend on the image: GroupNorm of the learned triplane tokens,
        proj_in (transformer_1d.py:181-189) and the first block's self-attention."""
        b, w = self.cfg["backbone"], self._w
        D = b["num_attention_heads"] * b["attention_head_dim"]
        T = w["emb_ct"].shape[1]
        xn = self._b("bb_xn", (T, w["emb_ct"].shape[0]), self.adt)
        stats = self._b("gn_stats", (2 * b["norm_num_groups"],), torch.float32)
        ops.groupnorm_tokens(w["emb_ct"], b["norm_num_groups"], w["gn_w"], w["gn_b"], 1e-6, xn, stats)
        h = self._b("bb_h", (T, D), torch.float32)
        st = self._stream_state("bb", h)
        if self.precision == "bf16":
            ops.gemm(xn, w["pin_w"], bias=w["pin_b"], out_f32=h, out_bf16=st["hb"], stats_out=st["stats"])
        else:
            self._gemm(xn, w["pin_w"], bias=w["pin_b"], out_f32=h)
        return st

    def _backbone_head_cached(self):
        """Everything in front of block 0's cross-attention depends on the weights alone: _backbone_head, the first block's
        self-attention and its cross-attention query projection (7 launches in bf16 mode).  Computed once per prepared model, at
        the first forward, with the kernels and operands a forward would use -- the same bits -- and kept in buffers of their
        own that no forward writes: h0 (+ hb0, stats0 in bf16 mode) and q0.  _prepare drops it (load_state_dict, to(), a change of
        precision or limb format all go through there)."""
        key = (self.precision, self.limb_format, self.l3p)
        hc = self._head0
        if hc is not None and hc["key"] == key:
            return hc
        with ops.single_image_tiles(0):   # (a caller's stacked-pass tile choice does not apply to this one-image work)
            st = self._backbone_head()
            L = self._w["blocks"][0]
            self._self_attention(st, L)
            q = self._b("bb_q", st["h"].shape, self.adt)
            self._ln_gemm(st, L, "ca_q", 1e-5, out_bf16=q)
        hc = {"key": key, "h0": st["h"].clone(), "q0": q.clone()}
        if self.precision == "bf16":
            hc["hb0"], hc["stats0"] = st["hb"].clone(), st["stats"].clone()
        # once per model: later forwards read the cache from any stream (the tokenizer's, a caller's) without an event of its own
        torch.cuda.current_stream(self.device).synchronize()
        self._head0 = hc
        return hc

    def _head_state(self, hc):
        """The work state of one image's pass: block 0's residual GEMM fills it from the cached stream."""
        return self._stream_state("bb", self._b("bb_h", tuple(hc["h0"].shape), torch.float32))

    def _backbone_tail(self, st, batch=1):
        w = self._w
        C = self.cfg["tokenizer"]["num_channels"]
        h = st["h"]
        M, D = h.shape
        res = w["emb_tc"]                       # the learned tokens: the same residual rows for every image of a batch
        if batch > 1:
            key = "emb_tc_x%d" % batch
            if key not in w:
                w[key] = res.repeat(batch, 1).contiguous()
            res = w[key]
        out = self._b("bb_out", (M, C), torch.float32)
        if self.precision == "bf16":
            outb = self._b("bb_outb", (M, C), BF16)
            ops.gemm(st["hb"], w["pout_w"], bias=w["pout_b"], residual=res, out_f32=out, out_bf16=outb)  # hb = bf16(h)
        else:
            ops.gemm_f32(h, w["pout_w"], bias=w["pout_b"], residual=res, out=out, l3=self.l3)
            outb = out
        return out, outb

    def _broadcast_state(self, hc, batch):
        """The cached residual stream of ONE image (the image-independent head of the backbone) copied into a stacked state of `batch`."""
        T, D = hc["h0"].shape
        st = self._stream_state("bb", self._b("bb_h", (batch * T, D), torch.float32))
        st["h"].view(batch, T, D).copy_(hc["h0"][None])
        if self.precision == "bf16":
            st["hb"].view(batch, T, D).copy_(hc["hb0"][None])
            st["stats"].view(-1, batch, T, 2).copy_(hc["stats0"][:, None])
        return st

    def encode_images(self, images):
        """encode_image for a batch (system.py:82-115 with batch_size = len(images)): ONE pass of the tokenizer and the backbone
        over the stacked token rows of all images -- weight panels are read once per batch, every Linear is one launch of
        B x 3072 (B x 1025) rows, every attention one launch over B x heads.  The image-independent head of the backbone
        (GroupNorm, proj_in, first self-attention, first query projection) comes from the per-model cache and is copied into
        the B streams.  Returns the output tokens of all images stacked: (fp32 [B*3*S*S, C], bf16 copy)."""
        B = len(images)
        if B == 1:
            return self.encode_image(images[0])
        main = torch.cuda.current_stream(self.device)
        last_tok = getattr(self, "_tok_last", None)
        if last_tok is not None:
            main.wait_event(last_tok)
        hc = self._backbone_head_cached()
        # Every GEMM of the pass picks the tile form ONE image takes (ops.single_image_tiles): the stacked pass then accumulates every
        # output and every LayerNorm slice statistic in the single-image order, and each image gets the scene code of its own pass,
        # bit for bit (test_full_size_batched_forward_equals_single_image_passes) -- which is what lets TSR.run batch by default.
        T = self.cfg["image_tokenizer"]
        n_side = images[0].shape[0] // T["patch_size"]
        with ops.single_image_tiles(n_side * n_side + 1 if self.batch_exact else 0):
            ctx, _ = self.image_tokens(list(images))
        st = self._broadcast_state(hc, B)
        with ops.single_image_tiles(3 * self.cfg["tokenizer"]["plane_size"] ** 2 if self.batch_exact else 0):
            st = self._run_blocks(st, ctx, batch=B, ctx_tokens=n_side * n_side + 1, head=hc)
            return self._backbone_tail(st, B)

    def backbone_tokens(self, ctx: torch.Tensor):
        """Triplane1DTokenizer + Transformer1D for one image; ctx bf16 [Tc, cross_dim].
        Returns the output tokens token-major: fp32 [3*S*S, C] (+ bf16 copy)."""
        hc = self._backbone_head_cached()
        st = self._run_blocks(self._head_state(hc), ctx, head=hc)
        return self._backbone_tail(st)

    def encode_image(self, image_hwc: torch.Tensor):
        """image_tokens + backbone_tokens for one [S,S,3] fp32 device image on the current stream.  (Until the head of the backbone
        was cached per model, it was issued here on a second HIP stream under the ViT.)"""
        main = torch.cuda.current_stream(self.device)
        last_tok = getattr(self, "_tok_last", None)
        if last_tok is not None:  # tokens_async shares the tokenizer's work buffers: finish it first
            main.wait_event(last_tok)
        hc = self._backbone_head_cached()
        ctx, _ = self.image_tokens(image_hwc)
        st = self._run_blocks(self._head_state(hc), ctx, head=hc)
        return self._backbone_tail(st)

    def _preprocess(self, im) -> torch.Tensor:
        """ImagePreprocessor (tsr/utils.py:62-112): uint8 / PIL -> float / 255 on the host, then the antialiased bilinear resize
        to cond_image_size on the GPU (sculpt_resize_aa_bilinear)."""
        size = self.cfg["cond_image_size"]
        img = self._upload(_to_float_hwc(im)).contiguous()
        if img.shape[-1] != 3:
            raise ValueError("TSR.forward expects RGB images (composite RGBA on grey first, preprocessing.py:122)")
        if img.shape[0] != size or img.shape[1] != size:
            img = ops.resize_aa_bilinear(img, size)
        return img

    def tokens_async(self, image) -> PendingTokens:
        """Upload + ImagePreprocessor + DINO image tokenizer of ONE image, queued on a second HIP stream.  The tokenizer is
        ~1.0 ms of launches of 72 - 200 workgroups that leave most CUs idle; queued here for image i + 1 before the backbone,
        density grid and marching cubes of image i are queued on the current stream, it runs beside them (11.40 -> 11.08 ms per
        image, tools/try_vit_prefetch.py) -- same kernels on the same operands, bit-identical tokens.  The tokens land in one
        of two slots; a slot is rewritten only after the backbone that read it has been through (forward_tokens)."""
        if self._w is None:
            raise _lib.SculptError("TSR: call load_state_dict() and to(device) before tokens_async()")
        tok = getattr(self, "_tok_stream", None)
        if tok is None:
            tok = self._tok_stream = torch.cuda.Stream(self.device)
            self._tok_ring = {"i": 0, "slots": [{"ctx": None, "consumed": None} for _ in range(2)]}
        slot = self._tok_ring["slots"][self._tok_ring["i"] % 2]
        self._tok_ring["i"] += 1
        main = torch.cuda.current_stream(self.device)
        fork = torch.cuda.Event()
        fork.record(main)  # a serial forward() queued earlier uses the same tokenizer buffers on the current stream
        with torch.cuda.stream(tok), torch.no_grad():
            tok.wait_event(fork)
            if slot["consumed"] is not None:
                tok.wait_event(slot["consumed"])
            ctx, _ = self.image_tokens(self._preprocess(image))
            if isinstance(ctx, ops.Limbs):   # three-limb mode, limbs once: the tokens travel as limbs
                if not isinstance(slot["ctx"], ops.Limbs) or (slot["ctx"].rows, slot["ctx"].cols, slot["ctx"].fmt) != (ctx.rows, ctx.cols, ctx.fmt):
                    slot["ctx"] = ops.Limbs(ctx.rows, ctx.cols, data=torch.empty_like(ctx.data), fmt=ctx.fmt)
                slot["ctx"].data.copy_(ctx.data)
            else:
                if not isinstance(slot["ctx"], torch.Tensor) or slot["ctx"].shape != ctx.shape or slot["ctx"].dtype != ctx.dtype:
                    slot["ctx"] = torch.empty_like(ctx)
                slot["ctx"].copy_(ctx)
            ready = torch.cuda.Event()
            ready.record(tok)
        self._tok_last = ready
        return PendingTokens(slot["ctx"], ready, slot, image)

    def forward_tokens(self, tokens: PendingTokens) -> torch.Tensor:
        """The rest of forward() for one image whose tokens come from tokens_async: backbone + upsampler on the current stream
        -> scene code fp32 [1, 3, 40, 64, 64]."""
        main = torch.cuda.current_stream(self.device)
        main.wait_event(tokens.ready)
        hc = self._backbone_head_cached()
        st = self._run_blocks(self._head_state(hc), tokens.ctx, head=hc)
        consumed = torch.cuda.Event()
        consumed.record(main)
        tokens._slot["consumed"] = consumed
        _, outb = self._backbone_tail(st)
        out = self.scene_code(outb)[None]
        if self.precision == "fp16l2" and tokens.image is not None and not bool(torch.isfinite(out).all()):
            return self._range_fallback([tokens.image])   # forward()'s range fallback: straight to the three-limb twin
        return out

    def scene_code(self, tokens_bf16: torch.Tensor, batch: int = 1):
        """detokenize + TriplaneUpsampleNetwork: tokens [batch*3*S*S, C] -> planes fp32 [3, Co, 2S, 2S] ([batch, 3, ...] for batch > 1)."""
        w = self._w
        S = self.cfg["tokenizer"]["plane_size"]
        Co = self.cfg["post_processor"]["out_channels"]
        g = self._b("up_g", (tokens_bf16.shape[0], w["up_w"].shape[0]), torch.float32)
        self._gemm(tokens_bf16, w["up_w"], out_f32=g)
        planes = torch.empty((batch, 3, Co, 2 * S, 2 * S), dtype=torch.float32, device=tokens_bf16.device)
        T = tokens_bf16.shape[0] // batch
        for b in range(batch):
            ops.upsample_scatter(g[b * T:(b + 1) * T], w["up_b"], planes[b], S, Co)
        return planes if batch > 1 else planes[0]

    def _upload(self, t: torch.Tensor) -> torch.Tensor:
        """Host image -> HBM without blocking the host: a pageable source makes hipMemcpyAsync synchronous (the host waits for
        the stream to drain and for the copy), so it is first copied into one of three pinned staging buffers (a 3 MB host
        memcpy) and sent from there; a slot is reused once the copy that read it has completed."""
        if t.device.type != "cpu":
            return t.to(self.device, non_blocking=True)
        if t.is_pinned():
            return t.to(self.device, non_blocking=True)
        ring = getattr(self, "_stage", None)
        if ring is None:
            ring = self._stage = {"i": 0, "slots": [[None, None] for _ in range(3)]}
        slot = ring["slots"][ring["i"] % 3]
        ring["i"] += 1
        n = t.numel()
        if slot[1] is not None:
            slot[1].synchronize()
        if slot[0] is None or slot[0].numel() < n:
            slot[0] = torch.empty(max(n, 3 * 512 * 512), dtype=torch.float32, pin_memory=True)
        stage = slot[0][:n].view(t.shape)
        # a plain single-threaded memcpy: torch's CPU copy_ is an OpenMP parallel_for, and waking the (sleeping) worker threads of
        # a 256-core host once per image costs ~20 ms -- measured: 11.4 -> 31 ms per step
        np.copyto(stage.numpy(), t.numpy() if t.is_contiguous() else t.contiguous().numpy())
        d = stage.to(self.device, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(self.device))
        return d

    def forward(self, image, device=None) -> torch.Tensor:
        """system.py:82-115: image(s) -> scene_codes fp32 [B, 3, 40, 64, 64] on the device."""
        if self._w is None:
            if device is not None and self._sd is not None:
                self.to(device)
            else:
                raise _lib.SculptError("TSR: call load_state_dict() and to(device) before forward()")
        images = [self._preprocess(im) for im in _as_image_list(image)]
        codes = []
        step = max(1, int(self.max_batch))
        for i in range(0, len(images), step):
            group = images[i:i + step]
            n_tok = 3 * self.cfg["tokenizer"]["plane_size"] ** 2   # a batch entry's rows / V^T columns must start 16-byte aligned
            if len(group) == 1 or n_tok % 8 or any(tuple(g.shape) != tuple(group[0].shape) for g in group):
                for im in group:
                    _, outb = self.encode_image(im)
                    codes.append(self.scene_code(outb)[None])
            else:   # the reference's batched pass (system.py:82-115)
                _, outb = self.encode_images(group)
                with ops.single_image_tiles(n_tok if self.batch_exact else 0):   # the upsampler's GEMM too (encode_images)
                    codes.append(self.scene_code(outb, len(group)))
        out = torch.cat(codes, 0) if len(codes) > 1 else codes[0]
        if self.precision == "fp16l2" and not bool(torch.isfinite(out).all()):
            # an fp16 limb overflowed (an activation of 65504 or more in magnitude) or the input was not finite: never hand on a
            # silently wrong scene code -- the same images go through a three-limb twin of this model ("bf16l3": the fp32 exponent
            # range), built on first need; range_fallbacks counts the calls that needed it
            return self._range_fallback(image)
        return out

    def _range_fallback(self, image):
        """fp16l2: the images of a call whose scene code came out non-finite, through the "bf16l3" twin of this model (built from the
        CURRENT weights on first need; load_state_dict drops it)."""
        self.range_fallbacks += 1
        twin = self._range_twin
        if twin is None:
            twin = self._range_twin = TSR(self.cfg, self.pos_embed_mode, precision="bf16l3", decoder_precision=self.decoder_precision,
                                          decoder_filter=self.decoder_filter)
            twin.load_state_dict(self._sd)
            twin.to(self.device)
        twin.max_batch = self.max_batch
        return twin.forward(image)

    __call__ = forward

    # ------------------------------------------------------------------ previews
    def _need_weights(self, caller):
        if self.decoder is None:
            raise _lib.SculptError("TSR.%s: the model has no weights on a device yet (load_state_dict + to(device))" % caller)

    def _field(self, scene_code, channel_last=True):
        """The scene code as the kernels take it: an ops.ChannelLastPlanes as it is; a tensor [3, C, H, W] (or [1, 3, C, H, W]: the
        leading 1 is dropped) on the model's device and, with channel_last, made into an ops.ChannelLastPlanes (one launch)."""
        if isinstance(scene_code, ops.ChannelLastPlanes):
            return scene_code
        if scene_code.ndim == 5 and scene_code.shape[0] == 1:
            scene_code = scene_code[0]
        scene_code = scene_code.to(self.device)
        return ops.ChannelLastPlanes(scene_code) if channel_last else scene_code

    def _turntable_rays(self, n_views, elevation_deg, camera_distance, fovy_deg, height, width):
        """The cameras of render, render_passes and render_mesh (get_spherical_cameras) on the device -> (rays_o, rays_d)."""
        rays_o, rays_d = get_spherical_cameras(n_views, elevation_deg, camera_distance, fovy_deg, height, width)
        return rays_o.to(self.device, non_blocking=True), rays_d.to(self.device, non_blocking=True)

    def render(self, scene_codes, n_views: int, elevation_deg: float = 0.0, camera_distance: float = 1.9, fovy_deg: float = 40.0,
               height: int = 256, width: int = 256, return_type: str = "pt"):
        """Upstream TripoSR's `model.render`: turntable pictures straight from the scene codes -> per scene code a list of n_views pictures.
        return_type "pt": float32 [height, width, 3] tensors on the device (nothing is synchronised); "np": float32 arrays;
        "pil": PIL images of (x * 255) truncated to uint8.  All views of one scene code are one launch of the ray kernel, over
        planes converted to channel-last once."""
        if return_type not in ("pt", "np", "pil"):
            raise ValueError("return_type must be 'pt', 'np' or 'pil'")
        self._need_weights("render")
        rays_o, rays_d = self._turntable_rays(n_views, elevation_deg, camera_distance, fovy_deg, height, width)
        images = []
        with torch.no_grad():
            for code in scene_codes:
                planes = self._field(code)
                views = self.renderer(self.decoder, planes, rays_o, rays_d)
                if return_type == "pt":
                    images.append(list(views.unbind(0)))
                    continue
                host = views.cpu().numpy()
                if return_type == "np":
                    images.append([host[i] for i in range(n_views)])
                else:
                    from PIL import Image

                    images.append([Image.fromarray((host[i] * 255.0).astype(np.uint8)) for i in range(n_views)])
        return images

    def render_passes(self, scene_codes, n_views: int, elevation_deg: float = 0.0, camera_distance: float = 1.9,
                      fovy_deg: float = 40.0, height: int = 256, width: int = 256,
                      passes=("color", "opacity", "depth", "normal"), return_type: str = "pt"):
        """render with passes beside the colour picture -> per scene code a list of n_views dicts {pass: picture}.  passes: any of
        "color" ([height, width, 3], render's picture bit for bit), "opacity" ([height, width]: what the ray absorbed, the mask of
        the others), "rgba" ([height, width, 4], premultiplied: a cut-out to lay over a backdrop), "depth" ([height, width]:
        distance from the camera, 0 where opacity is 0, noisy where it is small) and "normal" ([height, width, 3]: unit normals of
        the density field in world space, 0 where there is none) -- tsr/passes.py has the rules.  return_type as render; "pil"
        gives RGB / L / RGBA with straight alpha / mode F / RGB of n * 0.5 + 0.5.  Only what the passes need is computed: the
        field's gradient (4.5 x the time of the picture alone) only for "normal".  Unknown or no passes: ValueError, before
        anything is launched."""
        passes = render_pass_rules.check_passes(passes)
        if return_type not in render_pass_rules.RETURN_TYPES:
            raise ValueError("return_type must be 'pt', 'np' or 'pil'")
        self._need_weights("render_passes")
        rays_o, rays_d = self._turntable_rays(n_views, elevation_deg, camera_distance, fovy_deg, height, width)
        images = []
        with torch.no_grad():
            for code in scene_codes:
                planes = self._field(code)
                views = self.renderer.render_passes(self.decoder, planes, rays_o, rays_d, passes)
                images.append(render_pass_rules.convert(views, return_type))
        return images

    def render_mesh(self, mesh: Mesh, n_views: int, elevation_deg: float = 0.0, camera_distance: float = 1.9, fovy_deg: float = 40.0,
                    height: int = 256, width: int = 256, passes=("color",), return_type: str = "pt", ambient: float = 0.3,
                    light=None):
        """Turntable pictures of the finished MESH -- what extract_meshes, simplify and the bakes produced, as an engine that
        loads the exported asset would show it -- under the cameras of render and render_passes: pixel (i, j) of view k is
        the same ray in all three.  -> a list of n_views dicts {pass: picture}.  passes: any of "color" ([height, width, 3]:
        texture, else vertex colours, else grey, unlit on white: the counterpart of render's picture), "shaded" (lit by a
        headlight, or from `light`, the direction towards a fixed light; `ambient` is the share the occlusion scales),
        "opacity", "rgba" (premultiplied), "depth", "normal" (the normal map decoded through the exported frame, in world
        space), "occlusion" and "face" (int32 [height, width], -1 off the mesh) -- Mesh.render / ops.mesh_render have the rules.
        return_type as render_passes: "pt" (device tensors, nothing is synchronised beyond the index build), "np" or "pil"
        (occlusion as L, face as mode I, the others as tsr/passes.py makes them).  Needs a device, no weights.  All views are one
        launch over one index of the mesh.  Unknown or no passes: ValueError, before anything is launched."""
        passes = ops.mesh_render_passes(passes)
        if return_type not in render_pass_rules.RETURN_TYPES:
            raise ValueError("return_type must be 'pt', 'np' or 'pil'")
        if self.device is None:
            raise _lib.SculptError("TSR.render_mesh: the model is on no device yet (to(device))")
        rays_o, rays_d = self._turntable_rays(n_views, elevation_deg, camera_distance, fovy_deg, height, width)
        on_device = mesh._derive(_f32(mesh.vertices, self.device), torch.as_tensor(mesh.faces).to(self.device).contiguous(),
                                 normal_map_space=mesh.normal_map_space,
                                 **{name: None if getattr(mesh, name) is None else _f32(getattr(mesh, name), self.device) for name in TENSOR_FIELDS})
        with torch.no_grad():
            views = on_device.render(rays_o, rays_d, passes=passes, ambient=ambient, light=light, outward=self.WINDING_OUTWARD)
        if return_type == "pt":
            return render_pass_rules.convert(views, "pt")
        host = [{p: v.cpu().numpy() for p, v in view.items()} for view in render_pass_rules.convert(views, "pt")]
        if return_type == "np":
            return host
        return [{p: _mesh_pass_to_pil(p, v) for p, v in view.items()} for view in host]

    def field_normals(self, points, scene_code):
        """Outward unit normals of the density field of `scene_code` ([3, C, H, W] or an ops.ChannelLastPlanes) at `points`
        [..., 3] in world units: -grad / |grad| of the raw density, one launch (ops.field_normals) -> f32 [..., 3] on the
        device, exactly 0 where the gradient is 0 (a point outside the scene's box on every axis)."""
        self._need_weights("field_normals")
        scene_code = self._field(scene_code, channel_last=False)   # the renderer takes the plain tensor
        with torch.no_grad():
            return self.renderer.query_normals(self.decoder, _f32(points, self.device), scene_code)

    # ------------------------------------------------------------------ mesh extraction
    def set_marching_cubes_resolution(self, resolution: int):
        if self.isosurface_helper is not None and self.isosurface_helper.resolution == resolution:
            return
        self.isosurface_helper = MarchingCubeHelper(resolution)

    def bake_texture(self, mesh: Mesh, scene_code, texture_resolution: int = 2048, island_padding: float = 0.02, unwrapper=None) -> Mesh:
        """Upstream TripoSR's --bake-texture: unwrap `mesh`, query the colour field of `scene_code` ([3, C, H, W]) once per
        covered texel, pad the charts -> a Mesh with the same vertices and faces, vertex_colors None, uvs f32 [3*Nf, 2] per face
        corner (origin bottom-left) and texture f32 [res, res, 3] (row 0 at the top), all on the device.
        Stages: ops.vertex_normals -> unwrapper(v_pos, v_nrm, faces, island_padding) (default: one cached
        sf3d.unwrap.BoxProjectionUnwrapper; sf3d.bake.cell_atlas_unwrapper, the hook form of ops.uv_cell_atlas, is the
        deterministic stand-in) -> ops.bake_rasterize on the per-corner UVs -> ops.bake_scene_color (one fused launch) ->
        ops.dilate_fill with res // 150 iterations, the padding rule of the SF3D bake.  Nothing here waits for the device (the
        box-projection unwrapper itself reads two small sums back).  With self.atlas = "charts" (an instance setting, default
        "box") the default unwrapper is one cached sf3d.unwrap.ChartUnwrapper: connected charts, eight integers read per round."""
        self._need_weights("bake_texture")
        res = int(texture_resolution)
        if res < 1:
            raise ValueError("TSR.bake_texture: texture_resolution must be positive")
        with torch.no_grad():
            v, f, uv, rast = self._atlas(mesh, res, island_padding, unwrapper)
            color, mask = ops.bake_scene_color(self._field(scene_code), self.decoder, v, f, rast, radius=self.renderer.cfg.radius)
            color = self._padded(color, mask, res)
        return Mesh(mesh.vertices, mesh.faces, None, uvs=uv, texture=color)   # nothing of `mesh` but its geometry is carried

    def _atlas(self, mesh, res, island_padding, unwrapper, keep_uvs=False):
        """What the two bakes share: the mesh on the device, its per-corner UVs (the mesh's own with keep_uvs, when it has
        some; else the unwrapper's) and the atlas rasterised at `res` -> (v f32 [Nv,3], f [Nf,3], uv f32 [3Nf,2], rast)."""
        if self.atlas not in self.ATLASES:   # before anything is launched
            raise ValueError("TSR.atlas must be one of %s, got %r" % (", ".join(repr(a) for a in self.ATLASES), self.atlas))
        v = _f32(mesh.vertices, self.device)
        f = torch.as_tensor(mesh.faces).to(self.device).contiguous()
        if keep_uvs and mesh.uvs is not None:
            uv = _f32(mesh.uvs, self.device)
        else:
            if unwrapper is None and self.atlas == "charts":
                if self._chart_unwrapper is None:
                    from ..sf3d.unwrap import ChartUnwrapper

                    self._chart_unwrapper = ChartUnwrapper()
                unwrapper = self._chart_unwrapper
            if unwrapper is None:
                if self._unwrapper is None:
                    from ..sf3d.unwrap import BoxProjectionUnwrapper

                    self._unwrapper = BoxProjectionUnwrapper()
                unwrapper = self._unwrapper
            uv, corner = unwrapper(v, ops.vertex_normals(v, f), f, island_padding)
            uv = uv.to(torch.float32)[corner.reshape(-1).long()].contiguous()   # per corner, whatever rows the unwrapper shares
        rast = ops.bake_rasterize(uv, torch.arange(3 * f.shape[0], device=self.device, dtype=torch.int32).view(-1, 3), res)
        return v, f, uv, rast

    @staticmethod
    def _padded(image, mask, res):
        """The padding rule of the SF3D bake: res // 150 rounds of ops.dilate_fill around the charts."""
        it = res // 150
        if it > 0:
            image = ops.dilate_fill(image.permute(2, 0, 1)[None].contiguous(), mask[None, None], iterations=it)[0].permute(1, 2, 0).contiguous()
        return image

    NORMAL_MAP_FLAT = {"tangent": (0.5, 0.5, 1.0), "object": (0.5, 0.5, 0.5)}

    # class-level defaults of the two attributes __init__ sets: extract_meshes reads them on every call, also on an object that
    # was made without __init__
    occlusion_map = None
    _occlusion_source = None
    # None until a call of extract_meshes(report=True | "full"), then one ops.mesh_report dict per image of that call
    last_reports = None
    # None | what ops.project_rule accepts (True, n, (n, cells)): when set, extract_meshes bakes the texture, and the normal map when
    # self.normal_map is set, AT THE SURFACE (bake_surface_maps) with its own threshold and resolution.  None: nothing new is launched
    bake_project = None
    # None | what ops.displacement_rule accepts (True, n, (n, cells)): when set, extract_meshes bakes a displacement map beside a
    # texture bake (bake_displacement_map on the baked mesh's atlas) and leaves it on the mesh as the plain attribute
    # `displacement` (a tsr.displacement.DisplacementMap, no Mesh field).  None: nothing new is launched
    displacement_map = None
    # None | what ops.thickness_rule accepts (True, k, (k, max_distance)): when set, extract_meshes bakes a thickness map beside a
    # texture bake (bake_thickness_map on the baked mesh's atlas, against the mesh itself) and leaves it on the mesh as the plain
    # attribute `thickness` (a tsr.thickness.ThicknessMap, no Mesh field).  None: nothing new is launched
    thickness_map = None
    # None | what ops.curvature_rule accepts (True, rings): when set, extract_meshes bakes a curvature map beside a texture bake
    # (bake_curvature_map on the baked mesh's atlas, the mesh's own curvature) and leaves it on the mesh as the plain attribute
    # `curvature` (a tsr.curvature.CurvatureMap, no Mesh field).  None: nothing new is launched
    curvature_map = None
    # "box" | "charts": the unwrapper _atlas makes when no unwrapper= is passed.  "box": sf3d.unwrap.BoxProjectionUnwrapper, as
    # before.  "charts": sf3d.unwrap.ChartUnwrapper -- charts that are connected pieces of surface, however many layers the
    # object has, shelf-packed.  Anything else is a ValueError before a launch.
    ATLASES = ("box", "charts")
    atlas = "box"
    _chart_unwrapper = None   # the cached ChartUnwrapper
    _quads = None   # extract_meshes -> _reshaped: the extractor's quads as a Catmull-Clark cage; and back: the refined quads

    def _iso_target(self, threshold, cells, resolution):
        """The iso-surface density_act = threshold in the raw density, and a trust radius in cells of a `resolution`^3 lattice
        -> (target = float32(ln(threshold) - density_bias), computed in double; max_dist = cells x the lattice spacing
        2 radius / (resolution - 1))."""
        cfg = self.renderer.cfg
        return float(np.float32(math.log(float(threshold)) - float(cfg.density_bias))), cells * 2.0 * float(cfg.radius) / (int(resolution) - 1)

    def _iso_search(self, caller, threshold, rule, resolution):
        """What a public method that searches for the iso-surface checks and works out, from rule = (steps, cells) and
        `resolution` (default: the marching-cubes resolution set last) -> (steps, target, max_dist) with _iso_target's two.
        The threshold's ValueError comes before the weights are asked for, the resolution's after."""
        steps, cells = rule
        if not threshold > 0:
            raise ValueError("TSR.%s: threshold must be positive, got %r" % (caller, threshold))
        self._need_weights(caller)
        if resolution is None:
            if self.isosurface_helper is None:
                raise ValueError("TSR.%s: no resolution given and no marching-cubes resolution set yet" % caller)
            resolution = self.isosurface_helper.resolution
        if int(resolution) < 2:
            raise ValueError("TSR.%s: resolution must be at least 2, got %r" % (caller, resolution))
        return (steps,) + self._iso_target(threshold, cells, resolution)

    def _low_poly_frame(self, v, f, uv):
        """The tangent frame of the low-poly mesh the normal maps are stored in -> (corner_normals [3*Nf, 3], corner_tangents [3*Nf, 4])."""
        corner_n = (self.WINDING_OUTWARD * ops.vertex_normals(v, f))[f.reshape(-1).long()].contiguous()
        return corner_n, ops.corner_tangents(v, f, uv, corner_n)

    def bake_normal_map(self, mesh: Mesh, scene_code, resolution=None, space="tangent", island_padding: float = 0.02,
                        unwrapper=None) -> Mesh:
        """The last step of a high-to-low workflow: the surface detail of the density field of `scene_code` ([3, C, H, W]),
        which simplify removed from the geometry, baked into a normal map over `mesh`'s atlas.  Per covered texel the field's
        outward unit normal (-grad density / |grad density|, ops.field_normals' bits) at the texel's point on the mesh, either as
        it is (space="object") or in the mesh's own tangent frame (space="tangent", the MikkTSpace / Blender / glTF convention).
        Atlas: a mesh that has uvs keeps them and `resolution` defaults to its texture's size; a mesh without is unwrapped as
        bake_texture does and `resolution` defaults to 2048.
        Stages: ops.vertex_normals * WINDING_OUTWARD -> per-corner normals [faces] -> ops.corner_tangents -> ops.bake_rasterize
        -> ops.bake_scene_normal (one fused launch) -> encode 0.5 + 0.5 n -> ops.dilate_fill with res // 150 rounds; texels the
        padding does not reach hold the flat value, (0.5, 0.5, 1) in tangent space and (0.5, 0.5, 0.5) in object space.
        -> a Mesh with the input's vertices, faces, vertex colours, uvs (or the new ones) and texture, plus normal_map f32
        [res, res, 3] (row 0 at the top), normal_map_space, corner_normals [3*Nf, 3] and corner_tangents [3*Nf, 4], on the
        device.  Nothing here waits for the device beyond what the unwrapper reads back."""
        if space not in self.NORMAL_MAP_FLAT:
            raise ValueError("TSR.bake_normal_map: space must be 'tangent' or 'object', got %r" % (space,))
        self._need_weights("bake_normal_map")
        res = _atlas_resolution(resolution, mesh, "bake_normal_map", ("texture",))
        with torch.no_grad():
            v, f, uv, rast = self._atlas(mesh, res, island_padding, unwrapper, keep_uvs=True)
            corner_n, corner_t = self._low_poly_frame(v, f, uv)
            n, mask = ops.bake_scene_normal(self._field(scene_code), self.decoder, v, f, rast, radius=self.renderer.cfg.radius,
                                            frame=(corner_n, corner_t) if space == "tangent" else None)
            coded = self._coded_normals(n, mask, res, space)
        return mesh._derive(mesh.vertices, mesh.faces, ("vertex_colors", "texture", "vertex_normals", "vertex_occlusion", "occlusion_map"),
                            uvs=mesh.uvs if mesh.uvs is not None else uv, normal_map=coded, normal_map_space=space,
                            corner_normals=corner_n, corner_tangents=corner_t)

    def bake_surface_maps(self, mesh: Mesh, scene_code, threshold: float = 25.0, project=True, resolution=None, atlas_resolution=None,
                          texture=True, normal_map="tangent", island_padding: float = 0.02, unwrapper=None) -> Mesh:
        """bake_texture and bake_normal_map as a baker does them: every covered texel first goes from its point on the low-poly
        face to the HIGH-poly surface -- the iso-surface density_act = threshold of the field of `scene_code`, reached by
        project_mesh's rule (project: True = (8, 1.0), an int n, or (n, cells) of a `resolution`^3 lattice: ops.project_rule;
        resolution: default the marching-cubes resolution set last) -- and colour and normal are read THERE.  After simplify the
        face interiors lie off the surface by their chord error, which project= on the vertices does not cure.
        One atlas (a mesh that has uvs keeps them; atlas_resolution defaults as in bake_normal_map) and ONE projection of the
        texels (ops.bake_surface_route: ops.bake_scene_surface_composed by default, the single fused launch of
        ops.bake_scene_surface with SCULPT_DISTANCE_FORM=fusedsurface; the same bits, the composed route is the faster one on
        these atlases) serve both maps: the normal map (normal_map: "tangent",
        "object" or None) comes out of that projection, the texture (texture=True) is the colour field at the projected points of the
        covered texels through the point query (ops.triplane_query on channel-last planes: picking the covered texels waits for
        the device).  The low-poly frame does not move: corner_normals and corner_tangents are bake_normal_map's.  Padding, flat
        values and encoding are exactly those of bake_texture / bake_normal_map.
        -> a Mesh with the input's vertices, faces and what bake_normal_map carries, plus uvs, texture and / or normal_map,
        normal_map_space, corner_normals, corner_tangents, on the device.  texture=False with normal_map=None is a ValueError."""
        rule = ops.project_rule(project)   # a ValueError before anything is launched
        if normal_map is not None and normal_map not in self.NORMAL_MAP_FLAT:
            raise ValueError("TSR.bake_surface_maps: normal_map must be None, 'tangent' or 'object', got %r" % (normal_map,))
        if not texture and normal_map is None:
            raise ValueError("TSR.bake_surface_maps: nothing to bake (texture=False and normal_map=None)")
        steps, target, max_dist = self._iso_search("bake_surface_maps", threshold, rule, resolution)
        res = _atlas_resolution(atlas_resolution, mesh, "bake_surface_maps", ("texture", "normal_map"))
        cfg = self.renderer.cfg
        with torch.no_grad():
            v, f, uv, rast = self._atlas(mesh, res, island_padding, unwrapper, keep_uvs=True)
            planes = self._field(scene_code)
            corner_n = corner_t = None
            if normal_map is not None:
                corner_n, corner_t = self._low_poly_frame(v, f, uv)
            point, n, mask, _ = ops.bake_surface_route()(planes, self.decoder, v, f, rast, target, max_dist, steps=steps,
                                                         radius=cfg.radius, frame=(corner_n, corner_t) if normal_map == "tangent" else None)
            new = {}
            if texture:
                color = torch.zeros_like(point)
                color[mask] = ops.triplane_query(planes, self.decoder, point[mask], radius=cfg.radius, density_bias=cfg.density_bias,
                                                 want=("color",))["color"]
                new["texture"] = self._padded(color, mask, res)
            if normal_map is not None:
                new.update(normal_map=self._coded_normals(n, mask, res, normal_map), normal_map_space=normal_map,
                           corner_normals=corner_n, corner_tangents=corner_t)
        # a baked texture replaces the vertex colours, as in bake_texture; a map that is not baked here stays (with its tag)
        keep = ("vertex_normals", "vertex_occlusion", "occlusion_map") + (() if texture else ("vertex_colors", "texture")) \
            + (() if normal_map is not None else ("normal_map", "corner_normals", "corner_tangents"))
        return mesh._derive(mesh.vertices, mesh.faces, keep, uvs=mesh.uvs if mesh.uvs is not None else uv, **new)

    def bake_displacement_map(self, mesh: Mesh, scene_code, threshold: float = 25.0, displacement=True, resolution=None,
                              atlas_resolution=None, island_padding: float = 0.02, unwrapper=None):
        """The map a Multires / displacement workflow needs: per texel of `mesh`'s atlas the signed height along the LOW-poly
        normal at which the field of `scene_code` reaches its iso-surface density_act = threshold.  Subdividing the low mesh
        and displacing by it gives back the detail that simplify removed; a normal map only shades that detail.
        displacement: True = (8 steps, 2 cells), an int n, or (n, cells) of a `resolution`^3 lattice (ops.displacement_rule;
        resolution: default the marching-cubes resolution set last): the search stays within max_dist = cells x the lattice
        spacing on either side of the face.  The direction is the per-vertex normal ops.vertex_normals * WINDING_OUTWARD -- the
        one bake_normal_map builds its frame from -- interpolated at the texel; the search is the safeguarded Newton rule of
        DESIGN.md 3.1h (ops.bake_displacement_route: ops.bake_displacement, which lists the covered texels on the device and
        never waits for it, by default; the composed route with SCULPT_DISTANCE_FORM=composeddisplacement; the same bits).
        Atlas: as bake_normal_map -- a mesh that has uvs keeps them, one without is unwrapped and comes back with them.
        -> (mesh, DisplacementMap): the mesh as it came, with uvs; the map (tsr/displacement.py) holds the rule's height where
        the texel converged and +0 elsewhere, padded by res // 150 rounds of ops.dilate_fill like the other maps, with mask,
        status, max_dist, midlevel = 0.5 and scale = 2 max_dist.  It is no Mesh field: hand it to Mesh.export(path,
        displacement=map)."""
        from .displacement import DisplacementMap

        rule = ops.displacement_rule(displacement)   # a ValueError before anything is launched
        steps, target, max_dist = self._iso_search("bake_displacement_map", threshold, rule, resolution)
        res = _atlas_resolution(atlas_resolution, mesh, "bake_displacement_map", ("texture", "normal_map", "occlusion_map"))
        cfg = self.renderer.cfg
        with torch.no_grad():
            v, f, uv, rast = self._atlas(mesh, res, island_padding, unwrapper, keep_uvs=True)
            planes = self._field(scene_code)
            normals = (self.WINDING_OUTWARD * ops.vertex_normals(v, f)).contiguous()
            route = ops.bake_displacement_route()
            height, mask, ex = route(planes, self.decoder, v, f, normals, rast, target, max_dist, steps=steps, radius=cfg.radius,
                                     want=("residual", "status", "evals"))
            before = route(planes, self.decoder, v, f, normals, rast, target, max_dist, steps=0, radius=cfg.radius,
                           want=("residual",))[2]["residual"]   # one evaluation at h = 0: what info() compares with
            kept = torch.where(ex["status"] == 0, height, torch.zeros_like(height))
            padded = self._padded(kept[..., None].expand(res, res, 3), mask, res)[..., 0].contiguous()
        out = mesh if mesh.uvs is not None else mesh._derive(mesh.vertices, mesh.faces,
                                                             ("vertex_colors", "vertex_normals", "vertex_occlusion", "quads"), uvs=uv)
        return out, DisplacementMap(padded, mask, ex["status"], max_dist, evals=ex["evals"], residual0=before, residual=ex["residual"],
                                    rule=rule)

    def _coded_normals(self, n, mask, res, space):
        """A normal image as a map: encoded 0.5 + 0.5 n, padded, the flat value where the padding does not reach."""
        flat = torch.tensor(self.NORMAL_MAP_FLAT[space], dtype=torch.float32, device=self.device)
        # dilate_fill averages over a texel's neighbourhood as it finds it, so the image is 0 outside the charts going in; an
        # encoded unit normal has a component above 0, and so has every average of some: a texel that is still (0, 0, 0)
        # coming out is one the padding did not reach
        coded = self._padded(torch.where(mask[..., None], 0.5 + 0.5 * n, torch.zeros_like(n)), mask, res)
        return torch.where((coded != 0).any(-1, keepdim=True), coded, flat)

    def bake_occlusion_map(self, mesh: Mesh, source=None, resolution=None, occlusion=True, cage=None, seed=0,
                           island_padding: float = 0.02, unwrapper=None) -> Mesh:
        """What a baker pairs with the normal map: the ambient occlusion of the HIGH-poly surface in the low-poly mesh's atlas,
        glTF's material.occlusionTexture.  Per covered texel the cosine-weighted share of `occlusion`'s directions (True: 64, k,
        or (k, max_distance): ops.occlusion_rule; `seed` rotates the set) along which a ray leaves without hitting the surface
        (ops.bake_occlusion_route: the composed route by default, the one fused launch of ops.bake_occlusion with
        SCULPT_DISTANCE_FORM=fusedbake; the same bits, the composed one is faster on these atlases).  source=None: the mesh against itself, cage must be None.  source=a Mesh (the
        mesh as it was before simplify): every texel's point is first snapped onto that surface along the low mesh's normal,
        within `cage` on either side (None: 2^-6 of the longest side of the source's bounds), and takes that surface's facet
        normal; a texel whose ray finds nothing keeps its own point and normal.
        Atlas: as bake_normal_map -- a mesh that has uvs keeps them and `resolution` defaults to its texture's (else its normal
        map's) size; a mesh without is unwrapped as bake_texture does and `resolution` defaults to 2048.  Needs a device, no weights.
        Stages: ops.vertex_normals * WINDING_OUTWARD -> ops.bake_rasterize -> the occlusion bake -> ops.dilate_fill with
        res // 150 rounds (on the value + 1, since 0 is a legitimate occlusion: what is still 0 afterwards was not reached);
        texels the padding does not reach, and texels whose point or normal is not finite, hold 1.0 (open).
        -> a Mesh with everything the input carried plus occlusion_map f32 [res, res] (row 0 at the top, 1 = open) and
        occlusion_map_rule = (k, max_distance), on the device."""
        rule = ops.occlusion_rule(occlusion)   # a ValueError before anything is launched
        if self.device is None:
            raise _lib.SculptError("TSR.bake_occlusion_map: the model is on no device yet (to(device))")
        if source is not None and not isinstance(source, Mesh):
            raise ValueError("TSR.bake_occlusion_map: source must be a Mesh or None, got %r" % (type(source).__name__,))
        if source is None and cage is not None:
            raise ValueError("TSR.bake_occlusion_map: cage snaps the texels onto a source; without a source it must be None")
        res = _atlas_resolution(resolution, mesh, "bake_occlusion_map", ("texture", "normal_map"))
        with torch.no_grad():
            v, f, uv, rast = self._atlas(mesh, res, island_padding, unwrapper, keep_uvs=True)
            normals = (self.WINDING_OUTWARD * ops.vertex_normals(v, f)).contiguous()
            src = None if source is None else (_f32(source.vertices, self.device), torch.as_tensor(source.faces).to(self.device).contiguous())
            ao, mask = ops.bake_occlusion_route()(v, f, normals, rast, occlusion=rule, seed=seed, source=src, cage=cage)
            valid = mask & torch.isfinite(ao)
            shifted = torch.where(valid, ao + 1.0, torch.zeros_like(ao))
            spread = self._padded(shifted[..., None].expand(res, res, 3), valid, res)[..., 0]
            padded = torch.where(spread != 0, (spread - 1.0).clamp(0.0, 1.0), torch.ones_like(ao))
            ao_map = torch.where(valid, ao, torch.where(mask, torch.ones_like(ao), padded)).contiguous()
        return mesh._derive(mesh.vertices, mesh.faces, ("vertex_colors", "texture", "vertex_normals", "vertex_occlusion", "normal_map",
                                                        "corner_normals", "corner_tangents"),
                            uvs=mesh.uvs if mesh.uvs is not None else uv, occlusion_map=ao_map, occlusion_map_rule=rule)

    def bake_thickness_map(self, mesh: Mesh, source=None, resolution=None, thickness=True, cone=60.0, cage=None, seed=0,
                           island_padding: float = 0.02, unwrapper=None):
        """The thickness map a baker ships beside normal and AO: the wall thickness -- the shape diameter -- of the HIGH-poly
        surface in the low-poly mesh's atlas.  Per covered texel the rays of a cone of half-angle `cone` degrees about the
        inward normal (`thickness`: True = 32 rays, k, or (k, max_distance): ops.thickness_rule; `seed` rotates the set) are
        followed to where they leave the body through the back of a face; the map holds their weighted mean length
        (ops.bake_thickness; outward = WINDING_OUTWARD).  source, cage and the atlas: as bake_occlusion_map -- source=None: the
        mesh against itself, cage must be None; source=a Mesh (the mesh before simplify): every texel is first snapped onto it.
        Needs a device, no weights.
        Stages: ops.vertex_normals * WINDING_OUTWARD -> ops.bake_rasterize -> ops.bake_thickness -> ops.dilate_fill with
        res // 150 rounds on thickness + 1 over the texels with a finite value (what is still 0 afterwards was not reached).
        -> (mesh, ThicknessMap): the mesh as it came, with uvs; the map (tsr/thickness.py) with thickness (padded), thinnest,
        valid, mask and rule.  It is no Mesh field: the map has its own save()."""
        from .thickness import ThicknessMap

        rule = ops.thickness_rule(thickness)   # a ValueError before anything is launched
        ops._thickness_rules(rule, cone, None, seed, self.WINDING_OUTWARD)
        if self.device is None:
            raise _lib.SculptError("TSR.bake_thickness_map: the model is on no device yet (to(device))")
        if source is not None and not isinstance(source, Mesh):
            raise ValueError("TSR.bake_thickness_map: source must be a Mesh or None, got %r" % (type(source).__name__,))
        if source is None and cage is not None:
            raise ValueError("TSR.bake_thickness_map: cage snaps the texels onto a source; without a source it must be None")
        res = _atlas_resolution(resolution, mesh, "bake_thickness_map", ("texture", "normal_map", "occlusion_map"))
        with torch.no_grad():
            v, f, uv, rast = self._atlas(mesh, res, island_padding, unwrapper, keep_uvs=True)
            normals = (self.WINDING_OUTWARD * ops.vertex_normals(v, f)).contiguous()
            src = None if source is None else (_f32(source.vertices, self.device), torch.as_tensor(source.faces).to(self.device).contiguous())
            th, thin, valid, mask = ops.bake_thickness(v, f, normals, rast, thickness=rule, cone=cone, seed=seed,
                                                       outward=self.WINDING_OUTWARD, source=src, cage=cage)
            known = mask & torch.isfinite(th)
            shifted = torch.where(known, th + 1.0, torch.zeros_like(th))
            spread = self._padded(shifted[..., None].expand(res, res, 3), known, res)[..., 0]
            padded = torch.where(spread != 0, (spread - 1.0).clamp(min=0.0), torch.zeros_like(th))
            th_map = torch.where(mask, th, padded).contiguous()
        out = mesh if mesh.uvs is not None else mesh._derive(mesh.vertices, mesh.faces,
                                                             ("vertex_colors", "vertex_normals", "vertex_occlusion", "quads"), uvs=uv)
        return out, ThicknessMap(th_map, thin, valid, mask, rule=rule)

    def bake_curvature_map(self, mesh: Mesh, source=None, resolution=None, curvature=True, cage=None, island_padding: float = 0.02,
                           unwrapper=None):
        """The curvature map a baker ships beside normal, AO and thickness: mean and Gaussian curvature in the low-poly mesh's
        atlas -- grey is flat, white convex, black concave; what edge wear and dirt masks are made from.  `curvature`: True or
        the number of rings in 0 .. 8 the integrated curvature is summed over (ops.curvature_rule).  source=None: the mesh's
        own curvature, interpolated over its faces; cage must be None.  source=a Mesh (the mesh before simplify): the curvature
        of THAT mesh, read where every texel lands on it (the snap of bake_occlusion_map; cage as there); a texel whose snap ray
        hits nothing keeps the low mesh's value.  Needs a device, no weights.
        Stages: ops.vertex_normals * WINDING_OUTWARD -> ops.bake_rasterize -> ops.bake_curvature (outward = WINDING_OUTWARD) ->
        ops.dilate_fill with res // 150 rounds over the covered texels with finite values (what is still 0 afterwards was not
        reached).
        -> (mesh, CurvatureMap): the mesh as it came, with uvs; the map (tsr/curvature.py) with mean and gauss (padded), mask
        and rule.  It is no Mesh field: the map has its own save()."""
        from .curvature import CurvatureMap

        rule = ops.curvature_rule(curvature)   # a ValueError before anything is launched
        if self.device is None:
            raise _lib.SculptError("TSR.bake_curvature_map: the model is on no device yet (to(device))")
        if source is not None and not isinstance(source, Mesh):
            raise ValueError("TSR.bake_curvature_map: source must be a Mesh or None, got %r" % (type(source).__name__,))
        if source is None and cage is not None:
            raise ValueError("TSR.bake_curvature_map: cage snaps the texels onto a source; without a source it must be None")
        res = _atlas_resolution(resolution, mesh, "bake_curvature_map", ("texture", "normal_map", "occlusion_map"))
        with torch.no_grad():
            v, f, uv, rast = self._atlas(mesh, res, island_padding, unwrapper, keep_uvs=True)
            normals = (self.WINDING_OUTWARD * ops.vertex_normals(v, f)).contiguous()
            src = None if source is None else (_f32(source.vertices, self.device), torch.as_tensor(source.faces).to(self.device).contiguous())
            mean, gauss, mask = ops.bake_curvature(v, f, normals, rast, curvature=rule, outward=self.WINDING_OUTWARD, source=src, cage=cage)
            known = mask & torch.isfinite(mean) & torch.isfinite(gauss)
            zero = torch.zeros_like(mean)
            image = torch.stack([torch.where(known, mean, zero), torch.where(known, gauss, zero), known.to(mean.dtype)], -1)
            spread = self._padded(image, known, res)     # the third channel is not 0 where a chart or the padding reaches
            reached = spread[..., 2] != 0
            mean_map = torch.where(mask, mean, torch.where(reached, spread[..., 0], zero)).contiguous()
            gauss_map = torch.where(mask, gauss, torch.where(reached, spread[..., 1], zero)).contiguous()
        out = mesh if mesh.uvs is not None else mesh._derive(mesh.vertices, mesh.faces,
                                                             ("vertex_colors", "vertex_normals", "vertex_occlusion", "quads"), uvs=uv)
        return out, CurvatureMap(mean_map, gauss_map, mask, rule=rule)

    def _projected(self, v_pos, t_pos_idx, planes, threshold, project, resolution):
        """ops.mesh_project with this model's field, at _iso_target's target and max_dist (the geometry chain of extract_meshes
        comes here with its checks made: no _iso_search)."""
        steps, cells = ops.project_rule(project)
        target, max_dist = self._iso_target(threshold, cells, resolution)
        return ops.mesh_project(planes, self.decoder, v_pos, t_pos_idx, target, max_dist, steps=steps, radius=self.renderer.cfg.radius)[0]

    def project_mesh(self, mesh: Mesh, scene_code, threshold: float = 25.0, project=True, resolution=None) -> Mesh:
        """`mesh` with its vertices on the iso-surface density_act = threshold of the field of `scene_code` ([3, C, H, W] or an
        ops.ChannelLastPlanes): per vertex at most n Newton steps along the density's gradient inside a trust radius of `cells`
        lattice cells of a `resolution`^3 lattice (project: True = (8, 1.0), an int n, or (n, cells): ops.project_rule;
        resolution: default the marching-cubes resolution set last), then the fold guard (ops.mesh_project).  The faces are the
        same and the vertices keep their indices, so vertex_colors, uvs and texture are carried over as they are;
        vertex_normals is dropped, as Mesh.smooth drops it: the vertices have moved (TSR.field_normals at the new vertices
        gives the normals of the surface they now lie on).  What extract_meshes(project=...) does as its last geometry step;
        also the way to project the gathered mesh of extract_mesh_sharded.  Nothing waits for the device."""
        steps_cells = ops.project_rule(project)   # a ValueError before anything is launched
        self._iso_search("project_mesh", threshold, steps_cells, resolution)   # its ValueErrors too
        if resolution is None:
            resolution = self.isosurface_helper.resolution
        if not isinstance(scene_code, ops.ChannelLastPlanes):
            scene_code = self._field(scene_code, channel_last=False).contiguous()
        with torch.no_grad():
            v = _f32(mesh.vertices, self.device)
            f = torch.as_tensor(mesh.faces).to(self.device).contiguous()
            v = self._projected(v, f, scene_code, threshold, steps_cells, resolution)
        return mesh._derive(v, mesh.faces, ("vertex_colors", "uvs", "texture", "quads"))

    def extract_meshes(self, scene_codes, enable_texture=False, resolution: int = 256, threshold: float = 25.0,
                       x_range=None, density_events=None, bake_texture: int = 0, normals=None, isosurface="marching_cubes",
                       keep_components=None, fill_holes=None, voxel_remesh=None, report=None, simplify=None, smooth=None,
                       project=None, subdivide=None, occlusion=None) -> List[Mesh]:
        """The arithmetic of system.py:171-200 without the Blender sink: returns device tensors.
        density_events: optional (start, stop) torch events recorded around the dense-grid launch (bench.py's live
        per-launch timing of the dominant kernel, on the stream it is launched on).
        bake_texture: with enable_texture, a resolution > 0 bakes a UV texture of that size (TSR.bake_texture) instead of
        computing vertex colours; 0 (default): vertex colours as before.  With self.normal_map = "tangent" | "object" (an
        instance setting, default None) every mesh a texture is baked for also gets a normal map over the same atlas at the same
        resolution (TSR.bake_normal_map): Mesh.normal_map, normal_map_space, corner_normals, corner_tangents.  With
        self.occlusion_map = True | k | (k, max_distance) (an instance setting too, default None: nothing more is launched) it also
        gets an ambient-occlusion map over that atlas (TSR.bake_occlusion_map: Mesh.occlusion_map, occlusion_map_rule), baked
        against the mesh as it entered simplify when simplify is given, else against itself.  With self.bake_project = True | n |
        (n, cells) (an instance setting too, default None: nothing new is launched) the texture, and the normal map when
        self.normal_map is set, are baked AT THE SURFACE: every texel is projected from the low-poly face onto the iso-surface
        of this call's threshold first (TSR.bake_surface_maps, one projection for both maps).
        isosurface: "marching_cubes" (default: the reference's Lewiner mesh, bit for bit what it was without the keyword) or
        "surface_nets" (ops.surface_nets: one vertex inside every cell the surface passes through, one quad across every
        sign-changing lattice edge -- no sliver triangles, and an all-quad mesh in Mesh.quads beside the triangles in
        Mesh.faces, which split each quad along its shorter diagonal and wind like marching cubes' (TSR.WINDING_OUTWARD)).
        Both take the two-pass grid and its sign planes under the same guard.  Mesh.quads stays while the faces are the
        extractor's: smooth and project keep it, keep_components, simplify and the triangle schemes of subdivide drop it;
        subdivide=(n, "catmull_clark") refines it (below).  The mesh is open where
        the surface meets the box, and naive surface nets puts ONE vertex into a cell with an ambiguous sign pattern, so a
        noisy field gives non-manifold edges (the mesh steps classify and hold such vertices).  project=True after it puts the
        vertices onto the field's iso-surface (dual contouring in effect).  Anything else is a ValueError before any launch.
        run, run_async, run_batched, run_pipelined, batch.run_sharded and extract_mesh_sharded do not take the option yet.
        normals: None (default): Mesh.vertex_normals stays unset.  "field": the outward unit normals of the density field at the
        vertices (TSR.field_normals: the gradient of the field whose iso-surface the mesh is).  "faces": area-weighted averages of
        the facet normals (ops.vertex_normals).  Either way f32 [Nv, 3] per shared vertex, also on a baked mesh.
        keep_components: None (default): the mesh is what marching cubes returns, and nothing more is launched.  "largest", an
        int >= 1 (minimum faces) or a float in (0, 1) (fraction of the largest component's faces): the other connected
        components -- the floaters around the object -- are dropped on the device right after marching cubes
        (ops.mesh_keep_components), so the colours, the baked atlas and the normals see only what is kept.
        simplify: None (default): nothing is launched, nothing changes.  An int >= 1 (target faces) or a float in (0, 1) (ratio of
        the faces left after keep_components): quadric-error edge collapses on the device (ops.mesh_simplify) after
        keep_components and before the colours, the bake and the normals, which are therefore evaluated at the final vertices.
        smooth: None (default): nothing is launched, nothing changes.  An int n in 1 .. 1000 (n iterations with lam = 0.5,
        mu = -0.53) or a tuple (n, lam, mu) (ops.smooth_rule): Taubin's lambda|mu filter on the device (ops.mesh_smooth) after
        keep_components and BEFORE simplify, so that the quadrics are built on the clean surface; faces and indices are
        unchanged.  Mesh.smooth lets a caller choose another order.
        project: None (default): nothing is launched, nothing changes.  True (8 Newton steps inside a trust radius of one lattice
        cell), an int n in 1 .. 64 or a tuple (n, cells) (ops.project_rule): every vertex is moved onto the iso-surface
        density_act = threshold of the field itself and folded faces are undone (ops.mesh_project, TSR.project_mesh) -- the
        LAST geometry step, after keep_components, smooth, simplify and subdivide and before the colours, the bake and the normals,
        which are therefore evaluated at the projected vertices; faces and indices are unchanged.  Needs threshold > 0.
        subdivide: None (default): nothing is launched, nothing changes.  An int n in 1 .. 6 (n levels of the Loop scheme) or a
        tuple (n, "loop" | "midpoint" | "catmull_clark") (ops.subdivide_rule): every face becomes four per level on the device
        (ops.mesh_subdivide) AFTER simplify and BEFORE project -- simplify leaves a light, irregular cage, subdivide refines it
        into a semi-regular surface, and project puts the vertices that now exist between the lattice points onto the field's
        iso-surface.  Mesh.subdivide lets a caller choose another order.  (n, "catmull_clark") is the all-quad scheme of
        Blender's Subdivision Surface and Multires modifiers (ops.mesh_catmull_clark), at the same place in the chain: it starts
        from the extractor's quads while they are still valid (isosurface="surface_nets" with no keep_components and no
        simplify; every quad becomes four per level), otherwise from the triangles (every triangle becomes three quads, then
        four per level -- simplify=0.1, subdivide=(1, "catmull_clark") is an all-quad, semi-regular mesh of about the marching
        cubes face budget).  Mesh.quads then holds the refined quads and Mesh.faces their split along the shorter diagonal;
        a following project keeps both; normals=, colours and the bakes see the final triangles.
        voxel_remesh: None (default): nothing is launched, nothing changes.  An int R in 8 .. 1024 (cells along the longest side
        of the mesh's bounds) or a tuple (R, band_cells) (ops.voxel_rule): the mesh is rebuilt from its inside on a voxel lattice
        (ops.mesh_voxel_remesh: integer winding counts, a banded signed-distance volume, marching cubes) AFTER keep_components
        and BEFORE smooth, so that the filter and the quadrics see the fused, closed surface: overlapping parts become one, and
        the holes where the extractor met the box close.  It makes new faces, so Mesh.quads is dropped and Catmull-Clark starts
        from the triangles.  run, run_async, run_batched, run_pipelined, batch.run_sharded and extract_mesh_sharded do not
        take the option yet: call Mesh.voxel_remesh on a device mesh instead.
        fill_holes: None (default): nothing is launched, and the meshes are bit for bit what they were.  True (every border loop)
        or an int max_edges >= 3 (loops of at most that many edges; ops.holes_rule): the border loops -- the holes where the
        surface meets the box -- are capped with fans on the device (ops.mesh_fill_holes) AFTER keep_components and BEFORE
        voxel_remesh, smooth and simplify, which then get a closed surface without resampling: every vertex and face of the
        extractor stays exactly as it is, a loop of four or more edges gets one vertex at its centroid and a face per edge, a
        loop of three one face.  It makes new faces, so Mesh.quads is dropped and Catmull-Clark starts from the triangles.  NOT
        claimed: a fan is a good cap for a short or roughly planar, star-shaped loop, and nothing more; a long loop that wraps
        round an edge or a corner of the box gets a fan that cuts through the mesh -- max_edges is the control, report="full"
        the check, voxel_remesh the answer for such loops.  Pass it by keyword, like voxel_remesh and report.  run, run_async,
        run_batched, run_pipelined, batch.run_sharded and extract_mesh_sharded do not take the option yet: call Mesh.fill_holes
        on a device mesh instead.
        occlusion: None (default): nothing is launched, nothing changes.  True (64 directions), an int k in 1 .. 1024 or a tuple
        (k, max_distance) (ops.occlusion_rule): Mesh.vertex_occlusion = the ambient occlusion of the final mesh against itself,
        f32 [Nv], 1 = open, 0 = occluded -- Mesh.ambient_occlusion(occlusion, outward=TSR.WINDING_OUTWARD), one fused ray
        kernel (ops.mesh_occlusion) over the mesh's own grid.  Not a geometry step: it is computed with the colours and the
        normals, after the geometry chain, and changes no vertex and no face.  run, run_async, run_batched, run_pipelined,
        batch.run_sharded and extract_mesh_sharded do not take the option yet (their host hand-off copies four arrays): call
        Mesh.ambient_occlusion on a device mesh instead.
        report: None (default): nothing is launched, nothing changes.  True leaves self.last_reports, one dict per image: what
        each FINAL device mesh is (ops.mesh_report without self-intersections: edge census, Euler number, genus, area, volume),
        computed after everything else and before the hand-off; "full" adds the self-intersection count.  The returned meshes
        are bit for bit those of the call without the keyword.  Pass it by keyword: it stands with the keywords the other
        entry points do not take yet, so that the tail of the signature stays (..., subdivide, occlusion)."""
        if not (report is None or report is True or (isinstance(report, str) and report == "full")):
            raise ValueError("report must be None, True or 'full', got %r" % (report,))
        if normals not in (None, "field", "faces"):
            raise ValueError("normals must be None, 'field' or 'faces', got %r" % (normals,))
        ops.isosurface_rule(isosurface)   # a ValueError before anything is launched
        if occlusion is not None:
            ops.occlusion_rule(occlusion)   # a ValueError before anything is launched
        if self.occlusion_map is not None:
            ops.occlusion_rule(self.occlusion_map)
        if self.displacement_map is not None:
            ops.displacement_rule(self.displacement_map)
            if not threshold > 0:
                raise ValueError("displacement_map needs a positive threshold (the surface is ln(threshold) in the raw density), got %r" % (threshold,))
        if self.thickness_map is not None:
            ops.thickness_rule(self.thickness_map)
        if self.curvature_map is not None:
            ops.curvature_rule(self.curvature_map)
        if self.bake_project is not None:
            ops.project_rule(self.bake_project)
            if not threshold > 0:
                raise ValueError("bake_project needs a positive threshold (the surface is ln(threshold) in the raw density), got %r" % (threshold,))
        geometry = dict(keep_components=keep_components, simplify=simplify, smooth=smooth, project=project, subdivide=subdivide,
                        voxel_remesh=voxel_remesh, fill_holes=fill_holes)
        self._check_geometry(threshold, **geometry)   # a ValueError before anything is launched
        bake = int(bake_texture) if enable_texture else 0
        self.set_marching_cubes_resolution(resolution)
        r = self.renderer.cfg.radius
        R = resolution
        out = []
        if report is not None:
            self.last_reports = []
        quads_of = {}   # what the surface-nets extractor leaves beside the (vertices, faces) that _extract_filtered hands on
        if isosurface == "surface_nets":
            def mc(v, sign_planes=None):
                v_pos, quads_of["quads"], faces = ops.surface_nets(v.view(R, R, R), 0.0, vert_div=R - 1.0, vert_mul=r - (-r), vert_add=-r,
                                                                   faces_i64=True, sign_planes=sign_planes)
                return v_pos, faces
        else:
            def mc(v, sign_planes=None):
                return ops.marching_cubes(v.view(R, R, R), 0.0, reference_order=True, vert_div=R - 1.0, vert_mul=r - (-r), vert_add=-r,
                                          sign_planes=sign_planes)

        mc.takes_sign_planes = True
        keeps_faces = keep_components is None and simplify is None and subdivide is None and voxel_remesh is None and fill_holes is None
        catmull_clark = self._is_catmull_clark(subdivide)
        for scene_code in scene_codes:
            planes = scene_code.contiguous()
            dkw = dict(radius=r, density_bias=self.renderer.cfg.density_bias, out_add=-threshold)
            # density_act - threshold == -(-(density_act - threshold))  (system.py:184, isosurface.py:45)
            if self._filter_applies(planes, R, threshold):
                v_pos, t_pos_idx = self._extract_filtered(planes, R, mc, dkw, density_events)
            else:
                vol = ops.density_grid(planes, self.decoder, R, precision=self.decoder_precision, events=density_events, **dkw)
                v_pos, t_pos_idx = mc(vol)   # (both decoder modes have the fp32 range: a NaN here is a NaN of the model)
            quads = quads_of.pop("quads", None)
            # Catmull-Clark refines the extractor's quads while they still cover the faces (smooth keeps them), else the triangles
            self._quads = (quads if catmull_clark and keep_components is None and simplify is None and voxel_remesh is None
                           and fill_holes is None else None)
            v_pos, t_pos_idx = self._reshaped(v_pos, t_pos_idx, planes, threshold, R, **geometry)
            out.append(self._textured(v_pos, t_pos_idx, planes, enable_texture, bake, normals, occlusion, threshold=threshold, R=R))
            refined, self._quads = self._quads, None
            if keeps_faces:   # the faces are still the extractor's
                out[-1].quads = quads
            elif catmull_clark:   # the faces are the split of the refined quads
                out[-1].quads = refined
            if report is not None:
                self.last_reports.append(ops.mesh_report(out[-1].vertices, out[-1].faces, self_intersections=report == "full"))
        return out

    @staticmethod
    def _is_catmull_clark(subdivide):
        """Whether a `subdivide` that ops.subdivide_rule accepts names the all-quad scheme (only a tuple can)."""
        return isinstance(subdivide, tuple) and len(subdivide) == 2 and subdivide[1] == "catmull_clark"

    @staticmethod
    def _check_geometry(threshold, keep_components=None, simplify=None, smooth=None, project=None, subdivide=None, voxel_remesh=None,
                        fill_holes=None):
        """The rules of the geometry options that are set (ops.*_rule; an option left None is not looked at): a ValueError
        here comes before anything is launched."""
        if keep_components is not None:
            ops.keep_rule(keep_components)
        if fill_holes is not None:
            ops.holes_rule(fill_holes)
        if voxel_remesh is not None:
            ops.voxel_rule(voxel_remesh)
        if simplify is not None:
            ops.simplify_rule(simplify)
        if smooth is not None:
            ops.smooth_rule(smooth)
        if subdivide is not None:
            ops.subdivide_rule(subdivide)
        if project is not None:
            ops.project_rule(project)
            if not threshold > 0:
                raise ValueError("project needs a positive threshold (the surface is ln(threshold) in the raw density), got %r" % (threshold,))

    def _reshaped(self, v_pos, t_pos_idx, planes, threshold, R, keep_components=None, simplify=None, smooth=None, project=None,
                  subdivide=None, voxel_remesh=None, fill_holes=None):
        """The geometry half of extract_meshes, in its fixed order: keep_components -> fill_holes -> voxel_remesh -> smooth -> simplify -> subdivide -> project,
        each only when set -> (v_pos, t_pos_idx).  A new geometry step goes in here, and into _check_geometry, and nowhere else."""
        if keep_components is not None:
            v_pos, t_pos_idx = ops.mesh_keep_components(v_pos, t_pos_idx, keep_components)[:2]
        if fill_holes is not None:
            v_pos, t_pos_idx = ops.mesh_fill_holes(v_pos, t_pos_idx, fill_holes)[:2]
        if voxel_remesh is not None:
            v_pos, t_pos_idx = ops.mesh_voxel_remesh(v_pos, t_pos_idx, voxel_remesh)
        if smooth is not None:
            v_pos = ops.mesh_smooth(v_pos, t_pos_idx, smooth)
        self._occlusion_source = None
        if simplify is not None:
            if self.occlusion_map is not None:   # the high-poly surface the occlusion map is baked against (_textured)
                self._occlusion_source = Mesh(v_pos, t_pos_idx)
            v_pos, t_pos_idx = ops.mesh_simplify(v_pos, t_pos_idx, simplify)[:2]
        if subdivide is not None:
            if self._is_catmull_clark(subdivide):   # the quads extract_meshes left in _quads, else the triangles; the refined quads go back
                cage = t_pos_idx if self._quads is None else self._quads
                v_pos, self._quads, t_pos_idx = ops.mesh_catmull_clark(v_pos, cage, subdivide[0])[:3]
            else:
                v_pos, t_pos_idx = ops.mesh_subdivide(v_pos, t_pos_idx, subdivide)[:2]
        if project is not None:
            v_pos = self._projected(v_pos, t_pos_idx, planes, threshold, project, R)
        return v_pos, t_pos_idx

    # What turns ops.vertex_normals of an extract_meshes mesh outwards: marching cubes (reference_order: face columns [1, 0, 2])
    # on density_act - threshold, positive inside, winds its faces counter-clockwise seen from outside -- on the analytic
    # sphere every face's cross(b - a, c - a) points away from the centre.  tests/test_gpu_mesh_ray.py pins the sign against
    # TSR.field_normals on the model's mesh.
    WINDING_OUTWARD = 1.0

    def _textured(self, v_pos, t_pos_idx, planes, enable_texture, bake, normals=None, occlusion=None, threshold=25.0, R=None):
        """The appearance half of extract_meshes: nothing, vertex colours (system.py:189-193) or a baked texture; and the
        vertex normals and the ambient occlusion when asked for.  threshold, R: the surface and the lattice of the extraction,
        for the bake at the surface (self.bake_project)."""
        source, self._occlusion_source = self._occlusion_source, None
        if enable_texture and bake > 0 and self.bake_project is not None:   # both maps from one projection of the texels
            mesh = self.bake_surface_maps(Mesh(v_pos, t_pos_idx), planes, threshold=threshold, project=self.bake_project, resolution=R,
                                          atlas_resolution=bake, normal_map=self.normal_map)
            if self.occlusion_map is not None:
                mesh = self.bake_occlusion_map(mesh, source=source, occlusion=self.occlusion_map)
        elif enable_texture and bake > 0:
            mesh = self.bake_texture(Mesh(v_pos, t_pos_idx), planes, bake)
            if self.normal_map is not None:   # the same atlas, the texture's resolution
                mesh = self.bake_normal_map(mesh, planes, space=self.normal_map)
            if self.occlusion_map is not None:   # the same atlas and resolution too; against the mesh as it entered simplify
                mesh = self.bake_occlusion_map(mesh, source=source, occlusion=self.occlusion_map)
        else:
            color = None
            if enable_texture:
                color = self.renderer.query_triplane(self.decoder, v_pos, planes)["color"]
            mesh = Mesh(v_pos, t_pos_idx, color)
        if enable_texture and bake > 0 and self.displacement_map is not None:   # the texture's atlas and resolution
            mesh, mesh.displacement = self.bake_displacement_map(mesh, planes, threshold=threshold, displacement=self.displacement_map,
                                                                 resolution=R)
        if enable_texture and bake > 0 and self.thickness_map is not None:   # the texture's atlas and resolution
            mesh, mesh.thickness = self.bake_thickness_map(mesh, thickness=self.thickness_map)
        if enable_texture and bake > 0 and self.curvature_map is not None:   # the texture's atlas and resolution
            mesh, mesh.curvature = self.bake_curvature_map(mesh, curvature=self.curvature_map)
        if normals == "field":
            mesh.vertex_normals = self.field_normals(v_pos, planes)
        elif normals == "faces":
            mesh.vertex_normals = ops.vertex_normals(v_pos, t_pos_idx)
        if occlusion is not None:
            mesh.vertex_occlusion = Mesh(v_pos, t_pos_idx).ambient_occlusion(occlusion, outward=self.WINDING_OUTWARD)
        return mesh

    # -- the two-pass ("filtered") density grid: calibration, guard, fallback (csrc/density_filter.hip)
    FILTER_SAFETY = 8.0        # margin = FILTER_SAFETY x the largest coarse error of the calibration probe
    FILTER_GUARD = 1.0 / 3.0   # a call whose re-evaluated points show a coarse error above FILTER_GUARD x margin is redone in full
    FILTER_PROBE = 64          # lattice of the calibration probe
    FILTER_MAX_MARGIN = 2.0    # a model whose coarse pass is this far off (log units of density) gains nothing: filter off

    def _filter_applies(self, planes, R, threshold):
        return (self.decoder_filter and self.decoder_precision == "bf16l3" and self.filter_info["usable"] and threshold > 0
                and self.decoder.n_hidden >= 1 and 32 <= R <= 1024)

    def calibrate_decoder_filter(self, planes):
        """Margin of the two-pass density grid for this model, measured on `planes` (one scene code [3, C, H, W]): every point of a
        64^3 lattice through both the one-product pass and the three-limb arithmetic (SCULPT_FILTER_MARK_ALL); margin =
        FILTER_SAFETY x the largest |log d~ - log d|.  IEEE-half operands when the probe stays finite, bf16 otherwise; a model
        for which neither gives a usable margin runs unfiltered."""
        info, r = self.filter_info, self.renderer.cfg.radius
        info["calibrations"] += 1
        for coarse in ("fp16", "bf16"):
            _, st = ops.density_grid_filtered(planes, self.decoder, self.FILTER_PROBE, 0.0, radius=r,
                                              density_bias=self.renderer.cfg.density_bias, out_add=0.0, coarse=coarse, mark_all=True)
            s = ops.filter_stats(st)
            if s["n_nonfinite"] == 0 and np.isfinite(s["max_err"]):
                margin = max(self.FILTER_SAFETY * s["max_err"], 1e-3)
                if margin <= self.FILTER_MAX_MARGIN:
                    info.update(margin=margin, coarse=coarse, probe_max_err=s["max_err"])
                    return info
        info.update(usable=False, margin=None)
        return info

    def _extract_filtered(self, planes, R, mc, dkw, density_events=None, x_begin=0, x_end=None):
        """The two-pass grid of lattice planes [x_begin, x_end) + mc(volume) (marching cubes: its count read-back waits for an
        event recorded behind the count phase, and the grid call's statistics copy is queued BEFORE that phase on the same stream,
        so the statistics have landed when it returns), under the run-time guard."""
        info = self.filter_info
        dkw = dict(dkw, x_begin=x_begin, x_end=x_end)
        if info["margin"] is None:
            self.calibrate_decoder_filter(planes)
            if not info["usable"]:
                return mc(ops.density_grid(planes, self.decoder, R, precision="bf16l3", events=density_events, **dkw))
        host = getattr(self, "_filter_stats_host", None)
        if host is None:
            host = self._filter_stats_host = torch.zeros(ops.FILTER_STATS_WORDS, dtype=torch.int32).pin_memory()
        vol, _ = ops.density_grid_filtered(planes, self.decoder, R, info["margin"], coarse=info["coarse"], events=density_events,
                                           stats_host=host, **dkw)
        err = None
        # a whole grid (not a slab): marching cubes takes its cell signs from the grid's sign planes and reads the volume only
        # where a cell is active; SCULPT_MC_SIGN_PLANES=0: the plain count phase over the whole volume (A/B)
        signs = None
        if x_begin == 0 and (x_end is None or x_end == R) and getattr(mc, "takes_sign_planes", False) and _MC_SIGN_PLANES:
            signs = ops.filter_sign_planes(R, planes.device)
        try:
            # waits for the counts (sculpt_mc_count_read: an event behind the count phase, not the whole stream -- the emit may still
            # be running).  density_grid_filtered queued the copy into `host` before the count launch, on the same stream, so the
            # event covers it: the statistics have landed with the counts.  Keep that order.
            mesh = mc(vol) if signs is None else mc(vol, signs)
        except Exception as e:  # an empty / out-of-range surface raises in both evaluations; checked below before it is believed
            mesh, err = None, e
        st = ops.filter_stats(host)
        info["last"] = st
        seen = ops.filter_guard_error(st)
        if seen <= self.FILTER_GUARD * info["margin"]:
            info["filtered"] += 1
            if err is not None:
                raise err
            return mesh
        # the coarse pass was further off than the calibration allows for: this grid in full, and a margin that covers what was seen
        info["fallbacks"] += 1
        info["margin"] = None
        vol = ops.density_grid(planes, self.decoder, R, precision="bf16l3", out=vol, **dkw)
        mesh = mc(vol)
        self.calibrate_decoder_filter(planes)
        if info["usable"] and info["margin"] is not None and np.isfinite(seen):
            info["margin"] = min(max(info["margin"], self.FILTER_SAFETY * seen), self.FILTER_MAX_MARGIN)
        return mesh

    def extract_mesh_sharded(self, scene_code, resolution: int = 512, threshold: float = 25.0, enable_texture=False):
        """BASELINE config 5: the voxel grid of ONE image split into slabs along the slowest lattice axis over
        the ranks of the default process group (RCCL over xGMI), one padded all-gather of the per-slab
        triangles, identical result on every rank and identical to the single-GPU mesh
        (sculptmate_amd/slab.py).  Without a process group the slabs run one after the other here.
        It takes no keep_components: components cross the slabs, so the gathered mesh is filtered afterwards, with
        Mesh.keep_components.  It takes no smooth either, for the same reason (a slab's cut is an open border, whose vertices
        smoothing holds fixed): smooth the gathered mesh with Mesh.smooth.  It takes no project: use TSR.project_mesh on the
        gathered mesh.  It takes no subdivide either (a slab's cut would be refined as a crease): use Mesh.subdivide on the
        gathered mesh."""
        import torch.distributed as dist

        from .. import slab

        r = self.renderer.cfg.radius
        planes = scene_code.contiguous()
        kw = dict(radius=r, density_bias=self.renderer.cfg.density_bias, threshold=threshold,
                  precision=self.decoder_precision)
        if self._filter_applies(planes, resolution, threshold):
            # every slab through the two-pass grid (cells inside the slab's planes only: the halo plane is part of the slab)
            dkw = dict(radius=r, density_bias=self.renderer.cfg.density_bias, out_add=-threshold)
            kw["run"] = lambda x0, x1, mc: self._extract_filtered(planes, resolution, mc, dkw, None, x0, x1)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            part = slab.extract_slab(planes, self.decoder, resolution, dist.get_rank(), dist.get_world_size(), **kw)
            v_pos, t_pos_idx = slab.gather_and_assemble(part, planes.device)
        else:
            v_pos, t_pos_idx = slab.extract_mesh_slabs_local(planes, self.decoder, resolution, 1, **kw)
        color = None
        if enable_texture:
            color = self.renderer.query_triplane(self.decoder, v_pos, planes)["color"]
        return Mesh(v_pos, t_pos_idx, color)

    def extract_mesh(self, scene_codes, enable_texture=False, mesh_name="NewMesh", resolution: int = 256,
                     threshold: float = 25.0, bake_texture: int = 0, normals=None, isosurface="marching_cubes", keep_components=None,
                     fill_holes=None, voxel_remesh=None, report=None, simplify=None, smooth=None, project=None, subdivide=None, occlusion=None):
        """system.py:171-200: same signature (+ bake_texture, normals, occlusion, report and the geometry options keep_components, fill_holes, voxel_remesh,
        smooth, simplify, subdivide, project, all described at extract_meshes: the sink receives the final mesh); pushes each mesh into the sink (Blender when
        `bpy` is importable, exactly like the reference's import_obj_blender) and also returns the meshes.  A baked mesh goes to
        the textured sink (per-loop UVs + an image-texture material; with self.normal_map = "tangent" also normal_image=, the
        baked normal map, which Blender's sink wires through a Normal Map node).  The sinks take no normals (Blender shades a mesh with
        shared vertices smooth by itself) and no occlusion; both stay on the returned meshes.  isosurface (extract_meshes): a mesh with
        quads goes to the plain sink as quads, in place of the faces (Blender's from_pydata takes any polygon size); the
        textured sink stays on triangles, which its per-corner UVs belong to."""
        meshes = self.extract_meshes(scene_codes, enable_texture, resolution, threshold, bake_texture=bake_texture, normals=normals,
                                     isosurface=isosurface, keep_components=keep_components, simplify=simplify, smooth=smooth, project=project,
                                     subdivide=subdivide, occlusion=occlusion, voxel_remesh=voxel_remesh, report=report, fill_holes=fill_holes)
        sink = self.mesh_sink or _default_sink()
        for m in meshes:
            if m.texture is not None:
                tsink = self.textured_mesh_sink or (_default_textured_sink() if self.mesh_sink is None else None)
                if tsink is not None:
                    # only a model whose normal_map is set hands the sink a normal image: a five-argument sink stays valid.  An
                    # object-space map is not one a Normal Map node in its default (tangent) setting can decode: it stays on the mesh
                    extra = {}
                    if self.normal_map is not None and m.normal_map is not None and m.normal_map_space == "tangent":
                        extra["normal_image"] = m.normal_map_image()
                    tsink(_host(m.vertices), _host(m.faces), _host(m.uvs), m.texture_image(), mesh_name, **extra)
                elif sink is not None:   # a caller's own four-argument sink: the geometry, without colours
                    sink(_host(m.vertices), _host(m.faces), None, mesh_name)
                continue
            if sink is not None:
                sink(m.vertices.cpu().numpy(), (m.faces if m.quads is None else m.quads).cpu().numpy(),
                     None if m.vertex_colors is None else m.vertex_colors.cpu().numpy(), mesh_name)
        return meshes

    def run_async(self, image, mc_resolution: int = 256, threshold: float = 25.0, enable_texture: bool = False, tokens=None,
                  normals=None, keep_components=None, simplify=None, smooth=None, project=None, subdivide=None):
        """One host image -> PendingMesh.  The image goes host -> HBM, the forward and the mesh extraction are queued on
        the current stream, and the mesh (the reference's `.cpu().numpy()` at system.py:200) is copied device -> pinned
        host memory on a separate copy stream, so the copy of mesh i runs under the kernels of image i + 1.
        PendingMesh.result() waits for that copy only.  tokens: the PendingTokens of THIS image from tokens_async (then
        `image` is not touched again): a caller with several images queues the tokens of image i + 1 before this call (run)."""
        with torch.no_grad():
            codes = self.forward([image], self.device) if tokens is None else self.forward_tokens(tokens)
            m = self.extract_meshes(codes, enable_texture, mc_resolution, threshold, normals=normals,
                                    keep_components=keep_components, simplify=simplify, smooth=smooth, project=project,
                                    subdivide=subdivide)[0]
        return self._mesh_to_host_async(m)

    def _mesh_to_host_async(self, m) -> PendingMesh:
        """Device mesh -> PendingMesh: vertices / faces / colours / normals copied into pinned host buffers on the copy stream."""
        main = torch.cuda.current_stream(self.device)
        copy = getattr(self, "_copy_stream", None)
        if copy is None:
            copy = self._copy_stream = torch.cuda.Stream(self.device)
        ready = torch.cuda.Event()
        ready.record(main)
        pool = getattr(self, "_pin_pool", None)
        if pool is None:
            pool = self._pin_pool = _PinnedPool()
        host, leases = [], []
        with torch.cuda.stream(copy):
            copy.wait_event(ready)
            for t in (m.vertices, m.faces, m.vertex_colors, m.vertex_normals):
                if t is None:
                    host.append(None)
                    continue
                lease, h = pool.take(t.shape, t.dtype)
                h.copy_(t, non_blocking=True)
                t.record_stream(copy)  # the device block must not be reused before the copy has read it
                host.append(h)
                leases.append(lease)
            done = torch.cuda.Event()
            done.record(copy)
        return PendingMesh(host, done, tuple(leases))

    def run(self, images, mc_resolution: int = 256, threshold: float = 25.0, enable_texture: bool = False, batch=None,
            normals=None, keep_components=None, simplify=None, smooth=None, project=None, subdivide=None) -> List[Mesh]:
        """Headless entry point: images -> list of Mesh with host (NumPy) arrays; the device -> host copy of mesh i overlaps the
        kernels that follow it.
        batch (images per transformer pass; None = the default): in the bf16 mode a stacked pass of several images gives each
        image the scene code of its own single-image pass BIT FOR BIT (every GEMM keeps the single-image tile form,
        ops.single_image_tiles), so several images run RUN_BATCH = 8 per pass by default -- the reference's batched forward
        (system.py:82-115), 3.5-3.9 instead of 5.2 ms of transformer per image -- and the meshes are those of one-at-a-time calls
        (test_run_batches_by_default_and_returns_the_serial_meshes).  The limb modes default to one image per pass with the
        tokenizer look-ahead (run_pipelined).  batch=1 forces that everywhere.
        normals: None, "field" or "faces" (extract_meshes): Mesh.vertex_normals as float32 [Nv, 3] on the host.
        keep_components, smooth, simplify, subdivide, project: the geometry options of extract_meshes, described there."""
        images = _as_image_list(images)
        if batch is None:
            batch = self.RUN_BATCH if (self.precision == "bf16" and len(images) >= 2) else 1
        kw = dict(normals=normals, keep_components=keep_components, simplify=simplify, smooth=smooth, project=project, subdivide=subdivide)
        if batch <= 1 or len(images) < 2:
            return [p.result() for p in self.run_pipelined(images, mc_resolution, threshold, enable_texture, **kw)]
        return [p.result() for p in self.run_batched(images, batch, mc_resolution, threshold, enable_texture, **kw)]

    RUN_BATCH = 8   # images per transformer pass of TSR.run in the bf16 mode (4: 139.7, 8: 143.5 meshes/s device to device)

    def run_batched(self, images, batch: int = 4, mc_resolution: int = 256, threshold: float = 25.0, enable_texture: bool = False,
                    normals=None, keep_components=None, simplify=None, smooth=None, project=None, subdivide=None):
        """images (host or device) -> list of PendingMesh through batched forward passes of `batch` images each."""
        images = list(images)
        pending = []
        keep = self.max_batch
        try:
            self.max_batch = max(1, int(batch))
            for i in range(0, len(images), self.max_batch):
                with torch.no_grad():
                    codes = self.forward(images[i:i + self.max_batch], self.device)
                    for m in self.extract_meshes(codes, enable_texture, mc_resolution, threshold, normals=normals,
                                                 keep_components=keep_components, simplify=simplify, smooth=smooth, project=project,
                                                 subdivide=subdivide):
                        pending.append(self._mesh_to_host_async(m))
        finally:
            self.max_batch = keep
        return pending

    def run_pipelined(self, images, mc_resolution: int = 256, threshold: float = 25.0, enable_texture: bool = False, normals=None,
                      keep_components=None, simplify=None, smooth=None, project=None, subdivide=None):
        """images (host or device) -> list of PendingMesh, with the tokenizer of image i + 1 queued beside the backbone /
        density grid / marching cubes of image i (tokens_async) and the device -> host copy of mesh i under image i + 1."""
        images = list(images)
        kw = dict(normals=normals, keep_components=keep_components, simplify=simplify, smooth=smooth, project=project, subdivide=subdivide)
        if len(images) < 2:
            return [self.run_async(im, mc_resolution, threshold, enable_texture, **kw) for im in images]
        pending, nxt = [], self.tokens_async(images[0])
        for i, im in enumerate(images):
            cur = nxt
            nxt = self.tokens_async(images[i + 1]) if i + 1 < len(images) else None
            pending.append(self.run_async(im, mc_resolution, threshold, enable_texture, tokens=cur, **kw))
        return pending


def _run_sharded(self, images, mc_resolution: int = 256, threshold: float = 25.0, enable_texture: bool = False, **kw):
    """A batch over the ranks of the default process group, one image per GPU at a time (sculptmate_amd/batch.py): returns
    ({index: Mesh} for this rank's images, [(index, rank, n_vertices, n_faces)] for all of them)."""
    from .. import batch

    with torch.no_grad():
        return batch.run_sharded(self, images, mc_resolution, threshold, enable_texture, **kw)


TSR.run_sharded = _run_sharded


def _as_image_list(image):
    if isinstance(image, (np.ndarray, torch.Tensor)) and image.ndim == 4:
        return [image[i] for i in range(image.shape[0])]
    return image if isinstance(image, (list, tuple)) else [image]


def _to_float_hwc(image):
    """ImagePreprocessor.convert_and_resize's conversion step (tsr/utils.py:68-77), without the resize."""
    if not isinstance(image, (np.ndarray, torch.Tensor)):  # PIL.Image
        image = np.array(image)
    if isinstance(image, np.ndarray):
        image = torch.from_numpy(image.astype(np.float32) / 255.0) if image.dtype == np.uint8 else torch.from_numpy(image)
    return image.to(torch.float32)


def _default_sink():
    try:
        import bpy  # noqa: F401
    except Exception:
        return None
    from .blender_sink import import_obj_blender

    return import_obj_blender


def _default_textured_sink():
    try:
        import bpy  # noqa: F401
    except Exception:
        return None
    from .blender_sink import import_textured_blender

    return import_textured_blender


def load_config(yaml_path: str, vit_json_path: Optional[str] = None):
    """checkpoints/config.yaml (+ config.json for the ViT) -> the dict TSR takes."""
    import json

    import yaml

    with open(yaml_path) as f:
        y = yaml.safe_load(f)
    cfg = {k: (dict(v) if isinstance(v, dict) else v) for k, v in DEFAULT_CFG.items()}
    cfg["cond_image_size"] = y.get("cond_image_size", cfg["cond_image_size"])
    tok = y.get("tokenizer", {})
    cfg["tokenizer"].update({k: tok[k] for k in ("plane_size", "num_channels") if k in tok})
    bb = dict(y.get("backbone", {}))
    if isinstance(bb.get("in_channels"), str):  # "${tokenizer.num_channels}"
        bb["in_channels"] = cfg["tokenizer"]["num_channels"]
    cfg["backbone"].update({k: bb[k] for k in cfg["backbone"] if k in bb})
    cfg["post_processor"].update(y.get("post_processor", {}))
    cfg["decoder"].update(y.get("decoder", {}))
    cfg["renderer"].update(y.get("renderer", {}))
    if vit_json_path and os.path.exists(vit_json_path):
        with open(vit_json_path) as f:
            j = json.load(f)
        for k in cfg["image_tokenizer"]:
            if k in j:
                cfg["image_tokenizer"][k] = j[k]
    return cfg
