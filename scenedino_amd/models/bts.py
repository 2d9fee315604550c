"""BTSNet -- the feature-field model, MI355X-native.

Mirror of scenedino.models.bts.BTSNet (/root/reference/scenedino/models/bts.py:22-595):
same constructor, attributes, ``encode`` semantics and ``forward`` return contract,
same state_dict keys (``encoder.*``, ``code_xyz._freqs/_phases``,
``heads.<name>.lin_in/lin_out.*``).  The per-point work (projection, positional
code, bilinear feature gather, ResnetFC MLP, softplus, colour sampling) runs in the
hand-written gfx950 kernels of libsdhip.so (``sd_field_query``; and, through
``render_fused``, the fused render+composite kernel ``sd_render_fused``).

Precision: ``precision="fp16"`` (default; f16 projected grid, f16 bilinear blend and
f16 MFMA, fp32 accumulate and fp32 geometry / compositing -- the reference's own AMP
dtype), ``"bf16"`` (BASELINE configs[1]'s dtype: the DINO output layer on bf16 MFMA, every
operand upstream of sigma in f16 -- an 8-bit mantissa there moves the composited depth past
SURVEY §8(c)'s 1e-2 m contract, tools/lowp_depth_emul.py) or ``"fp32"`` (f32 grid +
exact-f32 MFMA) for fp32-tolerance parity with the reference.  Both 16-bit modes meet the
1e-2 m depth contract.  Set via ``conf["precision"]`` or ``net.set_precision``.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..mlp_pack import PackedMLP
from ..pack_cache import module_key, steps, tensor_key, track_steps

EPS = 1e-3  # scenedino/common/cameras/pinhole.py:3
PRECISIONS = {"fp32": _lib.SD_F32, "bf16": _lib.SD_BF16, "fp16": _lib.SD_F16}


# the frame's render inputs made inside the projection launch (sd_project_grid_nhwc_inputs);
# SCENEDINO_AMD_FRAME_FUSED=0: their own sd_frame_inputs launch (A/B switch)
_FRAME_FUSED = __import__("os").environ.get("SCENEDINO_AMD_FRAME_FUSED", "1") != "0"


def voxel_chunks(n_points: int) -> int:
    """Chunks of a large predict_voxels query (SCENEDINO_AMD_VOXEL_CHUNKS, default 1: one
    field launch, then one seg-head launch); chunks below 2^18 points are not split."""
    import os
    k = max(1, int(os.environ.get("SCENEDINO_AMD_VOXEL_CHUNKS", "1")))
    return max(1, min(k, n_points >> 18))


def _id_list(ids):
    """View ids as a list of ints (None stays None): lists, tuples, tensors and arrays alike,
    without calling bool() on a multi-element tensor."""
    if ids is None:
        return None
    if hasattr(ids, "tolist"):
        ids = ids.tolist()
    if isinstance(ids, (int, float)):
        ids = [ids]
    return [int(i) for i in ids]


def _cam_records(poses_w2c, Ks):
    """(..., 4, 4) w2c and (..., 3, 3) K -> (..., 36) camera records (C ABI layout,
    sd_cam_records)."""
    return _lib.cam_records(poses_w2c, Ks)


def _take(t, ids):
    """t[:, ids] (bts.py:140-160).  A run of consecutive non-negative view ids is a slice
    view instead of an index gather: the same values, one kernel launch less per tensor
    per encode."""
    if (isinstance(ids, (list, tuple)) and len(ids) > 0 and isinstance(ids[0], int)
            and ids[0] >= 0 and ids[0] + len(ids) <= t.shape[1]
            and list(ids) == list(range(ids[0], ids[0] + len(ids)))):
        return t[:, ids[0]:ids[0] + len(ids)]
    return t[:, ids]


def _crop(img, top: int, left: int, height: int, width: int):
    """torchvision.transforms.functional.crop on a tensor: a slice, zero-filled where the
    window leaves the image (torchvision's tensor crop pads the missing border with 0)."""
    h, w = img.shape[-2:]
    bottom, right = top + height, left + width
    if top >= 0 and left >= 0 and bottom <= h and right <= w:
        return img[..., top:bottom, left:right]
    pad = (max(-left + min(0, right), 0), max(right - max(w, left), 0),
           max(-top + min(0, bottom), 0), max(bottom - max(h, top), 0))
    return F.pad(img[..., max(top, 0):bottom, max(left, 0):right], pad, value=0.0)


def shift_loss_images(images_loss, shift, h: int, w: int):
    """bts.py:197-205: ``transforms.Pad(8, padding_mode="edge")`` then
    ``functional.crop(i = 8 + shift[0], j = 8 + shift[1], h, w)`` on the (n, v, 3, H, W)
    loss images.  The reference tests ``shift != (0, 0)``, which is always True for the
    trainer's tensor and a crop at (8, 8) is the identity, so a zero shift is skipped
    here (same result, no copy)."""
    s0, s1 = (int(v) for v in shift)  # the trainer's CPU tensor (no device sync)
    if (s0, s1) == (0, 0):
        return images_loss
    n, v = images_loss.shape[:2]
    x = F.pad(images_loss.flatten(0, 1), (8, 8, 8, 8), mode="replicate")  # torchvision "edge"
    return _crop(x, 8 + s0, 8 + s1, h, w).unflatten(0, (n, v))


class BTSNet(nn.Module):
    def __init__(self, conf, encoder: nn.Module, code_xyz, heads: dict,
                 final_pred_head: str | None = None, uncertainty_predictor: nn.Module | None = None,
                 ren_nc=None, downstream_head: nn.Module | None = None):
        super().__init__()
        self.encoder = encoder
        self.code_xyz = code_xyz
        self.heads = nn.ModuleDict(heads)
        self.uncertainty_predictor = uncertainty_predictor
        self.extra_outs = self.encoder.extra_outs
        self.final_pred_head = final_pred_head if final_pred_head else list(self.heads.keys())[0]
        self.requires_bottleneck_feats = False
        self.use_viewdirs = conf.get("use_viewdirs", False)
        self.d_min, self.d_max = conf.get("z_near", 3), conf.get("z_far", 80)
        self.learn_empty = conf.get("learn_empty", True)
        self.empty_empty = conf.get("empty_empty", False)
        self.inv_z = conf.get("inv_z", True)
        self.color_interpolation = conf.get("color_interpolation", "bilinear")
        self.code_mode = conf.get("code_mode", "z")
        self.flip_augmentation = conf.get("flip_augmentation", False)
        self.return_sample_depth = conf.get("return_sample_depth", False)
        self.sample_color = conf.get("sample_color", True)
        self.predict_dino = conf.get("predict_dino", False)
        d_in = self.encoder.latent_size + self.code_xyz.d_out
        if self.sample_color and self.predict_dino:
            d_out = 1 + conf.get("dino_dims", 16)
        elif self.sample_color:
            d_out = 1
        else:
            d_out = 4
        self._d_in, self._d_out = d_in, d_out
        if self.learn_empty:
            self.empty_feature = nn.Parameter(torch.randn((self.encoder.latent_size,)))
        self._scale = 0
        self.downstream_head = downstream_head
        self.gt_classes = downstream_head.gt_classes if downstream_head is not None else None
        self.precision = conf.get("precision", "fp16")
        # "proj": 16-bit modes render from the projected grid P = W_in[:, :C] G + b_in
        # (sd_project_grid + sd_render_proj); "grid": per-sample C-channel gather
        # (sd_render_fused, also the only fp32 path)
        self.fused_mode = conf.get("fused_mode", "proj")
        self.kernel_timer = None  # optional: .start(name) / .stop(name) around launches
        self.render_into = None   # optional (R, D + 1 + 3 nv) f32 buffer for dino|depth|rgb
        self._packed = None
        self._packed_key = None
        # bumped by invalidate_packed (every training-path forward calls it): an optimizer step
        # may update the head in place without bumping the parameters' version counters
        # (torch's fused Adam), so the packed weights and the projected grid P made from them
        # are keyed by it and by the count of optimizer steps that touched this net
        # (pack_cache.track_steps, from the first training-path forward) too
        self._param_gen = 0
        self._grid_cache = None
        self._in_pass, self._pass_nhwc = False, None  # training-path NHWC grid per pass
        self._grid_key = None
        self._loss_features = None
        self._loss_pending = None
        self.grid_c_combine = None
        self.color_frame_filter = None
        self.grid_f_extra = None

    # -- reference API --------------------------------------------------------
    def set_scale(self, scale):
        self._scale = scale

    def get_scale(self):
        return self._scale

    def compute_grid_transforms(self, *args, **kwargs):
        pass

    def set_precision(self, precision: str):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        self.precision = precision
        self._packed = None
        self._grid_cache = None

    def encode(self, images, Ks, poses_c2w, ids_encoder=None, ids_render=None, ids_loss=None,
               images_alt=None, combine_ids=None, color_frame_filter=None,
               loss_feature_grid_shift=None):
        """Same semantics as bts.py:112-259 (encoder call, pose inversion, stored grids).

        loss_feature_grid_shift (trainer.py:186-198 passes ``torch.randint(-p/2, p/2, (2,))``
        every training step): the loss images are edge-padded by 8 and cropped at
        (8 + s0, 8 + s1) before the gt-encoder pass (bts.py:197-205), see
        ``shift_loss_images``."""
        if combine_ids is not None:
            raise NotImplementedError("combine_ids is a multi-view training option outside "
                                      "the MI355X hot path (every shipped config passes None)")
        with torch.autocast(device_type=images.device.type, enabled=False):
            # torch.inverse's LU (same kernels) without its device-to-host error check,
            # which would stall the launch queue once per frame
            # (made row-major once here: the batched inverse comes back column-major, and
            # every camera-record build would otherwise copy it)
            poses_w2c = torch.linalg.inv_ex(poses_c2w.float())[0].contiguous()
        if ids_encoder is None:
            images_encoder, Ks_encoder, poses_w2c_encoder = images, Ks, poses_w2c
        else:
            images_encoder = _take(images, ids_encoder)
            Ks_encoder = _take(Ks, ids_encoder)
            poses_w2c_encoder = _take(poses_w2c, ids_encoder)
        images_loss = images if ids_loss is None else _take(images, ids_loss)
        images = images_alt if images_alt is not None else images * 0.5 + 0.5
        if ids_render is None:
            images_render, Ks_render, poses_w2c_render = images, Ks, poses_w2c
        else:
            images_render = _take(images, ids_render)
            Ks_render = _take(Ks, ids_render)
            poses_w2c_render = _take(poses_w2c, ids_render)
        n_, nv_, c_, h_, w_ = images_encoder.shape
        n_l, nv_l = images_loss.shape[:2]
        do_flip = self.flip_augmentation and self.training and bool(torch.rand(1) > 0.5)
        if do_flip:
            images_encoder = torch.flip(images_encoder, dims=(-1,))
        lat = self.encoder(images_encoder.reshape(n_ * nv_, c_, h_, w_))
        if do_flip:
            lat = [torch.flip(x, dims=(-1,)) for x in lat]
        _, _, hh, ww = lat[0].shape
        # nearest resize to the first level's size (bts.py:197); at equal size it is the
        # identity, so that level (the 126-503 MB f32 grid) is viewed, not copied
        lat = [(x if tuple(x.shape[-2:]) == (hh, ww) else F.interpolate(x, size=(hh, ww)))
               .view(n_, nv_, -1, hh, ww) for x in lat]
        if self.extra_outs > 0:
            self.grid_f_extra = [x[:, :, -self.extra_outs:] for x in lat]
            lat = [x[:, :, :-self.extra_outs] for x in lat]
        else:
            self.grid_f_extra = None
        self.grid_f_features = lat
        self.grid_f_Ks = Ks_encoder
        self.grid_f_poses_w2c = poses_w2c_encoder
        self.grid_f_combine = None
        self.grid_c_imgs = images_render.detach()
        self.grid_c_Ks = Ks_render
        self.grid_c_poses_w2c = poses_w2c_render
        self.grid_c_combine = None
        # colour view = encoder view (the single-frame render): one set of camera records
        # for both, which lets the render kernel re-use the encoder projection for colours
        self._same_views = _id_list(ids_encoder) == _id_list(ids_render)
        # the ground-truth (loss) features: a second ViT pass (bts.py:207) that only the
        # training loss reads -- run on first access of grid_l_loss_features (SURVEY
        # §8(f) rank 3), so a pure render / voxel query never pays for it
        if loss_feature_grid_shift is not None:
            images_loss = shift_loss_images(images_loss, loss_feature_grid_shift, h_, w_)
        gt_in = images_loss.reshape(n_l * nv_l, c_, h_, w_).detach().clone()
        self._loss_pending = (gt_in, n_l, nv_l)
        self._loss_features = None
        self.color_frame_filter = color_frame_filter
        self._grid_cache = None

    @property
    def grid_l_loss_features(self):
        if self._loss_features is None and getattr(self, "_loss_pending", None) is not None:
            gt_in, n_l, nv_l = self._loss_pending
            lat_loss = self.encoder(gt_in, ground_truth=True)
            _, _, hl, wl = lat_loss[0].shape
            self._loss_features = [x.view(n_l, nv_l, -1, hl, wl) for x in lat_loss]
            self._loss_pending = None
        return self._loss_features

    @grid_l_loss_features.setter
    def grid_l_loss_features(self, value):
        self._loss_features = value
        self._loss_pending = None

    # -- device-side state for the kernels ------------------------------------
    def _dtype(self):
        if self.precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        return PRECISIONS[self.precision]

    def _use_proj(self) -> bool:
        if self.fused_mode not in ("proj", "grid"):
            raise ValueError("fused_mode must be 'proj' or 'grid'")
        # learn_empty substitutes a learned vector for out-of-frustum samples: the projected
        # grid has no slot for it, so those models render through the grid kernel
        return self.fused_mode == "proj" and self.precision != "fp32" and not self.learn_empty

    def fused_supported(self, K: int) -> bool:
        """The projected 16-bit render kernel takes K % 16 == 0, K <= 128 and D % 16 == 0,
        D <= 512 (D >= 128 through hidden-space compositing + the per-ray head GEMM); the
        grid kernel K % 32 == 0 and D in {32, 64, 128}; other shapes go through
        sd_field_query + sd_composite (also native)."""
        D = self._d_out - 1
        if self._differentiable():
            return False  # the renderer takes its generic (autograd) compositing path
        if self._use_proj():
            return K % 16 == 0 and K <= 128 and D % 16 == 0 and D <= 512
        return K % 32 == 0 and K <= 128 and D in (32, 64, 128)

    def _timed(self, name, fn):
        t = self.kernel_timer
        if t is not None:
            t.start(name)
        r = fn()
        if t is not None:
            t.stop(name)
        return r

    def _mlp(self):
        head = self.heads[self.final_pred_head]
        if getattr(head, "n_blocks", 0) != 0 or getattr(head, "d_latent", 0) != 0:
            raise NotImplementedError("fused field kernel supports ResnetFC(n_blocks=0) heads "
                                      "(every shipped config)")
        if len(self.heads) != 1:
            raise NotImplementedError("fused field kernel supports a single prediction head")
        ps = (head.lin_in.weight, head.lin_in.bias, head.lin_out.weight, head.lin_out.bias)
        empty = self.empty_feature if self.learn_empty else None
        key = tensor_key(*ps, *([empty] if empty is not None else [])) + (
            self.precision, getattr(self, "_param_gen", 0), steps(self))
        if self._packed is None or self._packed_key != key:
            self._packed = PackedMLP(*ps, dtype=self._dtype(), empty_feature=empty)
            self._packed_key = key
        return self._packed

    def invalidate_packed(self):
        """Drop the inference kernels' packed head weights and everything made from them (the
        projected grid P): the next query / render re-packs from the parameters as they are
        then.  Parameter updates are seen through the tensors' version counters and through
        torch optimizer steps (the step hook); call this after an update neither shows --
        ``.data`` writes, a custom optimizer that does not go through ``Optimizer.step``, or
        the replay of a HIP graph that captured the step."""
        self._packed = None
        self._packed_q = None
        self._param_gen = getattr(self, "_param_gen", 0) + 1  # stales P's cache entries as well

    def _mlp_projq(self):
        """Field MLP over the projected grid: first layer [I_128 | W_in's code columns] with
        a zero bias (P already holds W_in[:, :C] G + b_in), the output layer unchanged."""
        head = self.heads[self.final_pred_head]
        self._mlp()
        key = self._packed_key
        if getattr(self, "_packed_q", None) is None or self._packed_q[0] != key:
            W_in, W_out = head.lin_in.weight.detach(), head.lin_out.weight.detach()
            C = W_in.shape[1] - self.code_xyz.d_out
            dh = W_in.shape[0]
            Wq = torch.cat((torch.eye(dh, device=W_in.device, dtype=W_in.dtype), W_in[:, C:]), 1)
            bq = torch.zeros(dh, device=W_in.device, dtype=W_in.dtype)
            self._packed_q = (key, PackedMLP(Wq, bq, W_out, head.lin_out.bias.detach(),
                                             dtype=self._dtype()))
        return self._packed_q[1]

    def _grids(self):
        g = self.grid_f_features[self._scale]
        key = (id(g), g._version, id(self.grid_c_imgs), self.grid_c_imgs._version,
               id(self.grid_f_poses_w2c), id(self.grid_c_poses_w2c), self.precision)
        if self._grid_cache is not None and self._grid_key == key:
            return self._grid_cache
        B, nvf, C, Hf, Wf = g.shape
        if nvf != 1:
            raise NotImplementedError("the field kernels take exactly one encoder view "
                                      "(ids_encoder=[0], as every shipped config)")
        imgs = self.grid_c_imgs
        n, nv, c3, H, W = imgs.shape
        # the colour images and the encoder cameras (sd_frame_inputs) are made on first use
        # (_frame): inside the projection launch when the projected render runs next
        # grid_nchw feeds the inference kernels only (packing / projection): held DETACHED.
        # A view with a grad_fn would keep the grid leaf's AccumulateGrad node alive across
        # steps, bound to the stream of the step that created it -- the round-4 graph-mode
        # training crash: the node was made on the legacy default stream by an eager
        # warm-up step, and the captured backward then had the engine make that stream wait on
        # the capture stream, which the default stream cannot join (host segfault in HIP).
        cache = {
            "grid_nchw": g.detach().reshape(B, C, Hf, Wf), "grid": None, "proj": None, "proj_exact": None,
            "C": C, "Hf": Hf, "Wf": Wf, "B": B,
            "cam_f": None, "img": None, "cam_c": None, "nv": nv, "Hc": H, "Wc": W,
            "frame": (imgs.reshape(n * nv, c3, H, W).float().contiguous(),
                      self.grid_f_poses_w2c[:, 0], self.grid_f_Ks[:, 0]),
        }
        self._grid_cache, self._grid_key = cache, key
        return cache

    def _set_frame(self, gc, img, cam_f):
        B, nv = gc["B"], gc["nv"]
        gc["img"], gc["cam_f"], gc["frame"] = img, cam_f, None
        if nv == 1 and getattr(self, "_same_views", False):
            gc["cam_c"] = cam_f.view(B, 1, -1)
        else:
            gc["cam_c"] = _cam_records(self.grid_c_poses_w2c, self.grid_c_Ks)

    def _frame(self, gc):
        """The cached frame's packed colour images and camera records (one sd_frame_inputs
        launch, unless the projection launch already made them)."""
        if gc["frame"] is not None:
            imgs, w2c, Ks = gc["frame"]
            self._set_frame(gc, *_lib.frame_inputs(imgs, w2c, Ks))
        return gc

    def _grid_nhwc(self, gc):
        """Encoder grid packed NHWC in the field dtype (sd_render_fused / sd_field_query;
        f16 for both 16-bit modes, _lib.FIELD_DTYPE)."""
        if gc["grid"] is None:
            gc["grid"] = _lib.pack_grid(gc["grid_nchw"].float(), _lib.FIELD_DTYPE[self._dtype()])
        return gc["grid"]

    def _grid_proj(self, gc, m, exact_grid=False):
        """Projected grid P = W_in[:, :C] G + b_in, (B, Hf, Wf, 128) (sd_render_proj).
        exact_grid: the grid enters the projection as a hi + lo f16 pair (SD_PROJ_EXACT_GRID;
        the K > 64 renders ask for it).  The plain and the exact P are two cache
        entries, each valid for the packed weights it was projected with: a K <= 64 render or
        a query never reads the exact P, so what a call returns does not depend on which
        renders of the frame ran before it."""
        slot = "proj_exact" if exact_grid else "proj"
        hit = gc[slot]
        if hit is None or hit[0] != self._packed_key:
            g = gc["grid_nchw"].float()  # NCHW or the native encoder's channels-last grid
            if gc["frame"] is not None and _FRAME_FUSED:  # a new frame: its render inputs in the same launch
                imgs, w2c, Ks = gc["frame"]
                res = self._timed("project", lambda: _lib.project_grid_inputs(
                    g, m.rec, m.dtype, imgs, w2c, Ks, exact_grid=exact_grid))
                p = res[0]
                self._set_frame(gc, res[1], res[2])
            else:
                p = self._timed("project", lambda: _lib.project_grid(
                    g, m.rec, m.dtype, exact_grid=exact_grid))
            hit = gc[slot] = (self._packed_key, p)
        return hit[1]

    def _differentiable(self) -> bool:
        """Training path (autograd through sd_field_gather / ResnetFC / sd_composite) when
        grad mode is on and the module trains or its feature grid carries a gradient;
        otherwise the fused inference kernels."""
        if not torch.is_grad_enabled():
            return False
        g = self.grid_f_features[self._scale] if self.grid_f_features else None
        return self.training or (g is not None and g.requires_grad)

    def wants_single_chunk(self) -> bool:
        """Renderer hook: the training path takes all of a pass's points in one call (the
        eval_batch_size chunking of nerf.py:268-326 only bounds memory; the results are the
        same, and per-chunk launch + autograd overhead dominates a 262 144-point step)."""
        return self._differentiable()

    def begin_pass(self):
        """Renderer hook: the chunked model calls of one compositing pass follow."""
        self._in_pass, self._pass_nhwc = True, None

    def end_pass(self):
        self._in_pass, self._pass_nhwc = False, None

    def _check_supported(self):
        if self.grid_c_combine is not None or self.color_frame_filter is not None:
            raise NotImplementedError("grid_c_combine / color_frame_filter (training) unsupported")
        if self.grid_f_extra is not None:
            raise NotImplementedError("extra encoder outputs unsupported")
        if not (self.sample_color and self.predict_dino) or self.code_mode != "z" or not self.inv_z:
            raise NotImplementedError("field kernels implement predict_dino + sample_color, "
                                      "code_mode=z, inv_z (every shipped config)")
        if (self.d_min, self.d_max) != (3, 80):
            raise NotImplementedError("field kernels bake z_near=3, z_far=80 into the code")

    # -- hot path -------------------------------------------------------------
    def render_fused(self, rays, z, sb, hard_alpha_cap, want_weights=True, want_alphas=True,
                     want_rgb_samps=False, K=None, z_seed=None, lindisp=True, z_offset=0):
        """Fused field query + alpha compositing for all rays (used by NeRFRenderer).
        rays (R, ray_dim) fp32, z (R, K) fp32 on the GPU; R = sb * rays_per_sb.
        z None: K depths per ray drawn as sd_sample_z(seed=z_seed, lindisp) would -- inside
        the projected render kernel (no (R, K) array), or by sd_sample_z for the grid
        kernel."""
        self._check_supported()
        m = self._mlp()
        gc = self._grids()
        if gc["C"] != m.C:
            raise ValueError(f"feature grid has {gc['C']} channels, the MLP expects {m.C}")
        proj = self._use_proj()
        rays = rays.float().contiguous()
        if z is None:
            if K is None or z_seed is None:
                raise ValueError("render_fused: z=None needs K and z_seed")
            if not proj:
                z = _lib.sample_z(rays, K, lindisp, seed=z_seed, offset=int(z_offset))
        R = rays.shape[0]
        K = z.shape[1] if z is not None else K
        if R % sb or gc["B"] != sb:
            raise ValueError(f"rays ({R}) must split into {sb} super-batches matching the "
                             f"encoded batch ({gc['B']})")
        dev = rays.device
        nv = gc["nv"]
        maps = getattr(self, "render_into", None)
        if maps is not None:
            # render straight into packed [dino | depth | rgb] rows (the all-gather send
            # buffer of the multi-GPU path): strided views, no pack copy; dino leads the
            # row so its 16-B vector stores stay aligned (width 68 at D = 64, nv = 1)
            if not proj or tuple(maps.shape) != (R, m.D + 1 + 3 * nv) or maps.stride(1) != 1 \
                    or maps.dtype != torch.float32 or maps.device != dev:
                raise ValueError(f"render_into must be a float32 ({R}, {m.D + 1 + 3 * nv}) row-major "
                                 "tensor on the render device (16-bit projected render)")
            dino, depth, rgb = maps[:, :m.D], maps[:, m.D], maps[:, m.D + 1:]
        else:
            depth = torch.empty(R, device=dev)
            dino = torch.empty(R, m.D, device=dev)
            rgb = torch.empty(R, 3 * nv, device=dev)
        out = {
            "depth": depth,
            "dino": dino,
            "rgb": rgb,
            "invalid": torch.empty(R, K, nv, device=dev),
            "invalid_f": torch.empty(R, K, device=dev, dtype=torch.bool),  # bytes 0 / 1
            "weights": torch.empty(R, K, device=dev) if want_weights else None,
            "alphas": torch.empty(R, K, device=dev) if want_alphas else None,
            "rgb_samps": torch.empty(R, K, 3 * nv, device=dev) if want_rgb_samps else None,
        }
        if z is not None:
            z = z.contiguous()
        # K > 64 (configs[3]'s 128 samples): the projection's grid rounding alone moves the
        # composited depth by up to 5.8e-3 m, so those renders project the grid exactly
        # (hi + lo operands); K <= 64 meets the 1e-2 m bound with one rounding
        grid = self._grid_proj(gc, m, exact_grid=K > 64) if proj else self._grid_nhwc(gc)
        self._frame(gc)
        args = _lib.SdRenderArgs(
            rays=rays.data_ptr(), ray_dim=rays.shape[1], R=R, rays_per_sb=R // sb, K=K,
            z=z.data_ptr() if z is not None else None, grid=grid.data_ptr(), Hf=gc["Hf"],
            Wf=gc["Wf"],
            cam_f=gc["cam_f"].data_ptr(), img=gc["img"].data_ptr(), nv=nv, Hc=gc["Hc"],
            Wc=gc["Wc"], cam_c=gc["cam_c"].data_ptr(), hard_alpha_cap=int(bool(hard_alpha_cap)),
            depth=out["depth"].data_ptr(), dino=out["dino"].data_ptr(),
            rgb=out["rgb"].data_ptr(),
            weights=out["weights"].data_ptr() if want_weights else None,
            alphas=out["alphas"].data_ptr() if want_alphas else None,
            invalid=out["invalid"].data_ptr(), invalid_f=out["invalid_f"].data_ptr(),
            rgb_samps=out["rgb_samps"].data_ptr() if want_rgb_samps else None,
            z_lindisp=int(bool(lindisp)), z_seed=(z_seed or 0) & (2**64 - 1), z_offset=int(z_offset),
            ld_depth=depth.stride(0) if maps is not None else 0,
            ld_dino=dino.stride(0) if maps is not None else 0,
            ld_rgb=rgb.stride(0) if maps is not None else 0,
            grid_dtype=_lib.SD_OF_TORCH[grid.dtype])
        if proj:
            wb = _lib.render_proj_work_bytes(R, m.D)
            work = torch.empty(wb // 4, device=dev) if wb > 0 else None
            args.work = work.data_ptr() if work is not None else None
            self._last_render_work = work  # diagnostics (tools/ovf_count.py: the overflow list)
            self._timed("render", lambda: _lib.render_proj(args, m.head_rec, rays))
        else:
            self._timed("render", lambda: _lib.render_fused(args, m.rec, rays))
        return out

    def _tile_order(self, xyz, gc):
        """Visiting order of sd_field_query's 32-point tiles for large voxel queries: tiles
        sorted by the 16-texel cell their middle point projects to (column-major over the
        grid image, points behind the camera last), so the workgroups of an XCD gather
        neighbouring texels of the projected grid from its L2 instead of every tile
        fetching its own (SSCBench's (x, y) voxel columns project to vertical segments).
        Speed only: outputs stay at their point indices.  Cached per (points, camera)."""
        n, P, _ = xyz.shape
        NP = n * P
        nt = (NP + 31) // 32
        w2c, Ks = self.grid_f_poses_w2c, self.grid_f_Ks
        key = (xyz.data_ptr(), xyz._version, NP, w2c.data_ptr(), w2c._version, Ks.data_ptr(),
               Ks._version, gc["Hf"], gc["Wf"])
        c = self.__dict__.setdefault("_order_cache", {})  # (chunked queries: one per chunk)
        if key in c:
            return c[key]
        dev = xyz.device
        idx = (torch.arange(nt, device=dev) * 32 + 16).clamp_max(NP - 1)
        pts = xyz.reshape(NP, 3).float().index_select(0, idx)
        b = torch.div(idx, P, rounding_mode="floor")
        R = w2c[:, 0, :3, :3].float()[b]
        t = w2c[:, 0, :3, 3].float()[b]
        cam = torch.einsum("tij,tj->ti", R, pts) + t
        uvw = torch.einsum("tij,tj->ti", Ks[:, 0].float()[b], cam)
        z = uvw[:, 2]
        front = z > 1e-3
        u = (uvw[:, 0] / z.clamp_min(1e-3)).clamp(-2, 2)
        v = (uvw[:, 1] / z.clamp_min(1e-3)).clamp(-2, 2)
        ub = ((u + 2) * (gc["Wf"] / 32)).floor()
        vb = ((v + 2) * (gc["Hf"] / 32)).floor()
        cell = torch.where(front, ub * 4096 + vb, torch.full_like(ub, 2.0 ** 24))
        order = torch.argsort(b.double() * 2.0 ** 26 + cell.double(), stable=True).to(torch.int32)
        if len(c) >= 16:
            c.clear()
        c[key] = order
        return order

    def query(self, xyz, colors: bool = True, dino_dtype=torch.float32, locality=None):
        """Raw per-point field: sigma (n,P), dino (n,P,D), rgb (n,P,3nv), invalid (n,P,nv),
        invalid_features (n,P) -- all from sd_field_query.  colors=False skips the colour
        sampling (the predict_segmentation path, bts.py:528-533): rgb / invalid are None.
        dino_dtype bfloat16: dino for sd_seg_query, which rounds its input to bf16 anyway.
        locality (default: colour-free queries of >= 2^18 points, the SSCBench voxels):
        visit the point tiles in projected-texel order (_tile_order; same outputs)."""
        self._check_supported()
        m = self._mlp()
        gc = self._grids()
        if gc["C"] != m.C:
            raise ValueError(f"feature grid has {gc['C']} channels, the MLP expects {m.C}")
        if self._use_proj():
            # 16-bit projected mode: the same field kernel on the projected grid P
            # (B, Hf, Wf, 128) = W_in[:, :C] G + b_in with an identity first layer for its
            # 128 columns (gather 4 x 256 B per point instead of 4 x 512 B, 8 instead of 16
            # grid k-steps); P is the one the renders use, projected once per encode
            grid = self._grid_proj(gc, m)
            m = self._mlp_projq()
        else:
            grid = self._grid_nhwc(gc)
        self._frame(gc)
        n, P, _ = xyz.shape
        if n != gc["B"]:
            raise ValueError(f"xyz batch {n} != encoded batch {gc['B']}")
        dev = xyz.device
        nv = gc["nv"] if colors else 0
        xyz = xyz.float().contiguous()
        sigma = torch.empty(n, P, device=dev)
        dino = torch.empty(n, P, m.D, device=dev, dtype=dino_dtype)
        rgb = torch.empty(n, P, 3 * nv, device=dev) if colors else None
        inv = torch.empty(n, P, nv, device=dev) if colors else None
        invf = torch.empty(n, P, device=dev, dtype=torch.bool)  # bytes 0 / 1
        if locality is None:
            locality = not colors and n * P >= (1 << 18)
        order = self._tile_order(xyz, gc) if locality else None
        args = _lib.SdFieldArgs(
            xyz=xyz.data_ptr(), B=n, P=P, grid=grid.data_ptr(), Hf=gc["Hf"],
            Wf=gc["Wf"],
            cam_f=gc["cam_f"].data_ptr(), img=gc["img"].data_ptr() if colors else None, nv=nv,
            Hc=gc["Hc"], Wc=gc["Wc"], cam_c=gc["cam_c"].data_ptr(), sigma=sigma.data_ptr(),
            dino=dino.data_ptr(), rgb=rgb.data_ptr() if colors else None,
            invalid=inv.data_ptr() if colors else None, invalid_f=invf.data_ptr(),
            dino_dtype=_lib.SD_BF16 if dino_dtype == torch.bfloat16 else _lib.SD_F32,
            grid_dtype=_lib.SD_OF_TORCH[grid.dtype],
            tile_order=order.data_ptr() if order is not None else None)
        self._timed("field", lambda: _lib.field_query(args, m.rec, xyz))
        return sigma, dino, rgb, inv, invf

    def _fused_train_mlp(self, head, C, n_rows) -> bool:
        """Training under a 16-bit autocast with the shipped head (ResnetFC n_blocks = 0,
        ReLU, input = C grid channels + the positional code) at a shape the sd_mlp_train
        kernels run (mlp_pack.fused_train_shape_ok: d_hidden 128, D a multiple of 8 up to 64,
        C a multiple of 32 up to 256, n_rows rows below 4 GiB): gather + MLP as the fused
        kernels.  Any other head or shape takes FieldGather + FieldMLP."""
        from ..mlp_pack import fused_train_shape_ok
        return (torch.is_autocast_enabled("cuda")
                and head.lin_in.in_features == C + self.code_xyz.d_out
                and torch.get_autocast_dtype("cuda") in (torch.float16, torch.bfloat16)
                and type(head).__name__ == "ResnetFC" and getattr(head, "n_blocks", 1) == 0
                and getattr(head, "d_latent", 1) == 0 and isinstance(head.activation, nn.ReLU)
                and getattr(head, "view_number", None) in (None, 0)
                and fused_train_shape_ok(head.lin_in.weight.shape[0], head.lin_in.in_features,
                                         head.lin_out.weight.shape[0] - 1, C, n_rows,
                                         head.lin_in.in_features + 1))

    def _query_diff(self, xyz):
        """query() with autograd (training path, scenedino_amd/autograd.py): the grid is
        gathered by sd_field_gather (backward sd_field_gather_bwd) and the prediction head
        runs as its own nn.Linear layers, so gradients reach grid_f_features and the head
        parameters as in bts.py:476-595."""
        from ..autograd import FieldGather, FieldGatherMLP, FieldMLP, GatherAcc, GridNHWC
        self._check_supported()
        # a training step follows: the inference kernels' packed weights are stale from here
        # on (an optimizer may update the parameters in place without bumping their version
        # counters -- torch's fused Adam does -- so the version key alone cannot tell).  An
        # inference query between this forward and the step re-packs the pre-step weights, so
        # the step invalidates them again (the optimizer step hook)
        track_steps(self)
        self.invalidate_packed()
        head = self.heads[self.final_pred_head]
        if len(self.heads) != 1:
            raise NotImplementedError("the field path supports a single prediction head")
        gc = self._frame(self._grids())
        g = self.grid_f_features[self._scale]
        n, P, _ = xyz.shape
        if n != gc["B"]:
            raise ValueError(f"xyz batch {n} != encoded batch {gc['B']}")
        # NHWC copy of the grid (differentiable); shared by the chunks of one compositing
        # pass (begin_pass / end_pass from the renderer), else made per call
        key = (id(g), g._version)
        nh = self._pass_nhwc
        if nh is None or nh[0] != key:
            # (B, 1, C, Hf, Wf) -> (B, C, Hf, Wf) as a view: its backward is a view too,
            # where g[:, 0]'s select backward zero-fills and copies the whole grid gradient
            g0 = g.flatten(0, 1) if g.shape[1] == 1 else g[:, 0]
            nh = (key, GridNHWC.apply(g0), GatherAcc())
            if self._in_pass:
                self._pass_nhwc = nh
        if self._fused_train_mlp(head, gc["C"], n * P):
            sigma, dino, invf, rgb, inv = FieldGatherMLP.apply(
                nh[1], xyz.float().contiguous(), gc["cam_f"], gc["img"], gc["cam_c"], True, nh[2],
                self.empty_feature if self.learn_empty else None, head.lin_in.weight,
                head.lin_in.bias, head.lin_out.weight, head.lin_out.bias)
            return sigma, dino, rgb, inv, invf
        x, invf, rgb, inv = FieldGather.apply(nh[1], xyz.float().contiguous(), gc["cam_f"],
                                              gc["img"], gc["cam_c"], True, nh[2])
        x = x.reshape(n * P, -1)
        if self.learn_empty:  # bts.py:311-319: out-of-frustum samples see the learned vector
            C = gc["C"]
            e = self.empty_feature.to(x.dtype).view(1, C)
            x = torch.cat((torch.where(invf.reshape(-1, 1), e, x[:, :C]), x[:, C:]), 1)
        if (type(head).__name__ == "ResnetFC" and getattr(head, "n_blocks", 1) == 0
                and getattr(head, "d_latent", 1) == 0 and isinstance(head.activation, nn.ReLU)
                and getattr(head, "view_number", None) in (None, 0)):
            out = FieldMLP.apply(x, head.lin_in.weight, head.lin_in.bias,
                                 head.lin_out.weight, head.lin_out.bias).reshape(n, P, -1)
        else:  # any other head: its own forward on [feat | code] (bts.py:502-514)
            out = head(x[:, :-1].reshape(n * P, 1, -1)).reshape(n, P, -1)
        sigma = F.softplus(out[..., 0])
        return sigma, out[..., 1:], rgb, inv, invf

    # -- segmentation head (SSCBench / inference_3d) ----------------------------
    def _dim_reduction(self):
        dr = getattr(self.encoder, "dim_reduction", None)
        if dr is None or not (hasattr(dr, "linear_in") and hasattr(dr, "linear_out")):
            return None
        return dr

    def _seg_rec(self, with_head: bool):
        """PackedSegHead for encoder.dim_reduction (+ downstream_head's stego path)."""
        from ..seg_pack import PackedSegHead
        dr = self._dim_reduction()
        if dr is None:
            raise NotImplementedError("sd_seg_query needs encoder.dim_reduction = MlpDimReduction "
                                      "(dim_reduction_arch: mlp, every shipped config)")
        dh = self.downstream_head if with_head else None
        stego = getattr(dh, "stego_head", None) if dh is not None else None
        clus = getattr(dh, "stego_cluster_head", None) if dh is not None else None
        fp8 = getattr(self, "seg_precision", "bf16") == "fp8"
        # steps(dh): the k-means centres train through plain autograd, under the head's count
        key = module_key(dr, stego, clus) + (with_head, fp8, steps(dh) if dh is not None else 0)
        cache = getattr(self, "_seg_cache", None)
        if cache is None or cache[0] != key:
            rec = PackedSegHead(dr, stego, clus, device=dr.linear_in.weight.device,
                                fp8=fp8 and with_head)
            self._seg_cache = cache = (key, rec)
        return cache[1]

    def predict_voxels(self, xyz, voxel_size: float = 0.2, prediction_mode="stego_kmeans"):
        """SSCBench per-chunk query, GPU-resident (evaluate_model_sscbench.py:717-742 at
        factor 1 with USE_ALPHA_WEIGHTING): xyz (1, P, 3) -> sigma (P,) f32 and the
        alpha-weighted class seg (P,) uint8 = label if 1 - exp(-voxel_size sigma) > 0 else 0.
        sd_field_query (no colours) + sd_seg_query; the 768-d features never reach HBM."""
        if prediction_mode != "stego_kmeans":
            raise NotImplementedError("predict_voxels implements prediction_mode='stego_kmeans' "
                                      "(the SSCBench 'scenedino' mode)")
        if self.downstream_head is None:
            raise ValueError("predict_voxels needs a downstream (segmentation) head")
        rec = self._seg_rec(True)
        n_, P_all, _ = xyz.shape
        nch = voxel_chunks(n_ * P_all)
        if n_ == 1 and nch > 1 and not torch.cuda.is_current_stream_capturing():
            return self._predict_voxels_chunked(xyz, rec, voxel_size, nch)
        sigma, dino, _, _, _ = self.query(xyz, colors=False, dino_dtype=torch.bfloat16)
        P = sigma.numel()
        _, seg, _ = self._timed("seg", lambda: _lib.seg_query(
            dino.reshape(P, -1), rec.rec, sigma=sigma.reshape(P), voxel_size=voxel_size,
            want_labels=False, want_seg=True))
        return sigma.reshape(P), seg

    def _predict_voxels_chunked(self, xyz, rec, voxel_size, nch):
        """predict_voxels over ``nch`` point chunks, the field query of chunk i + 1 on the
        current stream while the seg head of chunk i runs on a side stream (the two kernels'
        workgroups share the CUs: k_field waits on its grid gathers, k_seg_head on its MFMA
        chains).  Same outputs as one launch of each (point-wise kernels)."""
        P = xyz.shape[1]
        main = torch.cuda.current_stream(xyz.device)
        side = getattr(self, "_seg_side", None)
        if side is None or side.device != xyz.device:
            side = self._seg_side = torch.cuda.Stream(device=xyz.device)
        # chunk bounds on 256-point boundaries (whole k_seg_head workgroups)
        cut = [min(P, ((P * i // nch) + 255) // 256 * 256) for i in range(nch)] + [P]
        sigmas, segs = [], []
        for a, b in zip(cut[:-1], cut[1:]):
            if b <= a:
                continue
            sigma, dino, _, _, _ = self.query(xyz[:, a:b], colors=False,
                                              dino_dtype=torch.bfloat16)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                _, seg, _ = self._timed("seg", lambda: _lib.seg_query(
                    dino.reshape(b - a, -1), rec.rec, sigma=sigma.reshape(-1),
                    voxel_size=voxel_size, want_labels=False, want_seg=True))
            dino.record_stream(side)
            sigma.record_stream(side)
            seg.record_stream(main)
            sigmas.append(sigma.reshape(-1))
            segs.append(seg)
        main.wait_stream(side)
        return torch.cat(sigmas), torch.cat(segs)

    def forward(self, xyz: torch.Tensor, **kwargs):
        """Same return contract as bts.py:476-595."""
        only_density = kwargs.get("only_density", False)
        render_flow = kwargs.get("render_flow", False)
        predict_segmentation = kwargs.get("predict_segmentation", False)
        prediction_mode = kwargs.get("prediction_mode", "stego_kmeans")
        if render_flow:
            raise NotImplementedError("render_flow is a training-only option")
        with torch.profiler.record_function("model_inference"):
            n_, n_pts, _ = xyz.shape
            if not predict_segmentation and self._differentiable():
                sigma, dino, rgb, inv, invf = self._query_diff(xyz)
            else:
                sigma, dino, rgb, inv, invf = self.query(xyz, colors=not predict_segmentation)
            sigma = sigma.unsqueeze(-1)
            if predict_segmentation:  # bts.py:584-592
                D = dino.shape[-1]
                fused = (self._dim_reduction() is not None and
                         (self.downstream_head is None or prediction_mode == "stego_kmeans"))
                if not fused:  # a foreign dim reduction / another head mode: their own forward
                    dino_full = self.encoder.expand_dim(dino)
                    seg = (self.downstream_head(dino_full, mode=prediction_mode)
                           if self.downstream_head is not None else None)
                else:
                    with_head = self.downstream_head is not None
                    rec = self._seg_rec(with_head)
                    labels, _, full = self._timed("seg", lambda: _lib.seg_query(
                        dino.reshape(-1, D).contiguous(), rec.rec, want_labels=with_head,
                        want_full=True))
                    dino_full = full.view(n_, n_pts, -1)
                    seg = labels.view(n_, n_pts).long() if with_head else None
                if seg is not None:
                    seg = F.one_hot(seg, self.gt_classes)
                return dino_full, None, sigma, seg
            if only_density:
                rgb = torch.zeros((n_, n_pts, rgb.shape[-1]), device=sigma.device)
                invalid = invf.unsqueeze(-1).to(sigma.dtype)
            else:
                invalid = inv
            state_dict = {"invalid_features": invf.reshape(1, n_ * n_pts, 1),
                          "dino_features": dino}
            return rgb, invalid, sigma, None, state_dict
