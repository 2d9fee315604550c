"""Ground-truth feature wrappers of ``mode="upsample-gt"``, MI355X build.

Mirror of scenedino/models/backbones/dino/upsampler.py:17-205 (``MultiScaleCropGT_kornia``,
``InterpolatedGT``) and dinov2_module.py:69-76 (``build_gt_upsampling_wrapper``): per-pixel DINO
targets for the loss, the gt encoder's token grids of the image, its flip and ``num_views - 2``
random crops, upsampled, warped back onto the image and averaged where valid.

``MultiScaleCropGT`` has two routes with the same results:

* the torch route, a restatement of ``forward_chunk`` / ``_accumulate_predictions`` line by line
  (four channel chunks, NaN masking, ``nanmean``), on any device and dtype.  kornia is not a
  dependency: ``warp_perspective`` below restates its definition (normalise the homography,
  ``align_corners=True`` meshgrid, ``F.grid_sample``);
* the native route (``sd_msc_gt``, csrc/sdhip_msc.hip) on GPU f32 grids inside the kernel's
  domain: one launch that writes the (B, C, H, W) result once.

``last_route`` names the route of the latest call; ``native = False`` forces the torch route.

The views come from ``sample_views(n_images)``, which a test or a user can replace on the
instance.  The default draws a Bernoulli(0.5) flip and a ``RandomResizedCrop`` box per view on
torch's RNG.  **Parity unpinned**: the reference draws with kornia, which cannot be installed
beside this build, so neither its draw order nor its reading of the ``ratio`` argument (the
reference passes H / W-based bounds) is compared; ``ratio`` is a constructor argument for that
reason.  Given the views, the geometry is fixed: flip first, then crop to the box and resize to
the image with ``align_corners=True``.

The wrappers hold the gt encoder without registering it as a submodule, so the owning module's
``state_dict`` has no ``gt_wrapper.*`` keys (the weights arrive through ``gt_encoder.*``).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn


def _inv3(m):
    """Inverse of (..., 3, 3) matrices by the adjugate (no solver library, no host sync)."""
    a, b, c = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2]
    d, e, f = m[..., 1, 0], m[..., 1, 1], m[..., 1, 2]
    g, h, i = m[..., 2, 0], m[..., 2, 1], m[..., 2, 2]
    co = torch.stack([e * i - f * h, c * h - b * i, b * f - c * e,
                      f * g - d * i, a * i - c * g, c * d - a * f,
                      d * h - e * g, b * g - a * h, a * e - b * d], dim=-1)
    det = a * co[..., 0] + b * co[..., 3] + c * co[..., 6]
    return (co / det.unsqueeze(-1)).reshape(m.shape)


def _normal_transform_pixel(h, w, like):
    """Pixel -> [-1, 1] coordinates with ``align_corners=True`` (kornia's
    normal_transform_pixel; a size of 1 divides by 1e-14 as there)."""
    wd = 1e-14 if w == 1 else w - 1.0
    hd = 1e-14 if h == 1 else h - 1.0
    return like.new_tensor([[2.0 / wd, 0.0, -1.0], [0.0, 2.0 / hd, -1.0], [0.0, 0.0, 1.0]])


def warp_perspective(src, M, dsize, mode="bilinear"):
    """kornia.geometry.warp_perspective(src, M, dsize, mode, padding_mode="zeros",
    align_corners=True) from its definition: M (B, 3, 3) maps source to destination pixel
    coordinates; destination pixel q samples the source at M^-1 q."""
    H, W = src.shape[-2:]
    h, w = dsize
    M = M.to(src.dtype)
    dst_norm_trans_src_norm = _normal_transform_pixel(h, w, src) @ (
        M @ _inv3(_normal_transform_pixel(H, W, src)))
    src_norm_trans_dst_norm = _inv3(dst_norm_trans_src_norm)
    ys = torch.linspace(-1, 1, h, dtype=src.dtype, device=src.device)
    xs = torch.linspace(-1, 1, w, dtype=src.dtype, device=src.device)
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    pts = torch.stack([gx, gy, torch.ones_like(gx)], dim=-1).reshape(1, h * w, 3)
    p = pts @ src_norm_trans_dst_norm.transpose(1, 2)
    grid = (p[..., :2] / p[..., 2:]).reshape(-1, h, w, 2)
    return F.grid_sample(src, grid, mode=mode, padding_mode="zeros", align_corners=True)


def view_transforms(boxes, flips, image_size):
    """(n, k, 3, 3) f32 homographies T = T_crop T_flip from image to augmented-view pixel
    coordinates: T_flip maps u -> W-1-u, T_crop maps u -> (u - x0)(W-1)/(w-1) and
    v -> (v - y0)(H-1)/(h-1), for boxes (n, k, 4) = [x0, y0, w, h] and flips (n, k)."""
    H, W = image_size
    boxes = torch.as_tensor(boxes, dtype=torch.float64)
    flips = torch.as_tensor(flips).to(torch.bool)
    x0, y0, w, h = boxes.unbind(-1)
    sx, sy = (W - 1) / (w - 1), (H - 1) / (h - 1)
    T = torch.zeros(*boxes.shape[:-1], 3, 3, dtype=torch.float64)
    T[..., 0, 0] = torch.where(flips, -sx, sx)
    T[..., 0, 2] = torch.where(flips, sx * (W - 1 - x0), -sx * x0)
    T[..., 1, 1] = sy
    T[..., 1, 2] = -sy * y0
    T[..., 2, 2] = 1.0
    return T.float()


class MultiScaleCropGT(nn.Module):
    """upsampler.py:17-194 (``MultiScaleCropGT_kornia``)."""

    max_chunk = 16  # upsampler.py:184

    def __init__(self, gt_encoder: nn.Module, num_views: int = 4,
                 image_size: Tuple[int, int] = (192, 640),
                 scale: Tuple[float, float] = (0.5, 1.0),
                 ratio: Optional[Tuple[float, float]] = None) -> None:
        super().__init__()
        if num_views < 2:
            raise ValueError("MultiScaleCropGT: num_views counts the image and its flip (>= 2)")
        object.__setattr__(self, "gt_encoder", gt_encoder)  # not a registered submodule
        self.augmentations_per_sample = int(num_views)
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.scale = (float(scale[0]), float(scale[1]))
        if ratio is None:  # crops within 20 % of the image's aspect
            r = self.image_size[1] / self.image_size[0]
            ratio = (r / 1.2, r * 1.2)
        self.ratio = (float(ratio[0]), float(ratio[1]))
        self.native = True        # False: always the torch route
        self.last_route = None    # "native" / "torch": the route of the latest call
        self.last_reason = None   # why the latest call left the native route (None: it did not)

    # ------------------------------------------------------------------------ views
    def _draw_box(self):
        """torchvision's RandomResizedCrop.get_params rule on torch's RNG: area fraction
        uniform in ``scale``, aspect w / h log-uniform in ``ratio``, up to 10 tries, then the
        central fallback; origin uniform over the integer positions."""
        H, W = self.image_size
        lo, hi = math.log(self.ratio[0]), math.log(self.ratio[1])
        tries = torch.rand(10, 2)
        for frac, lr in tries.tolist():
            area = H * W * (self.scale[0] + frac * (self.scale[1] - self.scale[0]))
            aspect = math.exp(lo + lr * (hi - lo))
            w = int(round(math.sqrt(area * aspect)))
            h = int(round(math.sqrt(area / aspect)))
            if 2 <= w <= W and 2 <= h <= H:
                y0 = int(torch.randint(0, H - h + 1, (1,)))
                x0 = int(torch.randint(0, W - w + 1, (1,)))
                return x0, y0, w, h
        in_ratio = W / H
        if in_ratio < self.ratio[0]:
            w, h = W, int(round(W / self.ratio[0]))
        elif in_ratio > self.ratio[1]:
            h, w = H, int(round(H * self.ratio[1]))
        else:
            w, h = W, H
        w, h = min(max(w, 2), W), min(max(h, 2), H)
        return (W - w) // 2, (H - h) // 2, w, h

    def sample_views(self, n_images: int):
        """-> (boxes (n, V-2, 4) int64 [x0, y0, w, h], flips (n, V-2) bool), on the CPU.
        Replaceable on the instance (tests inject views)."""
        k = self.augmentations_per_sample - 2
        boxes = torch.zeros(n_images, k, 4, dtype=torch.int64)
        flips = torch.zeros(n_images, k, dtype=torch.bool)
        for i in range(n_images):
            for j in range(k):
                flips[i, j] = bool(torch.rand(()) < 0.5)
                boxes[i, j] = torch.tensor(self._draw_box())
        return boxes, flips

    def _get_augmentations(self, images, transforms):
        """upsampler.py:132-161 for given transforms (b, V-2, 3, 3): (b, V, 3, H, W) views in
        the reference's order, the augmented ones as grid samples of the image at T^-1."""
        b, c, h, w = images.shape
        k = self.augmentations_per_sample - 2
        out = images.new_empty(b, k + 2, c, h, w)
        out[:, -1] = images
        out[:, -2] = images.flip(dims=(-1,))
        if k:
            rep = images[:, None].expand(b, k, c, h, w).reshape(b * k, c, h, w)
            out[:, :-2] = warp_perspective(rep, transforms.flatten(0, 1), (h, w),
                                           "bilinear").reshape(b, k, c, h, w)
        return out

    # ------------------------------------------------------------------- torch route
    @staticmethod
    def _affine_transform_valid_pixels(transform, mask):
        """upsampler.py:56-79."""
        H, W = mask.shape[2:]
        valid_pixels = warp_perspective(mask, transform, (H, W), mode="nearest")
        return torch.where(valid_pixels > 0.999, torch.ones_like(valid_pixels),
                           torch.zeros_like(valid_pixels))

    def _accumulate_predictions(self, features, transforms):
        """upsampler.py:81-130."""
        B, N, C, H, W = features.shape
        features_base = features[:, -2:]
        if N > 2:
            features_augmented = features[:, :-2].flatten(0, 1)
            transforms_inv = _inv3(transforms.flatten(0, 1).to(features.dtype))
            features_resampled = warp_perspective(features_augmented, transforms_inv, (H, W),
                                                  mode="bilinear")
            features_resampled = features_resampled.reshape(B, -1, C, H, W)
            features_resampled = torch.cat((features_resampled, features_base), dim=1)
        else:
            features_resampled = features_base.clone()
        features_resampled[:, -2] = features_resampled[:, -2].flip(dims=(-1,))
        if N > 2:
            mask = torch.ones(B * (N - 2), 1, H, W, dtype=features_resampled.dtype,
                              device=features_resampled.device)
            valid_pixels = self._affine_transform_valid_pixels(transforms_inv, mask)
            valid_pixels = valid_pixels.reshape(B, N - 2, 1, H, W)
            valid_pixels = F.pad(valid_pixels, (0, 0, 0, 0, 0, 0, 0, 2), value=1)
            features_resampled[valid_pixels.repeat(1, 1, C, 1, 1) == 0.0] = torch.nan
        return features_resampled.nanmean(dim=1)

    def accumulate(self, features, transforms, h, w, normalize=True):
        """upsampler.py:170-181 after the gt encoder, torch ops: features (b, V, C, hp, wp)
        token grids, transforms (b, V-2, 3, 3) -> (b, C, h, w)."""
        b, V, C = features.shape[:3]
        features = F.interpolate(features.reshape(b * V, C, *features.shape[3:]), size=(h, w),
                                 mode="bilinear")
        features = features.view(b, V, C, h, w)
        chunks = torch.chunk(features, chunks=4, dim=2)
        chunks = [self._accumulate_predictions(chunk, transforms) for chunk in chunks]
        acc = torch.cat(chunks, dim=1)
        if not normalize:
            return acc
        return acc / torch.linalg.norm(acc, dim=1, keepdim=True)

    # ------------------------------------------------------------------ native route
    def native_domain(self, features, transforms):
        """None if ``sd_msc_gt`` takes these operands, else the reason."""
        if not features.is_cuda:
            return "features are not on a GPU"
        if features.dtype != torch.float32 or transforms.dtype != torch.float32:
            return f"dtype {features.dtype} / {transforms.dtype} (f32 only)"
        if not features.is_contiguous():
            return "features are not contiguous"
        V, C = features.shape[1:3]
        if not 2 <= V <= 8:
            return f"{V} views (2..8)"
        if C > 1024:
            return f"{C} channels (<= 1024)"
        return None

    def combine(self, features, transforms, h, w, normalize=True):
        """Token grids (b, V, C, hp, wp) and transforms (b, V-2, 3, 3) -> targets (b, C, h, w)
        on the native route where it applies, else the torch route."""
        transforms = transforms.to(features.device)
        reason = self.native_domain(features, transforms) if self.native else "native = False"
        if reason is None:
            from .... import _lib
            try:
                out = _lib.msc_gt(features, transforms.contiguous(), h, w, normalize)
                self.last_route, self.last_reason = "native", None
                return out
            except (RuntimeError, TypeError, ValueError) as e:  # the entry point's own domain
                reason = str(e)
        self.last_route, self.last_reason = "torch", reason
        return self.accumulate(features, transforms, h, w, normalize)

    def forward_chunk(self, images, transforms):
        """upsampler.py:163-181 for given transforms."""
        b, _, h, w = images.shape
        images_aug = self._get_augmentations(images, transforms.to(images.device))
        features = self.gt_encoder(images_aug.flatten(0, 1))[-1]
        features = features.reshape(b, -1, *features.shape[1:])
        return self.combine(features, transforms, h, w)

    def forward(self, images):
        """upsampler.py:183-194.  The views of all images are drawn once, so the result does
        not depend on the chunking."""
        n = images.shape[0]
        boxes, flips = self.sample_views(n)
        transforms = view_transforms(boxes, flips, images.shape[-2:]).to(images.device)
        aug_no_images = n * self.augmentations_per_sample
        if aug_no_images > self.max_chunk:
            no_chunks = aug_no_images // self.max_chunk
            parts = zip(torch.chunk(images, no_chunks), torch.chunk(transforms, no_chunks))
            return [torch.cat([self.forward_chunk(i, t) for i, t in parts], dim=0)]
        return [self.forward_chunk(images, transforms)]


class InterpolatedGT(nn.Module):
    """upsampler.py:197-205."""

    def __init__(self, arch: str, gt_encoder: nn.Module, image_size: Tuple[int, int]):
        super().__init__()
        from .dinov2_module import NoDecoder
        self.upsampler = NoDecoder(image_size, arch, normalize_features=False)
        object.__setattr__(self, "gt_encoder", gt_encoder)  # not a registered submodule

    def forward(self, x):
        return self.upsampler(self.gt_encoder(x))


def build_gt_upsampling_wrapper(arch: str, gt_encoder: nn.Module, image_size: Tuple[int, int]):
    """dinov2_module.py:69-76."""
    if arch in ("nearest", "bilinear", "bicubic"):
        return InterpolatedGT(arch, gt_encoder, image_size)
    if arch == "multiscale-crop":
        return MultiScaleCropGT(gt_encoder, num_views=4, image_size=image_size)
    raise NotImplementedError(f"upsampler_arch {arch!r}")
