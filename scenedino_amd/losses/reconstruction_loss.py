"""Reconstruction loss of the first training stage: photometric (L1 + SSIM, minimum over the
rendered views, masked by the invalid policy), DINO feature reconstruction (cosine) and the two
edge-aware smoothness regularisers.

Mirror of scenedino/losses/reconstruction_loss.py:175-356 (same config keys,
``get_loss_metric_names``, result keys and reading of ``data``), restated for this package: the
reference module imports ``kornia`` without using it, and reads every metric back to the host.

Two routes compute the same numbers:

* the torch route (``torch_forward``) covers every option -- criteria ``l1``, ``l1+ssim``, ``l2``,
  ``cosine``; the five invalid policies; median thresholding; a ``fine`` block; several scales;
  ``dino_artifacts`` -- on any device and dtype.  It is the CPU path and the tests' oracle.
* the native route (``sd_recon_loss_fwd`` / ``sd_recon_loss_bwd``, csrc/sdhip_recon_loss.hip;
  one autograd node) is taken per scale when the tensors are on the GPU and the configuration
  is inside ``native_domain``'s conditions; everything else takes the torch route.

Metric entries are detached 0-dim tensors on the loss's device (the reference's ``x.item()``
values without the host round trip), so a call never synchronises.

Behaviours of the reference kept on purpose: the depth regulariser pairs depth patches in
(pc, n) order with image patches in (n, pc) order; the invalid mask comes from scale 0 only; a
regulariser that is exactly zero is left out; the DINO term is a ``nanmean``; ``rgb_gt`` is read
as ``[..., :3]``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

SSIM_C1 = 0.01 ** 2
SSIM_C2 = 0.03 ** 2
# 3 x 3 Gaussian window of the SSIM averages (held in float32, then cast, as the reference does)
SSIM_WINDOW = ((0.0947, 0.1183, 0.0947), (0.1183, 0.1478, 0.1183), (0.0947, 0.1183, 0.0947))

# invalid policies of the native route -> include/sdhip.h SD_RL_POLICY_*
NATIVE_POLICIES = {"weight_guided": 0, "strict": 1, "none": 2, None: 2}


# ------------------------------------------------------------------------ criteria
def _gauss3(x):
    k = torch.tensor(SSIM_WINDOW, dtype=torch.float32).to(x.device).to(x.dtype)
    return F.conv2d(x, k.repeat(x.shape[1], 1, 1, 1), padding=0, groups=x.shape[1])


def ssim_term(x, y):
    """clamp(1 - SSIM, 0, 1) / 2 per channel on zero-padded 3 x 3 Gaussian statistics."""
    x, y = F.pad(x, (1, 1, 1, 1)), F.pad(y, (1, 1, 1, 1))
    mu_x, mu_y = _gauss3(x), _gauss3(y)
    mu_xx, mu_yy, mu_xy = mu_x ** 2, mu_y ** 2, mu_x * mu_y
    s_x, s_y, s_xy = _gauss3(x ** 2) - mu_xx, _gauss3(y ** 2) - mu_yy, _gauss3(x * y) - mu_xy
    num = (2 * mu_xy + SSIM_C1) * (2 * s_xy + SSIM_C2)
    den = (mu_xx + mu_yy + SSIM_C1) * (s_x + s_y + SSIM_C2)
    return torch.clamp(1 - num / den, 0, 1) / 2


def l1_ssim(a, b):
    return 0.85 * ssim_term(a, b).mean(dim=1) + 0.15 * (a - b).abs().mean(dim=1)


def make_criterion(name):
    if name == "l1":
        return lambda a, b: (a - b).abs().mean(dim=1)
    if name == "l1+ssim":
        return l1_ssim
    if name == "l2":
        return lambda a, b: ((a - b) ** 2 / 2).mean(dim=1)
    if name == "cosine":
        return lambda a, b: 1 - F.cosine_similarity(a, b, dim=1)
    raise ValueError(f"Unknown reconstruction error: {name}")


# ------------------------------------------------------------------------ regularisers
def edge_aware_smoothness(img, x, temperature=1):
    """(B, h, w): |right / down difference of x|, channel mean, weighted by
    exp(-temperature * the same difference of img), zero at the last column / row."""
    x_dx = (x[:, :, :, :-1] - x[:, :, :, 1:]).abs().mean(1, keepdim=True)
    x_dy = (x[:, :, :-1, :] - x[:, :, 1:, :]).abs().mean(1, keepdim=True)
    i_dx = (img[:, :, :, :-1] - img[:, :, :, 1:]).abs().mean(1, keepdim=True)
    i_dy = (img[:, :, :-1, :] - img[:, :, 1:, :]).abs().mean(1, keepdim=True)
    x_dx = x_dx * torch.exp(-temperature * i_dx)
    x_dy = x_dy * torch.exp(-temperature * i_dy)
    return (F.pad(x_dx, (0, 1)) + F.pad(x_dy, (0, 0, 0, 1)))[:, 0]


def _gt_patches(data, h, w):
    g = data["rgb_gt"][..., :3]
    return g.unsqueeze(-2).permute(0, 1, 4, 5, 2, 3).reshape(-1, 3, h, w)


def paired_depth(depth):
    """(n, pc, h, w) -> (pc * n, h, w): the reference flattens the depth patches in (pc, n)
    order while the image patches stay in (n, pc) order."""
    return depth.permute(1, 0, 2, 3).reshape(-1, depth.shape[2], depth.shape[3])


def _reg_depth(data, scale):
    d = paired_depth(data["coarse"][scale]["depth"])
    h, w = d.shape[-2:]
    u = 1 / d.reshape(-1, 1, h, w).clamp(1e-3, 80)
    u = u / u.mean(dim=[2, 3], keepdim=True)
    return edge_aware_smoothness(_gt_patches(data, h, w), u, temperature=1).mean()


def _reg_dino(data, scale):
    f = data["coarse"][scale]["dino_features"]
    _, _, h, w, _, c = f.shape
    f = f.permute(0, 1, 4, 5, 2, 3).reshape(-1, c, h, w)
    return edge_aware_smoothness(_gt_patches(data, h, w), f, temperature=25).mean()


REGULARIZATIONS = {"edge_aware_smoothness": _reg_depth, "dino_edge_aware_smoothness": _reg_dino}


# ------------------------------------------------------------------------ invalid policies
def _weighted_invalid(invalids, weights):
    return (invalids.to(weights.dtype) * weights.unsqueeze(-1)).sum(-2) > 0.9


def _policy_strict(invalids, **kw):
    return torch.all(torch.any(invalids > 0.5, dim=-2), dim=-1, keepdim=True)


def _policy_weight_guided(invalids, **kw):
    return torch.all(_weighted_invalid(invalids, kw["weights"]), dim=-1, keepdim=True)


def _policy_occ_weight_guided(invalids, **kw):
    return _policy_weight_guided(invalids, **kw) | ~(kw["occ"].to(kw["weights"].dtype) > 0.5)


def _policy_weight_guided_diverse(invalids, **kw):
    ray_std = torch.std(kw["rgb_samps"], dim=-3).mean(-1)
    flat = (invalids.to(torch.float32) * kw["weights"].unsqueeze(-1)).sum(-2) > 0.9
    return torch.all(flat | (ray_std < 0.01), dim=-1, keepdim=True)


def _policy_none(invalids, **kw):
    return torch.zeros_like(_policy_strict(invalids), dtype=torch.bool)


POLICIES = {"strict": _policy_strict, "weight_guided": _policy_weight_guided,
            "weight_guided_diverse": _policy_weight_guided_diverse,
            "occ_weight_guided": _policy_occ_weight_guided, "none": _policy_none,
            None: _policy_none}


# ------------------------------------------------------------------------ the native node
class _NativeReconLoss(torch.autograd.Function):
    """One node: forward sd_recon_loss_fwd, backward sd_recon_loss_bwd.  Returns (rec_loss (),
    terms (4) = [rgb, dino, depth smoothness, dino smoothness]); only rec_loss is
    differentiable."""

    @staticmethod
    def forward(ctx, rgb, depth, dino, down, rgb_gt, invalid, weights, dino_gt, artifacts, cfg):
        from .. import _lib
        need = tuple(ctx.needs_input_grad[:4])
        rec, terms, state = _lib.recon_loss_fwd(rgb, rgb_gt, invalid, weights, depth, dino, down,
                                                dino_gt, artifacts, cfg)
        ctx.cfg, ctx.need, ctx.state = cfg, need, state
        ctx.save_for_backward(rgb, rgb_gt, depth, dino, down, dino_gt, artifacts)
        ctx.mark_non_differentiable(terms)
        return rec, terms

    @staticmethod
    def backward(ctx, g_rec, _g_terms):
        from .. import _lib
        rgb, rgb_gt, depth, dino, down, dino_gt, artifacts = ctx.saved_tensors
        g = g_rec if g_rec.dtype == torch.float32 and g_rec.is_contiguous() else \
            g_rec.float().contiguous()
        d = _lib.recon_loss_bwd(g, rgb, rgb_gt, depth, dino, down, dino_gt, artifacts, ctx.cfg,
                                ctx.state, ctx.need)
        return d[0], d[1], d[2], d[3], None, None, None, None, None, None


class ReconstructionLoss:
    def __init__(self, config, use_automasking: bool = False) -> None:
        g = config.get
        self.rgb_fine_crit = self.rgb_coarse_crit = None
        self._names = {}
        for part in ("fine", "coarse"):
            c = g(part, None)
            if c is None:
                continue
            self._names[part] = (c.get("criterion", "l2"), c.get("dino_criterion", "l2"))
            setattr(self, f"rgb_{part}_crit", make_criterion(self._names[part][0]))
            setattr(self, f"dino_{part}_crit", make_criterion(self._names[part][1]))
            setattr(self, f"lambda_{part}", c.get("lambda", 1))
        self.policy_name = g("invalid_policy", "strict")
        if self.policy_name not in POLICIES:
            raise ValueError(f"Unknown invalid policy: {self.policy_name}")
        self.invalid_policy = POLICIES[self.policy_name]
        self.ignore_invalid = self.invalid_policy is not _policy_none
        self.regularizations = []
        for r in config["regularizations"]:
            if r["type"] not in REGULARIZATIONS:
                raise ValueError(f"Unknown regularization type: {r['type']}")
            self.regularizations.append((r["type"], REGULARIZATIONS[r["type"]], r["lambda"]))
        self.median_thresholding = g("median_thresholding", False)
        self.reconstruct_dino = g("reconstruct_dino", False)
        self.lambda_dino_coarse = g("lambda_dino_coarse", 1)
        self.lambda_dino_fine = g("lambda_dino_fine", 1)
        self.temperature_dino = g("temperature_dino", 1)
        self.native = True        # False: always the torch route
        self.last_route = None    # "native" / "torch": the route of the latest call

    def get_loss_metric_names(self) -> list[str]:
        names = ["rec_loss"]
        for part, crit in (("fine", self.rgb_fine_crit), ("coarse", self.rgb_coarse_crit)):
            if crit is not None:
                names.append(f"loss_rgb_{part}")
                if self.reconstruct_dino:
                    names.append(f"loss_dino_{part}")
        return names + [r[0] for r in self.regularizations]

    # -------------------------------------------------------------------- torch route
    def _rgb_loss(self, pred, gt, invalid, criterion):
        b, pc, h, w, nv, ch = pred.shape
        loss = criterion(pred.permute(0, 1, 4, 5, 2, 3).reshape(-1, ch, h, w),
                         gt.permute(0, 1, 4, 5, 2, 3).reshape(-1, ch, h, w))
        loss = loss.view(b, pc, nv, h, w).permute(0, 1, 3, 4, 2).unsqueeze(-1).amin(-2)
        if self.ignore_invalid and invalid is not None:
            loss = loss * (1 - invalid.to(torch.float32))
        if self.median_thresholding:
            # mean of the entries at or below the per-sample median, as a masked mean (the
            # reference's boolean index, without its host sync)
            thr = torch.median(loss.view(b, -1), dim=-1)[0].view(-1, 1, 1, 1, 1)
            keep = (loss <= thr).to(loss.dtype)
            return (loss * keep).sum() / keep.sum()
        return loss.mean()

    @staticmethod
    def _dino_loss(pred, gt, criterion):
        c = pred.shape[-1]
        return criterion(pred.reshape(-1, c), gt.reshape(-1, c)).nanmean()

    @staticmethod
    def _dino_pred(part, data):
        d = part["dino_features_downsampled"] if "dino_features_downsampled" in part \
            else part["dino_features"]
        return d, data["dino_gt"].unsqueeze(-2).expand(d.shape)

    def torch_forward(self, data, scales=None, invalid=None):
        """The loss in torch ops: {name: 0-dim tensor}, un-normalised sums over ``scales`` (all
        by default); ``rec_loss`` carries the graph, the other entries are detached."""
        n_scales = len(data["coarse"])
        inv_c = inv_f = None
        if self.rgb_coarse_crit is not None:
            c0 = data["coarse"][0]
            inv_c = invalid if invalid is not None else \
                self.invalid_policy(c0["invalid"], weights=c0["weights"])
            dev = inv_c.device
        if self.rgb_fine_crit is not None:
            f0 = data["fine"][0]
            inv_f = self.invalid_policy(f0["invalid"], weights=f0["weights"])
            dev = inv_f.device
        out = {name: torch.tensor(0.0, device=dev) for name in self.get_loss_metric_names()}

        def add(name, value, lam):
            out[name] = out[name] + value.detach()
            out["rec_loss"] = out["rec_loss"] + value * lam

        T = self.temperature_dino
        for scale in (range(n_scales) if scales is None else scales):
            if self.rgb_coarse_crit is not None:
                coarse = data["coarse"][scale]
                dino_c, dino_gt = self._dino_pred(coarse, data)
            if self.rgb_fine_crit is not None:
                fine = data["fine"][scale]
                dino_f, dino_gt_f = self._dino_pred(fine, data)
                if self.rgb_coarse_crit is None:
                    dino_gt = dino_gt_f
            if "dino_artifacts" in data and self.rgb_coarse_crit is not None:
                dino_c = dino_c + data["dino_artifacts"].unsqueeze(-2).expand(dino_c.shape)
            if self.rgb_coarse_crit is not None:
                gt = data["rgb_gt"].unsqueeze(-2).expand(coarse["rgb"].shape)
                add("loss_rgb_coarse",
                    self._rgb_loss(coarse["rgb"], gt, inv_c, self.rgb_coarse_crit),
                    self.lambda_coarse)
                if self.reconstruct_dino:
                    v = self._dino_loss(T * dino_c, T * dino_gt, self.dino_coarse_crit)
                    out["loss_dino_coarse"] = out["loss_dino_coarse"] + v.detach()
                    out["rec_loss"] = out["rec_loss"] + v * self.lambda_coarse * self.lambda_dino_coarse
            if self.rgb_fine_crit is not None:
                gt = data["rgb_gt"].unsqueeze(-2).expand(fine["rgb"].shape)
                add("loss_rgb_fine", self._rgb_loss(fine["rgb"], gt, inv_f, self.rgb_fine_crit),
                    self.lambda_fine)
                if self.reconstruct_dino:
                    v = self._dino_loss(dino_f, dino_gt, self.dino_fine_crit)
                    out["loss_dino_fine"] = out["loss_dino_fine"] + v.detach()
                    out["rec_loss"] = out["rec_loss"] + v * self.lambda_fine * self.lambda_dino_fine
            for name, fn, lam in self.regularizations:
                # a regulariser that is exactly zero is left out (the reference's `if reg_loss:`),
                # selected on the device
                v = fn(data, scale)
                v = torch.where(v != 0, v, torch.zeros_like(v))
                add(name, v, lam)
        return out

    # -------------------------------------------------------------------- native route
    def native_domain(self, data):
        """None if every scale of ``data`` can take the native route, else the reason."""
        if self.rgb_fine_crit is not None or self.rgb_coarse_crit is None:
            return "a fine block / no coarse block"
        if self._names["coarse"][0] != "l1+ssim":
            return "coarse.criterion is not l1+ssim"
        if self.reconstruct_dino and self._names["coarse"][1] != "cosine":
            return "dino_criterion is not cosine"
        if self.policy_name not in NATIVE_POLICIES:
            return f"invalid_policy {self.policy_name}"
        if self.median_thresholding:
            return "median thresholding"
        f32 = torch.float32
        c0 = data["coarse"][0]
        gt = data["rgb_gt"]
        if c0["invalid"].dim() != 6 or c0["weights"].dtype != f32 or gt.dtype != f32 \
                or gt.shape[-1] < 3 or c0["invalid"].dtype not in (f32, torch.bool):
            return "invalid / weights / rgb_gt layout"
        for part in data["coarse"]:
            rgb = part["rgb"]
            if rgb.device.type != "cuda" or rgb.dim() != 6 or rgb.dtype != f32 or rgb.shape[-1] != 3:
                return "rgb is not an f32 (n, pc, h, w, nv, 3) device tensor"
            n, pc, h, w, nv, _ = rgb.shape
            if not (2 <= h <= 16 and 2 <= w <= 16 and 1 <= nv <= 8):
                return "patch size / view count"
            if tuple(c0["invalid"].shape[:4]) != (n, pc, h, w) or c0["invalid"].shape[5] != nv \
                    or tuple(c0["weights"].shape) != tuple(c0["invalid"].shape[:5]) \
                    or tuple(gt.shape[:4]) != (n, pc, h, w):
                return "shapes of scale 0's mask inputs"
            regs = [r[0] for r in self.regularizations]
            if "edge_aware_smoothness" in regs and (
                    part["depth"].dtype != f32 or tuple(part["depth"].shape) != (n, pc, h, w)):
                return "depth layout"
            if "dino_edge_aware_smoothness" in regs:
                f = part["dino_features"]
                if f.dtype not in (f32, torch.bfloat16) or f.dim() != 6 or f.shape[4] != 1 \
                        or tuple(f.shape[:4]) != (n, pc, h, w) or f.shape[5] % 64 or f.shape[5] > 768:
                    return "dino_features layout"
            if self.reconstruct_dino:
                d, g = self._dino_pred(part, data)[0], data["dino_gt"]
                if d.dtype != f32 or g.dtype != f32 or d.numel() != g.numel() \
                        or d.shape[-1] != g.shape[-1] or d.shape[-1] % 64 or d.shape[-1] > 768:
                    return "downsampled DINO layout"
                a = data.get("dino_artifacts")
                if a is not None and (a.dtype != f32 or a.numel() != g.numel()):
                    return "dino_artifacts layout"
        return None

    def _native_scale(self, data, scale):
        part = data["coarse"][scale]
        c0 = data["coarse"][0]
        regs = {r[0]: r[2] for r in self.regularizations}
        rgb = part["rgb"]
        n, pc, h, w, nv, _ = rgb.shape
        P = n * pc
        inv = c0["invalid"]
        if inv.dtype != torch.float32:
            inv = inv.to(torch.float32)
        K = inv.shape[4]
        depth = dino = down = dino_gt = art = None
        if "edge_aware_smoothness" in regs:
            depth = paired_depth(part["depth"]).contiguous()
        if "dino_edge_aware_smoothness" in regs:
            dino = part["dino_features"].contiguous().view(P, h, w, -1)
        if self.reconstruct_dino:
            d = self._dino_pred(part, data)[0]
            C = d.shape[-1]
            down = d.contiguous().view(-1, C)
            dino_gt = data["dino_gt"].contiguous().view(-1, C)
            if data.get("dino_artifacts") is not None:
                art = data["dino_artifacts"].contiguous().view(-1, C)
        cfg = dict(policy=NATIVE_POLICIES[self.policy_name], lambda_coarse=float(self.lambda_coarse),
                   lambda_dino=float(self.lambda_dino_coarse), temperature=float(self.temperature_dino),
                   lambda_depth=float(regs.get("edge_aware_smoothness", 0.0)),
                   lambda_dsmooth=float(regs.get("dino_edge_aware_smoothness", 0.0)))
        rec, terms = _NativeReconLoss.apply(
            rgb.contiguous().view(P, h, w, nv, 3), depth, dino, down,
            data["rgb_gt"][..., :3].contiguous().view(P, h, w, 3), inv.contiguous().view(P, h, w, K, nv),
            c0["weights"].contiguous().view(P, h, w, K), dino_gt, art, cfg)
        out = {"rec_loss": rec, "loss_rgb_coarse": terms[0]}
        if self.reconstruct_dino:
            out["loss_dino_coarse"] = terms[1]
        if "edge_aware_smoothness" in regs:
            out["edge_aware_smoothness"] = terms[2]
        if "dino_edge_aware_smoothness" in regs:
            out["dino_edge_aware_smoothness"] = terms[3]
        return out

    def __call__(self, data) -> dict[str, torch.Tensor]:
        n_scales = len(data["coarse"])
        if self.native and self.native_domain(data) is None:
            self.last_route = "native"
            out = None
            for scale in range(n_scales):
                one = self._native_scale(data, scale)
                out = one if out is None else {k: out[k] + one[k] for k in out}
        else:
            self.last_route = "torch"
            out = self.torch_forward(data)
        if n_scales != 1:
            out = {k: v / n_scales for k, v in out.items()}
        return {k: out[k] for k in self.get_loss_metric_names()}
