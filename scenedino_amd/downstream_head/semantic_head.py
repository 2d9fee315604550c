"""Unsupervised SSC head, MI355X build.

Mirror of scenedino/downstream_head/semantic_head.py (SemanticHead :41-282,
StegoClusterHead :285-305, KMeansParamHead :308-373, LinearHead :460-477, MLPHead
:480-501): same class names, constructor arguments, return keys, sub-module / parameter /
buffer names (``stego_head.linear_path.0``, ``stego_head.nonlinear_path.{0,2}``,
``{direct,stego}_cluster_head.cluster_centers``, ``.pseudo_assignment``,
``{direct,stego}_linear_head.linear``), so reference checkpoints load unchanged.

Inference: BTSNet.forward(..., predict_segmentation=True) and the SSCBench voxel query never
call ``forward`` here: BTSNet hands the 64-d DINO codes straight to the folded gfx950 kernel
``sd_seg_query`` (transform_expand + stego + cosine k-means in registers, csrc/sdhip_seg.hip),
which reads these modules' parameters.  ``forward`` on already-expanded 768-d features
evaluates the same math with device tensor ops.

Training (``forward_training``, the reference's downstream stage, trainer_downstream.py:72-214):
  * the image rows (n v h w rows of input_dim) go through ``sd_stego_train_fwd`` without saves
    (they are detached downstream) and both cluster heads through ``sd_cluster_probe``; the
    Dropout2d on the 768-d features is a column scale of the probe, so the normalised and
    dropped copy of the features is never written;
  * the three differentiable StegoClusterHead calls on crop rows (self, kNN partner, random
    partner) are one ``_StegoTrainFn`` over ``sd_stego_train_fwd`` / ``_bwd`` plus
    ``sd_conv_wgrad`` (taps = 1) for the six parameter gradients; inputs are detached in the
    reference, so there is no input gradient;
  * both linear probes (with ``segs``) are one ``sd_linear_probe`` call each: normalisation,
    Dropout2d scale, logits, argmax, cross-entropy and the gradients of W and b in one pass over
    the raw rows (``_LinearProbeFn``; MLPHead stays on torch ops); the label ids map through a
    cached device table (``_train_id_lut``);
  * correlations and StegoLoss are torch ops by default (the reference's
    StegoLoss reads ``data["segmentation"]["stego_corr"]``).  With ``head.lazy_corr = True`` that
    entry is a ``StegoCorrMap``: a read-only mapping with the same six keys that holds the operand
    rows and builds a correlation tensor only when it is indexed, so this package's StegoLoss can
    take its fused route (``sd_stego_corr_fwd`` / ``_bwd``) without any (nc, P, P) tensor.
Dropout masks are drawn with torch on the (groups, channels) mask tensors and applied by the
kernels; ``head._draws`` (a dict, see ``_draw``) supplies any mask or random index instead.  The
reference's kNN / random partner calls hand a 3-D tensor to Dropout2d, which torch treats as
(N, C, L) (a deprecated quirk: one mask per (code channel, point), shared by the crops); here
those calls drop whole code channels per crop, as the batched self call does.
CPU tensors and shapes outside the kernels' domain run the same math in torch ops.
CRF post-processing (``apply_crf``): with ``head.native_crf = True`` every result gains a
``<name>_crf`` entry from this package's dense CRF (downstream_head/crf.py: ``sd_dense_crf`` on the
GPU, all results of an image in one call; parity with pydensecrf itself unpinned); with the switch
off ``apply_crf`` raises, as pydensecrf is not shipped.  KMeansIterHead (pykeops) is out of scope.
"""
from __future__ import annotations

from collections.abc import Mapping

import torch
import torch.nn.functional as F
from torch import nn

from .. import _lib
from ..pack_cache import module_key, steps, track_steps


# False: every path below takes its torch-op fallback (tools/stego_train_bench.py's baseline)
_NATIVE = True
# False: LinearHead alone takes its torch-op route (tools/linear_probe_bench.py's baseline)
_NATIVE_PROBES = True


def _norm(x):
    # semantic_head.py:37-38
    return F.normalize(x, dim=-1, eps=1e-10)


def _five_crop(features, sample_factor=1):
    """semantic_head.py:15-34: centre and four quadrant crops of (n, v, h, w, 1, c), side
    min(h, w) / 2, every sample_factor-th pixel, concatenated over dim 0 (crop-major)."""
    _, _, h, w, _, _ = features.shape
    if h % (4 * sample_factor) or w % (4 * sample_factor):
        raise ValueError("_five_crop: h and w must be multiples of 4 * sample_factor")
    shift, half = sample_factor // 2, min(h, w) // 4
    centres = ((h // 2, w // 2), (3 * h // 4, w // 4), (3 * h // 4, 3 * w // 4),
               (h // 4, w // 4), (h // 4, 3 * w // 4))
    return torch.cat([features[:, :, cy - half + shift:cy + half + shift:sample_factor,
                               cx - half + shift:cx + half + shift:sample_factor]
                      for cy, cx in centres])


def _rows_scale(m, rows_per_group, M):
    """(G, C) group scales -> (M, C) row scales (row r uses group r // rows_per_group)."""
    return m.repeat_interleave(rows_per_group, dim=0)[:M]


def _kitti_labels():
    """The KITTI-360 label table of the reference's dataset package, or None."""
    try:
        from datasets.kitti_360 import labels as table
    except Exception:  # noqa: BLE001
        return None
    return table


class _StegoTrainFn(torch.autograd.Function):
    """x (M, d_in) f32, detached -> StegoClusterHead in train mode (M, 64) f32 with gradients
    to the six convolution parameters.  The parameters are inputs so that autograd routes
    their gradients; the kernels read the packed copies."""

    @staticmethod
    def forward(ctx, x, wl, bl, wn1, bn1, wn2, bn2, head, m_lin, m_non, rows_per_group, normalize):
        pack = head._train_pack()
        y, saved = _lib.stego_train_fwd(x, pack, m_lin, m_non, rows_per_group, save=True,
                                        normalize=normalize)
        ctx.saved, ctx.pack, ctx.masks = saved, pack, (m_lin, m_non, rows_per_group)
        ctx.shapes = (wl.shape, wn1.shape, wn2.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        from ..models.backbones.dino.dim_reduction import _wgrad
        xh, mid, _ = ctx.saved
        m_lin, m_non, rpg = ctx.masks
        _, n_wl, n_bl, n_wn1, n_bn1, n_wn2, n_bn2 = ctx.needs_input_grad[:7]
        want_lin, want_n1, want_n2 = n_wl or n_bl, n_wn1 or n_bn1, n_wn2 or n_bn2
        dlin, dnon, dmid = _lib.stego_train_bwd(dy.float().contiguous(), ctx.saved, ctx.pack,
                                                m_lin, m_non, rpg, want_lin=want_lin,
                                                want_non2=want_n2, want_non1=want_n1)
        g = [None] * 6
        if want_lin:
            g[0], g[1] = _wgrad(xh, dlin, n_bl)
        if want_n1:
            g[2], g[3] = _wgrad(xh, dmid, n_bn1)
        if want_n2:
            g[4], g[5] = _wgrad(mid, dnon, n_bn2)
        for i, shape in zip((0, 2, 4), ctx.shapes):
            g[i] = g[i].view(shape) if g[i] is not None else None
        need = ctx.needs_input_grad[1:7]
        return (None, *(gi if nd else None for gi, nd in zip(g, need)), None, None, None, None, None)


class StegoClusterHead(nn.Module):
    def __init__(self, in_channels, out_channels, mid_channels=None):
        super().__init__()
        mid = in_channels if mid_channels is None else mid_channels
        self.linear_path = nn.Sequential(nn.Conv2d(in_channels, out_channels, (1, 1)),
                                         nn.Dropout2d(p=0.1))
        self.nonlinear_path = nn.Sequential(nn.Conv2d(in_channels, mid, (1, 1)), nn.ReLU(),
                                            nn.Conv2d(mid, out_channels, (1, 1)),
                                            nn.Dropout2d(p=0.1))
        self._packed = None

    @staticmethod
    def _lin(conv, x):
        return F.linear(x, conv.weight.reshape(conv.weight.shape[0], -1), conv.bias)

    def forward(self, x):
        """1x1 convolutions over the channel (last) dim, as linear maps; L2-normalised."""
        lin = self._lin(self.linear_path[0], x)
        mid = torch.relu(self._lin(self.nonlinear_path[0], x))
        out = lin + self._lin(self.nonlinear_path[2], mid)
        return _norm(out).to(x.dtype)

    def _convs(self):
        return self.linear_path[0], self.nonlinear_path[0], self.nonlinear_path[2]

    def _native(self, x):
        lin, nl0, nl2 = self._convs()
        d = lin.weight.shape[1]
        return (_NATIVE and x.is_cuda and x.dtype == torch.float32 and d in (384, 768) and x.shape[0] >= 1
                and lin.weight.shape[0] == 64 and tuple(nl0.weight.shape[:2]) == (d, d)
                and tuple(nl2.weight.shape[:2]) == (64, d))

    def _train_pack(self):
        """PackedStegoTrain of the current weights."""
        from ..seg_pack import PackedStegoTrain
        key = module_key(self)
        if self._packed is None or self._packed[0] != key:
            self._packed = (key, PackedStegoTrain(self))
        return self._packed[1]

    def train_rows(self, x, m_lin=None, m_non=None, rows_per_group=1, normalize=True,
                   differentiable=True):
        """Train-mode forward on rows x (M, d_in), detached: y (M, 64) f32 =
        normalize(m_lin o (Wl xh + bl) + m_non o (Wn2 relu(Wn1 xh + bn1) + bn2)) with
        xh = normalize(x) (normalize) or x; m_* (G, 64) Dropout2d scales of row groups or None.
        differentiable: gradients reach the convolution parameters that require them."""
        x = x.detach().float().contiguous()
        convs = self._convs()
        params = [t for c in convs for t in (c.weight, c.bias)]
        grad = differentiable and torch.is_grad_enabled() and any(p.requires_grad for p in params)
        if self._native(x):
            if grad:
                track_steps(self)
                return _StegoTrainFn.apply(x, *params, self, m_lin, m_non, rows_per_group,
                                           normalize)
            y, _ = _lib.stego_train_fwd(x, self._train_pack(), m_lin, m_non, rows_per_group,
                                        normalize=normalize)
            return y
        with torch.set_grad_enabled(grad):
            # a pass without gradients reads detached parameters: under autocast the cast of a
            # leaf made here would be cached and reused, without a graph, by the next
            # differentiable pass of the same autocast region
            w = [p if grad else p.detach() for p in params]
            lin2 = lambda i, t: F.linear(t, w[2 * i].reshape(w[2 * i].shape[0], -1), w[2 * i + 1])  # noqa: E731
            xh = _norm(x) if normalize else x
            lin = lin2(0, xh)
            non = lin2(2, torch.relu(lin2(1, xh)))
            if m_lin is not None:
                lin = lin * _rows_scale(m_lin, rows_per_group, x.shape[0])
            if m_non is not None:
                non = non * _rows_scale(m_non, rows_per_group, x.shape[0])
            return _norm(lin + non)


class StegoCorrMap(Mapping):
    """``data["segmentation"]["stego_corr"]`` under ``SemanticHead.lazy_corr``: the six keys of
    the eager dict over the operand rows.  ``dino`` = (cropped, dino_nn, dino_random), detached
    (nc, P, c) rows; ``stego`` = (stego_self, stego_nn, stego_random), un-normalised (nc, P, 64)
    rows with their autograd edge.  Indexing a key builds that one correlation tensor with
    ``SemanticHead._compute_stego_correlation`` and caches it (the reference's StegoLoss edits
    the DINO ones in place; the operand rows are never touched)."""
    PAIRS = ("self", "nn", "random")

    def __init__(self, dino, stego, corr):
        self.dino, self.stego = tuple(dino), tuple(stego)
        self._corr = corr
        self._cache = {}

    def _key(self, key):
        kind, _, rest = key.partition("_") if isinstance(key, str) else ("", "", "")
        pair = rest[:-len("_corr")] if rest.endswith("_corr") else ""
        if kind not in ("dino", "stego") or pair not in self.PAIRS:
            raise KeyError(key)
        return kind, self.PAIRS.index(pair)

    def __getitem__(self, key):
        kind, i = self._key(key)
        if key not in self._cache:
            rows = self.dino if kind == "dino" else self.stego
            self._cache[key] = self._corr(rows[0], rows[i])
        return self._cache[key]

    def __iter__(self):
        for pair in self.PAIRS:
            yield f"dino_{pair}_corr"
            yield f"stego_{pair}_corr"

    def __len__(self):
        return 6

    @property
    def materialised(self):
        """Keys whose tensor has been built."""
        return tuple(self._cache)


class KMeansParamHead(nn.Module):
    def __init__(self, n_classes: int, gt_classes: int, dim: int):
        super().__init__()
        self.n_classes = n_classes
        self.dim = dim
        self.init_type = "random"
        self.cluster_centers = nn.Parameter(torch.randn(n_classes, dim))
        self.centroids_initialized = False
        self.register_buffer("pseudo_assignment", torch.arange(0, n_classes).remainder(gt_classes))

    def _native(self, flat):
        return (_NATIVE and flat.is_cuda and flat.dtype in (torch.float32, torch.bfloat16)
                and flat.shape[0] >= 1 and 64 <= self.dim <= 768 and self.dim % 64 == 0
                and 1 <= self.n_classes <= 32)

    def forward(self, features, weight=None, _mask=None, _rows_per_group=1):
        """semantic_head.py:322-373.  loss = mean(-w_i xh_i . c_label_i): the labels are
        piecewise constant, so it is -(1/N) sum_k c_k . S_k with S_k = sum_{label = k} w_i xh_i
        held constant (sd_cluster_probe) and autograd through F.normalize(cluster_centers).
        _mask (G, dim) / _rows_per_group: column scales of row groups applied before the
        normalisation (forward_training's Dropout2d; normalisation is scale-invariant)."""
        flat = features.detach().flatten(0, -2) if _mask is not None else features.flatten(0, -2)
        N = flat.shape[0]
        if not self.centroids_initialized and self.training:
            if self.init_type != "random":
                raise NotImplementedError("KMeansParamHead: init_type 'random' only")
            self.cluster_centers.data = torch.randn(self.n_classes, self.dim,
                                                    device=self.cluster_centers.device)
            self.centroids_initialized = True
        centres = F.normalize(self.cluster_centers, dim=1)
        if self._native(flat) and not flat.requires_grad:
            w = None if weight is None else weight.detach().flatten().float().contiguous()
            labels, S, _ = _lib.cluster_probe(flat.contiguous(), centres.detach().float().contiguous(),
                                              _mask, _rows_per_group, w)
            labels = labels.long()
            loss = -(centres * S).sum() / N
        else:
            x = flat if _mask is None else flat * _rows_scale(_mask, _rows_per_group, N)
            scores = F.normalize(x.float(), dim=1) @ centres.t()
            labels = scores.argmax(dim=1)
            picked = -scores.gather(1, labels[:, None]).squeeze(1)
            loss = torch.mean(picked if weight is None else picked * weight.flatten())
        labels = labels.view(*features.shape[:-1])
        return {"pseudo_segs_pred": labels,
                "segs_pred": self.pseudo_assignment[labels].long(),
                "loss": loss}


def _probe_loss(logit, target):
    # semantic_head.py:473-475: view 0, classes to dim 1
    target = target.long().to(logit.device)
    return F.cross_entropy(logit[:, 0].movedim(-1, 1).squeeze(-1), target, ignore_index=-1)


class _LinearProbeFn(torch.autograd.Function):
    """rows x (N, d), detached -> (mean cross-entropy over the valid rows, pred (N) int32) with
    gradients to W and b: sd_linear_probe emits gW and gb in its forward pass, so the backward
    is a scale by the incoming scalar.  No host read: loss_sum / n_valid is NaN when no row is
    valid, as F.cross_entropy's mean is."""

    @staticmethod
    def forward(ctx, W, b, x, target, m, rows_per_group, normalize):
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        pred, loss_sum, n_valid, gW, gb, _ = _lib.linear_probe(
            x, W.detach().float().contiguous(), b.detach().float().contiguous(), target, m,
            rows_per_group, normalize, want_grad=want)
        nv = n_valid.float()
        if want:
            # no valid row: zero gradients beside the NaN loss, as F.cross_entropy gives
            ctx.save_for_backward(gW / nv.clamp(min=1.0), gb / nv.clamp(min=1.0))
        ctx.mark_non_differentiable(pred)
        return (loss_sum / nv).squeeze(0), pred

    @staticmethod
    def backward(ctx, dloss, _dpred):
        gW, gb = ctx.saved_tensors
        need = ctx.needs_input_grad
        return (gW * dloss if need[0] else None, gb * dloss if need[1] else None,
                None, None, None, None, None)


class LinearHead(nn.Module):
    def __init__(self, dim: int, gt_classes: int):
        super().__init__()
        self.linear = nn.Linear(dim, gt_classes)

    def _native(self, flat):
        lin = self.linear
        C, d = lin.weight.shape
        return (_NATIVE and _NATIVE_PROBES and flat.is_cuda
                and flat.dtype in (torch.float32, torch.bfloat16)
                and not flat.requires_grad and flat.shape[0] >= 1 and 64 <= d <= 768
                and d % 64 == 0 and 1 <= C <= 32 and lin.bias is not None
                and lin.weight.is_cuda and lin.weight.dtype == torch.float32)

    def forward(self, features, target=None, _mask=None, _rows_per_group=1, _normalize=False):
        """semantic_head.py:468-477 on xh = (_normalize ? _norm(features) : features) o _mask
        (_mask (G, dim) / _rows_per_group: column scales of row groups, forward_training's
        Dropout2d after its _norm).  segs_pred (int64) covers every view, loss view 0 only.
        Rows on the GPU that need no gradient take sd_linear_probe (the rows of views > 0 with
        target -1); anything else the same function in torch ops."""
        flat = features.flatten(0, -2)
        N = flat.shape[0]
        if self._native(flat):
            flat = flat.contiguous()
            m = None if _mask is None else _mask.float().contiguous()
            W, b = self.linear.weight, self.linear.bias
            if target is None:
                pred = _lib.linear_probe(flat, W.detach().contiguous(), b.detach().contiguous(),
                                         None, m, _rows_per_group, _normalize)[0]
                return {"segs_pred": pred.long().view(features.shape[:-1])}
            n, v = features.shape[:2]
            tgt = target.to(device=flat.device, dtype=torch.int64).reshape(n, 1, -1)
            if v > 1:
                tgt = torch.cat([tgt, tgt.new_full((n, v - 1, tgt.shape[2]), -1)], dim=1)
            loss, pred = _LinearProbeFn.apply(W, b, flat, tgt.reshape(N), m, _rows_per_group,
                                              _normalize)
            return {"segs_pred": pred.long().view(features.shape[:-1]), "loss": loss}
        x = _norm(features.float()) if _normalize else features
        if _mask is not None:
            G = _mask.shape[0]
            if N == G * _rows_per_group:
                x = (x.reshape(G, _rows_per_group, -1) * _mask[:, None, :]).view(x.shape)
            else:
                x = x * _rows_scale(_mask, _rows_per_group, N).view(x.shape)
        logit = self.linear(x).float()
        result = {"segs_pred": logit.argmax(-1)}
        if target is not None:
            result["loss"] = _probe_loss(logit, target)
        return result


class MLPHead(nn.Module):
    def __init__(self, dim: int, gt_classes: int):
        super().__init__()
        self.linear1 = nn.Linear(dim, 2 * dim)
        self.linear2 = nn.Linear(2 * dim, gt_classes)
        self.activation = nn.ReLU()

    def forward(self, features, target=None):
        logit = self.linear2(self.activation(self.linear1(features))).float()
        result = {"segs_pred": logit.argmax(-1)}
        if target is not None:
            result["loss"] = _probe_loss(logit, target)
        return result


class SemanticHead(nn.Module):
    def __init__(self, n_classes, gt_classes, input_dim, code_dim, buffer_size=0,
                 patch_sample_size=0, knn_neighbors=0, mode="2d", mlp_head=False,
                 apply_crf=False):
        super().__init__()
        self.n_classes = n_classes
        self.gt_classes = gt_classes
        self.input_dim = input_dim
        self.code_dim = code_dim
        self.knn_neighbors = knn_neighbors
        self.mode = mode
        self.apply_crf = apply_crf
        # kNN feature buffers: plain attributes as in the reference (not in the state dict);
        # they follow the features' device on first use
        self.buffer_size = buffer_size
        self.buffer_idx = 0
        self.buffer_filled = 1
        if buffer_size > 0:
            self.dino_patch_buffer = torch.zeros((buffer_size, patch_sample_size, input_dim))
            self.dino_gap_buffer = torch.zeros((buffer_size, input_dim))
        else:
            self.dino_patch_buffer = self.dino_gap_buffer = None
        self.direct_cluster_head = KMeansParamHead(n_classes, gt_classes, input_dim)
        self.stego_head = StegoClusterHead(input_dim, code_dim)
        self.stego_cluster_head = KMeansParamHead(n_classes, gt_classes, code_dim)
        head = MLPHead if mlp_head else LinearHead
        self.direct_linear_head = head(input_dim, gt_classes)
        self.stego_linear_head = head(code_dim, gt_classes)
        self.dropout = nn.Dropout2d(p=.1)
        self.dropout1d = nn.Dropout1d(p=.1)
        self._draws = None
        self._label_colors = None
        # True: forward_training leaves a StegoCorrMap instead of the six correlation tensors
        self.lazy_corr = False
        # True: apply_crf runs this package's dense CRF (downstream_head/crf.py) instead of raising
        self.native_crf = False

    @classmethod
    def from_conf(cls, config):
        g = config.get
        return cls(n_classes=g("n_classes"), gt_classes=g("gt_classes"),
                   input_dim=g("input_dim"), code_dim=g("code_dim"),
                   buffer_size=g("buffer_size", 0), patch_sample_size=g("patch_sample_size", 0),
                   knn_neighbors=g("knn_neighbors", 0), mode=g("mode", "2d"),
                   mlp_head=g("mlp_head", False), apply_crf=g("apply_crf", False))

    def _folded_labels(self, features):
        """segs_pred of mode stego_kmeans for features that MlpDimReduction.transform_expand
        produced (and nobody modified since): the folded kernel sd_seg_query on the 64-d codes
        (transform_expand + stego + k-means in registers), or None."""
        prov = getattr(features, "_sd_expand", None)
        if prov is None or features.requires_grad or torch.is_grad_enabled() and self.training:
            return None
        codes, dr, key, version = prov
        from ..seg_pack import PackedSegHead
        if features._version != version or module_key(dr) != key:
            return None
        # steps(self): the k-means centres train through plain autograd, under this head's count
        hkey = module_key(dr, self.stego_head, self.stego_cluster_head) + (steps(self),)
        cache = getattr(self, "_fold_cache", None)
        if cache is None or cache[0] != hkey or cache[1] is not dr:
            cache = self._fold_cache = (hkey, dr, PackedSegHead(
                dr, self.stego_head, self.stego_cluster_head, device=codes.device))
        labels, _, _ = _lib.seg_query(codes, cache[2].rec, want_labels=True)
        return labels.view(features.shape[:-1]).long()

    def forward(self, features, mode="stego_kmeans"):
        """semantic_head.py:107-120 (segs_pred for the given mode).  stego_kmeans on
        features straight from MlpDimReduction.transform_expand (the 2-D demo's
        expand_dim -> downstream_head) runs as the folded sd_seg_query kernel on their
        64-d codes; any other input or mode evaluates the chain with device tensor ops."""
        if mode == "stego_kmeans":
            labels = self._folded_labels(features)
            if labels is not None:
                return labels
        if mode == "direct_linear" and isinstance(self.direct_linear_head, LinearHead):
            # the probe normalises the rows itself (sd_linear_probe): no normalised copy
            return self.direct_linear_head(features, _normalize=True)["segs_pred"]
        features = _norm(features)
        if mode == "stego_kmeans":
            return self.stego_cluster_head(self.stego_head(features))["segs_pred"]
        if mode == "stego_linear":
            return self.stego_linear_head(self.stego_head(features))["segs_pred"]
        if mode == "direct_kmeans":
            return self.direct_cluster_head(features)["segs_pred"]
        if mode == "direct_linear":
            return self.direct_linear_head(features)["segs_pred"]
        raise NotImplementedError(f"Mode '{mode}' is not known!")

    # ------------------------------------------------------------------ training
    def _draw(self, name, make):
        """A random draw of forward_training: ``self._draws[name]`` when the dict has it (tests
        inject every mask and index), else make().  Names: ``dino`` (n v, input_dim), ``img_lin``
        / ``img_non`` (n v, 64), ``crop`` (crops, input_dim; mode 3d), ``{self,nn,random}_{lin,
        non}`` (crops, 64) dropout scales (values 0 or 1 / (1 - p)); ``nn_pick`` (crops) in
        [0, knn_neighbors) and ``random_idx`` (crops) in [0, buffer_filled)."""
        d = self._draws
        if d is not None and name in d:
            return d[name]
        return make()

    def _scale(self, name, groups, channels, p, device):
        """Dropout scales (groups, channels) f32, or None in eval mode / at p = 0."""
        if not self.training:
            return None

        def make():
            if p <= 0:
                return None
            return (torch.rand(groups, channels, device=device) >= p).float() / (1.0 - p)

        m = self._draw(name, make)
        return None if m is None else m.to(device=device, dtype=torch.float32).contiguous()

    def _update_buffer(self, buffer, x):
        # semantic_head.py:272-282
        n = x.size(0)
        if n >= self.buffer_size:
            buffer[:] = x[-self.buffer_size:]
            return 0
        indices = (torch.arange(n) + self.buffer_idx) % self.buffer_size
        buffer[indices.to(buffer.device)] = x
        return (self.buffer_idx + n) % self.buffer_size

    def _compute_stego_correlation(self, tensor1, tensor2):
        return torch.einsum("npf,nqf->npq", _norm(tensor1), _norm(tensor2))

    def forward_training(self, data, visualize=False, sample_factor=4):
        """semantic_head.py:122-235, same control flow and result keys."""
        if self.apply_crf and not self.native_crf:
            # head.native_crf = True runs this package's dense CRF instead
            raise NotImplementedError("apply_crf needs pydensecrf, which this build does not ship")
        raw =data["coarse"][0]["dino_features"].detach()  # (n, v, h, w, 1, c), un-normalised
        n, v, h, w, _, c = raw.shape
        dev = raw.device
        sh = self.stego_head
        p_lin, p_non = sh.linear_path[1].p, sh.nonlinear_path[3].p
        if self.training and torch.is_grad_enabled():
            track_steps(self)
        rows = raw.reshape(n * v * h * w, c)
        m_img = (self._scale("img_lin", n * v, self.code_dim, p_lin, dev),
                 self._scale("img_non", n * v, self.code_dim, p_non, dev))
        m_dino = self._scale("dino", n * v, c, self.dropout.p, dev)
        # image rows: detached downstream, so the forward-only pass
        stego_features = sh.train_rows(rows, *m_img, rows_per_group=h * w, normalize=True,
                                       differentiable=False).view(n, v, h, w, 1, -1)
        nv_used = v

        data["segmentation"] = {}
        if data["sample_surface_sigma"] is not None:
            if self.mode == "3d":
                cropped = _norm(data["sample_surface_dino_features"].detach().squeeze(0).float())
                nc, P = cropped.shape[:2]
                m_crop = self._scale("crop", nc, c, self.dropout1d.p, dev)
                if m_crop is not None:
                    cropped = cropped * m_crop[:, None, :]
                self_in = cropped
                m_self = (self._scale("self_lin", nc, self.code_dim, p_lin, dev),
                          self._scale("self_non", nc, self.code_dim, p_non, dev))
            elif self.mode == "2d":
                nv_used = 1
                normed = _norm(_five_crop(raw[:, :1], sample_factor).float())
                normed = normed.flatten(0, 1).flatten(1, 2).squeeze(-2)  # (5 n, P, c)
                nc, P = normed.shape[:2]
                first = torch.arange(n, device=dev) * v  # mask group of view 0 of every image
                cropped = normed
                if m_dino is not None:
                    cropped = normed * m_dino[first].repeat(5, 1)[:, None, :]
                # the crops of the image pass: the same rows with their image's masks
                self_in = normed
                m_self = tuple(None if m is None else m[first].repeat(5, 1).contiguous()
                               for m in m_img)
            else:
                raise NotImplementedError(f"SemanticHead mode '{self.mode}'")
            gap = _norm(cropped.mean(dim=-2))

            if self.training:
                if self.dino_patch_buffer is None:
                    raise ValueError("forward_training in train mode needs buffer_size > 0")
                if self.dino_patch_buffer.device != dev:
                    self.dino_patch_buffer = self.dino_patch_buffer.to(dev)
                    self.dino_gap_buffer = self.dino_gap_buffer.to(dev)
                new_idx = self._update_buffer(self.dino_patch_buffer, cropped)
                assert new_idx == self._update_buffer(self.dino_gap_buffer, gap)
                if new_idx < self.buffer_idx:
                    self.buffer_filled = self.buffer_size
                else:
                    self.buffer_filled = max(new_idx, self.buffer_filled)
                self.buffer_idx = new_idx
            patch_buffer = self.dino_patch_buffer.to(dev)
            gap_buffer = self.dino_gap_buffer.to(dev)

            sims = torch.einsum("nf,mf->nm", gap, gap_buffer)
            topk = torch.topk(sims, self.knn_neighbors + 1, dim=1)[1][:, 1:]
            pick = self._draw("nn_pick", lambda: torch.randint(self.knn_neighbors, (nc,)))
            nn_idx = topk[torch.arange(nc, device=dev), torch.as_tensor(pick).to(dev)]
            dino_nn = patch_buffer[nn_idx].detach()
            rnd = self._draw("random_idx", lambda: torch.randint(self.buffer_filled, (nc,)))
            dino_random = patch_buffer[torch.as_tensor(rnd).to(dev)].detach()
            m_nn = (self._scale("nn_lin", nc, self.code_dim, p_lin, dev),
                    self._scale("nn_non", nc, self.code_dim, p_non, dev))
            m_rnd = (self._scale("random_lin", nc, self.code_dim, p_lin, dev),
                     self._scale("random_non", nc, self.code_dim, p_non, dev))

            # the three differentiable StegoClusterHead calls as one: rows [self | nn | random]
            x3 = torch.cat([self_in.reshape(nc * P, c), dino_nn.reshape(nc * P, c),
                            dino_random.reshape(nc * P, c)])
            masks = []
            for i in range(2):
                ms = (m_self[i], m_nn[i], m_rnd[i])
                if all(m is None for m in ms):
                    masks.append(None)
                else:
                    one = torch.ones(nc, self.code_dim, device=dev)
                    masks.append(torch.cat([one if m is None else m for m in ms]).contiguous())
            y3 = sh.train_rows(x3, *masks, rows_per_group=P, normalize=False).view(3, nc, P, -1)
            stego_self, stego_nn, stego_random = y3[0], y3[1], y3[2]

            corr = self._compute_stego_correlation
            # lazy: the partner rows as views of the stacked crop rows (one tensor kept alive)
            x3v = x3.view(3, nc, P, c)
            data["segmentation"]["stego_corr"] = StegoCorrMap(
                (x3v[0] if cropped is self_in else cropped, x3v[1], x3v[2]),
                (stego_self, stego_nn, stego_random), corr) if self.lazy_corr else {
                "dino_self_corr": corr(cropped, cropped),
                "stego_self_corr": corr(stego_self, stego_self),
                "dino_nn_corr": corr(cropped, dino_nn),
                "stego_nn_corr": corr(stego_self, stego_nn),
                "dino_random_corr": corr(cropped, dino_random),
                "stego_random_corr": corr(stego_self, stego_random),
            }
        else:
            data["sample_surface_sigma"] = torch.Tensor([0.0])
            data["sample_surface_dino_features"] = torch.Tensor([0.0])

        # the cluster heads train on detached features (mode 2d keeps view 0 only)
        feats = raw[:, :nv_used]
        stego_features = stego_features[:, :nv_used].detach()
        m_direct = m_dino
        if m_dino is not None and nv_used != v:
            m_direct = m_dino[torch.arange(n, device=dev) * v].contiguous()
        direct = self.direct_cluster_head(feats, _mask=m_direct, _rows_per_group=h * w) \
            if m_direct is not None else self.direct_cluster_head(feats)
        stego = self.stego_cluster_head(stego_features)
        results = data["segmentation"]["results"] = {"direct_cluster": direct,
                                                     "stego_cluster": stego}

        if "segs" in data:
            segs = data["segs"][0]
            idx = segs.long() + 1  # ids in [-1, 255]; any other id maps to 0, as in the loop
            known = (idx >= 0) & (idx <= 256)
            seg_target = (self._train_id_lut(segs.device, segs.dtype == torch.uint8)[idx.clamp(0, 256)] * known).to(dev)
            if isinstance(self.direct_linear_head, LinearHead):
                # the raw rows: the probe normalises, then applies the Dropout2d scale
                results["direct_linear"] = self.direct_linear_head(
                    feats, seg_target, _mask=m_direct, _rows_per_group=h * w, _normalize=True)
                results["stego_linear"] = self.stego_linear_head(stego_features, seg_target)
            else:
                dino_features = _norm(feats.float())
                if m_direct is not None:
                    dino_features = dino_features * m_direct.view(n, nv_used, 1, 1, 1, c)
                results["direct_linear"] = self.direct_linear_head(dino_features, seg_target)
                results["stego_linear"] = self.stego_linear_head(stego_features, seg_target)
            data["segmentation"]["target"] = seg_target

        if self.apply_crf:
            self._add_crf_results(results, data["coarse"][0]["rgb"].detach())

        if self._colors(dev) is not None:
            vis = data["segmentation"]["visualization"] = {
                name: self.visualize(result["segs_pred"]) for name, result in results.items()}
            if "segs" in data:
                vis["target"] = self.visualize(data["segmentation"]["target"])
        return data

    def _add_crf_results(self, results, rgb):
        """semantic_head.py:224-233 with ``native_crf``: every result gains ``<name>_crf`` =
        {"segs_pred": its labels after the dense CRF (downstream_head/crf.py)}, same shape and
        dtype.  rgb (n, v, h, w, 1, 3) in [0, 1].  The reference's forward_crf squeezes, so it
        handles n = v = 1 only; here every (n, v) image of a result runs on its own, all results
        of one image in one inference (one native call).  The class count is gt_classes (every
        segs_pred lies in [0, gt_classes)), so no host read is made."""
        from .crf import dense_crf_labels_multi
        names = list(results)
        preds = [results[k]["segs_pred"] for k in names]
        out = [torch.empty_like(p) for p in preds]
        n, v = rgb.shape[:2]
        for i in range(n):
            for j in range(max(p.shape[1] for p in preds)):
                if j >= v:
                    raise ValueError("SemanticHead: a result has more views than data['coarse'][0]['rgb']")
                idx = [r for r, p in enumerate(preds) if j < p.shape[1]]
                image = rgb[i, j].reshape(rgb.shape[2], rgb.shape[3], 3).permute(2, 0, 1)
                refined = dense_crf_labels_multi(image, [preds[r][i, j] for r in idx], self.gt_classes)
                for r, lab in zip(idx, refined):
                    out[r][i, j] = lab
        for name, o in zip(names, out):
            results[name + "_crf"] = {"segs_pred": o}

    def update_model_eval(self, metrics):
        self.direct_cluster_head.pseudo_assignment[:] = metrics["direct_cluster_assignment"]
        self.stego_cluster_head.pseudo_assignment[:] = metrics["stego_cluster_assignment"]

    def _train_id_lut(self, device, uint8=False):
        """(257) int64 on device: entry id + 1 is map_kitti_id_to_train_id's value for the label
        id in [-1, 255] (0 for an id the table lacks, trainId 255 -> -1), built once per label
        table instead of one host copy per label and step.  uint8: the table for uint8 labels,
        where the loop's comparison wraps a negative table id (-1 matches 255)."""
        table = _kitti_labels()
        if table is None:
            raise RuntimeError("SemanticHead: 'segs' needs the KITTI-360 label table "
                               "(datasets.kitti_360.labels), which is not importable")
        cache = getattr(self, "_lut_cache", None)
        if cache is None or cache[0] is not table:
            luts = torch.zeros(2, 257, dtype=torch.int64)
            for lab in table.labels:  # in table order: a later entry of the same id wins
                if -1 <= lab.id <= 255:
                    luts[0, lab.id + 1] = lab.trainId
                if -256 <= lab.id <= 255:
                    luts[1, lab.id % 256 + 1] = lab.trainId
            luts[luts == 255] = -1
            cache = self._lut_cache = (table, {torch.device("cpu"): luts})
        device = torch.device(device)
        if device not in cache[1]:
            cache[1][device] = cache[1][torch.device("cpu")].to(device)
        return cache[1][device][int(uint8)]

    def map_kitti_id_to_train_id(self, labels):
        table = _kitti_labels()
        if table is None:
            raise RuntimeError("SemanticHead: 'segs' needs the KITTI-360 label table "
                               "(datasets.kitti_360.labels), which is not importable")
        result = torch.zeros(labels.shape).long()
        for lab in table.labels:
            result[labels.cpu() == lab.id] = lab.trainId
        result[result == 255] = -1
        return result

    def _colors(self, device):
        if self._label_colors is None:
            table = _kitti_labels()
            if table is None:
                return None
            colors = [torch.Tensor(table.trainId2label[i].color) for i in range(self.gt_classes)]
            colors.append(torch.Tensor([0, 0, 0]))
            self._label_colors = torch.stack(colors, dim=0) / 255.0
        if self._label_colors.device != device:
            self._label_colors = self._label_colors.to(device)
        return self._label_colors

    def visualize(self, labels):
        colors = self._colors(labels.device)
        if colors is None:
            raise RuntimeError("SemanticHead.visualize needs the KITTI-360 label table "
                               "(datasets.kitti_360.labels), which is not importable")
        return colors[labels.long()]

    def parameters_lr(self):
        return [
            (1.0, self.stego_head.parameters()),
            (10.0, self.direct_cluster_head.parameters()),
            (10.0, self.stego_cluster_head.parameters()),
            (10.0, self.direct_linear_head.parameters()),
            (10.0, self.stego_linear_head.parameters()),
        ]
