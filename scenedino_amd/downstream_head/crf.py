"""Dense-CRF post-processing, MI355X build.

Mirror of scenedino/downstream_head/crf.py (``dense_crf`` :20-43) without pydensecrf: mean-field
inference of the fully connected CRF that ``DenseCRF2D`` defines with its default arguments (Potts
compatibility, diagonal kernels, symmetric normalisation), a Gaussian and a bilateral potential
over the N = H W pixels of one image:

    f^g_i = (x_i, y_i) / sxy_g
    f^b_i = (x_i / sxy_b, y_i / sxy_b, r_i / srgb, g_i / srgb, b_i / srgb)
    k^p_ij = exp(-|f^p_i - f^p_j|^2 / 2)            for every j, j = i included
    n^p_i  = (sum_j k^p_ij + 1e-20)^(-1/2)
    Q^0_i  = softmax_c(-U_i)
    Q^{t+1}_i = softmax_c(-U_i(c) + sum_p w_p n^p_i sum_j k^p_ij n^p_j Q^t_j(c)),   t < iters
    labels_i = argmax_c Q^{iters}_i(c)               (lowest index on a tie)

pydensecrf evaluates the pair sums with a permutohedral-lattice approximation; here they are
evaluated exactly, the definition that approximation targets.  Parity with pydensecrf's own
numbers is unpinned: the package is not a dependency of this build and nothing here is compared
against it.

Two routes, the same mathematics:
  native  ``sd_dense_crf`` (csrc/sdhip_crf.hip) for CUDA tensors inside its domain: all results of
          one image in one call, the pair weights computed once per iteration for all of them;
  torch   the bilateral sums blocked over key columns (every query row adds the blocks in the
          same ascending order; on the GPU the tall (N, block) x (block, classes) float64 product
          of a key block ran some seventy times faster than the wide one of a query-row block),
          the Gaussian ones as two separable factors, all in float64 with no pair dropped, on any
          device: the route the CPU tests pin against the brute-force oracle, and the fallback
          outside the native domain.
``last_route`` names the route of the most recent call ("native" or "torch").
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from .. import _lib

# scenedino/downstream_head/crf.py:12-17
MAX_ITER = 10
POS_W = 3
POS_XY_STD = 0.3
Bi_W = 4
Bi_XY_STD = 20
Bi_RGB_STD = 3

# False: every call takes the torch route (tools/crf_bench.py's baseline)
_NATIVE = True
last_route = None

_TORCH_BLOCK_BYTES = 32 << 20  # one (block, N) float64 temporary of the torch route (x 8 on a GPU)


def _params(iters=None, w_g=None, sxy_g=None, w_b=None, sxy_b=None, srgb=None):
    pick = lambda v, d: d if v is None else v  # noqa: E731
    return {"iters": int(pick(iters, MAX_ITER)), "w_g": float(pick(w_g, POS_W)),
            "sxy_g": float(pick(sxy_g, POS_XY_STD)), "w_b": float(pick(w_b, Bi_W)),
            "sxy_b": float(pick(sxy_b, Bi_XY_STD)), "srgb": float(pick(srgb, Bi_RGB_STD))}


def image_to_uint8(image):
    """(3, H, W) float image -> (H, W, 3) uint8, contiguous: trunc(255 clamp(x, 0, 1)).  The
    reference goes through ``to_pil_image``, which truncates 255 x with ``.byte()`` and so wraps
    a value outside [0, 1]; here such a value is clamped.  Its BGR flip is immaterial (one srgb
    for all channels).  A uint8 image passes through (channels moved last)."""
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"dense_crf: image must be (3, H, W), got {tuple(image.shape)}")
    if image.dtype == torch.uint8:
        return image.permute(1, 2, 0).contiguous()
    x = image.detach().float().clamp(0.0, 1.0) * 255.0
    return x.to(torch.uint8).permute(1, 2, 0).contiguous()


def unary_from_logits(logits, size):
    """(c, h', w') logits -> U (c, H W) float32 = -log softmax of the logits resized bilinearly
    (align_corners=False) to size = (H, W)."""
    x = logits.detach().float()
    if tuple(x.shape[1:]) != tuple(size):
        x = F.interpolate(x.unsqueeze(0), size=tuple(size), mode="bilinear", align_corners=False)[0]
    return (-F.log_softmax(x, dim=0)).reshape(x.shape[0], -1).contiguous()


def unary_from_labels(labels, num_classes):
    """Labels (H W) -> the unary of their one-hot logits, (num_classes, H W) float32:
    log(e + c - 1) - [c = label], without the one-hot tensor's softmax."""
    lab = labels.reshape(-1).long()
    lse = math.log(math.e + num_classes - 1)
    U = torch.full((num_classes, lab.numel()), lse, dtype=torch.float32, device=lab.device)
    U.scatter_(0, lab[None], lse - 1.0)
    return U


def _native_ok(image_u8, unaries, p):
    if not (_NATIVE and image_u8.is_cuda and image_u8.is_contiguous()):
        return False
    H, W = image_u8.shape[:2]
    return (1 <= H <= 4096 and 1 <= W <= 4096 and H * W <= 1 << 20
            and 1 <= len(unaries) <= _lib.CRF_MAX_RESULTS
            and all(2 <= u.shape[0] <= _lib.CRF_MAX_CLASSES for u in unaries)
            and 0 <= p["iters"] <= 64 and 0 < p["sxy_g"] <= _lib.CRF_MAX_SXY_G
            and 0 < p["sxy_b"] < math.inf and 0 < p["srgb"] < math.inf
            and 0 <= p["w_g"] < math.inf and 0 <= p["w_b"] < math.inf)


def _torch_inference(image_u8, unaries, p):
    """The model above in float64, blocked over query rows: [Q (c_r, N) float64 per result]."""
    dev = image_u8.device
    H, W = image_u8.shape[:2]
    N = H * W
    f64 = torch.float64
    idx = torch.arange(N, device=dev)
    cls = [u.shape[0] for u in unaries]
    CT = sum(cls)
    U = torch.cat([u.to(f64).t() for u in unaries], dim=1)  # (N, CT)
    # bilateral exponent -|f_i - f_j|^2 / 2 = f_i.f_j - |f_i|^2 / 2 - |f_j|^2 / 2 as one float64
    # product of augmented features (in float64 the cancellation is below 1e-11 of an exponent)
    fb = torch.cat([torch.stack([idx % W, idx // W], dim=1).to(f64) / p["sxy_b"],
                    image_u8.reshape(N, 3).to(f64) / p["srgb"]], dim=1)
    half = -0.5 * (fb * fb).sum(1, keepdim=True)
    one = torch.ones_like(half)
    fq, fk = torch.cat([fb, half, one], dim=1), torch.cat([fb, one, half], dim=1).t().contiguous()
    # the Gaussian kernel is separable: K^g = K^y (x) K^x
    ax = torch.arange(max(H, W), device=dev, dtype=f64)
    kfull = torch.exp(-0.5 * ((ax[:, None] - ax[None, :]) / p["sxy_g"]) ** 2)
    ky, kx = kfull[:H, :H], kfull[:W, :W]
    block = max(1, min(N, (8 if dev.type == "cuda" else 1) * _TORCH_BLOCK_BYTES // (8 * N)))

    def bilateral(j0, j1):
        """Columns j0 .. j1 of K^b, (N, j1 - j0)."""
        return torch.exp_(fq @ fk[:, j0:j1])

    def softmax(x):
        return torch.cat([torch.softmax(s, dim=1) for s in x.split(cls, dim=1)], dim=1)

    Q = softmax(-U)
    if p["iters"] > 0:
        ng = ((ky.sum(1)[:, None] * kx.sum(1)[None, :]).reshape(N) + 1e-20) ** -0.5
        nb = torch.zeros(N, dtype=f64, device=dev)
        for j0 in range(0, N, block):
            nb += bilateral(j0, min(j0 + block, N)).sum(1)
        nb = (nb + 1e-20) ** -0.5
    for _ in range(p["iters"]):
        Qb = Q * nb[:, None]
        msg = torch.zeros_like(Q)
        for j0 in range(0, N, block):
            j1 = min(j0 + block, N)
            msg.addmm_(bilateral(j0, j1), Qb[j0:j1])
        msg *= p["w_b"] * nb[:, None]
        gauss = torch.einsum("yv,xu,vuc->yxc", ky, kx, (Q * ng[:, None]).view(H, W, CT)).reshape(N, CT)
        msg += p["w_g"] * ng[:, None] * gauss
        Q = softmax(msg - U)
    return [q.t().contiguous() for q in Q.split(cls, dim=1)]


def crf_inference(image_u8, unaries, want_q=False, **params):
    """image_u8 (H, W, 3) uint8, unaries a list of (c_r, H W) float32 on its device ->
    (labels (R, H W) int64, [Q (c_r, H W) float32 per result] or None).  Sets ``last_route``."""
    global last_route
    p = _params(**params)
    if image_u8.dtype != torch.uint8 or image_u8.dim() != 3 or image_u8.shape[2] != 3:
        raise ValueError("crf_inference: image must be (H, W, 3) uint8")
    N = image_u8.shape[0] * image_u8.shape[1]
    if not unaries or any(u.dim() != 2 or u.shape[1] != N or u.device != image_u8.device
                          for u in unaries):
        raise ValueError("crf_inference: unaries must be (c, H W) tensors on the image's device")
    if p["iters"] < 0:
        raise ValueError("crf_inference: iters must be >= 0")
    if _native_ok(image_u8, unaries, p):
        cls = [u.shape[0] for u in unaries]
        U = unaries[0] if len(unaries) == 1 else torch.cat(unaries, dim=0)
        labels, q = _lib.dense_crf(image_u8, U.float().contiguous(), cls, want_q=want_q, **p)
        last_route = "native"
        return labels, (list(q.split(cls, dim=0)) if want_q else None)
    qs = _torch_inference(image_u8.contiguous(), unaries, p)
    last_route = "torch"
    labels = torch.stack([q.argmax(dim=0) for q in qs])
    return labels, ([q.float() for q in qs] if want_q else None)


def dense_crf_labels_multi(image, labels, num_classes=None, **params):
    """``dense_crf_labels`` for several label maps of one image in one inference (one native
    call): labels a list of tensors of H W elements each, num_classes None, an int, or one entry
    per map.  Returns the refined maps, shape and dtype of the inputs."""
    u8 = image_to_uint8(image)
    if not isinstance(num_classes, (list, tuple)):
        num_classes = [num_classes] * len(labels)
    unaries = []
    for lab, c in zip(labels, num_classes):
        lab = lab.to(u8.device)
        c = int(lab.max()) + 1 if c is None else int(c)  # None: one host read, as the reference
        unaries.append(unary_from_labels(lab, c))
    out, _ = crf_inference(u8, unaries, **params)
    return [o.reshape(lab.shape).to(device=lab.device, dtype=lab.dtype) for o, lab in zip(out, labels)]


def dense_crf_labels(image, labels, num_classes=None, **params):
    """SemanticHead.forward_crf (semantic_head.py:237-241) on device tensors: image (3, H, W)
    float in [0, 1] (``image_to_uint8``), labels of H W elements -> the labels after the CRF on
    the unary of their one-hot logits, same shape and dtype.  num_classes None: labels.max() + 1
    as the reference (one host read); pass it where it is known."""
    return dense_crf_labels_multi(image, [labels], [num_classes], **params)[0]


def dense_crf_q(image, logits, **params):
    """``dense_crf`` on device tensors: image (3, H, W) float, logits (c, h', w') -> Q^{iters}
    (c, H, W) float32 on the image's device."""
    u8 = image_to_uint8(image)
    H, W = u8.shape[:2]
    _, qs = crf_inference(u8, [unary_from_logits(logits.to(u8.device), (H, W))], want_q=True, **params)
    return qs[0].reshape(-1, H, W)


def dense_crf(image_tensor, output_logits):
    """scenedino/downstream_head/crf.py:20-43 with its constants: a (c, H, W) numpy array."""
    return dense_crf_q(image_tensor, output_logits).cpu().numpy()
