"""CPU formulas of the STEGO head's training path, restated from the reference
(scenedino/downstream_head/semantic_head.py: StegoClusterHead :285-305 with its Dropout2d layers
written as explicit scales, KMeansParamHead._kmeans_cosine :361-373, forward_training :122-235)
for tests/test_stego_train.py, test_cluster_probe.py and test_semantic_head_train.py, plus the
seeded weights and inputs the reference fixture (tests/golden/make_golden_stego.py) shares
with the tests.

Yardstick (tests/test_expand_train.py's rule): a native tensor's rel-L2 distance to the CPU
fp32 evaluation of a formula is at most 2 x the rel-L2 error of the same formula under CPU
bf16 autocast, measured on the same inputs, per tensor, and printed.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

BF = torch.bfloat16
STEGO_NAMES = ("linear_path.0.weight", "linear_path.0.bias", "nonlinear_path.0.weight",
               "nonlinear_path.0.bias", "nonlinear_path.2.weight", "nonlinear_path.2.bias")


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def check(native, f32, f16, names, what=""):
    """The yardstick over the named tensors of three dicts; prints every figure first."""
    for n in names:
        print(f"{what} {n}: native rel-L2 {rel_l2(native[n], f32[n]):.6f}, "
              f"autocast oracle {rel_l2(f16[n], f32[n]):.6f}")
    for n in names:
        g = native[n].float().cpu()
        assert g.shape == f32[n].shape and bool(torch.isfinite(g).all()), n
        e = rel_l2(f16[n], f32[n])
        assert math.isfinite(e) and e > 0, f"{n}: the autocast yardstick is {e}"
        r = rel_l2(g, f32[n])
        assert r <= 2 * e, f"{what} {n}: rel-L2 {r:.6f} > 2 x {e:.6f}"


def rows_scale(m, rows_per_group, M):
    return m.repeat_interleave(rows_per_group, dim=0)[:M]


def dropout_scales(groups, channels, gen, p=0.1):
    """About p zeros, the rest 1 / (1 - p): what Dropout2d multiplies a (group, channel) by."""
    return (torch.rand(groups, channels, generator=gen) >= p).float() / (1 - p)


# ------------------------------------------------------------------------ StegoClusterHead
def stego_formula(x, wl, bl, wn1, bn1, wn2, bn2, m_lin=None, m_non=None, rows_per_group=1,
                  normalize=True):
    """x (M, d_in) -> (M, 64): linear_path + nonlinear_path (1x1 convolutions as matrices,
    Dropout2d as the given scales), L2-normalised; the input normalised first (normalize)."""
    M = x.shape[0]
    xh = F.normalize(x, dim=-1, eps=1e-10) if normalize else x
    lin = F.linear(xh, wl.reshape(wl.shape[0], -1), bl)
    non = F.linear(F.relu(F.linear(xh, wn1.reshape(wn1.shape[0], -1), bn1)),
                   wn2.reshape(wn2.shape[0], -1), bn2)
    if m_lin is not None:
        lin = lin * rows_scale(m_lin, rows_per_group, M)
    if m_non is not None:
        non = non * rows_scale(m_non, rows_per_group, M)
    return F.normalize(lin + non, dim=-1, eps=1e-10)


def stego_inputs(M, d_in, rows_per_group=48, zero_row=None):
    """Rows of mixed scale, weights giving pre-activations of about unit spread (half of mid is
    dead), masks with about 10 % zeros, an output gradient."""
    g = torch.Generator().manual_seed(7000 * d_in + M)
    G = (M + rows_per_group - 1) // rows_per_group
    d = {"x": torch.randn(M, d_in, generator=g) * (torch.rand(M, 1, generator=g) * 3 + 0.05),
         "linear_path.0.weight": torch.randn(64, d_in, 1, 1, generator=g),
         "linear_path.0.bias": torch.randn(64, generator=g) * 0.1,
         "nonlinear_path.0.weight": torch.randn(d_in, d_in, 1, 1, generator=g),
         "nonlinear_path.0.bias": torch.randn(d_in, generator=g) * 0.1,
         "nonlinear_path.2.weight": torch.randn(64, d_in, 1, 1, generator=g) * (1.4 / math.sqrt(d_in)),
         "nonlinear_path.2.bias": torch.randn(64, generator=g) * 0.1,
         "m_lin": dropout_scales(G, 64, g), "m_non": dropout_scales(G, 64, g),
         "dy": torch.randn(M, 64, generator=g), "rows_per_group": rows_per_group}
    if zero_row is not None:
        d["x"][zero_row] = 0.0
    return d


def stego_eval(d, autocast, masks=True):
    """{"y", six parameter gradients} of sum(y * dy) on the CPU, fp32 or under bf16 autocast."""
    leaves = [d[n].clone().requires_grad_(True) for n in STEGO_NAMES]
    with torch.autocast("cpu", dtype=BF, enabled=autocast):
        y = stego_formula(d["x"], *leaves, d["m_lin"] if masks else None,
                          d["m_non"] if masks else None, d["rows_per_group"])
    gs = torch.autograd.grad((y.float() * d["dy"]).sum(), leaves)
    out = {n: g.float() for n, g in zip(STEGO_NAMES, gs)}
    out["y"] = y.detach().float()
    return out


# ------------------------------------------------------------------------ KMeansParamHead
def probe_xhat(x, m=None, rows_per_group=1):
    x = x.float()
    if m is not None:
        x = x * rows_scale(m, rows_per_group, x.shape[0])
    return F.normalize(x, dim=1)


def probe_stats(xh, centres, labels, w=None):
    """S (K, d) = sum_{label_i = k} w_i xh_i as the matmul one_hot^T (w xh), and the loss
    -sum_k c_k . S_k / N (KMeansParamHead's mean(cluster_loss * weight))."""
    K = centres.shape[0]
    hot = F.one_hot(labels.long(), K).to(torch.float32)
    if w is not None:
        hot = hot * w[:, None]
    S = hot.t() @ xh
    loss = -(F.normalize(centres, dim=1) * S.float()).sum() / xh.shape[0]
    return S, loss


def kmeans_loss(x, centres, w=None, labels=None, m=None, rows_per_group=1):
    """KMeansParamHead.forward's loss (semantic_head.py:349-373); labels: the one-hot
    assignment to use instead of the formula's own argmax."""
    scores = probe_xhat(x, m, rows_per_group).matmul(F.normalize(centres, dim=1).t())
    if labels is None:
        labels = torch.argmax(scores, dim=1)
    probs = F.one_hot(labels.long(), centres.shape[0]).to(torch.float32)
    cluster_loss = -(probs * scores).sum(1)
    wf = torch.ones(x.shape[0]) if w is None else w
    return torch.mean(cluster_loss * wf), labels


# ------------------------------------------------------------------------ SemanticHead fixture
HEAD_ARGS = dict(n_classes=19, gt_classes=19, input_dim=768, code_dim=64, buffer_size=8,
                 patch_sample_size=16, knn_neighbors=2)
HEAD_SEEDS = {"3d": 11, "2d": 12}
STEGO_LOSS = dict(random_weight=0.6702352279261414, knn_weight=0.4156436438453117,
                  self_weight=0.08146997886146659, random_shift=0.8709334888837256,
                  knn_shift=0.18458300726748128, self_shift=0.43610463774158115)


def head_state(seed):
    """Seeded parameters of SemanticHead(19, 19, 768, 64) by state-dict key (the linear probes
    keep their constructor values: no gradient reaches them without ``segs``)."""
    g = torch.Generator().manual_seed(seed)
    d = 768
    st = {"stego_head.linear_path.0.weight": torch.randn(64, d, 1, 1, generator=g),
          "stego_head.linear_path.0.bias": torch.randn(64, generator=g) * 0.1,
          "stego_head.nonlinear_path.0.weight": torch.randn(d, d, 1, 1, generator=g),
          "stego_head.nonlinear_path.0.bias": torch.randn(d, generator=g) * 0.1,
          "stego_head.nonlinear_path.2.weight": torch.randn(64, d, 1, 1, generator=g) * (1.4 / math.sqrt(d)),
          "stego_head.nonlinear_path.2.bias": torch.randn(64, generator=g) * 0.1,
          "direct_cluster_head.cluster_centers": torch.randn(19, d, generator=g)}
    # the stego centres: the head's output at the direct centres, scaled and perturbed, so that
    # features clustered around the direct centres have wide margins in both heads
    codes = stego_formula(st["direct_cluster_head.cluster_centers"],
                          *(st["stego_head." + n] for n in STEGO_NAMES))
    st["stego_cluster_head.cluster_centers"] = codes * 3 + 0.05 * torch.randn(19, 64, generator=g)
    return st


def head_step_inputs(seed, step, mode):
    """The data dict of one step (n = 2, v = 1, h = 16, w = 32, 3 crops of 16 points) and the
    number of crops its mode forms.  The image features are clustered around the seeded
    direct centres so that the k-means margins are wide (the fixture's generator checks
    them); a 2-D step has 5 n = 10 crops of 4 x 4 points at sample_factor 2."""
    g = torch.Generator().manual_seed(1000 * seed + step)
    n, v, h, w, c = 2, 1, 16, 32, 768
    dirs = F.normalize(head_state(seed)["direct_cluster_head.cluster_centers"], dim=1) * math.sqrt(c)
    pick = torch.randint(19, (n, v, h, w), generator=g)
    img = (dirs[pick] + 0.3 * torch.randn(n, v, h, w, c, generator=g)) * \
        (torch.rand(n, v, h, w, 1, generator=g) * 2 + 0.1)
    crops = dirs[torch.randint(19, (3, 16), generator=g)] + 0.7 * torch.randn(3, 16, c, generator=g)
    nc = 3 if mode == "3d" else 5 * n
    data = {"coarse": [{"rgb": torch.rand(n, v, h, w, 1, 3, generator=g),
                        "dino_features": img.unsqueeze(-2)}],
            "sample_surface_sigma": torch.rand(1, 3, 16, generator=g),
            "sample_surface_dino_features": crops.unsqueeze(0)}
    return data, nc
