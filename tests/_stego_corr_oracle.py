"""Torch formulas of the STEGO correlation loss for tests/test_stego_corr.py and
test_stego_corr_gpu.py, restated from the reference (scenedino/downstream_head/semantic_head.py
:181-188,268-270 for the correlations, scenedino/losses/stego_loss.py:40-46,71-79 for their
reduction, the in-place row-mean removal included), plus the seeded operand rows the tests share.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

# weights and shifts of configs/training/loss/semantic.yaml, in (self, knn, random) order
YAML_WEIGHTS = (0.08146997886146659, 0.4156436438453117, 0.6702352279261414)
YAML_SHIFTS = (0.43610463774158115, 0.18458300726748128, 0.8709334888837256)


def norm(x):
    return F.normalize(x, dim=-1, eps=1e-10)


def corr(t1, t2):
    return torch.einsum("npf,nqf->npq", norm(t1), norm(t2))


def reference_pair_loss(dino_corr, stego_corr, weight, shift, pointwise):
    """stego_loss.py:71-79 on two correlation tensors; edits dino_corr in place when pointwise."""
    if pointwise:
        old_mean = dino_corr.mean()
        dino_corr -= dino_corr.mean(dim=-1, keepdim=True)
        dino_corr = dino_corr - dino_corr.mean() + old_mean
    return (-weight * stego_corr.clamp(0) * (dino_corr - shift)).mean()


def factored_dino(A, B):
    """The pointwise centring without an in-place edit: D - A^ . mean_q B^ + mean of that."""
    Ah, Bh = norm(A), norm(B)
    r = torch.einsum("npf,nf->np", Ah, Bh.mean(dim=1))
    return torch.einsum("npf,nqf->npq", Ah, Bh) - r[..., None] + r.mean()


def pair_losses(A, Bs, a, bs, weights, shifts, pointwise):
    """The fused route's formula: one loss per pair.  Bs[i] / bs[i] None: the self pair.
    max(S, 0) is written as relu, whose autograd rule is the indicator 1[S > 0] the kernel uses
    (clamp's rule is 1[S >= 0]: it differs only where S is exactly zero, a zero code row, which
    it would hand a gradient of 1 / 1e-10 through the clamped norm)."""
    out = []
    for B, b, w, sh in zip(Bs, bs, weights, shifts):
        B, b = (A, a) if B is None else (B, b)
        D = factored_dino(A, B) if pointwise else corr(A, B)
        out.append((-w * torch.relu(corr(a, b)) * (D - sh)).mean())
    return torch.stack(out)


def evaluate(rows, weights, shifts, pointwise, up, dtype=torch.float64, autocast=False):
    """{"loss" (n_pairs), "d_a", "d_b<i>" per partner} of sum(up * losses): the formula in
    ``dtype`` on the CPU, or in f32 under bf16 autocast."""
    cast = (lambda t: None if t is None else t.detach().cpu().to(torch.float32 if autocast else dtype))
    A, Bs = cast(rows["A"]), [cast(t) for t in rows["Bs"]]
    a = cast(rows["a"]).requires_grad_(True)
    bs = [None if t is None else cast(t).requires_grad_(True) for t in rows["bs"]]
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        loss = pair_losses(A, Bs, a, bs, weights, shifts, pointwise)
    leaves = [a] + [b for b in bs if b is not None]
    grads = torch.autograd.grad((loss.to(a.dtype) * up.detach().cpu().to(a.dtype)[:len(bs)]).sum(), leaves)
    out = {"loss": loss.detach(), "d_a": grads[0]}
    k = 1
    for i, b in enumerate(bs):
        if b is not None:
            out[f"d_b{i}"] = grads[k]
            k += 1
    return out


def make_rows(nc, P, Q, d, n_pairs=3, self_pair=True, separated=False, zero_rows=False, seed=0):
    """Seeded operand rows: A (nc, P, d), a (nc, P, 64), partners (nc, Q, ..) (the first pair is
    the self pair when self_pair).  DINO rows share a common direction so that D has the spread
    of real features.  separated: every code row sits near one of four orthogonal directions or
    their negatives, so that no |S| lies near zero.  zero_rows: code row (0, 1) and DINO row
    (0, 2) of the A side are zero."""
    g = torch.Generator().manual_seed(9000 + 131 * seed + 7 * P + Q + d + nc)
    common = torch.randn(d, generator=g)

    def dino(n):
        return (common + 1.5 * torch.randn(nc, n, d, generator=g)) * (torch.rand(nc, n, 1, generator=g) * 2 + 0.2)

    def code(n):
        if not separated:
            return torch.randn(nc, n, 64, generator=g) * (torch.rand(nc, n, 1, generator=g) * 3 + 0.1)
        # blocks of 16 channels: direction k is the all-ones vector of block k, signed
        k = torch.randint(4, (nc, n), generator=g)
        sign = torch.randint(2, (nc, n), generator=g) * 2.0 - 1.0
        base = torch.zeros(nc, n, 64)
        # every row also carries a fixed share of every other block, so S is +-(1 - small) or
        # about +-0.3, never near zero
        for blk in range(4):
            base[..., 16 * blk:16 * blk + 16] = torch.where(k == blk, 1.0, 0.35)[..., None]
        base = base * sign[..., None] + 0.01 * torch.randn(nc, n, 64, generator=g)
        return base * (torch.rand(nc, n, 1, generator=g) * 3 + 0.1)

    rows = {"A": dino(P), "a": code(P), "Bs": [], "bs": []}
    for i in range(n_pairs):
        if i == 0 and self_pair:
            rows["Bs"].append(None)
            rows["bs"].append(None)
        else:
            rows["Bs"].append(dino(Q))
            rows["bs"].append(code(Q))
    if zero_rows:
        rows["a"][0, 1 % P] = 0.0
        rows["A"][0, 2 % P] = 0.0
    return rows


def min_abs_S(rows):
    """The smallest |S| over every pair, on the f64 formula."""
    a = rows["a"].double()
    vals = []
    for b in rows["bs"]:
        vals.append(corr(a, a if b is None else b.double()).abs().min())
    return float(torch.stack(vals).min())
