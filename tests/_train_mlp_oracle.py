"""CPU oracle of the fused training MLP (csrc/sdhip_mlp.hip) for tests/test_train_mlp_shapes.py.

The operation, on rows x = [feat (C) | code (d_code) | 1] held in a 16-bit dtype:

    out = relu(x[:, :d_in] W_in^T + b_in) W_out^T + b_out,  sigma = softplus(out_0),  dino = out_1..D

and its gradients dx[:, :C], dW_in, db_in, dW_out, db_out for given d_sigma (N), d_dino (N, D).
``evaluate`` computes all of it in float64 (the reference) or under CPU autocast in the rows'
dtype (the yardstick: what the reference's own nn.Linear pair under autocast would give).

Tolerance rule (as tests/test_expand_train.py and tests/test_stego_train.py): a
native tensor lies within 2 x the rel-L2 error of the autocast evaluation against the float64
one, per tensor, on the same inputs.  A tensor whose yardstick is degenerate in a case (0, not
finite, or 0.1 and more) is named in ``dropped`` with the reason; at most one per case.

Input families:
  random     weights of the scale of tests/test_train_mlp.py, rows ~ N(0, 1).
  dead       every hidden bias negative, 10 % of the units at -50 (off in every row), and every
             fifth row (i % 5 == 2) with zero features and code: its pre-activations are the
             biases, so all 128 units are exactly off in it and its dx, dH rows are exactly 0.
  saturated  hidden unit 0 copies column C of the row (weight 1, bias 0), out_0 reads unit 0 alone
             (weight 1) with b_out[0] = -30, and column C runs over [0, 60] in even steps over the
             rows: out_0 = x[:, C] - 30 covers [-30, 30], exactly (one nonzero product per sum), so
             a comparison of the softplus derivative sees the derivative's arithmetic and not an
             error of out_0.  N = 1: out_0 = -12.  |d_sigma| lies in [4096, 8192) in the rows with
             out_0 < -7.5 and in [1, 2) in the others: the product d_sigma sigmoid(out_0) stays a
             normal fp16 number down to out_0 = -17 (4096 x 4.1e-8 = 1.7e-4 > 6.1e-5), and no
             fp16 weight gradient of the autocast evaluation overflows.
  padded     random, in rows of ldx = kx + 8 with NaN in the pad columns and NaN in 64 rows past
             N inside the same allocation (``alloc``): a read past the used columns or past N
             poisons a sum.
"""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

D_CODE = 39
NAMES_OUT = ("sigma", "dino")
NAMES_GRAD = ("dx", "W_in", "b_in", "W_out", "b_out")
ALL = NAMES_OUT + NAMES_GRAD
FAMILIES = ("random", "dead", "saturated", "padded")
BAND = (-17.0, -8.0)  # out_0 range of the per-element softplus-derivative check


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def make_inputs(N, C, d_code, D, dtype, family, seed):
    """dict: x (N, kx) 16-bit rows with the ones column last, alloc = the allocation the kernels
    get its first N rows of (x itself; the padded family: (N + 64, kx + 8) with NaN around x),
    W_in, b_in, W_out, b_out (f32), d_sigma (N), d_dino (N, D) (f32)."""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(seed)
    d_in = C + d_code
    kx = d_in + 1
    W_in = torch.randn(128, d_in, generator=g) * 0.08
    b_in = torch.randn(128, generator=g) * 0.1
    W_out = torch.randn(1 + D, 128, generator=g) * 0.1
    b_out = torch.randn(1 + D, generator=g) * 0.1
    x = torch.randn(N, kx, generator=g)
    d_sigma = torch.randn(N, generator=g)
    d_dino = torch.randn(N, D, generator=g)
    if family == "dead":
        b_in = -b_in.abs() - 0.05
        b_in[torch.randperm(128, generator=g)[:13]] = -50.0
        x[2::5, :d_in] = 0.0
    if family == "saturated":
        W_in[0] = 0.0
        W_in[0, C] = 1.0
        b_in[0] = 0.0
        W_out[0] = 0.0
        W_out[0, 0] = 1.0
        b_out[0] = -30.0
        x[:, C] = torch.linspace(0.0, 60.0, N) if N > 1 else torch.tensor([18.0])
        mag = torch.where(x[:, C] < 22.5, 4096.0, 1.0) * (1.0 + torch.rand(N, generator=g))
        d_sigma = torch.where(d_sigma < 0, -1.0, 1.0) * mag
    x[:, d_in] = 1.0
    x = x.to(dtype)
    alloc = x
    if family == "padded":
        alloc = torch.full((N + 64, kx + 8), float("nan"), dtype=dtype)
        alloc[:N, :kx] = x
    return dict(x=x, alloc=alloc, N=N, W_in=W_in, b_in=b_in, W_out=W_out, b_out=b_out,
                d_sigma=d_sigma, d_dino=d_dino, C=C, D=D, d_in=d_in, dtype=dtype)


def evaluate(x, W_in, b_in, W_out, b_out, d_sigma, d_dino, C, autocast=None):
    """All of ALL (+ out_0, and dy_sigma = the out_0 column of the output gradient) for rows x
    (N, d_in + 1; the last column is not read: the bias is b_in).  autocast None: float64
    throughout.  autocast = a 16-bit dtype: the parameters stay f32, the rows are rounded to the
    dtype and the two F.linear run under torch.autocast("cpu"), softplus in f32 -- the op
    sequence of bts.py:502-541 under the trainer's autocast."""
    d_in = W_in.shape[1]
    if autocast is None:
        cast = lambda t: t.detach().double().clone().requires_grad_(True)
        xl = cast(x)
        ps = [cast(t) for t in (W_in, b_in, W_out, b_out)]
        out = F.linear(torch.relu(F.linear(xl[:, :d_in], ps[0], ps[1])), ps[2], ps[3])
        out.retain_grad()
        sigma, dino = F.softplus(out[:, 0]), out[:, 1:]
    else:
        xl = x.detach().to(autocast).clone().requires_grad_(True)
        ps = [t.detach().float().clone().requires_grad_(True) for t in (W_in, b_in, W_out, b_out)]
        with torch.autocast("cpu", dtype=autocast):
            out = F.linear(torch.relu(F.linear(xl[:, :d_in], ps[0], ps[1])), ps[2], ps[3])
        out.retain_grad()
        sigma, dino = F.softplus(out[:, 0].float()), out[:, 1:].float()
    loss = (sigma * d_sigma.to(sigma.dtype)).sum() + (dino * d_dino.to(dino.dtype)).sum()
    loss.backward()
    r = {"sigma": sigma.detach(), "dino": dino.detach(), "dx": xl.grad[:, :C].clone(),
         "W_in": ps[0].grad, "b_in": ps[1].grad, "W_out": ps[2].grad, "b_out": ps[3].grad,
         "out_0": out[:, 0].detach(), "dy_sigma": out.grad[:, 0].clone()}
    return r


def yardsticks(ref, amp, names=ALL):
    return {n: rel_l2(amp[n], ref[n]) for n in names}


def degenerate(e):
    return not (math.isfinite(e) and 0.0 < e < 0.1)


@functools.lru_cache(maxsize=None)
def case(N, C, D, dtype, family, seed=0, d_code=D_CODE):
    """(inputs, float64 evaluation, autocast evaluation, yardsticks, dropped) of a case, once.
    dropped: {tensor: reason} for the tensors whose yardstick is degenerate."""
    d = make_inputs(N, C, d_code, D, dtype, family, 7919 * seed + 1000 * C + 10 * D + N)
    args = (d["x"], d["W_in"], d["b_in"], d["W_out"], d["b_out"], d["d_sigma"], d["d_dino"], C)
    ref = evaluate(*args)
    amp = evaluate(*args, autocast=dtype)
    ys = yardsticks(ref, amp)
    dropped = {n: f"autocast yardstick {e:.3g} is degenerate" for n, e in ys.items() if degenerate(e)}
    return d, ref, amp, ys, dropped


def band_rows(ref):
    o = ref["out_0"]
    return (o >= BAND[0]) & (o <= BAND[1])


def band_error(got, ref, dtype):
    """Worst per-element relative error of got (the out_0 column of the output gradient, any
    dtype) against the float64 d_sigma sigmoid(out_0) rounded to dtype, over the rows with out_0
    in BAND; None if the case has no such row."""
    m = band_rows(ref)
    if not bool(m.any()):
        return None
    want = ref["dy_sigma"][m].to(dtype).double()
    assert bool((want != 0).all())
    return float(((got[m].double().cpu() - want).abs() / want.abs()).max())


def sigma_abs_bound(d, ref):
    """Bound on |sigma - float64 sigma| per row for a 16-bit evaluation with f32 accumulation: 4
    standard deviations of the rounding-error model.  Each rounding to the dtype is an
    independent relative error of at most u (unit roundoff), of standard deviation at most
    u / sqrt(3).  Rounding W_in and b_in (the rows are 16-bit already) gives pre-activation k the
    variance (u^2 / 3) (sum_j (W_kj x_j)^2 + b_k^2); it reaches out_0 through the live units,
    times W_out[0, k]; rounding the hidden row and W_out[0] adds 2 (u^2 / 3) sum_k (h_k W_out[0, k])^2;
    softplus is 1-Lipschitz.  1e-6 (1 + |out_0|) covers the f32 sums and softplus.  (The worst
    case, every error at u with the same sign, is about sigma itself in bf16: no check.)"""
    u = 2.0 ** -11 if d["dtype"] == torch.float16 else 2.0 ** -8
    x = d["x"][:, :d["d_in"]].double()
    W, b, w0 = d["W_in"].double(), d["b_in"].double(), d["W_out"][0].double()
    h = torch.relu(F.linear(x, W, b))
    var_pre = (x ** 2) @ (W ** 2).t() + b ** 2
    var = (var_pre * (h > 0)) @ (w0 ** 2) + 2 * ((h * w0) ** 2).sum(1)
    return 4 * u / math.sqrt(3) * var.sqrt() + 1e-6 * (1 + ref["out_0"].abs())
