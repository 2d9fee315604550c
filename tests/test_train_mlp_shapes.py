"""The fused training MLP (csrc/sdhip_mlp.hip: sd_mlp_train_fwd / _bwd / sd_mlp_train_wgrad) at
every fragment geometry the router admits, and the router itself.

Shapes (C, D) with the 39-d code, kx = C + 40:
  (32, 8)    1 wxf tile, KS = 5;  U = 1 (out_0 shares the dino tile), KO = 1
  (64, 24)   2 wxf tiles, KS = 7; U = 1, KO = 2
  (64, 32)   U = 2 with out_0 alone in tile 1 at row 0, KO = 3
  (96, 40)   KS = 9, U = 2, KO = 3
  (256, 64)  the shipped head: KS = 19, U = 3, KO = 5, 8 wxf tiles
  (256, 56)  U = 2, KO = 4 under the shipped grid
N in {1, 33, 300}: one row, one tile plus one row, and more than 8 waves x 32 rows (a second
workgroup and a ragged last tile).  Both 16-bit dtypes.

Tolerance: the yardstick rule of tests/_train_mlp_oracle.py -- each native tensor
within 2 x the rel-L2 error of the CPU autocast evaluation against float64, same inputs.
Measured yardsticks over the cases here, each over the tensors its case keeps (min .. max; the
large dx / W_in / b_in figures are cases where a ReLU mask flips under 16-bit rounding):

              fp16                  bf16                  worst native / yardstick on MI355X
  sigma       8.3e-05 .. 2.7e-04    7.6e-04 .. 2.2e-03    1.02, 1.21
  dino        2.8e-04 .. 6.6e-04    2.3e-03 .. 4.3e-03    1.07, 1.14
  dx          4.3e-04 .. 3.1e-02    3.0e-03 .. 5.8e-02    1.08, 1.11
  W_in        3.2e-04 .. 3.3e-02    2.9e-03 .. 6.9e-02    1.00, 1.00
  b_in        3.1e-04 .. 3.2e-02    2.4e-03 .. 6.9e-02    1.02, 1.08
  W_out       2.8e-04 .. 4.5e-04    2.3e-03 .. 3.7e-03    0.92, 0.92
  b_out       1.7e-04 .. 4.1e-04    1.4e-03 .. 2.9e-03    1.01, 1.00

Dropped from a case's list (DROPS, one tensor per case at the most), each held to a bound of
its own instead:
  sigma of the saturated family.  out_0 is exact in both evaluations by construction, so the
    yardstick (7e-9 .. 3e-8) measures f32 rounding of softplus and no 16-bit rounding.  Held per
    element to 1e-6 relative (expf and log1pf within 2 ulp each, log1p's condition number at most
    1: 4 ulp = 5e-7; measured 8.7e-8), the rows above the threshold 20 included.
  sigma at N = 1.  One number: its yardstick is a single rounding error, which falls anywhere
    down to 0 (3e-6 .. 1.4e-3 here; the kernel's error, always below the unit roundoff, was
    0.5 x to 15 x that).  Held to oracle.sigma_abs_bound, 4 standard deviations of the rounding
    model of the two layers (measured at most 0.19 of it).

The softplus derivative (k_mlp_bwd, from the saved sigma): the out_0 column of dY per element
against float64 d_sigma sigmoid(out_0) rounded to the dtype, rows with out_0 in [-17, -8].  The
autocast evaluation's own worst relative error on that band, at N = 300 (45 rows in the band in
steps of 0.2; at N = 1 and 33 every out_0 in the band is a 16-bit number and its error is 0):
fp16 7.8e-03 / 8.1e-03 / 8.1e-03, bf16 6.1e-02 / 6.5e-02 / 6.8e-02 at (64, 24) / (64, 32) /
(256, 64) (out_0 rounded to 16 bits in [-17, -14)).  The kernel is held to 2 x the N = 300 figure
of its shape and dtype.  The former expression 1.f - expf(-sigma) cancels below out_0 = -12
(steps of 6e-8 on values of 6e-6 and less, 0 below -17.3) and missed that bound in both dtypes:
worst error 0.375 (fp16), 0.352 (bf16), at N = 33 and 300 of every shape.  -expm1f(-sigma) is
exact to f32 rounding: measured 0, every element equal to the rounded float64 value.

C ABI forward, scatter and determinism checks: the constants of tests/test_train_mlp.py and
tests/test_train.py::test_fused_mlp_scatter_gpu (1e-2; 1e-5; bit equality).
"""
from __future__ import annotations

import ctypes
import pytest
import torch
import torch.nn.functional as F

import _train_mlp_oracle as oracle
from _helpers import build_net, rel_l2
from scenedino_amd import _lib

F16, BF16 = torch.float16, torch.bfloat16
SHAPES = [(32, 8), (64, 24), (64, 32), (96, 40), (256, 64), (256, 56)]
SAT_SHAPES = [(64, 24), (64, 32), (256, 64)]
NS = [1, 33, 300]
DTS = [F16, BF16]
CASES = ([(N, C, D, dt, fam) for fam in ("random", "dead", "padded") for C, D in SHAPES
          for N in NS for dt in DTS] +
         [(N, C, D, dt, "saturated") for C, D in SAT_SHAPES for N in NS for dt in DTS])
# tensors left out of a case's yardstick list, with the reason (module docstring)
DROPS = {c: ("sigma", "out_0 is exact in both evaluations: the yardstick is f32 rounding of "
                      "softplus; checked per element to 1e-6 instead") if c[4] == "saturated" else
            ("sigma", "one element: its yardstick is a single rounding error, anywhere down to 0; "
                      "held to 4 standard deviations of the rounding model (oracle.sigma_abs_bound) instead")
         for c in CASES if c[4] == "saturated" or c[0] == 1}
KN = torch.tensor([[0.7849, 0.0, -0.0312], [0.0, 2.9391, 0.2701], [0.0, 0.0, 1.0]])


def _names(c):
    return [n for n in oracle.ALL if c not in DROPS or DROPS[c][0] != n]


def _id(c):
    N, C, D, dt, fam = c
    return f"{fam}-C{C}-D{D}-N{N}-{'f16' if dt == F16 else 'bf16'}"


# ------------------------------------------------------------------------ CPU: the yardsticks
@pytest.mark.parametrize("fam", oracle.FAMILIES)
def test_autocast_yardstick_is_not_vacuous(fam):
    """Every yardstick a case keeps is neither 0 nor 0.1 and more; a dropped one is degenerate
    for the reason given (below 1e-6: f32 rounding alone); at most one tensor per case is
    dropped, and nothing is dropped that DROPS does not name."""
    for c in (c for c in CASES if c[4] == fam):
        _, _, _, ys, deg = oracle.case(*c)
        names = _names(c)
        assert len(oracle.ALL) - len(names) <= 1
        for n in names:
            assert 0 < ys[n] < 0.1, (_id(c), n, ys[n])
        assert set(deg) <= set(oracle.ALL) - set(names), (_id(c), deg)
        if c[0] == 1 and fam != "saturated":  # the bound that stands in holds for the autocast reference
            d, ref, amp = oracle.case(*c)[:3]
            assert float((amp["sigma"].double() - ref["sigma"]).abs()) <= float(oracle.sigma_abs_bound(d, ref))
        for n in set(oracle.ALL) - set(names):  # dropped for the reason DROPS gives
            assert ys[n] < 1e-6 if fam == "saturated" else oracle.case(*c)[1][n].numel() == 1, \
                (_id(c), n, ys[n])


@pytest.mark.parametrize("dt", DTS)
def test_band_yardstick_is_not_vacuous(dt):
    """The autocast evaluation's worst relative error of d_sigma sigmoid(out_0) on the band, at
    N = 300: nonzero, and small enough that 2 x it still separates a cancelled derivative (tens
    of percent at out_0 = -17) from a rounded one."""
    for C, D in SAT_SHAPES:
        e = _band_yardstick(C, D, dt)
        assert 0 < e < 0.1, (C, D, e)
        for N in NS:  # every case has rows in the band
            assert bool(oracle.band_rows(oracle.case(N, C, D, dt, "saturated")[1]).any())


def _band_yardstick(C, D, dt):
    _, ref, amp, _, _ = oracle.case(300, C, D, dt, "saturated")
    return oracle.band_error(amp["dy_sigma"], ref, dt)


def test_dead_family_has_dead_units_and_dead_rows():
    d, ref, _, _, _ = oracle.case(33, 64, 24, BF16, "dead")
    h = torch.relu(F.linear(d["x"][:, :d["d_in"]].double(), d["W_in"].double(), d["b_in"].double()))
    assert int((h == 0).all(0).sum()) >= 13 and bool((h[2::5] == 0).all()) and bool((h[0] > 0).any())
    assert not ref["dx"][2::5].any() and bool(ref["dx"][0].any())


def test_saturated_family_covers_the_softplus_threshold():
    _, ref, _, _, _ = oracle.case(300, 64, 24, BF16, "saturated")
    o = ref["out_0"]
    assert float(o.min()) == -30 and float(o.max()) == 30 and int((o > 20).sum()) > 10
    assert bool((o[1:] >= o[:-1]).all()) and float((o[1:] - o[:-1]).max()) < 0.51  # (16-bit rows)


# ------------------------------------------------------------------------ CPU: the router
def _fwd_args(C, kx, ldx, D, N, **kw):
    a = dict(x=16, N=N, ldx=ldx, kx=kx, dtype=_lib.SD_BF16, D=D, C=C, w1f=16, w2f=16, b_out=16,
             h=16, sigma=16, dino=16, d_sigma=16, d_dino=16, wtf=16, wxf=16, dy=16, dh=16, dx=16,
             lddx=C, dx_dtype=_lib.SD_F32)
    a.update(kw)
    return _lib.SdMlpTrainArgs(**a)


def _wgrad_refuses(kx, ldx, D):
    """sd_mlp_train_wgrad on arguments it must refuse (-1 before any HIP call)."""
    g = _lib.SdMlpWgradArgs(x=16, dh=16, dy=16, h=16, N=0, ldx=ldx, kx=kx, D=D, dtype=_lib.SD_BF16,
                            nparts=1, work=16, dw_in=16, db_in=16, dw_out=16, db_out=16)
    lib = _lib.load()
    return (lib.sd_mlp_train_wgrad(ctypes.byref(g), None) == -1
            and b"sd_mlp_train_wgrad: invalid" in lib.sd_last_error())


# (C, kx, ldx, D): on and just past each bound of ml_check and sd_mlp_train_wgrad
SHAPE_TABLE = ([(C, C + 40, C + 40, D) for D in (0, 3, 8, 64, 65, 72) for C in (32, 256, 288)] +
               [(32, 72, 80, 8), (32, 72, 71, 8), (32, 72, 76, 8),  # ldx >= kx in multiples of 8
                (32, 73, 80, 8), (32, 101, 104, 8),                # kx % 8 (wgrad alone)
                (256, 296, 320, 64), (256, 296, 328, 64),          # ldx <= 320 (wgrad alone)
                (256, 320, 320, 64), (288, 320, 320, 64),          # kx = 320 is in (C 288: a 31-d code)
                (64, 64, 64, 8), (64, 48, 48, 8),                  # C <= kx
                (16, 56, 56, 8), (0, 40, 40, 8), (32, 8, 8, 8)])   # C % 32, C > 0, kx > 8 (wgrad)


def test_shape_predicate_states_the_library_bounds():
    """fused_train_shape_ok (what BTSNet._fused_train_mlp and PackedTrainMLP ask) agrees with
    what sd_mlp_train_fwd, _bwd and sd_mlp_train_wgrad accept, row by row.  The library is
    asked at N = 0 (a valid sd_mlp_train_fwd / _bwd call returns before any launch) or on
    arguments it must refuse; validation runs before any HIP call, so this needs no device and
    leaves no HIP error behind.  Rows that would launch or fill memory assert the predicate
    alone."""
    from scenedino_amd.mlp_pack import fused_train_shape_ok
    lib = _lib.load()
    n_ok = 0
    for C, kx, ldx, D in SHAPE_TABLE:
        rf = lib.sd_mlp_train_fwd(ctypes.byref(_fwd_args(C, kx, ldx, D, 0)), None)
        if rf == -1:
            assert b"sd_mlp_train_fwd: invalid" in lib.sd_last_error()
        rb = lib.sd_mlp_train_bwd(ctypes.byref(_fwd_args(C, kx, ldx, D, 0)), None)
        assert rf in (0, -1) and rb == rf, (C, kx, ldx, D, rf, rb)
        # sd_mlp_train_wgrad zero-fills its outputs at N = 0, so it is asked only where its own
        # bounds (read off its argument check) say it refuses before that
        w_ok = 8 < kx <= 320 and kx % 8 == 0 and kx <= ldx <= 320 and ldx % 8 == 0 and 0 < D <= 64 and D % 8 == 0
        assert w_ok or _wgrad_refuses(kx, ldx, D), (kx, ldx, D)
        lib_ok = rf == 0 and w_ok
        assert fused_train_shape_ok(128, kx - 1, D, C, 0, ldx) == lib_ok, (C, kx, ldx, D, rf, w_ok)
        n_ok += lib_ok
    assert n_ok == 9  # (32 | 256) x (8 | 64); ldx 80; ldx 320; kx 320 at C 256 and 288; C = kx = 64
    # anchors: what the issue names
    ok = lambda D, C, n=0: fused_train_shape_ok(128, C + 39, D, C, n, C + 40)
    assert ok(64, 256) and ok(8, 32) and not ok(0, 256) and not ok(3, 256) and not ok(72, 256)
    assert not ok(64, 288) and not fused_train_shape_ok(64, 295, 64, 256, 0, 296)
    # the 4 GiB bound on the rows: 2^32 - 16 bytes is in, 2^32 is out (refused before any launch)
    assert 17895697 * 120 * 2 == 2 ** 32 - 16 and 2 ** 24 * 128 * 2 == 2 ** 32
    assert fused_train_shape_ok(128, 71, 8, 32, 17895697, 120)
    assert not fused_train_shape_ok(128, 71, 8, 32, 2 ** 24, 128)
    for fn in (lib.sd_mlp_train_fwd, lib.sd_mlp_train_bwd):
        assert fn(ctypes.byref(_fwd_args(32, 72, 128, 8, 2 ** 24)), None) == -1
        assert fn(ctypes.byref(_fwd_args(32, 72, 128, 8, -1)), None) == -1
        assert fn(None, None) == -1
    assert not fused_train_shape_ok(128, 71, 8, 32, -1, 128)
    # the shipped step (2 x 262144 points of 296 columns) is far inside
    assert fused_train_shape_ok(128, 295, 64, 256, 2 * 262144, 296)
    # null pointers are refused at N = 0 as well
    for kw in (dict(x=None), dict(w1f=None), dict(sigma=None)):
        assert lib.sd_mlp_train_fwd(ctypes.byref(_fwd_args(32, 72, 72, 8, 0, **kw)), None) == -1
    for kw in (dict(wtf=None), dict(dy=None), dict(d_dino=None), dict(lddx=16)):
        assert lib.sd_mlp_train_bwd(ctypes.byref(_fwd_args(32, 72, 72, 8, 0, **kw)), None) == -1


def test_packed_train_mlp_refuses_what_the_kernels_refuse():
    from scenedino_amd.mlp_pack import PackedTrainMLP
    w = lambda d_in, D: (torch.zeros(128, d_in), torch.zeros(128), torch.zeros(1 + D, 128),
                         torch.zeros(1 + D))
    PackedTrainMLP(*w(71, 8), _lib.SD_BF16, 32)
    PackedTrainMLP(*w(71, 8), _lib.SD_BF16, 32, 300, 80)
    for d_in, D, C, n, ldx in ((71, 3, 32, 0, None), (71, 0, 32, 0, None), (327, 64, 288, 0, None),
                               (71, 8, 32, 2 ** 24, 128), (71, 8, 32, 10, 76)):
        with pytest.raises(NotImplementedError, match="fused training MLP"):
            PackedTrainMLP(*w(d_in, D), _lib.SD_BF16, C, n, ldx)


class _Head(torch.nn.Module):
    def __init__(self, d_in, d_out, d_hidden=128):
        super().__init__()
        self.lin_in, self.lin_out = torch.nn.Linear(d_in, d_hidden), torch.nn.Linear(d_hidden, d_out)
        self.activation, self.n_blocks, self.d_latent = torch.nn.ReLU(), 0, 0


_Head.__name__ = "ResnetFC"


def test_router_asks_the_predicate(monkeypatch):
    """BTSNet._fused_train_mlp on the CPU (autocast state faked): the shipped head is fused, a
    density-only head, a 4-output head, a 288-channel grid and a step of 4 GiB of rows are not."""
    from scenedino_amd.models import bts
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: BF16)

    class Net:
        code_xyz = type("Code", (), {"d_out": 39})()
    route = lambda d_out, C, n: bts.BTSNet._fused_train_mlp(Net(), _Head(C + 39, d_out), C, n)
    assert route(65, 256, 2 * 262144) and route(9, 32, 1) and route(65, 256, 0)
    assert not route(1, 256, 100) and not route(4, 256, 100) and not route(65, 288, 100)
    assert not route(66, 256, 100) and not route(65, 256, 2 ** 32 // 592 + 1)
    assert route(65, 256, 2 ** 32 // 592)


# ------------------------------------------------------------------------ GPU helpers
def _native(d, dev="cuda"):
    """FieldMLPFused forward + backward on a case's inputs.  Returns the tensors of oracle.ALL,
    the full dx rows and the dY rows the backward handed to sd_mlp_train_wgrad."""
    from scenedino_amd import autograd as ag
    N, C = d["N"], d["C"]
    xr = d["alloc"].to(dev)[:N].requires_grad_(True)  # (the NaN rows stay behind it)
    ps = [d[k].to(dev).requires_grad_(True) for k in ("W_in", "b_in", "W_out", "b_out")]
    seen = {}
    real = _lib.mlp_train_wgrad

    def spy(x, dh, dy, h, kx, D, nparts=None):
        seen["dy"], seen["dh"], seen["h"] = dy, dh, h
        return real(x, dh, dy, h, kx, D, nparts=nparts)

    _lib.mlp_train_wgrad = spy
    try:
        sigma, dino = ag.FieldMLPFused.apply(xr, *ps, C)
        ((sigma * d["d_sigma"].to(dev)).sum() + (dino * d["d_dino"].to(dev)).sum()).backward()
    finally:
        _lib.mlp_train_wgrad = real
    torch.cuda.synchronize()
    r = {"sigma": sigma.detach(), "dino": dino.detach(), "dx": xr.grad[:, :C].float(),
         "W_in": ps[0].grad, "b_in": ps[1].grad, "W_out": ps[2].grad, "b_out": ps[3].grad}
    return r, xr.grad, seen


def _check(native, ref, ys, names, what):
    for n in names:
        print(f"{what} {n}: native rel-L2 {rel_l2(native[n], ref[n]):.3g}, yardstick {ys[n]:.3g}")
    for n in oracle.ALL:
        t = native[n].float().cpu()
        assert t.shape == ref[n].shape and bool(torch.isfinite(t).all()), (what, n)
    for n in names:
        r = rel_l2(native[n], ref[n])
        assert r <= 2 * ys[n], f"{what} {n}: rel-L2 {r:.3g} > 2 x {ys[n]:.3g}"


# ------------------------------------------------------------------------ GPU: a, b
@pytest.mark.gpu
@pytest.mark.parametrize("c", [c for c in CASES if c[4] != "saturated"], ids=_id)
def test_fused_mlp_against_the_yardstick(c):
    d, ref, _, ys, _ = oracle.case(*c)
    native, dx_full, seen = _native(d)
    _check(native, ref, ys, _names(c), _id(c))
    C, D = c[1], c[2]
    assert dx_full.shape == d["alloc"][:c[0]].shape and not dx_full[:, C:].any()
    assert bool((seen["h"][:, 128] == 1).all()) and not seen["h"][:, 129:].any()
    if c[0] == 1:  # sigma's yardstick is dropped at one row (DROPS): the rounding model's bound
        e, b = float((native["sigma"].double().cpu() - ref["sigma"]).abs()), float(oracle.sigma_abs_bound(d, ref))
        print(f"{_id(c)} sigma: |error| {e:.3g}, rounding bound {b:.3g}")
        assert e <= b
    if c[4] == "dead":  # rows with every unit off: exact zeros, not small numbers
        assert not seen["h"][2::5, :128].any() and not seen["dh"][2::5].any()
        assert not native["dx"][2::5].any()


@pytest.mark.gpu
@pytest.mark.parametrize("c", [c for c in CASES if c[4] == "saturated"], ids=_id)
def test_saturated_softplus_and_its_derivative(c):
    N, C, D, dt, _ = c
    d, ref, _, ys, _ = oracle.case(*c)
    native, _, seen = _native(d)
    _check(native, ref, ys, _names(c), _id(c))
    # sigma per element (its yardstick is dropped: see DROPS), the rows above the threshold too
    sg, want = native["sigma"].double().cpu(), ref["sigma"]
    e_sigma = float(((sg - want).abs() / want).max())
    print(f"{_id(c)} sigma: worst relative error {e_sigma:.3g}")
    assert e_sigma <= 1e-6
    # the out_0 column of dY on the band
    e = oracle.band_error(seen["dy"][:, D].float(), ref, dt)
    bound = 2 * _band_yardstick(C, D, dt)
    print(f"{_id(c)} dY[:, D] on out_0 in [-17, -8]: worst relative error {e:.3g}, "
          f"autocast reference {bound / 2:.3g}")
    assert e <= bound, f"{_id(c)}: {e:.3g} > 2 x {bound / 2:.3g}"


# ------------------------------------------------------------------------ GPU: c
def _pack_fwd(W_in, b_in, W_out, dt, C, dev):
    """w1f, w2f through the cached fragment index (PackedTrainMLP admits only shapes the whole
    step runs; the forward alone also takes kx % 8 != 0)."""
    from scenedino_amd import mlp_pack
    d_in, D = W_in.shape[1], W_out.shape[0] - 1
    idx, sizes, _ = mlp_pack._train_index(d_in, D, C, dev)
    src = torch.cat((torch.cat((W_in, b_in[:, None]), 1).reshape(-1), W_out[1:].reshape(-1),
                     W_out[:1].reshape(-1), torch.zeros(1))).to(dev)
    w1f, w2f, _, _ = torch.split(src[idx].to(dt), sizes)
    return w1f.contiguous(), w2f.contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("kx,C,D", [(72, 32, 8), (80, 64, 40), (101, 96, 56), (295, 256, 64)])
@pytest.mark.parametrize("dt", DTS)
def test_c_abi_forward_partial_k_steps(kx, C, D, dt):
    """sd_mlp_train_fwd's last k-step: kx = 72 (the upper half-wave's piece is read from past
    the buffer), 80 (no partial step), 101 and 295 (kx % 8 != 0: the masked piece).  NaN in
    columns kx .. ldx - 1 and in 64 rows past N.  Against a float64 matmul of the same 16-bit
    rows: rel-L2 <= 1e-2 (tests/test_train_mlp.py), no NaN anywhere."""
    dev, N = "cuda", 300
    ldx = (kx + 7) // 8 * 8 + 8
    g = torch.Generator().manual_seed(kx)
    W_in, b_in = torch.randn(128, kx - 1, generator=g) * 0.08, torch.randn(128, generator=g) * 0.1
    W_out, b_out = torch.randn(1 + D, 128, generator=g) * 0.1, torch.randn(1 + D, generator=g) * 0.1
    buf = torch.full((N + 64, ldx), float("nan"), dtype=dt)
    buf[:N, :kx] = torch.randn(N, kx, generator=g).to(dt)
    buf[:N, kx - 1] = 1
    x = buf.to(dev)[:N]
    w1f, w2f = _pack_fwd(W_in, b_in, W_out, dt, C, dev)
    bo = b_out.to(dev)
    h = torch.full((N + 1, 136), float("nan"), device=dev, dtype=dt)
    sigma, dino = torch.full((N + 1,), float("nan"), device=dev), torch.full((N + 1, D), float("nan"), device=dev)
    a = _lib.SdMlpTrainArgs(x=x.data_ptr(), N=N, ldx=ldx, kx=kx, dtype=_lib.SD_OF_TORCH[dt], D=D, C=C,
                            w1f=w1f.data_ptr(), w2f=w2f.data_ptr(), b_out=bo.data_ptr(),
                            h=h.data_ptr(), sigma=sigma.data_ptr(), dino=dino.data_ptr())
    _lib.mlp_train_fwd(a, x)
    torch.cuda.synchronize()
    X = buf[:N, :kx].double()
    H = torch.relu(X[:, :kx - 1] @ W_in.double().t() + b_in.double())
    out = H @ W_out.double().t() + b_out.double()
    for got, want, n in ((h[:N, :128], H, "h"), (sigma[:N], F.softplus(out[:, 0]), "sigma"),
                         (dino[:N], out[:, 1:], "dino")):
        assert bool(torch.isfinite(got).all()), n
        print(f"kx {kx} {n}: rel-L2 {rel_l2(got, want):.3g}")
        assert rel_l2(got, want) <= 1e-2, n
    assert bool((h[:N, 128] == 1).all()) and not h[:N, 129:].any()
    # the row past N of every output is untouched
    assert bool(h[N].isnan().all()) and bool(sigma[N].isnan()) and bool(dino[N].isnan().all())


# ------------------------------------------------------------------------ GPU: d
@pytest.mark.gpu
@pytest.mark.parametrize("C,D", [(32, 8), (64, 24)])
@pytest.mark.parametrize("dt", DTS)
def test_fused_scatter_small_grids(C, D, dt, monkeypatch):
    """ml_scatter with 1 and 2 wxf tiles (tests/test_train.py::test_fused_mlp_scatter_gpu runs 8):
    the grid gradient of the fused scatter against the dX rows + sd_field_gather_bwd of the same
    call, rel-L2 <= 1e-5 (f32 atomic order only); parameter gradients identical.  B = 2 frames of
    a 5 x 7 grid, P = 9 rays x 32 samples + 17 points: tiles straddle the frame boundary, the
    last one is ragged, and most points of a tile share texels."""
    from scenedino_amd import autograd as ag
    g = torch.Generator().manual_seed(100 + C)
    B, R, K, Hf, Wf = 2, 9, 32, 5, 7
    P = R * K + 17
    dev = "cuda"
    pix = torch.rand(B, R, 2, generator=g) * 2 - 1
    z = torch.sort(3 + 60 * torch.rand(B, R, K, generator=g), -1)[0]
    dirs = torch.cat((pix, torch.ones(B, R, 1)), -1) @ torch.inverse(KN).T
    xyz = (dirs.unsqueeze(2) * z.unsqueeze(-1)).reshape(B, R * K, 3)
    xyz[1] += torch.tensor([0.8, 0.0, 0.0]) * (1 - z[1].reshape(R * K, 1) / 63)  # samples cross texels
    xyz = torch.cat((xyz, torch.rand(B, 17, 3, generator=g) * 10 + 3), 1).contiguous().to(dev)
    cam_f = _lib.cam_records(torch.eye(4).expand(B, 4, 4).contiguous().to(dev),
                             KN.expand(B, 3, 3).contiguous().to(dev))
    grid = torch.randn(B, Hf, Wf, C, generator=g).to(dev)
    ps = [(torch.randn(s, generator=g) * 0.08).to(dev).requires_grad_(True)
          for s in ((128, C + 39), (128,), (1 + D, 128), (1 + D,))]
    gs, gd = torch.randn(B, P, generator=g).to(dev), torch.randn(B, P, D, generator=g).to(dev)

    def run(fused):
        monkeypatch.setattr(ag, "FUSED_SCATTER", fused)
        monkeypatch.setattr(ag, "DX16", True)
        gn = grid.clone().requires_grad_(True)
        for p in ps:
            p.grad = None
        with torch.autocast("cuda", dtype=dt):
            sigma, dino, *_ = ag.FieldGatherMLP.apply(gn, xyz, cam_f, None, None, False, None, None, *ps)
        ((sigma * gs).sum() + (dino * gd).sum()).backward()
        return gn.grad.clone(), [p.grad.clone() for p in ps]

    g_ref, p_ref = run(False)
    g_fus, p_fus = run(True)
    assert float(g_ref.abs().sum()) > 0 and bool(torch.isfinite(g_fus).all())
    print(f"C {C}: fused scatter vs rows + gather_bwd rel-L2 {rel_l2(g_fus, g_ref):.3g}")
    assert rel_l2(g_fus, g_ref) <= 1e-5
    for a, b in zip(p_fus, p_ref):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------ GPU: e
@pytest.mark.gpu
def test_two_launches_give_the_same_bits():
    d = oracle.case(300, 64, 24, BF16, "random")[0]
    a, dxa, sa = _native(d)
    b, dxb, sb = _native(d)
    for n in oracle.ALL:
        assert torch.equal(a[n], b[n]), n
    assert torch.equal(dxa, dxb)
    for n, w in (("dy", d["D"] + 1), ("dh", 128), ("h", 136)):  # (dY is written to column D)
        assert torch.equal(sa[n][:, :w].view(torch.int16), sb[n][:, :w].view(torch.int16)), n
    w1 = _lib.mlp_train_wgrad(d["alloc"].cuda(), sa["dh"], sa["dy"], sa["h"], d["d_in"] + 1, d["D"])
    w2 = _lib.mlp_train_wgrad(d["alloc"].cuda(), sa["dh"], sa["dy"], sa["h"], d["d_in"] + 1, d["D"], nparts=3)
    w3 = _lib.mlp_train_wgrad(d["alloc"].cuda(), sa["dh"], sa["dy"], sa["h"], d["d_in"] + 1, d["D"], nparts=3)
    for t, u, v, n in zip(w1, w2, w3, ("W_in", "b_in", "W_out", "b_out")):
        assert torch.equal(t, a[n]) and torch.equal(u, v), n


# ------------------------------------------------------------------------ GPU: routing
def _route_case(d_out, seed=5):
    g = torch.Generator().manual_seed(seed)
    B, C, Hf, Wf, H, W = 2, 64, 5, 7, 10, 14
    grid = torch.randn(B, C, Hf, Wf, generator=g)
    ws = (torch.randn(128, C + 39, generator=g) * 0.08, torch.randn(128, generator=g) * 0.1,
          torch.randn(d_out, 128, generator=g) * 0.1, torch.randn(d_out, generator=g) * 0.1)
    images = torch.rand(B, 1, 3, H, W, generator=g) * 2 - 1
    P = 150
    z = 3 + 40 * torch.rand(B, P, 1, generator=g)
    pix = torch.rand(B, P, 2, generator=g) * 1.8 - 0.9
    xyz = (torch.cat((pix, torch.ones(B, P, 1)), -1) @ torch.inverse(KN).T) * z
    gs = torch.randn(B, P, generator=g)
    gd = torch.randn(B, P, d_out - 1, generator=g)
    return grid, ws, images, xyz.contiguous(), gs, gd


class _Names:
    def __init__(self):
        self.names = []

    def start(self, n):
        self.names.append(n)

    def stop(self, n):
        pass


def _query_step(case, amp, monkeypatch):
    """One _query_diff forward + backward; (launch names, grid gradient NHWC, head gradients,
    the f32 gather rows)."""
    from scenedino_amd import autograd as ag
    grid, ws, images, xyz, gs, gd = case
    dev = "cuda"
    B = grid.shape[0]
    net = build_net(grid, *ws, "fp32", dev)
    pose = torch.eye(4).view(1, 1, 4, 4).expand(B, 1, 4, 4).contiguous()
    net.encode(images.to(dev), KN.view(1, 1, 3, 3).expand(B, 1, 3, 3).contiguous().to(dev),
               pose.to(dev), ids_encoder=[0], ids_render=[0])
    leaf = net.grid_f_features[0].detach().clone().requires_grad_(True)
    net.grid_f_features[0] = leaf
    net.train()
    rec = _Names()
    monkeypatch.setattr(ag, "kernel_timer", rec)
    with torch.autocast("cuda", dtype=amp or BF16, enabled=amp is not None):
        sigma, dino, *_ = net._query_diff(xyz.to(dev))
    ((sigma.float() * gs.to(dev)).sum() + (dino.float() * gd.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    head = net.heads["normal_head"]
    grads = [p.grad.detach().clone() for p in (head.lin_in.weight, head.lin_in.bias,
                                               head.lin_out.weight, head.lin_out.bias)]
    return rec.names, leaf.grad.detach().reshape(grid.shape).clone(), grads, net


@pytest.mark.gpu
@pytest.mark.parametrize("d_out", [4, 1, 65])
def test_query_diff_routes_by_shape(d_out, monkeypatch):
    """BTSNet._query_diff under bf16 autocast on a 2 x 64 x 5 x 7 grid: a 4-output and a
    density-only head complete on FieldGather + FieldMLP (the kernels refuse D = 3 and D = 0;
    the router used to hand them over and the step raised), the 65-output head still runs
    FieldGatherMLP.  Gradients of the grid and the head against the fp32 autograd path, within
    2 x the error of the CPU bf16-autocast MLP against float64 on the same gather rows (the
    grid's yardstick: both dX through the same sd_field_gather_bwd)."""
    case = _route_case(d_out)
    grid, ws, _, xyz, gs, gd = case
    names16, g16, p16, net = _query_step(case, BF16, monkeypatch)
    names32, g32, p32, _ = _query_step(case, None, monkeypatch)
    if d_out == 65:
        assert "mlp" in names16 and "mlp_bwd" in names16 and "gather_bwd" not in names16
    else:
        assert "mlp" not in names16 and "mlp_bwd" not in names16
        assert "gather" in names16 and "gather_bwd" in names16
    assert "mlp" not in names32 and "gather_bwd" in names32
    # yardsticks on the f32 rows of the same gather
    B, C, Hf, Wf = grid.shape
    dev = "cuda"
    cam_f = net._frame(net._grids())["cam_f"]
    gn = grid.permute(0, 2, 3, 1).contiguous().to(dev)
    x32 = _lib.field_gather(xyz.to(dev), gn, cam_f, None, None, False)[0].reshape(-1, C + 40).cpu()
    args = (x32, *ws, gs.reshape(-1), gd.reshape(gs.numel(), d_out - 1), C)
    ref, amp = oracle.evaluate(*args), oracle.evaluate(*args, autocast=BF16)
    scat = lambda dx: _lib.field_gather_bwd(xyz.to(dev), dx.float().reshape(B, -1, C).to(dev),
                                            cam_f, Hf, Wf, C).permute(0, 3, 1, 2)
    ys = {"grid": rel_l2(scat(amp["dx"]), scat(ref["dx"]))}
    ys.update({n: rel_l2(amp[n], ref[n]) for n in ("W_in", "b_in", "W_out", "b_out")})
    assert rel_l2(g32, scat(ref["dx"])) < 1e-4  # the fp32 path is the float64 formula
    got = dict(zip(("W_in", "b_in", "W_out", "b_out"), p16), grid=g16)
    want = dict(zip(("W_in", "b_in", "W_out", "b_out"), p32), grid=g32)
    for n, e in ys.items():
        r = rel_l2(got[n], want[n])
        print(f"d_out {d_out} {n}: native rel-L2 {r:.3g}, yardstick {e:.3g}")
    for n, e in ys.items():
        assert 0 < e < 0.1 and bool(torch.isfinite(got[n]).all()), (n, e)
        assert rel_l2(got[n], want[n]) <= 2 * e, (n, rel_l2(got[n], want[n]), e)
