"""sd_linear_probe (csrc/sdhip_linear_probe.hip) on the GPU: logits' argmax, per-row and summed
cross-entropy, the gradients of W and b, and LinearHead / SemanticHead on top of it, against
tests/_linear_probe_oracle.py's restated reference formula on the CPU.

Every shape runs with x in f32 and bf16, the Dropout2d scale on and off (48 rows per group, which
does not divide the 32-row tile) and ``normalize`` on and off; about 20 % of the targets are -1.
Two input families, no row left out of any check:
  (a) clustered rows x = (W^_cls + 0.3 randn / sqrt(d)) U(0.01, 3), W rows of norm 4..8.  The test
      asserts its own precondition (the smallest fp32 top-2 logit margin exceeds 4 x the largest
      absolute logit error of the CPU bf16 evaluation), then every pred must equal the fp32
      argmax.  With ``normalize`` off the kernel gets these rows already normalised, as the stego
      probe's caller hands them over: on the raw rows the U(0.01, 3) scale shrinks the margin of
      the smallest row a hundredfold while the error follows the largest row, and the
      precondition cannot hold (measured: margins 0.0003..0.1 against errors 0.03..0.08).  Raw
      rows with ``normalize`` off are family (b)'s.  Seed offsets: _linear_probe_oracle.inputs.
  (b) unstructured randn rows, where many margins are small: every pred must be near-optimal,
      z32[i, pred_i] >= max_k z32[i, k] - tol, tol = 2 x the largest absolute logit error of the
      CPU bf16 evaluation, measured here and asserted > 0.
Row losses are within the same tol of the fp32 ones (cross-entropy is 2-Lipschitz in the largest
logit error and tol carries the factor 2) and exactly 0 on ignored rows; loss_sum is the sum of
the row losses to fp32 summation error; n_valid is exact.  The mean loss is not held to the
autocast yardstick: its row errors cancel to fp32 rounding level, which is no yardstick.
gW / n_valid and gb / n_valid follow tests/_stego_oracle.py's yardstick (2 x the bf16-autocast
error of CPU autograd of the same formula).  With one class softmax is exactly 1 and both
gradients are exactly 0 in any precision: there the test asserts exact zeros instead (the
yardstick would be 0 / 0).
"""
from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

import _linear_probe_oracle as lo
import _stego_oracle as so

SHAPES = [(N, d, C) for N in (1, 33, 65, 1000, 4100) for d in (64, 384, 768) for C in (19, 32)] \
    + [(16417, 64, 19), (100, 64, 1)] \
    + [(1000, 128, 19), (1000, 256, 32)]  # the kernel's other column splits (d <= 128, d <= 256)
VARIANTS = [(dt, mk, nz) for dt in (torch.float32, torch.bfloat16) for mk in (False, True)
            for nz in (True, False)]
RPG = lo.RPG


@functools.lru_cache(maxsize=None)
def _oracle(family, N, d, C, dtype, mask, normalize):
    """x as the kernel reads it, W, b, m, target, fp32 logits, bf16-evaluation logits."""
    W, b, x, m, target = lo.inputs(family, N, d, C)
    if family == "a" and not normalize:
        x = F.normalize(x, dim=-1, eps=1e-10)
    x = x.to(dtype)
    m = m if mask else None
    xh = lo.xhat(x, m, RPG, normalize)
    return x, W, b, m, target, lo.logits(xh, W, b), lo.logits_bf16(xh, W, b)


_RUNS = {}


def _run(key, dev):
    """Two launches with every output: (pred, loss_sum, n_valid, gW, gb, row_loss) twice."""
    if key not in _RUNS:
        from scenedino_amd import _lib
        x, W, b, m, target = _oracle(*key)[:5]
        args = (x.to(dev), W.to(dev), b.to(dev), target.to(dev), None if m is None else m.to(dev), RPG,
                key[6])
        _RUNS[key] = tuple(_lib.linear_probe(*args, want_grad=True, want_row_loss=True)
                           for _ in range(2))
    return _RUNS[key]


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


def _keys(family, N, d, C):
    return [(family, N, d, C, dt, mk, nz) for dt, mk, nz in VARIANTS]


@pytest.mark.gpu
@pytest.mark.parametrize("N,d,C", SHAPES)
def test_clustered_rows_get_the_fp32_argmax(gpu, N, d, C):
    for key in _keys("a", N, d, C):
        z32, z16 = _oracle(*key)[5:7]
        err = float((z16 - z32).abs().max())
        if C > 1:
            top = z32.topk(2, dim=1).values
            margin = float((top[:, 0] - top[:, 1]).min())
        else:
            margin = float("inf")
        print(f"{key}: smallest fp32 top-2 margin {margin:.4f}, largest bf16 logit error {err:.4f}")
        assert err > 0 and margin > 4 * err
        pred = _run(key, gpu)[0][0]
        assert pred.dtype == torch.int32 and pred.shape == (N,)
        assert torch.equal(pred.cpu().long(), z32.argmax(dim=1))


@pytest.mark.gpu
@pytest.mark.parametrize("N,d,C", SHAPES)
def test_unstructured_rows_get_near_optimal_preds(gpu, N, d, C):
    for key in _keys("b", N, d, C):
        z32, z16 = _oracle(*key)[5:7]
        tol = 2 * float((z16 - z32).abs().max())
        pred = _run(key, gpu)[0][0].cpu().long()
        assert int(pred.min()) >= 0 and int(pred.max()) < C
        gap = z32.max(dim=1).values - z32.gather(1, pred[:, None]).squeeze(1)
        print(f"{key}: tol {tol:.5f}, largest gap {float(gap.max()):.6f}, "
              f"{int((pred != z32.argmax(dim=1)).sum())} preds differ from the fp32 argmax")
        assert tol > 0 and float(gap.max()) <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("N,d,C", SHAPES)
def test_row_losses_their_sum_and_the_valid_count(gpu, N, d, C):
    for family in ("a", "b"):
        for key in _keys(family, N, d, C):
            target, z32, z16 = _oracle(*key)[4:7]
            tol = 2 * float((z16 - z32).abs().max())
            _, loss_sum, n_valid, _, _, row_loss = _run(key, gpu)[0]
            rl, l32 = row_loss.cpu(), lo.row_loss(z32, target)
            valid = target >= 0
            worst = float((rl - l32).abs().max())
            print(f"{key}: tol {tol:.5f}, largest row-loss error {worst:.6f}, "
                  f"loss_sum {float(loss_sum):.6f}, sum of rows {float(rl.double().sum()):.6f}")
            assert tol > 0 and bool(torch.isfinite(rl).all()) and worst <= tol
            assert bool((rl[~valid] == 0).all())
            assert n_valid.dtype == torch.int32 and int(n_valid) == int(valid.sum())
            torch.testing.assert_close(loss_sum.cpu().double(), rl.double().sum().view(1),
                                       rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("N,d,C", SHAPES)
def test_gradients_against_cpu_autograd(gpu, N, d, C):
    for family in ("a", "b"):
        for key in _keys(family, N, d, C):
            x, W, b, m, target = _oracle(*key)[:5]
            _, _, n_valid, gW, gb, _ = _run(key, gpu)[0]
            nv = float(n_valid)
            native = {"gW": gW.cpu() / nv, "gb": gb.cpu() / nv}
            if C == 1:  # softmax over one class is exactly 1: g = 1 - 1
                assert not bool(native["gW"].any()) and not bool(native["gb"].any())
                continue
            f32 = lo.probe_eval(x, W, b, target, m, RPG, key[6], autocast=False)
            f16 = lo.probe_eval(x, W, b, target, m, RPG, key[6], autocast=True)
            so.check(native, f32, f16, ("gW", "gb"), what=str(key))


@pytest.mark.gpu
@pytest.mark.parametrize("N,d,C", SHAPES)
def test_two_launches_give_the_same_bits(gpu, N, d, C):
    for family in ("a", "b"):
        for key in _keys(family, N, d, C):
            first, second = _run(key, gpu)
            for a, b in zip(first, second):
                assert torch.equal(a, b)


@pytest.mark.gpu
def test_edge_cases(gpu):
    from scenedino_amd import _lib
    from scenedino_amd.downstream_head.semantic_head import LinearHead
    W, b, x, m, target = lo.inputs("b", 65, 64, 19)
    dev = lambda t: t.to(gpu)  # noqa: E731

    # all targets -1: nothing valid, exact zeros, and the Python loss is NaN with zero gradients
    none = torch.full((65,), -1)
    pred, loss_sum, n_valid, gW, gb, rl = _lib.linear_probe(dev(x), dev(W), dev(b), dev(none), dev(m), RPG,
                                                            True, want_grad=True, want_row_loss=True)
    assert int(n_valid) == 0 and float(loss_sum) == 0.0
    assert not bool(gW.any()) and not bool(gb.any()) and not bool(rl.any())
    head = LinearHead(64, 19).to(gpu)
    res = head(dev(x).view(1, 1, 65, 64), dev(none).view(1, 65))
    assert bool(torch.isnan(res["loss"]))
    res["loss"].backward()
    assert not bool(head.linear.weight.grad.any()) and not bool(head.linear.bias.grad.any())

    # a zero row with normalize: z = b, everything finite
    xz = x.clone()
    xz[40] = 0.0
    tz = target.clone()
    tz[40] = 3
    out = _lib.linear_probe(dev(xz), dev(W), dev(b), dev(tz), dev(m), RPG, True, want_grad=True,
                            want_row_loss=True)
    assert all(bool(torch.isfinite(t.float()).all()) for t in out)
    assert int(out[0][40]) == int(b.argmax())
    want = float(torch.logsumexp(b, 0) - b[3])
    assert abs(float(out[5][40]) - want) <= 1e-5 * max(1.0, abs(want))

    # two equal rows of W with equal biases: the lower index wins
    Wt, bt = W.clone(), b.clone()
    Wt[11], bt[11] = Wt[4], bt[4]
    xt = F.normalize(Wt, dim=1)[4].repeat(65, 1) * (torch.arange(65).view(-1, 1) * 0.1 + 0.05)
    pt = _lib.linear_probe(dev(xt), dev(Wt), dev(bt))[0]
    z = lo.logits(lo.xhat(xt), Wt, bt)
    assert torch.equal(z[:, 4], z[:, 11]) and torch.equal(z[:, 4], z.max(dim=1).values)
    assert bool((pt == 4).all())

    # |z| ~ 100: the loss is finite and inside the row-loss bound
    Wb = W * (200.0 / 6.0)
    xh = lo.xhat(x, m, RPG, True)
    z32, z16 = lo.logits(xh, Wb, b), lo.logits_bf16(xh, Wb, b)
    assert float(z32.abs().max()) > 90
    tol = 2 * float((z16 - z32).abs().max())
    big = _lib.linear_probe(dev(x), dev(Wb), dev(b), dev(target), dev(m), RPG, True, want_grad=True,
                            want_row_loss=True)
    assert all(bool(torch.isfinite(t.float()).all()) for t in big)
    worst = float((big[5].cpu() - lo.row_loss(z32, target)).abs().max())
    print(f"|z| up to {float(z32.abs().max()):.1f}: tol {tol:.4f}, largest row-loss error {worst:.5f}")
    assert worst <= tol

    # target None: only pred is written.  The interface takes no other output pointer then (they
    # must be NULL), so the sentinels stand where a stray write would land: around pred and
    # behind the work buffer's sd_linear_probe_work floats
    import ctypes
    lib = _lib.load()
    xd, Wd, bd = dev(x), dev(W), dev(b)
    nwork = int(lib.sd_linear_probe_work(65, 64, 19))
    work = torch.full((nwork + 64,), 123.0, device=gpu)
    buf = torch.full((64 + 65 + 64,), -7, device=gpu, dtype=torch.int32)
    a = _lib.SdLinearProbeArgs(x=xd.data_ptr(), W=Wd.data_ptr(), b=bd.data_ptr(), N=65,
                               rows_per_group=1, n_groups=0, d=64, C=19, x_dtype=_lib.SD_F32,
                               normalize=1, work=work.data_ptr(), pred=buf[64:].data_ptr())
    assert lib.sd_linear_probe(ctypes.byref(a), _lib.stream_of(xd)) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[64:129], _lib.linear_probe(xd, Wd, bd, dev(target))[0])
    assert bool((buf[:64] == -7).all()) and bool((buf[129:] == -7).all())
    assert bool((work[nwork:] == 123.0).all())
    only = _lib.linear_probe(xd, Wd, bd)
    assert torch.equal(only[0], buf[64:129]) and all(t is None for t in only[1:])


# ------------------------------------------------------------------ LinearHead / SemanticHead
def _probe_head(d, C, W, b, dev):
    from scenedino_amd.downstream_head.semantic_head import LinearHead
    head = LinearHead(d, C)
    with torch.no_grad():
        head.linear.weight.copy_(W)
        head.linear.bias.copy_(b)
    return head.to(dev)


@pytest.mark.gpu
def test_linear_head_loss_ignores_the_second_view(gpu):
    n, v, h, w, d, C = 2, 2, 5, 13, 64, 19
    N = n * v * h * w
    W, b, x, _, target = lo.inputs("b", N, d, C)
    head = _probe_head(d, C, W, b, gpu)
    feats = x.view(n, v, h, w, 1, d).to(gpu)
    tgt = target.view(n, v, h, w)[:, 0].contiguous().to(gpu)
    res = head(feats, tgt, _normalize=True)
    other = feats.clone()
    other[:, 1] = torch.flip(feats[:, 1], dims=(1, 2))
    res2 = head(other, tgt, _normalize=True)
    assert res["segs_pred"].shape == (n, v, h, w, 1) and res["segs_pred"].dtype == torch.int64
    assert torch.equal(res["loss"], res2["loss"])
    assert torch.equal(res["segs_pred"][:, 0], res2["segs_pred"][:, 0])
    assert not torch.equal(res["segs_pred"][:, 1], res2["segs_pred"][:, 1])
    # and it is view 0's loss
    rows0 = x.view(n, v, h * w, d)[:, 0].reshape(-1, d)
    z32 = lo.logits(lo.xhat(rows0), W, b)
    z16 = lo.logits_bf16(lo.xhat(rows0), W, b)
    want = F.cross_entropy(z32, tgt.cpu().flatten(), ignore_index=-1)
    assert abs(float(res["loss"].detach()) - float(want)) <= 2 * float((z16 - z32).abs().max())


@pytest.mark.gpu
def test_direct_probe_keeps_no_normalised_copy(gpu):
    """One direct_linear_head call on 96 MiB of rows raises the peak by less than half of that:
    neither a normalised nor a masked copy of the rows exists."""
    N, d, C = 32768, 768, 19
    W, b = lo.inputs("b", 33, d, C)[:2]
    head = _probe_head(d, C, W, b, gpu)
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(1, 1, 128, 256, 1, d, generator=g).to(gpu)
    tgt = torch.randint(-1, C, (1, 128, 256), generator=g).to(gpu)
    m = lo.dropout_scales(1, d, g).to(gpu)
    head(feats[:, :, :2], tgt[:, :2], _mask=m, _rows_per_group=512, _normalize=True)["loss"].backward()
    head.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = head(feats, tgt, _mask=m, _rows_per_group=128 * 256, _normalize=True)
    res["loss"].backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak rise {rise / 2 ** 20:.1f} MiB for {N * d * 4 / 2 ** 20:.0f} MiB of rows")
    assert bool(torch.isfinite(res["loss"])) and head.linear.weight.grad is not None
    assert rise < N * d * 4 / 2


@pytest.mark.gpu
def test_semantic_head_forward_direct_linear_is_the_fp32_argmax(gpu):
    from scenedino_amd.downstream_head.semantic_head import SemanticHead
    key = ("a", 1000, 768, 19, torch.float32, False, True)
    x, W, b, _, _, z32, z16 = _oracle(*key)
    top = z32.topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) > 4 * float((z16 - z32).abs().max())
    head = SemanticHead(**so.HEAD_ARGS).to(gpu).eval()
    with torch.no_grad():
        head.direct_linear_head.linear.weight.copy_(W)
        head.direct_linear_head.linear.bias.copy_(b)
        pred = head(x.view(10, 100, 768).to(gpu), mode="direct_linear")
    assert pred.shape == (10, 100) and pred.dtype == torch.int64
    assert torch.equal(pred.flatten().cpu(), z32.argmax(dim=1))


def _training_case(seed=11):
    """forward_training's inputs with two views, labels over the stub table's ids (one id the
    table lacks), every dropout draw injected."""
    n, v, h, w, c = 2, 2, 16, 32, 768
    data, nc = so.head_step_inputs(seed, 0, "3d")
    more, _ = so.head_step_inputs(seed, 1, "3d")
    data["coarse"][0]["dino_features"] = torch.cat(
        [data["coarse"][0]["dino_features"], more["coarse"][0]["dino_features"]], dim=1)
    data["coarse"][0]["rgb"] = torch.cat([data["coarse"][0]["rgb"], more["coarse"][0]["rgb"]], dim=1)
    g = torch.Generator().manual_seed(77)
    ids = torch.tensor([0, 1, 2, 5, 6, 9, 200, 255, -1, 100])
    data["segs"] = [ids[torch.randint(len(ids), (n, h, w), generator=g)]]
    draws = {"dino": so.dropout_scales(n * v, c, g), "img_lin": so.dropout_scales(n * v, 64, g),
             "img_non": so.dropout_scales(n * v, 64, g), "crop": so.dropout_scales(nc, c, g),
             "nn_pick": torch.randint(2, (nc,), generator=g), "random_idx": torch.randint(3, (nc,), generator=g)}
    for k in ("self", "nn", "random"):
        draws[k + "_lin"] = so.dropout_scales(nc, 64, g)
        draws[k + "_non"] = so.dropout_scales(nc, 64, g)
    Wd, bd = lo.inputs("b", 33, c, 19)[:2]
    Ws, bs = lo.inputs("b", 33, 64, 19)[:2]
    return data, draws, (Wd, bd, Ws, bs)


def _training_head(dev, probes):
    from scenedino_amd.downstream_head.semantic_head import SemanticHead
    head = SemanticHead(**so.HEAD_ARGS, mode="3d")
    head.load_state_dict(so.head_state(11), strict=False)
    head.direct_cluster_head.centroids_initialized = True
    head.stego_cluster_head.centroids_initialized = True
    with torch.no_grad():
        for lin, W, b in ((head.direct_linear_head.linear, probes[0], probes[1]),
                          (head.stego_linear_head.linear, probes[2], probes[3])):
            lin.weight.copy_(W)
            lin.bias.copy_(b)
    return head.to(dev).train()


def _to(data, dev):
    if isinstance(data, dict):
        return {k: _to(v, dev) for k, v in data.items()}
    if isinstance(data, list):
        return [_to(v, dev) for v in data]
    return data.to(dev) if torch.is_tensor(data) else data


def _training_step(dev, autocast=False):
    data, draws, probes = _training_case()
    head = _training_head(dev, probes)
    head._draws = draws
    with torch.autocast("cpu", dtype=so.BF, enabled=autocast):
        seg = head.forward_training(_to(data, dev))["segmentation"]
        res = seg["results"]
    (res["direct_linear"]["loss"].float() + res["stego_linear"]["loss"].float()).backward()
    out = {"direct_loss": res["direct_linear"]["loss"], "stego_loss": res["stego_linear"]["loss"],
           "direct_W": head.direct_linear_head.linear.weight.grad,
           "direct_b": head.direct_linear_head.linear.bias.grad,
           "stego_W": head.stego_linear_head.linear.weight.grad,
           "stego_b": head.stego_linear_head.linear.bias.grad}
    out = {k: t.detach().float().cpu().reshape(-1) if k.endswith("loss") else t.detach().float().cpu()
           for k, t in out.items()}
    return out, seg, head


@pytest.mark.gpu
def test_forward_training_with_segs_takes_the_kernel_twice(gpu, monkeypatch):
    """GPU-native against the same head on the CPU (torch ops, fp32 and under bf16 autocast):
    both probe losses inside tol, W.grad and b.grad by the yardstick, segs_pred's shape and
    dtype, and two sd_linear_probe calls per step."""
    from scenedino_amd import _lib
    lo.install_stub_labels(monkeypatch)
    calls = []
    real = _lib.linear_probe

    def spy(*a, **k):
        calls.append(a[0].shape)
        return real(*a, **k)

    monkeypatch.setattr(_lib, "linear_probe", spy)
    native, seg, head = _training_step(gpu)
    assert calls == [(2 * 2 * 16 * 32, 768), (2 * 2 * 16 * 32, 64)]
    f32, seg32, _ = _training_step("cpu")
    f16, _, _ = _training_step("cpu", autocast=True)
    assert len(calls) == 2  # the CPU head stays on torch ops

    data, draws, (Wd, bd, Ws, bs) = _training_case()
    target = seg32["target"]
    assert target.shape == (2, 16, 32) and int(target.min()) == -1 and int(target.max()) == 7
    assert torch.equal(seg["target"].cpu(), target)
    for name in ("direct_linear", "stego_linear"):
        sp = seg["results"][name]["segs_pred"]
        assert sp.shape == (2, 2, 16, 32, 1) and sp.dtype == torch.int64 and sp.is_cuda

    # tol per probe: 2 x the largest logit error of the bf16 evaluation of its chain
    img = data["coarse"][0]["dino_features"].reshape(-1, 768)
    xh = lo.xhat(img, draws["dino"], 512, True)
    tol_d = 2 * float((lo.logits_bf16(xh, Wd, bd) - lo.logits(xh, Wd, bd)).abs().max())
    st = so.head_state(11)
    Wst = [st["stego_head." + n] for n in so.STEGO_NAMES]
    y32 = so.stego_formula(img, *Wst, draws["img_lin"], draws["img_non"], 512)
    with torch.autocast("cpu", dtype=so.BF):
        y16 = so.stego_formula(img, *Wst, draws["img_lin"], draws["img_non"], 512).float()
    tol_s = 2 * float((lo.logits_bf16(y16, Ws, bs) - lo.logits(y32, Ws, bs)).abs().max())
    for name, tol in (("direct_loss", tol_d), ("stego_loss", tol_s)):
        err = abs(float(native[name]) - float(f32[name]))
        print(f"{name}: native {float(native[name]):.6f}, cpu {float(f32[name]):.6f}, tol {tol:.5f}")
        assert tol > 0 and err <= tol
    so.check(native, f32, f16, ("direct_W", "direct_b", "stego_W", "stego_b"), what="forward_training")
