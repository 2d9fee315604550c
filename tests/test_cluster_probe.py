"""sd_cluster_probe (csrc/sdhip_probe.hip): one pass of KMeansParamHead._kmeans_cosine and its
loss statistics, and KMeansParamHead's loss / centre gradient on top of it.

Two input families, no row left out of any check:
  (a) clustered rows x = (c_k + randn(d) / sqrt(d)) U(0, 3): the fp32 oracle's smallest top-2
      margin is asserted to exceed 2e-2 (tests/test_seg.py's margin), so every label must equal
      the oracle's;
  (b) unstructured randn rows, where many margins are under 2e-2: every native label must be
      near-optimal, s32[i, label_i] >= max_k s32[i, k] - tol with tol = 2 x the largest absolute
      score error of the CPU bf16 evaluation, measured here; the oracle's S is recomputed with
      the native labels.
S and the loss follow tests/_stego_oracle.py's yardstick (2 x the bf16-autocast error of the
same formula); counts are exact for the native labels.
"""
from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

import _stego_oracle as so

SHAPES = [(N, d, K) for N in (1, 63, 65, 1000, 4096) for d in (64, 384, 768) for K in (19, 32)]
VARIANTS = [(dt, mw) for dt in (torch.float32, torch.bfloat16) for mw in (False, True)]
RPG = 48


@functools.lru_cache(maxsize=None)
def _inputs(family, N, d, K):
    """Seed offset 3: family (a)'s precondition (every fp32 top-2 margin over 2e-2, asserted in
    the test) holds in all cases there, smallest margin 0.081 at (4096, 64, 32) with masks; at
    five of twelve offsets tried one d = 64 row of the 4096 falls under it."""
    g = torch.Generator().manual_seed(31 * N + 7 * d + K + (3 if family == "a" else 100000))
    centres = torch.randn(K, d, generator=g) * (torch.rand(K, 1, generator=g) + 0.5)
    if family == "a":
        c = F.normalize(centres, dim=1)
        x = (c[torch.randint(K, (N,), generator=g)] + torch.randn(N, d, generator=g) / d ** 0.5) \
            * (torch.rand(N, 1, generator=g) * 3)
    else:
        x = torch.randn(N, d, generator=g)
    m = so.dropout_scales((N + RPG - 1) // RPG, d, g)
    w = torch.rand(N, generator=g) + 0.5
    return x, centres, m, w


@functools.lru_cache(maxsize=None)
def _oracle(family, N, d, K, dtype, mw):
    """x as the kernel reads it, fp32 scores, bf16-evaluation scores."""
    x, centres, m, w = _inputs(family, N, d, K)
    x = x.to(dtype)
    m, w = (m, w) if mw else (None, None)
    xh = so.probe_xhat(x, m, RPG)
    c = F.normalize(centres, dim=1)
    s32 = xh @ c.t()
    s16 = (xh.to(so.BF) @ c.to(so.BF).t()).float()
    return x, centres, m, w, xh, s32, s16


_RUNS = {}


def _run(key, dev):
    if key not in _RUNS:
        from scenedino_amd import _lib
        x, centres, m, w = _oracle(*key)[:4]
        args = (x.to(dev), F.normalize(centres, dim=1).to(dev), None if m is None else m.to(dev), RPG,
                None if w is None else w.to(dev))
        _RUNS[key] = (_lib.cluster_probe(*args), _lib.cluster_probe(*args))
    return _RUNS[key]


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


def test_cpu_fallback_loss_is_the_reference_formula():
    """KMeansParamHead on CPU tensors (the torch-op path): loss and centre gradient equal the
    restated reference formula, with and without weights and column scales."""
    from scenedino_amd.downstream_head.semantic_head import KMeansParamHead
    x, centres, m, w = _inputs("a", 1000, 64, 19)
    for mw in (False, True):
        head = KMeansParamHead(19, 19, 64).train()
        head.centroids_initialized = True
        with torch.no_grad():
            head.cluster_centers.copy_(centres)
        res = head(x.view(10, 100, 64), weight=w.view(10, 100) if mw else None,
                   **(dict(_mask=m, _rows_per_group=RPG) if mw else {}))
        res["loss"].backward()
        leaf = centres.clone().requires_grad_(True)
        loss, labels = so.kmeans_loss(x, leaf, w if mw else None, m=m if mw else None, rows_per_group=RPG)
        loss.backward()
        assert torch.equal(res["pseudo_segs_pred"].flatten(), labels)
        assert res["pseudo_segs_pred"].shape == (10, 100)
        torch.testing.assert_close(res["loss"], loss, rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(head.cluster_centers.grad, leaf.grad, rtol=1e-4, atol=1e-7)


def test_first_train_call_redraws_the_centres():
    from scenedino_amd.downstream_head.semantic_head import KMeansParamHead
    head = KMeansParamHead(19, 19, 64)
    before = head.cluster_centers.detach().clone()
    head.eval()(torch.randn(5, 64))
    assert torch.equal(head.cluster_centers, before) and not head.centroids_initialized
    head.train()(torch.randn(5, 64))
    assert head.centroids_initialized and not torch.equal(head.cluster_centers, before)
    again = head.cluster_centers.detach().clone()
    head(torch.randn(5, 64))
    assert torch.equal(head.cluster_centers, again)


def _check_stats(key, labels, S, counts):
    """S, loss and counts of a run against the oracle evaluated with the run's labels."""
    _, N, d, K, _, _ = key
    _, centres, _, w, xh, _, _ = _oracle(*key)
    lab = labels.cpu().long()
    S32, l32 = so.probe_stats(xh, centres, lab, w)
    with torch.autocast("cpu", dtype=so.BF):
        S16, l16 = so.probe_stats(xh, centres, lab, w)
    assert torch.equal(counts.cpu().long(), torch.bincount(lab, minlength=K))
    cn = F.normalize(centres, dim=1)
    native = {"S": S, "loss": -(cn * S.cpu()).sum().view(1) / N}
    so.check(native, {"S": S32, "loss": l32.view(1)}, {"S": S16.float(), "loss": l16.float().view(1)},
             ("S", "loss"), what=str(key))


@pytest.mark.gpu
@pytest.mark.parametrize("N,d,K", SHAPES)
def test_clustered_rows_get_the_oracle_labels(gpu, N, d, K):
    for dt, mw in VARIANTS:
        key = ("a", N, d, K, dt, mw)
        s32 = _oracle(*key)[5]
        top = s32.topk(2, dim=1).values
        margin = float((top[:, 0] - top[:, 1]).min())
        print(f"{key}: smallest fp32 top-2 margin {margin:.4f}")
        assert margin > 2e-2
        (labels, S, counts), _ = _run(key, gpu)
        assert labels.dtype == torch.int32 and labels.shape == (N,)
        assert torch.equal(labels.cpu().long(), s32.argmax(dim=1))
        _check_stats(key, labels, S, counts)


@pytest.mark.gpu
@pytest.mark.parametrize("N,d,K", SHAPES)
def test_unstructured_rows_get_near_optimal_labels(gpu, N, d, K):
    for dt, mw in VARIANTS:
        key = ("b", N, d, K, dt, mw)
        s32, s16 = _oracle(*key)[5:7]
        tol = 2 * float((s16 - s32).abs().max())
        (labels, S, counts), _ = _run(key, gpu)
        lab = labels.cpu().long()
        assert int(lab.min()) >= 0 and int(lab.max()) < K
        gap = s32.max(dim=1).values - s32.gather(1, lab[:, None]).squeeze(1)
        print(f"{key}: tol {tol:.5f}, largest gap {float(gap.max()):.6f}, "
              f"{int((lab != s32.argmax(dim=1)).sum())} labels differ from the fp32 argmax")
        assert tol > 0 and float(gap.max()) <= tol
        _check_stats(key, labels, S, counts)


@pytest.mark.gpu
@pytest.mark.parametrize("N,d,K", SHAPES)
def test_two_launches_give_the_same_bits(gpu, N, d, K):
    for family in ("a", "b"):
        for dt, mw in VARIANTS:
            first, second = _run((family, N, d, K, dt, mw), gpu)
            for a, b in zip(first, second):
                assert torch.equal(a, b)


@pytest.mark.gpu
def test_ties_take_the_lowest_index_and_a_zero_row_gives_zeros(gpu):
    from scenedino_amd import _lib
    g = torch.Generator().manual_seed(5)
    c = F.normalize(torch.randn(19, 64, generator=g), dim=1)
    c[7] = c[3]
    c[12] = c[3]
    x = torch.randn(65, 64, generator=g)
    x[:40] = c[3] * (torch.rand(40, 1, generator=g) + 0.5) + 0.01 * torch.randn(40, 64, generator=g)
    x[50] = 0.0
    labels, S, counts = _lib.cluster_probe(x.to(gpu), c.to(gpu))
    assert bool((labels[:40] == 3).all()) and int(labels[50]) == 0
    assert not bool((labels == 7).any()) and not bool((labels == 12).any())
    assert bool(torch.isfinite(S).all()) and int(counts.sum()) == 65
    # the zero row adds nothing to S (the oracle's xh of it is zero too)
    S32, _ = so.probe_stats(so.probe_xhat(x), c, labels.cpu().long())
    assert so.rel_l2(S, S32) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("family,N,d,K", [("a", 1000, 768, 19), ("b", 1000, 768, 19),
                                          ("a", 4096, 64, 32), ("b", 65, 384, 19)])
def test_centre_gradient_through_the_python_head(gpu, family, N, d, K):
    """loss = -(1/N) sum_k c_k . S_k with plain autograd through F.normalize(cluster_centers),
    against CPU autograd of the reference formula (family b: with the native labels)."""
    from scenedino_amd.downstream_head.semantic_head import KMeansParamHead
    for mw in (False, True):
        x, centres, m, w = _inputs(family, N, d, K)
        head = KMeansParamHead(K, 19, d).to(gpu).train()
        head.centroids_initialized = True
        with torch.no_grad():
            head.cluster_centers.copy_(centres)
        res = head(x.to(gpu), weight=w.to(gpu) if mw else None,
                   **(dict(_mask=m.to(gpu), _rows_per_group=RPG) if mw else {}))
        res["loss"].backward()
        lab = res["pseudo_segs_pred"].cpu()
        assert res["segs_pred"].shape == (N,) and res["segs_pred"].dtype == torch.int64

        def cpu(autocast):
            leaf = centres.clone().requires_grad_(True)
            with torch.autocast("cpu", dtype=so.BF, enabled=autocast):
                loss, _ = so.kmeans_loss(x, leaf, w if mw else None, lab, m if mw else None, RPG)
            loss.float().backward()
            return {"loss": loss.detach().float().view(1), "centres": leaf.grad}

        native = {"loss": res["loss"].detach().view(1), "centres": head.cluster_centers.grad}
        so.check(native, cpu(False), cpu(True), ("loss", "centres"), what=f"{family} {N} {d} {K} mw={mw}")
