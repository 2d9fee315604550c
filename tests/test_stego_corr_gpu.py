"""GPU: the fused STEGO correlation loss (sd_stego_corr_fwd / _bwd, csrc/sdhip_stego_corr.hip)
against the f64 torch formula of tests/_stego_corr_oracle.py, and StegoLoss's fused route on
SemanticHead's lazy correlation mapping against the eager step on the same device.

Yardstick (the project's rule, tests/_stego_oracle.py): a native tensor's rel-L2 distance to the
f64 formula is at most 2 x the rel-L2 error of the same formula under CPU bf16 autocast on the same
inputs; both figures are computed here and printed.  The indicator 1[S > 0] can flip where |S| is
within bf16 rounding of zero, on both sides of that comparison; the ``separated`` case draws code
rows whose |S| stays above 1e-2 (asserted on the f64 oracle), so it holds with no flipped element.
"""
from __future__ import annotations

import functools
import math

import pytest
import torch

import _stego_corr_oracle as co
import _stego_oracle as so
from test_semantic_head_train import _to

UP = torch.tensor([0.7, 1.3, 0.4])
SHAPES = {"sub_tile": (1, 24, 24, 384), "ragged": (3, 80, 48, 768), "recipe_rows": (2, 576, 576, 768)}
# (n_pairs, self pair first, bf16 DINO rows, zero rows)
VARIANTS = {"three_pairs_zero_rows": (3, True, False, True), "self_alone": (1, True, False, False),
            "partner_alone_bf16": (1, False, True, False), "three_pairs_bf16": (3, True, True, False)}


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


@functools.lru_cache(maxsize=None)
def _case(shape, variant, pointwise, separated=False):
    """Rows and both CPU evaluations (f64, bf16 autocast) of one case, computed once."""
    nc, P, Q, d = SHAPES[shape]
    n_pairs, self_pair, bf16, zero = VARIANTS[variant]
    rows = co.make_rows(nc, P, Q, d, n_pairs, self_pair, separated=separated, zero_rows=zero)
    if bf16:  # every evaluation reads the rounded rows
        rows["A"] = rows["A"].bfloat16().float()
        rows["Bs"] = [None if t is None else t.bfloat16().float() for t in rows["Bs"]]
    w, s = co.YAML_WEIGHTS[:n_pairs], co.YAML_SHIFTS[:n_pairs]
    f64 = co.evaluate(rows, w, s, pointwise, UP)
    f16 = co.evaluate(rows, w, s, pointwise, UP, autocast=True)
    return rows, w, s, f64, f16, bf16


def _upload(rows, bf16, dev, up=UP):
    dt = torch.bfloat16 if bf16 else torch.float32
    partners = [(None, None) if B is None else (B.to(dev, dt), b.to(dev))
                for B, b in zip(rows["Bs"], rows["bs"])]
    return rows["A"].to(dev, dt), rows["a"].to(dev), partners, up.to(dev)


def _native(rows, w, s, pointwise, bf16, dev, up=UP, need=None):
    return _run(_upload(rows, bf16, dev, up), w, s, pointwise, need)


def _run(operands, w, s, pointwise, need=None):
    from scenedino_amd import _lib
    A, a, partners, up = operands
    loss, work = _lib.stego_corr_fwd(A, a, partners, w, s, pointwise)
    need = (True,) * (1 + len(partners)) if need is None else need
    d_a, d_b = _lib.stego_corr_bwd(up, A, a, partners, w, s, pointwise, work, need)
    out = {"loss": loss[:len(partners)]}
    if d_a is not None:
        out["d_a"] = d_a
    for i, g in enumerate(d_b):
        if g is not None:
            out[f"d_b{i}"] = g
    return out


def _check(native, f64, f16, what):
    names = tuple(f64)
    assert set(native) == set(names)
    so.check({k: native[k].reshape(f64[k].shape) for k in names}, f64, f16, names, what=what)


@pytest.mark.gpu
@pytest.mark.parametrize("pointwise", [False, True])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_against_the_f64_formula(gpu, shape, variant, pointwise):
    rows, w, s, f64, f16, bf16 = _case(shape, variant, pointwise)
    native = _native(rows, w, s, pointwise, bf16, gpu)
    _check(native, f64, f16, f"{shape} {variant} pointwise={pointwise}")
    if VARIANTS[variant][3]:  # the zero code row gets a zero gradient; everything is finite
        assert float(native["d_a"][0, 1 % rows["a"].shape[1]].abs().max()) == 0.0
        assert all(bool(torch.isfinite(v).all()) for v in native.values())
    if variant == "self_alone":  # both sides of the self pair land on the same rows
        assert set(native) == {"loss", "d_a"}


@pytest.mark.gpu
@pytest.mark.parametrize("pointwise", [False, True])
def test_separated_codes_meet_the_bound_without_a_flipped_indicator(gpu, pointwise):
    rows, w, s, f64, f16, bf16 = _case("ragged", "three_pairs_bf16", pointwise, separated=True)
    assert co.min_abs_S(rows) > 1e-2
    _check(_native(rows, w, s, pointwise, bf16, gpu), f64, f16, f"separated pointwise={pointwise}")


@pytest.mark.gpu
def test_repeats_streams_graph_replay_and_sync_free_calls_are_bit_equal(gpu):
    rows, w, s, _, _, bf16 = _case("ragged", "three_pairs_zero_rows", True)
    ops = _upload(rows, bf16, gpu)
    first = _run(ops, w, s, True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = _run(ops, w, s, True)  # forward and backward without a host synchronisation
    finally:
        torch.cuda.set_sync_debug_mode("default")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _run(ops, w, s, True)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _run(ops, w, s, True)
    for v in captured.values():
        v.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for k, v in first.items():
        for name, got in (("repeat", again), ("stream", other), ("graph", captured)):
            assert torch.equal(v, got[k]), (name, k)


@pytest.mark.gpu
def test_zero_upstream_gives_exact_zeros_and_unneeded_gradients_are_skipped(gpu):
    rows, w, s, _, _, bf16 = _case("ragged", "three_pairs_zero_rows", False)
    out = _native(rows, w, s, False, bf16, gpu, up=torch.zeros(3))
    for k in ("d_a", "d_b1", "d_b2"):
        assert torch.equal(out[k], torch.zeros_like(out[k])), k
    some = _native(rows, w, s, False, bf16, gpu, need=(False, False, True, False))
    full = _native(rows, w, s, False, bf16, gpu)
    assert set(some) == {"loss", "d_b1"} and torch.equal(some["d_b1"], full["d_b1"])


@pytest.mark.gpu
def test_operands_outside_the_domain_are_rejected_with_a_text(gpu):
    from scenedino_amd import _lib
    dev = gpu

    def call(A, a, partners=((None, None),)):
        return _lib.stego_corr_fwd(A, a, list(partners), (1.0,) * len(partners), (0.0,) * len(partners), False)

    ok_A, ok_a = torch.randn(2, 24, 384, device=dev), torch.randn(2, 24, 64, device=dev)
    assert call(ok_A, ok_a)[0].shape == (3,)
    bad = {"d = 512": (torch.randn(2, 24, 512, device=dev), ok_a),
           "code width 32": (ok_A, torch.randn(2, 24, 32, device=dev)),
           "non-contiguous": (torch.randn(2, 24, 768, device=dev)[..., ::2], ok_a),
           "f16": (ok_A.half(), ok_a),
           "P = 0": (torch.randn(2, 0, 384, device=dev), torch.randn(2, 0, 64, device=dev))}
    for what, (A, a) in bad.items():
        with pytest.raises((RuntimeError, ValueError, TypeError), match="sd_stego_corr") as e:
            call(A, a)
        assert len(str(e.value)) > 20, what
    with pytest.raises((RuntimeError, ValueError, TypeError), match="sd_stego_corr"):
        call(ok_A, ok_a, ((ok_A.half(), ok_a),))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------ the training step
# Shapes of the step test.  The memory bound compares whole-step peaks, so it can only show where
# the eager step's peak lies in its loss: per crop of P = 576 points the eager loss phase holds
# the six (P, P) tensors plus about nine more of that size for autograd (about 20 MB), the fused
# route the three operand row sets in f32 and bf16 plus the code-sized scratch (about 9 MB), and
# both hold the same saved activations of the head; the head's backward adds weight-gradient
# partial buffers of a fixed size (about 30 MB) in which the eager step still holds the six
# tensors and the fused one the f32 operand rows.  The loss phase dominates the eager peak, and
# the difference exceeds the six tensors, from about 11 crops on (the recipe has 20); below about
# 450 points per crop the operand rows outweigh the correlation tensors altogether.
HEAD_P = {"3d": 576, "2d": 576}   # 2d: 96 x 96 images at sample_factor 2 -> 24 x 24 points per crop
HEAD_NC = {"3d": 12, "2d": 10}    # 2d: five crops of each of two images


def _step_inputs(mode, step):
    """tests/_stego_oracle.head_step_inputs at more points per crop (the correlation tensors
    must outweigh the operand rows for the memory bound to say something)."""
    seed = so.HEAD_SEEDS[mode]
    g = torch.Generator().manual_seed(5000 * seed + step)
    n, v, c = 2, 1, 768
    h, w = (16, 32) if mode == "3d" else (96, 96)
    P = HEAD_P[mode]
    dirs = torch.nn.functional.normalize(
        so.head_state(seed)["direct_cluster_head.cluster_centers"], dim=1) * math.sqrt(c)
    img = (dirs[torch.randint(19, (n, v, h, w), generator=g)] + 0.3 * torch.randn(n, v, h, w, c, generator=g)) \
        * (torch.rand(n, v, h, w, 1, generator=g) * 2 + 0.1)
    k3 = HEAD_NC["3d"]
    crops = dirs[torch.randint(19, (k3, P), generator=g)] + 0.7 * torch.randn(k3, P, c, generator=g)
    data = {"coarse": [{"rgb": torch.rand(n, v, h, w, 1, 3, generator=g), "dino_features": img.unsqueeze(-2)}],
            "sample_surface_sigma": torch.rand(1, k3, P, generator=g),
            "sample_surface_dino_features": crops.unsqueeze(0)}
    nc = HEAD_NC[mode]
    draws = {"nn_pick": torch.randint(2, (nc,), generator=g),
             "random_idx": torch.randint(nc * (step + 1) if mode == "3d" else nc, (nc,), generator=g)}
    return data, draws, nc


def _make_head(mode, dev):
    from scenedino_amd.downstream_head.semantic_head import SemanticHead
    nc = HEAD_NC[mode]
    head = SemanticHead(**dict(so.HEAD_ARGS, patch_sample_size=HEAD_P[mode], buffer_size=4 * nc), mode=mode)
    head.load_state_dict(so.head_state(so.HEAD_SEEDS[mode]), strict=False)
    head.direct_cluster_head.centroids_initialized = True
    head.stego_cluster_head.centroids_initialized = True
    for m in head.modules():
        if isinstance(m, (torch.nn.Dropout2d, torch.nn.Dropout1d)):
            m.p = 0.0
    return head.to(dev).train()


def _two_steps(mode, dev, lazy, pointwise, autocast=False):
    from scenedino_amd.losses import StegoLoss
    head = _make_head(mode, dev)
    head.lazy_corr = lazy
    opt = torch.optim.Adam([{"params": list(p), "lr": 1e-4 * f} for f, p in head.parameters_lr()])
    loss_fn = StegoLoss(dict(so.STEGO_LOSS, pointwise=pointwise))
    out, peak = {}, 0
    for step in range(2):
        data, draws, nc = _step_inputs(mode, step)
        head._draws = draws
        data = _to(data, dev)
        if dev != "cpu":
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
        with torch.autocast("cpu", dtype=so.BF, enabled=autocast):
            data = head.forward_training(data, sample_factor=2 if mode == "2d" else 4)
            losses = loss_fn(data)
        opt.zero_grad(set_to_none=True)
        losses["total_loss"].float().backward()
        if dev != "cpu":
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
        t = f"step{step}_"
        out[t + "losses"] = torch.stack([losses[k].detach().float() for k in
                                         ("self_loss", "knn_loss", "random_loss", "total_loss")]).cpu()
        for name in so.STEGO_NAMES:
            out[t + "grad_" + name] = head.stego_head.get_parameter(name).grad.detach().float().cpu().clone()
        seg = data["segmentation"]
        out[t + "labels"] = torch.cat([seg["results"][k]["pseudo_segs_pred"].flatten().cpu()
                                       for k in ("direct_cluster", "stego_cluster")])
        out[t + "buffers"] = torch.cat([head.dino_patch_buffer.flatten().cpu(), head.dino_gap_buffer.flatten().cpu(),
                                        torch.tensor([float(head.buffer_idx), float(head.buffer_filled)])])
        corr = seg["stego_corr"]
        opt.step()
        shape = tuple(corr.dino[0].shape[:2]) if lazy else tuple(corr["dino_self_corr"].shape[:2])
        info = {"route": loss_fn.last_route, "materialised": corr.materialised if lazy else None,
                "peak": peak, "nc_P": shape}
        del data, seg, corr, losses
    return out, info


@functools.lru_cache(maxsize=None)
def _cpu_steps(mode, pointwise, autocast):
    return _two_steps(mode, "cpu", False, pointwise, autocast)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("pointwise", [False, True])
@pytest.mark.parametrize("mode", ["3d", "2d"])
def test_two_training_steps_on_the_fused_route_match_the_eager_steps(gpu, mode, pointwise):
    eager, e_info = _two_steps(mode, gpu, False, pointwise)
    fused, f_info = _two_steps(mode, gpu, True, pointwise)
    assert e_info["route"] == "torch" and f_info["route"] == "fused"
    assert f_info["materialised"] == ()  # no (nc, P, P) tensor was built
    f32, f16 = _cpu_steps(mode, pointwise, False), _cpu_steps(mode, pointwise, True)
    exact = [k for k in eager if k.endswith("labels") or k.endswith("buffers")]
    for k in exact:
        assert torch.equal(eager[k], fused[k]), k
    names = tuple(k for k in eager if k not in exact)
    # the yardstick: the eager step's own bf16-autocast error on the CPU
    so.check(fused, eager, {k: eager[k] + (f16[k] - f32[k]) for k in names}, names,
             what=f"{mode} pointwise={pointwise}")
    nc, P = f_info["nc_P"]
    assert P == HEAD_P[mode] and e_info["nc_P"] == (nc, P)
    six = 6 * nc * P * P * 4
    print(f"{mode}: peak eager {e_info['peak']} B, fused {f_info['peak']} B, six tensors {six} B")
    assert e_info["peak"] - f_info["peak"] >= six
