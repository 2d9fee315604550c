"""SemanticHead.forward_training (downstream_head/semantic_head.py), StegoLoss (losses/) and the
drop-in switch, against two recorded training steps of the reference head
(tests/golden/stego_train.npz, written by tests/golden/make_golden_stego.py from the seeded
parameters and inputs of tests/_stego_oracle.py; dropout p = 0, every randint draw recorded).

CPU: the torch-op fallback reproduces the fixture to fp32 rounding (rtol 1e-4).
GPU: the native path matches it within the yardstick of tests/_stego_oracle.py; the bound of
a tensor is 2 x the rel-L2 distance between the fixture and the same torch-op path run under
CPU bf16 autocast on the same inputs.  Labels are equal wherever the fixture's top-2 margin
exceeds 2e-2 (the generator checks that at least 95 % of the rows do).
"""
from __future__ import annotations

import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import _stego_oracle as so
from conftest import GOLDEN

CORR = ("dino_self_corr", "stego_self_corr", "dino_nn_corr", "stego_nn_corr", "dino_random_corr",
        "stego_random_corr")
SUB = {"stego_head.linear_path.0.weight": (slice(None), slice(None, None, 4)),
       "stego_head.nonlinear_path.0.weight": (slice(None, None, 16), slice(None)),
       "stego_head.nonlinear_path.2.weight": (slice(None), slice(None, None, 4))}


@functools.lru_cache(maxsize=None)
def _fixture():
    return {k: torch.as_tensor(np.asarray(v)) for k, v in np.load(os.path.join(GOLDEN, "stego_train.npz")).items()}


def _head(mode, dev, p=0.0):
    from scenedino_amd.downstream_head.semantic_head import SemanticHead
    head = SemanticHead(**so.HEAD_ARGS, mode=mode)
    head.load_state_dict(so.head_state(so.HEAD_SEEDS[mode]), strict=False)
    head.direct_cluster_head.centroids_initialized = True
    head.stego_cluster_head.centroids_initialized = True
    for m in head.modules():
        if isinstance(m, (torch.nn.Dropout2d, torch.nn.Dropout1d)):
            m.p = p
    return head.to(dev).train()


def _to(data, dev):
    if isinstance(data, dict):
        return {k: _to(v, dev) for k, v in data.items()}
    if isinstance(data, list):
        return [_to(v, dev) for v in data]
    return data.to(dev) if torch.is_tensor(data) else data


def _two_steps(mode, dev, autocast=False):
    """Both recorded steps through this package's head and StegoLoss: every tensor the fixture
    holds, by its key."""
    from scenedino_amd.losses import StegoLoss, make_loss
    fx = _fixture()
    head = _head(mode, dev)
    seed = so.HEAD_SEEDS[mode]
    out = {}
    for step in range(2):
        data, nc = so.head_step_inputs(seed, step, mode)
        t = f"{mode}_{step}_"
        head._draws = {"nn_pick": fx[t + "nn_pick"], "random_idx": fx[t + "random_idx"]}
        with torch.autocast("cpu", dtype=so.BF, enabled=autocast):
            data = head.forward_training(_to(data, dev), sample_factor=2 if mode == "2d" else 4)
            seg = data["segmentation"]
            for k in CORR:
                out[t + k] = seg["stego_corr"][k].detach().float().cpu().clone()  # pointwise edits in place
            for name in ("direct", "stego"):
                res = seg["results"][name + "_cluster"]
                assert set(res) == {"pseudo_segs_pred", "segs_pred", "loss"}
                out[t + name + "_labels"] = res["pseudo_segs_pred"].cpu()
                out[t + name + "_loss"] = res["loss"].detach().float().cpu()
            loss_fn = make_loss(dict(so.STEGO_LOSS, type="stego", pointwise=False))
            assert isinstance(loss_fn, StegoLoss)
            losses = loss_fn(data)
            assert set(losses) == set(loss_fn.get_loss_metric_names())
            total = losses["total_loss"]
        out[t + "total"] = total.detach().float().cpu()
        if step == 1:
            head.zero_grad(set_to_none=True)
            total.float().backward()
            for name, p in head.named_parameters():
                if p.grad is not None:
                    g = p.grad.reshape(p.shape[0], -1) if p.dim() == 4 else p.grad
                    out[f"{mode}_grad_{name}"] = (g[SUB[name]] if name in SUB else g).float().cpu()
        with torch.autocast("cpu", dtype=so.BF, enabled=autocast):
            out[t + "total_pointwise"] = StegoLoss(dict(so.STEGO_LOSS, pointwise=True))(data)[
                "total_loss"].detach().float().cpu()
    assert head.buffer_filled == (6 if mode == "3d" else 1) and head.buffer_idx == (6 if mode == "3d" else 0)
    return out


@functools.lru_cache(maxsize=None)
def _cpu_steps(mode, autocast):
    return _two_steps(mode, "cpu", autocast)


def _float_keys(mode):
    return [k for k, v in _fixture().items() if k.startswith(mode) and v.dtype == torch.float32
            and not k.endswith("_margin")]


def _labels_match(got, mode):
    fx = _fixture()
    for step in range(2):
        for name in ("direct", "stego"):
            t = f"{mode}_{step}_{name}"
            wide = fx[t + "_margin"] > 2e-2
            assert float(wide.float().mean()) >= 0.95
            a, b = got[t + "_labels"].flatten().long(), fx[t + "_labels"].flatten().long()
            assert a.shape == b.shape and torch.equal(a[wide], b[wide]), t


# ------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("mode", ["3d", "2d"])
def test_cpu_fallback_reproduces_the_reference_fixture(mode):
    fx, got = _fixture(), _cpu_steps(mode, False)
    keys = _float_keys(mode)
    assert len(keys) == 2 * (6 + 4) + 8
    for k in keys:
        torch.testing.assert_close(got[k].reshape(fx[k].shape), fx[k], rtol=1e-4, atol=1e-6, msg=k)
    _labels_match(got, mode)


def test_state_dict_keys_and_lr_groups_match_the_reference():
    from scenedino_amd.downstream_head.semantic_head import SemanticHead
    manifest = json.load(open(os.path.join(GOLDEN, "state_dict_manifest.json")))
    head = SemanticHead(**so.HEAD_ARGS, mode="3d")
    sd = head.state_dict()
    assert {k: list(v.shape) for k, v in sd.items()} == manifest["semantic_head"]
    assert not any("buffer" in k for k in sd)
    assert head.dino_patch_buffer.shape == (8, 16, 768) and head.dino_gap_buffer.shape == (8, 768)
    assert head.buffer_idx == 0 and head.buffer_filled == 1
    groups = head.parameters_lr()
    assert [f for f, _ in groups] == [1.0, 10.0, 10.0, 10.0, 10.0]
    mods = (head.stego_head, head.direct_cluster_head, head.stego_cluster_head,
            head.direct_linear_head, head.stego_linear_head)
    for (_, params), m in zip(groups, mods):
        assert [id(p) for p in params] == [id(p) for p in m.parameters()]


def test_linear_probes_return_a_loss_and_crf_is_refused():
    from scenedino_amd.downstream_head.semantic_head import LinearHead, MLPHead, SemanticHead
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(2, 1, 4, 8, 1, 64, generator=g)
    target = torch.randint(-1, 19, (2, 4, 8), generator=g)
    for cls in (LinearHead, MLPHead):
        head = cls(64, 19)
        assert set(head(feats)) == {"segs_pred"}
        res = head(feats, target)
        logit = (head.linear(feats) if cls is LinearHead else
                 head.linear2(torch.relu(head.linear1(feats))))[:, 0, :, :, 0]
        ref = torch.nn.functional.cross_entropy(logit.permute(0, 3, 1, 2), target, ignore_index=-1)
        torch.testing.assert_close(res["loss"], ref)
        assert res["segs_pred"].shape == (2, 1, 4, 8, 1)
    head = SemanticHead(**so.HEAD_ARGS, mode="3d", apply_crf=True)
    with pytest.raises(NotImplementedError, match="pydensecrf"):
        head.forward_training(so.head_step_inputs(11, 0, "3d")[0])


def test_eval_mode_and_missing_surface_samples_on_cpu():
    head = _head("3d", "cpu", p=0.1)
    data, _ = so.head_step_inputs(11, 0, "3d")
    head.forward_training(dict(data))
    state = (head.buffer_idx, head.buffer_filled, head.dino_patch_buffer.clone(), head.dino_gap_buffer.clone())
    head.eval()
    a = head.forward_training(dict(so.head_step_inputs(11, 1, "3d")[0]))["segmentation"]
    head._draws = None
    assert (head.buffer_idx, head.buffer_filled) == state[:2]
    assert torch.equal(head.dino_patch_buffer, state[2]) and torch.equal(head.dino_gap_buffer, state[3])
    assert set(a["results"]) == {"direct_cluster", "stego_cluster"}
    d2 = dict(so.head_step_inputs(11, 1, "3d")[0], sample_surface_sigma=None)
    b = head.forward_training(d2)
    assert "stego_corr" not in b["segmentation"] and float(b["sample_surface_sigma"]) == 0.0
    assert torch.equal(b["segmentation"]["results"]["stego_cluster"]["pseudo_segs_pred"],
                       a["results"]["stego_cluster"]["pseudo_segs_pred"])


def test_install_native_head_builds_this_packages_head(monkeypatch):
    """install(native_head=True) makes make_model build this package's SemanticHead; the
    default keeps the reference's make_downstream_head."""
    import sys
    import types
    from scenedino_amd import dropin, models as amd_models
    from scenedino_amd.models import backbones
    from scenedino_amd.downstream_head import SemanticHead
    flags = (dropin._NATIVE_ENCODER, dropin._TRAIN_DECODER, dropin._TRAIN_ENCODER, dropin._NATIVE_HEAD)
    try:
        ref = types.ModuleType("scenedino.downstream_head")
        ref.make_downstream_head = lambda conf: "reference head"
        monkeypatch.setitem(sys.modules, "scenedino.downstream_head", ref)
        monkeypatch.setattr(backbones, "make_backbone", lambda conf: torch.nn.Identity())
        monkeypatch.setattr(amd_models, "make_model",
                            lambda config, dconf, encoder, downstream_head: downstream_head)
        conf = dict(so.HEAD_ARGS, type="segmentation", mode="3d")
        assert dropin._NATIVE_HEAD is False
        assert dropin._ref_make_model({"encoder": {}}, conf) == "reference head"
        dropin._NATIVE_HEAD = True
        head = dropin._ref_make_model({"encoder": {}}, conf)
        assert isinstance(head, SemanticHead) and head.mode == "3d" and head.buffer_size == 8
        assert hasattr(head, "forward_training")
        assert dropin._ref_make_model({"encoder": {}}, None) is None
    finally:
        (dropin._NATIVE_ENCODER, dropin._TRAIN_DECODER, dropin._TRAIN_ENCODER, dropin._NATIVE_HEAD) = flags
    import inspect
    assert inspect.signature(dropin.install).parameters["native_head"].default is False


# ------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["3d", "2d"])
def test_native_path_matches_the_reference_fixture(gpu, mode):
    fx = _fixture()
    got = _two_steps(mode, gpu)
    f16 = _cpu_steps(mode, True)
    keys = _float_keys(mode)
    shaped = {k: got[k].reshape(fx[k].shape) for k in keys}
    shaped16 = {k: f16[k].reshape(fx[k].shape) for k in keys}
    so.check(shaped, {k: fx[k].reshape(fx[k].shape) for k in keys}, shaped16, keys, what=mode)
    _labels_match(got, mode)


@pytest.mark.gpu
def test_dropout_masks_against_the_oracle_formulas(gpu):
    """Injected masks (p = 0.1 scales) in mode 3d: the self / kNN / random codes, the image
    codes and both cluster losses against tests/_stego_oracle.py's formulas on the CPU."""
    import torch.nn.functional as F
    head = _head("3d", gpu, p=0.1)
    seed = so.HEAD_SEEDS["3d"]
    g = torch.Generator().manual_seed(99)
    st = so.head_state(seed)
    W = [st["stego_head." + n] for n in so.STEGO_NAMES]
    prev = None
    for step in range(2):
        data, nc = so.head_step_inputs(seed, step, "3d")
        draws = {"dino": so.dropout_scales(2, 768, g), "img_lin": so.dropout_scales(2, 64, g),
                 "img_non": so.dropout_scales(2, 64, g), "crop": so.dropout_scales(nc, 768, g),
                 "nn_pick": torch.randint(2, (nc,), generator=g),
                 "random_idx": torch.randint(3 * (step + 1), (nc,), generator=g)}
        for k in ("self", "nn", "random"):
            draws[k + "_lin"] = so.dropout_scales(nc, 64, g)
            draws[k + "_non"] = so.dropout_scales(nc, 64, g)
        head._draws = draws
        out = head.forward_training(_to(data, gpu))["segmentation"]

        # the same step in torch ops on the CPU
        crop = F.normalize(data["sample_surface_dino_features"][0], dim=-1, eps=1e-10) * draws["crop"][:, None]
        patches = crop if prev is None else torch.cat([prev, crop])
        gaps = F.normalize(patches.mean(1), dim=-1, eps=1e-10)
        buf = torch.zeros(8, 768)
        buf[:gaps.shape[0]] = gaps
        top = torch.topk(gaps[-nc:] @ buf.t(), 3, dim=1)[1][:, 1:]
        nn_rows = torch.cat([patches, torch.zeros(8 - patches.shape[0], 16, 768)])[
            top[torch.arange(nc), draws["nn_pick"]]]
        rnd_rows = patches[draws["random_idx"]]
        prev = patches

        def codes(rows, name):
            return so.stego_formula(rows.reshape(-1, 768), *W, draws[name + "_lin"], draws[name + "_non"],
                                    16, normalize=False).view(nc, 16, 64)

        def corr(a, b):
            return torch.einsum("npf,nqf->npq", F.normalize(a, dim=-1, eps=1e-10),
                                F.normalize(b, dim=-1, eps=1e-10))

        def cpu(autocast):
            with torch.autocast("cpu", dtype=so.BF, enabled=autocast):
                s, n_, r = codes(crop, "self"), codes(nn_rows, "nn"), codes(rnd_rows, "random")
                img = data["coarse"][0]["dino_features"].reshape(-1, 768)
                y = so.stego_formula(img, *W, draws["img_lin"], draws["img_non"], 512)
                ref = {"dino_nn_corr": corr(crop, nn_rows), "stego_self_corr": corr(s, s),
                       "stego_nn_corr": corr(s, n_), "stego_random_corr": corr(s, r)}
                dl, lab = so.kmeans_loss(img, st["direct_cluster_head.cluster_centers"], m=draws["dino"],
                                         rows_per_group=512)
                sl, _ = so.kmeans_loss(y.float(), st["stego_cluster_head.cluster_centers"])
                sc = so.probe_xhat(img, draws["dino"], 512) @ F.normalize(
                    st["direct_cluster_head.cluster_centers"], dim=1).t()
            ref.update(direct_loss=dl.view(1), stego_loss=sl.view(1))
            top = sc.float().topk(2, dim=1).values
            return {k: v.detach().float() for k, v in ref.items()}, lab, top[:, 0] - top[:, 1] > 2e-2

        f32, lab, wide = cpu(False)
        f16 = cpu(True)[0]
        native = {k: out["stego_corr"][k].detach() for k in f32 if k.endswith("corr")}
        native["direct_loss"] = out["results"]["direct_cluster"]["loss"].detach().view(1)
        native["stego_loss"] = out["results"]["stego_cluster"]["loss"].detach().view(1)
        so.check(native, f32, f16, tuple(f32), what=f"dropout step {step}")
        got = out["results"]["direct_cluster"]["pseudo_segs_pred"].flatten().cpu()
        assert float(wide.float().mean()) >= 0.95 and torch.equal(got[wide], lab[wide])


@pytest.mark.gpu
def test_eval_mode_leaves_the_buffers_untouched(gpu):
    head = _head("3d", gpu, p=0.1)
    head.forward_training(_to(so.head_step_inputs(11, 0, "3d")[0], gpu))
    assert head.dino_patch_buffer.is_cuda and head.buffer_idx == 3
    state = (head.buffer_idx, head.buffer_filled, head.dino_patch_buffer.clone(), head.dino_gap_buffer.clone())
    head.eval()
    d1 = head.forward_training(_to(so.head_step_inputs(11, 1, "3d")[0], gpu))["segmentation"]
    d2 = head.forward_training(_to(so.head_step_inputs(11, 1, "3d")[0], gpu))["segmentation"]
    assert (head.buffer_idx, head.buffer_filled) == state[:2]
    assert torch.equal(head.dino_patch_buffer, state[2]) and torch.equal(head.dino_gap_buffer, state[3])
    # no masks in eval mode: the same labels and self correlation twice
    assert torch.equal(d1["results"]["stego_cluster"]["pseudo_segs_pred"],
                       d2["results"]["stego_cluster"]["pseudo_segs_pred"])
    assert torch.equal(d1["stego_corr"]["stego_self_corr"], d2["stego_corr"]["stego_self_corr"])


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
def test_predict_voxels_sees_the_stepped_head(gpu, fused):
    """train step -> predict_voxels -> step -> predict_voxels: the folded sd_seg_query record
    follows the stego weights and the centres through Adam steps (a fused step bumps no
    version counter)."""
    from _helpers import build_net, load
    from test_seg import modules_from, seg_params
    from scenedino_amd import _lib
    from scenedino_amd.losses import StegoLoss
    from scenedino_amd.seg_pack import PackedSegHead
    fq = load("field_query.npz")
    net = build_net(fq["grid"], fq["W_in"], fq["b_in"], fq["W_out"], fq["b_out"], "fp32", gpu)
    dr = modules_from(seg_params(load("seg_head.npz"), "_768"))[0].to(gpu)
    head = _head("3d", gpu)
    net.encoder.dim_reduction, net.downstream_head, net.gt_classes = dr, head, 19
    Tn = lambda k: torch.as_tensor(fq[k]).to(gpu)  # noqa: E731
    net.encode(Tn("images"), Tn("Ks"), Tn("poses"), ids_encoder=[0], ids_render=[0])
    xyz = Tn("xyz")
    opt = torch.optim.Adam([{"params": list(p), "lr": 0.01 * f} for f, p in head.parameters_lr()],
                           fused=fused)
    loss_fn = StegoLoss(dict(so.STEGO_LOSS, pointwise=False))
    seen = []
    for step in range(2):
        data = head.train().forward_training(_to(so.head_step_inputs(11, step, "3d")[0], gpu))
        opt.zero_grad(set_to_none=True)
        loss_fn(data)["total_loss"].backward()
        if step == 0:
            with torch.no_grad():
                seen.append(net.predict_voxels(xyz)[1].clone())  # packs of the initial weights
        opt.step()
        assert head._step_gen == step + 1 and head.stego_head._step_gen == step + 1
        with torch.no_grad():
            sigma, seg = net.predict_voxels(xyz)
            dino = net.query(xyz, colors=False, dino_dtype=torch.bfloat16)[1]
            fresh = PackedSegHead(dr, head.stego_head, head.stego_cluster_head)
            want = _lib.seg_query(dino.reshape(sigma.numel(), -1), fresh.rec, sigma=sigma,
                                  voxel_size=0.2, want_labels=False, want_seg=True)[1]
        assert torch.equal(seg, want), step
        seen.append(seg.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
