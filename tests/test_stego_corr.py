"""CPU: the lazy correlation mapping of SemanticHead (``lazy_corr``), StegoLoss on it, the factored
pointwise centring the fused kernel uses, the C ABI of sd_stego_corr_* and the drop-in switch.
The GPU kernel itself is tested in tests/test_stego_corr_gpu.py."""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess
from collections.abc import Mapping

import numpy as np
import pytest
import torch

import _stego_corr_oracle as co
import _stego_oracle as so
from conftest import GOLDEN, ROOT
from test_dropin import fake_reference  # noqa: F401  (fixture: a stand-in scenedino package)
from test_semantic_head_train import CORR, SUB, _head, _to

STEGO_GRADS = tuple("stego_head." + n for n in so.STEGO_NAMES)


@functools.lru_cache(maxsize=None)
def _fixture():
    return {k: torch.as_tensor(np.asarray(v))
            for k, v in np.load(os.path.join(GOLDEN, "stego_train.npz")).items()}


def _step(head, mode, step):
    fx = _fixture()
    data, _ = so.head_step_inputs(so.HEAD_SEEDS[mode], step, mode)
    t = f"{mode}_{step}_"
    head._draws = {"nn_pick": fx[t + "nn_pick"], "random_idx": fx[t + "random_idx"]}
    return head.forward_training(_to(data, "cpu"), sample_factor=2 if mode == "2d" else 4)


@pytest.mark.parametrize("mode", ["3d", "2d"])
def test_lazy_mapping_materialises_the_eager_tensors(mode):
    from scenedino_amd.downstream_head.semantic_head import StegoCorrMap
    eager, lazy = _head(mode, "cpu"), _head(mode, "cpu")
    assert eager.lazy_corr is False
    lazy.lazy_corr = True
    for step in range(2):
        want = _step(eager, mode, step)["segmentation"]["stego_corr"]
        got = _step(lazy, mode, step)["segmentation"]["stego_corr"]
        assert type(want) is dict and isinstance(got, StegoCorrMap) and isinstance(got, Mapping)
        assert list(got) == list(want) == list(CORR) and len(got) == 6
        assert got.materialised == ()
        for k in CORR:
            assert torch.equal(got[k], want[k]), k
            assert got[k] is got[k]  # cached
        assert set(got.materialised) == set(CORR)
        assert got["stego_nn_corr"].requires_grad and not got["dino_nn_corr"].requires_grad
        with pytest.raises(KeyError):
            got["dino_other_corr"]
        with pytest.raises(TypeError):
            got["dino_self_corr"] = 0


@pytest.mark.parametrize("pointwise", [False, True])
def test_the_reference_loss_formula_runs_on_the_mapping(pointwise):
    """scenedino/losses/stego_loss.py:40-46,71-79 restated, in-place row-mean removal included:
    on the mapping it gives the eager dict's numbers and leaves the operand rows alone."""
    eager, lazy = _head("3d", "cpu"), _head("3d", "cpu")
    lazy.lazy_corr = True
    want = _step(eager, "3d", 0)["segmentation"]["stego_corr"]
    got = _step(lazy, "3d", 0)["segmentation"]["stego_corr"]
    rows = [t.detach().clone() for t in got.dino + got.stego]
    w = so.STEGO_LOSS

    def reference(c):
        return [co.reference_pair_loss(c[f"dino_{p}_corr"], c[f"stego_{p}_corr"], w[f"{n}_weight"],
                                       w[f"{n}_shift"], pointwise)
                for p, n in (("self", "self"), ("nn", "knn"), ("random", "random"))]

    for a, b in zip(reference(got), reference(want)):
        assert torch.equal(a, b)
    for before, after in zip(rows, got.dino + got.stego):
        assert torch.equal(before, after.detach())
    if pointwise:  # the quirk did edit the cached tensor
        assert not torch.equal(got["dino_nn_corr"], lazy._compute_stego_correlation(got.dino[0], got.dino[1]))


@pytest.mark.parametrize("case", ["random", "zero_row", "ragged"])
def test_factored_pointwise_form_equals_the_reference_op_sequence(case):
    P, Q = (24, 24) if case != "ragged" else (40, 17)
    rows = co.make_rows(3, P, Q, 384, n_pairs=2, self_pair=False, zero_rows=case == "zero_row")
    A, B = rows["A"].double(), rows["Bs"][0].double()
    if case == "zero_row":
        B[1, 3] = 0.0
    a, b = rows["a"].double(), rows["bs"][0].double()
    S = co.corr(a, b)
    for shift in (0.0, 0.43610463774158115):
        ref = co.reference_pair_loss(co.corr(A, B), S, 0.7, shift, True)
        fac = (-0.7 * S.clamp(0) * (co.factored_dino(A, B) - shift)).mean()
        assert bool(torch.isfinite(fac)) and abs(float(ref - fac)) <= 1e-12
    Dref = co.corr(A, B)
    old = Dref.mean()
    Dref -= Dref.mean(dim=-1, keepdim=True)
    Dref = Dref - Dref.mean() + old
    assert float((Dref - co.factored_dino(A, B)).abs().max()) <= 1e-12


@pytest.mark.parametrize("mode", ["3d", "2d"])
def test_loss_on_the_lazy_mapping_reproduces_the_reference_fixture(mode):
    """Both recorded steps with lazy_corr = True: StegoLoss (torch route on the CPU) gives the
    fixture's totals and stego parameter gradients, at the eager path's tolerances."""
    from scenedino_amd.losses import StegoLoss
    fx = _fixture()
    head = _head(mode, "cpu")
    head.lazy_corr = True
    for step in range(2):
        data = _step(head, mode, step)
        loss_fn = StegoLoss(dict(so.STEGO_LOSS, pointwise=False))
        total = loss_fn(data)["total_loss"]
        assert loss_fn.last_route == "torch"
        t = f"{mode}_{step}_"
        torch.testing.assert_close(total.detach(), fx[t + "total"], rtol=1e-4, atol=1e-6)
        if step == 1:
            head.zero_grad(set_to_none=True)
            total.backward()
            for name in STEGO_GRADS:
                p = head.get_parameter(name)
                g = p.grad.reshape(p.shape[0], -1) if p.dim() == 4 else p.grad
                g = g[SUB[name]] if name in SUB else g
                torch.testing.assert_close(g, fx[f"{mode}_grad_{name}"].reshape(g.shape), rtol=1e-4,
                                           atol=1e-6, msg=name)
        pw = StegoLoss(dict(so.STEGO_LOSS, pointwise=True))(data)["total_loss"]
        torch.testing.assert_close(pw.detach(), fx[t + "total_pointwise"], rtol=1e-4, atol=1e-6)


def test_loss_without_stego_corr_and_metric_names_are_unchanged():
    from scenedino_amd.losses import StegoLoss
    loss_fn = StegoLoss(dict(so.STEGO_LOSS))
    zero = torch.zeros(())
    data = {"segmentation": {"results": {"direct_cluster": {"loss": zero + 1.0},
                                         "stego_cluster": {"loss": zero + 2.0}}}}
    out = loss_fn(data)
    assert list(out) == loss_fn.get_loss_metric_names() == [
        "total_loss", "self_loss", "knn_loss", "random_loss", "direct_cluster_loss",
        "direct_linear_loss", "stego_cluster_loss", "stego_linear_loss"]
    assert out["self_loss"] == 0 and out["knn_loss"] == 0 and out["random_loss"] == 0
    assert float(out["total_loss"]) == 3.0 and loss_fn.last_route is None
    assert StegoLoss.fused_domain({"dino_self_corr": zero}) is not None


# ------------------------------------------------------------------------ C ABI and install
def test_entry_points_are_exported_and_reject_bad_arguments():
    from scenedino_amd import _lib
    lib = _lib.load()
    for n in ("sd_stego_corr_work", "sd_stego_corr_fwd", "sd_stego_corr_bwd"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert hasattr(_lib, "SdStegoCorrArgs")
    n = lib.sd_stego_corr_work(2, 80, 48, 768, 3, 1)
    assert n > 2 * (80 + 2 * 48) * 768 * 2 and n % 256 == 0
    assert lib.sd_stego_corr_work(2, 80, 48, 768, 3, 0) > n
    for bad in ((2, 80, 48, 512, 3, 1), (2, 0, 48, 768, 3, 1), (2, 80, 4097, 768, 3, 1),
                (0, 80, 48, 768, 3, 1), (2, 80, 48, 768, 4, 1)):
        assert lib.sd_stego_corr_work(*bad) == -1 and b"sd_stego_corr_work" in lib.sd_last_error()
    ok = dict(dino_a=256, stego_a=256, nc=2, P=24, Q=24, d=384, code_dim=64, n_pairs=1,
              dino_dtype=_lib.SD_F32, work=256, work_bytes=1 << 30, loss=256, up=256)
    for fn in (lib.sd_stego_corr_fwd, lib.sd_stego_corr_bwd):
        assert fn(None, None) == -1
        for change in (dict(d=512), dict(code_dim=32), dict(P=0), dict(dino_dtype=_lib.SD_F16),
                       dict(n_pairs=0), dict(dino_a=None), dict(work=None), dict(work_bytes=64),
                       dict(stego_a=260)):
            rc = fn(ctypes.byref(_lib.SdStegoCorrArgs(**dict(ok, **change))), None)
            assert rc == -1 and b"sd_stego_corr" in lib.sd_last_error(), change
    half = _lib.SdStegoCorrArgs(**ok)
    half.dino_b[0] = 256  # partner DINO rows without partner code rows
    assert lib.sd_stego_corr_fwd(ctypes.byref(half), None) == -1


def test_args_struct_layout_matches_the_c_header(tmp_path):
    from scenedino_amd import _lib
    py, cname = _lib.SdStegoCorrArgs, "sd_stego_corr_args"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sdhip.h"', "int main(void){",
             f'printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in
               subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(py) == int(got["size"])
    for fname, _ in py._fields_:
        assert getattr(py, fname).offset == int(got[fname]), fname


def test_install_sets_lazy_corr_only_with_both_switches(fake_reference, monkeypatch):  # noqa: F811
    from scenedino_amd import dropin, models as amd_models
    from scenedino_amd.downstream_head import SemanticHead
    from scenedino_amd.models import backbones
    monkeypatch.setattr(backbones, "make_backbone", lambda conf: torch.nn.Identity())
    monkeypatch.setattr(amd_models, "make_model",
                        lambda config, dconf, encoder, downstream_head: downstream_head)
    conf = dict(so.HEAD_ARGS, type="segmentation", mode="3d")
    try:
        dropin.install(native_head=True, native_loss=True)
        head = dropin._ref_make_model({"encoder": {}}, conf)
        assert isinstance(head, SemanticHead) and head.lazy_corr is True
        dropin.install(native_head=True)
        assert dropin._ref_make_model({"encoder": {}}, conf).lazy_corr is False
        dropin.install(native_loss=True)
        assert dropin._LAZY_CORR is False
    finally:
        dropin.install()
    assert dropin._LAZY_CORR is False and SemanticHead(**so.HEAD_ARGS).lazy_corr is False
