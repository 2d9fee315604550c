"""CPU: the 3-D crop sampler (scenedino_amd/training/crop3d.py) in torch ops against
tests/golden/crop3d.npz, the reference's own ``BTSDownstreamWrapper.sample_3d_crop`` run by
tests/golden/make_golden_crop3d.py on the inputs of tests/_crop3d_inputs.py; the edges of the
draws; the C ABI's declarations; and ``dropin.install(native_crops=True)``."""
import importlib
import os
import sys
import textwrap

import numpy as np
import pytest
import torch

import _crop3d_inputs as ci
from conftest import GOLDEN, ROOT

CASES = list(ci.CASES)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "crop3d.npz"), allow_pickle=False)


def _case(golden, name):
    return {k[len(name) + 1:]: torch.as_tensor(golden[k]) for k in golden.files
            if k.startswith(name + "_")}


def _run(c, **kw):
    from scenedino_amd.training import crop3d
    args = dict(z_far=ci.Z_FAR, n_crops=ci.N_CROPS, n_samples=ci.N_SAMPLES,
                sample_radius=ci.RADIUS, sigma_threshold=ci.THR, oversampling=ci.OVERSAMPLING,
                draws={"pick": c["pick"], "shift": c["shift"]})
    args.update(kw)
    return crop3d._sample_3d_crop_padded(ci.StandInNet(), c["poses"], c["projs"], c["depth"], **args)


def _ulps(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


@pytest.mark.parametrize("name", CASES)
def test_torch_route_matches_the_reference(golden, name):
    c = _case(golden, name)
    n = c["pick"].shape[0]
    assert ci.limits_are_robust(c["depth"][:, 0].numpy(), c["limits"].numpy())
    dino, occ, n_valid, aux = _run(c)
    assert torch.equal(aux["count"].long(), c["count"].long())
    assert torch.equal(aux["pixel"].long(), c["pixel"].long())
    assert _ulps(aux["limits"].numpy(), c["limits"].numpy()).max() <= 1
    # the positions handed to the net: the reference stacks the non-empty bins only
    filled = c["count"][0] > 0
    assert torch.equal(c["count"] > 0, filled.expand(n, -1))
    mine = aux["points"][:, filled]
    assert mine.shape == c["positions"].shape
    # two f32 roundings at 80 m are 1e-5 m
    assert float((mine - c["positions"]).abs().max()) <= 2e-5
    assert torch.equal(aux["points"][:, ~filled], torch.zeros_like(aux["points"][:, ~filled]))
    # which crops are kept, their order and the returned shapes
    sigma_ref, codes_ref = ci.StandInNet.field(c["positions"])
    kept_ref = torch.zeros(n, ci.N_CROPS, dtype=torch.bool)
    kept_ref[:, filled] = (sigma_ref > ci.THR).sum(-1) > ci.N_SAMPLES
    assert torch.equal(aux["slot"] >= 0, kept_ref.reshape(-1))
    k = int(n_valid)
    assert k == c["dino"].shape[1] == int(kept_ref.sum())
    assert torch.equal(aux["slot"][aux["slot"] >= 0], torch.arange(k, dtype=torch.int32))
    assert dino.shape == (n * ci.N_CROPS, ci.N_SAMPLES, 64) and occ.shape == dino.shape[:2]


@pytest.mark.parametrize("name", CASES)
def test_returned_arrays_at_the_stored_positions(golden, name):
    """The compaction and the occupancy on the stand-in evaluated at the reference's own
    positions: the reference's returned arrays."""
    from scenedino_amd.training import crop3d
    c = _case(golden, name)
    n = c["pick"].shape[0]
    filled = c["count"][0] > 0
    sigma = torch.zeros(n, ci.N_CROPS, ci.S)
    codes = torch.zeros(n, ci.N_CROPS, ci.S, 64)
    sigma[:, filled], codes[:, filled] = ci.StandInNet.field(c["positions"])
    # an empty bin with plenty of occupancy: crop_ok alone must drop it
    sigma[:, ~filled] = 1.0
    out, occ, n_valid, _ = crop3d.compact_torch(sigma.view(-1, ci.S), codes.view(-1, ci.S, 64),
                                                c["count"].reshape(-1).to(torch.int32), ci.THR,
                                                ci.N_SAMPLES)
    k = int(n_valid)
    assert (1, k, ci.N_SAMPLES, 64) == tuple(c["dino"].shape)
    assert (1, k, ci.N_SAMPLES, 1) == tuple(c["occ"].shape)
    torch.testing.assert_close(out[:k], c["dino"][0], rtol=1e-5, atol=0)
    torch.testing.assert_close(occ[:k], c["occ"][0, ..., 0], rtol=1e-5, atol=0)
    assert not out[k:].any() and not occ[k:].any()


def test_edge_case_counts(golden):
    """One crop with exactly n_samples occupied samples (dropped), one with n_samples + 1."""
    c = _case(golden, "edge")
    _, _, _, aux = _run(c)
    n_occ = (aux["sigma"] > ci.THR).sum(-1)
    assert n_occ[0] == ci.N_SAMPLES and n_occ[1] == ci.N_SAMPLES + 1
    assert aux["slot"][0] == -1 and aux["slot"][1] == 0


def test_public_function_matches_the_padded_one(golden):
    from scenedino_amd.training import sample_3d_crop
    c = _case(golden, "batch2")
    dino_p, occ_p, n_valid, _ = _run(c)
    dino, occ = sample_3d_crop(ci.StandInNet(), c["poses"], c["projs"], c["depth"], z_far=ci.Z_FAR,
                               n_crops=ci.N_CROPS, n_samples=ci.N_SAMPLES, sample_radius=ci.RADIUS,
                               sigma_threshold=ci.THR, oversampling=ci.OVERSAMPLING,
                               draws={"pick": c["pick"], "shift": c["shift"]})
    k = int(n_valid)
    assert dino.shape == c["dino"].shape and occ.shape == c["occ"].shape
    assert torch.equal(dino[0], dino_p[:k]) and torch.equal(occ[0, ..., 0], occ_p[:k])


def test_no_surviving_crop_returns_none(golden):
    from scenedino_amd.training import sample_3d_crop
    c = _case(golden, "full")
    out = sample_3d_crop(ci.StandInNet(), c["poses"], c["projs"], c["depth"], z_far=ci.Z_FAR,
                         n_crops=ci.N_CROPS, n_samples=ci.N_SAMPLES, sigma_threshold=10.0,
                         draws={"pick": c["pick"], "shift": c["shift"]})
    assert out == (None, None)


def test_default_draws_stay_in_the_ball(golden):
    from scenedino_amd.training import crop3d
    c = _case(golden, "full")
    torch.manual_seed(0)
    _, _, _, aux = crop3d._sample_3d_crop_padded(
        ci.StandInNet(), c["poses"], c["projs"], c["depth"], z_far=ci.Z_FAR, n_crops=ci.N_CROPS,
        n_samples=ci.N_SAMPLES, sample_radius=0.25)
    r = (aux["points"] - aux["centre"][:, :, None]).norm(dim=-1)
    assert float(r.max()) <= 0.25 * (1 + 1e-5) and float(r.max()) > 0.2


def test_frame_without_depth_below_z_far_loses_only_its_crops(golden):
    c = _case(golden, "batch2")
    c["depth"] = c["depth"].clone()
    c["depth"][0] = 150.0
    dino, occ, n_valid, aux = _run(c)
    assert not aux["count"][0].any() and aux["count"][1].all()
    assert (aux["pixel"][0] == -1).all() and (aux["slot"][:ci.N_CROPS] == -1).all()
    assert torch.isnan(aux["limits"][0]).all()
    alone = {k: v[1:] for k, v in c.items() if k in ("poses", "projs", "depth", "pick", "shift")}
    dino1, occ1, n1, aux1 = _run(alone)
    k = int(n_valid)
    assert k == int(n1) and k > 0
    assert torch.equal(dino[:k], dino1[:k]) and torch.equal(occ[:k], occ1[:k])
    assert torch.equal(aux["pixel"][1], aux1["pixel"][0])


@pytest.mark.parametrize("u, which", [(0.0, 0), (1.0 - 2.0 ** -24, -1)])
def test_draw_edges_pick_the_first_and_the_last_pixel(golden, u, which):
    c = _case(golden, "plateau")
    c["pick"] = torch.full_like(c["pick"], u)
    assert float(c["pick"].max()) < 1.0
    _, _, _, aux = _run(c)
    d = c["depth"][0, 0]
    w = d.shape[1]
    for i in range(ci.N_CROPS):
        inb = ((d > aux["limits"][0, i]) & (d < aux["limits"][0, i + 1])).flatten().nonzero()
        if len(inb) == 0:
            assert aux["pixel"][0, i].tolist() == [-1, -1]
            continue
        p = int(inb[which])
        assert aux["pixel"][0, i].tolist() == [p // w, p % w]


def test_abi_declares_the_crop_kernels():
    from scenedino_amd import _lib
    header = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    for name in ("sd_crop3d_centres", "sd_crop3d_compact"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 13
    from scenedino_amd import build
    assert "csrc/sdhip_crop3d.hip" in build.SOURCES


@pytest.fixture
def fake_reference(tmp_path, monkeypatch):
    """A stand-in ``scenedino`` checkout (the pattern of tests/test_dropin.py) with a downstream
    trainer module; ``request.param`` False leaves that module out."""
    root = tmp_path / "ref"
    files = {
        "scenedino/__init__.py": "",
        "scenedino/renderer/__init__.py": "from .nerf import NeRFRenderer\n",
        "scenedino/renderer/nerf.py": "class NeRFRenderer:\n    origin = 'reference'\n",
        "scenedino/models/__init__.py": "def make_model(config, downstream_config=None):\n    return 0\n",
        "scenedino/models/bts.py": "class BTSNet:\n    origin = 'reference'\n",
        "scenedino/common/__init__.py": "",
        "scenedino/common/ray_sampler.py": "class ImageRaySampler:\n    origin = 'reference'\n",
        "scenedino/training/__init__.py": "",
        "scenedino/training/trainer_downstream.py": textwrap.dedent("""
            class BTSDownstreamWrapper:
                def sample_3d_crop(self, poses, projs, depth, z_far=100, n_crops=5, n_samples=576,
                                   sample_radius=0.5, sigma_threshold=0.5):
                    return 'reference sample_3d_crop'
            """),
    }
    for rel, txt in files.items():
        f = root / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(txt)
    saved = {k: v for k, v in sys.modules.items() if k == "scenedino" or k.startswith("scenedino.")}
    for k in saved:
        del sys.modules[k]
    monkeypatch.syspath_prepend(str(root))
    yield root
    for k in [k for k in sys.modules if k == "scenedino" or k.startswith("scenedino.")]:
        del sys.modules[k]
    sys.modules.update(saved)


def test_install_native_crops_replaces_the_method(fake_reference, golden):
    import inspect
    import types
    from scenedino_amd import dropin
    dropin.install(native_crops=True)
    td = importlib.import_module("scenedino.training.trainer_downstream")
    fn = td.BTSDownstreamWrapper.sample_3d_crop
    assert fn is dropin._sample_3d_crop
    assert list(inspect.signature(fn).parameters) == [
        "self", "poses", "projs", "depth", "z_far", "n_crops", "n_samples", "sample_radius",
        "sigma_threshold"]
    # and it samples on self.renderer.net
    c = _case(golden, "full")
    me = td.BTSDownstreamWrapper()
    me.renderer = types.SimpleNamespace(net=ci.StandInNet())
    torch.manual_seed(0)
    dino, occ = me.sample_3d_crop(c["poses"], c["projs"], c["depth"], n_samples=ci.N_SAMPLES,
                                  sigma_threshold=0.2)
    assert dino.shape[2:] == (ci.N_SAMPLES, 64) and occ.shape == dino.shape[:3] + (1,)


def test_install_without_the_flag_leaves_the_method(fake_reference):
    from scenedino_amd import dropin
    dropin.install()
    td = importlib.import_module("scenedino.training.trainer_downstream")
    assert td.BTSDownstreamWrapper().sample_3d_crop(None, None, None) == "reference sample_3d_crop"


def test_install_native_crops_without_the_trainer_module(fake_reference):
    os.remove(fake_reference / "scenedino" / "training" / "trainer_downstream.py")
    from scenedino_amd import dropin
    dropin.install(native_crops=True)
    assert "scenedino.training.trainer_downstream" not in sys.modules
