"""Supersampled SSCBench query on the CPU (no GPU): sscbench.pool_voxels' torch route against
the reference's own downsample_and_predict (tests/golden/ssc_pool.npz, from
tests/golden/make_golden_ssc_pool.py), the pooling rules on hand-built voxels, the argument
checks, the unchanged factor-1 path, chunk invariance of query_voxels and the x-slab halo at
factor 2 over gloo."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _ssc_pool_oracle as PO
from _helpers import load
from scenedino_amd import sscbench


def _grow(t):
    return F.max_pool3d(t.unsqueeze(0), 3, 1, 1).squeeze(0)


def _embedded_predict(sigma_in, label_in, dims, f):
    """predict(points) over a zero fine grid of coarse ``dims`` with the recorded corner in it;
    the points are the fine flat indices."""
    sig = torch.zeros(tuple(f * d for d in dims))
    lab = torch.zeros(tuple(f * d for d in dims), dtype=torch.uint8)
    n = sigma_in.shape
    sig[:n[0], :n[1], :n[2]] = torch.as_tensor(sigma_in)
    lab[:n[0], :n[1], :n[2]] = torch.as_tensor(label_in)
    # alpha > 0 <=> sigma > 0 for the recorded values: predict_voxels' per-point seg
    lab = torch.where(sig > 0, lab, torch.zeros_like(lab))
    sig, lab = sig.reshape(-1), lab.reshape(-1)

    def predict(p):
        i = p[:, 0].long()
        return sig[i], lab[i]
    return predict


def _index_points(dims, f):
    n = int(np.prod(dims)) * f ** 3
    return torch.arange(n, dtype=torch.float32).view(n, 1).expand(n, 3)


@pytest.mark.parametrize("f", [2, 4])
def test_torch_route_matches_the_reference_function(f):
    d = load("ssc_pool.npz")
    sigma_in, label_in = torch.as_tensor(d[f"f{f}_sigma_in"]), torch.as_tensor(d[f"f{f}_label_in"])
    sig, seg = sscbench.pool_voxels(sigma_in, label_in, f, 0.2 / f)
    assert seg.dtype == torch.uint8 and sig.dtype == torch.float32
    assert torch.equal(seg, torch.as_tensor(d[f"f{f}_segs"]))
    # the whole driver on a (10, 10, 32) coarse grid: pooled, then grown
    dims = (10, 10, 32)
    sigmas, segs = sscbench.query_voxels(None, _index_points(dims, f), dims, factor=f,
                                         predict=_embedded_predict(sigma_in, label_in, dims, f),
                                         grow_fn=_grow, max_points=3 * f ** 3 * 320)
    want = torch.as_tensor(d[f"f{f}_sigmas"])
    assert torch.equal(sigmas[:9, :9].view(torch.int32), want.view(torch.int32))
    assert float(sigmas[9:].abs().sum() + sigmas[:, 9:].abs().sum()) == 0.0
    assert torch.equal(segs[:8, :8], torch.as_tensor(d[f"f{f}_segs"]))
    assert int(segs[8:].sum() + segs[:, 8:].sum()) == 0
    assert float(d[f"f{f}_sigmas_rest"]) == 0.0 and float(d[f"f{f}_segs_rest"]) == 0.0


def test_vis_grids_match_the_reference_function():
    d = load("ssc_pool.npz")
    f, dims = 2, (10, 10, 32)
    sigma_in, label_in = d["f2_sigma_in"], d["f2_label_in"]
    sigmas, segs = sscbench.query_voxels(None, _index_points(dims, f), dims, factor=f, pooled=False,
                                         predict=_embedded_predict(sigma_in, label_in, dims, f),
                                         grow_fn=_grow, max_points=2 * f ** 3 * 320)
    assert sigmas.shape == (20, 20, 64) and segs.shape == (20, 20, 64)
    want = torch.as_tensor(d["vis2_sigmas"])
    assert torch.equal(sigmas[:17, :17].view(torch.int32), want.view(torch.int32))
    assert torch.equal(segs[:16, :16], torch.as_tensor(d["vis2_segs"]))
    assert int(segs[16:].sum() + segs[:, 16:].sum()) == 0


@pytest.mark.parametrize("f", [2, 4, 8])
def test_hand_built_voxels(f):
    sigma, label, ncls, want, want_sigma = PO.hand_built(f)
    sig, seg = sscbench.pool_voxels(torch.as_tensor(sigma), torch.as_tensor(label), f, 0.1, ncls)
    assert seg.reshape(-1).tolist() == want.tolist()
    np.testing.assert_array_equal(sig.reshape(-1).numpy(), want_sigma)  # NaN == NaN here


@pytest.mark.parametrize("dims,f,ncls,seed", PO.CASES[:4])
def test_torch_route_matches_the_f64_oracle(dims, f, ncls, seed):
    sigma, label = PO.make_inputs(dims, f, ncls, seed)
    sig, seg = sscbench.pool_voxels(torch.as_tensor(sigma), torch.as_tensor(label), f, 0.2 / f, ncls)
    _, labels, margin, smax = PO.oracle(sigma, label, f, 0.2 / f, ncls)
    clear = margin > PO.MARGIN
    assert 1.0 - clear.mean() <= PO.MAX_EXCLUDED
    assert (seg.numpy() == labels)[clear].all()
    np.testing.assert_array_equal(sig.numpy(), smax)


def test_rejections():
    s, l = torch.zeros(16, 16, 16), torch.zeros(16, 16, 16, dtype=torch.uint8)
    for f in (3, 16, 1):
        with pytest.raises(ValueError):
            sscbench.pool_voxels(s, l, f, 0.1)
    with pytest.raises(ValueError, match="share one"):
        sscbench.pool_voxels(s[:6], l[:6], 4, 0.05)
    with pytest.raises(ValueError, match="domain"):
        sscbench.pool_voxels(s, l, 2, 0.1, native=True)  # CPU tensors
    for f in (3, 16):
        with pytest.raises(ValueError, match="factor"):
            sscbench.query_voxels(None, torch.zeros(8, 3), (1, 1, 1), factor=f,
                                  predict=lambda p: (p[:, 0], p[:, 0]))
        with pytest.raises(ValueError, match="factor"):
            sscbench.downsample_and_predict({}, None, torch.zeros(8, 3), f, "stego_kmeans")
    for f in (1, 2):
        with pytest.raises(NotImplementedError, match="feat_vis"):
            sscbench.downsample_and_predict({}, None, torch.zeros(8, 3), f, "stego_kmeans",
                                            vis=True, feat_vis=True)
    with pytest.raises(ValueError, match="fine voxel centres"):
        sscbench.query_voxels(None, torch.zeros(9, 3), (1, 1, 1), factor=2,
                              predict=lambda p: (p[:, 0], p[:, 0]))


def test_library_exports_the_entry_point_without_an_abi_bump():
    from scenedino_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "sd_ssc_pool") and "sd_ssc_pool" in _lib.SIGNATURES
    assert lib.sd_abi_version() == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "include",
                               "sdhip_ssc_pool.h")).read()
    assert "int sd_ssc_pool(" in header
    assert f"#define SD_SSC_POOL_MAX_CLASSES {_lib.SSC_POOL_MAX_CLASSES}" in header
    # argument checks come before any device call: they answer on a machine without a GPU
    for factor, ncls in ((3, 19), (16, 19), (2, 0), (2, 33)):
        assert lib.sd_ssc_pool(16, 16, 1, 1, 1, factor, 0.1, ncls, 32, 48, None) == -1
        assert b"sd_ssc_pool" in lib.sd_last_error()
    assert lib.sd_ssc_pool(None, None, 1, 1, 1, 2, 0.1, 19, None, None, None) == -1


class _RecordingNet:
    """Stands in for an encoded BTSNet: records how the voxel query was made."""

    def __init__(self):
        self.calls = []

    def compute_grid_transforms(self, *a, **k):
        pass

    def encode(self, *a, **k):
        pass

    def set_scale(self, *a):
        pass

    def predict_voxels(self, xyz, voxel_size=0.2, prediction_mode="stego_kmeans"):
        self.calls.append((tuple(xyz.shape), voxel_size, prediction_mode))
        p = xyz.reshape(-1, 3)
        sig = F.softplus(4 * torch.sin(p[:, 0] * 0.37) + p[:, 1] * 0.01) * (p[:, 2] % 3 != 0)
        seg = ((p[:, 0] * 5 + p[:, 1] * 3 + p[:, 2]).long() % 19).to(torch.uint8)
        return sig, torch.where(sig > 0, seg, torch.zeros_like(seg))


def test_factor_1_takes_the_unchanged_path(monkeypatch):
    """factor 1: one predict_voxels call over all points at voxel_size 0.2, one grow, the
    return types of the evaluator -- with or without ``vis``."""
    grown = []

    def grow3(t):
        grown.append(tuple(t.shape))
        return _grow(t)
    monkeypatch.setattr(sscbench._lib, "grow3", grow3)
    monkeypatch.setattr(sscbench, "pool_voxels", None)  # must not be reached
    data = {"imgs": [torch.zeros(3, 4, 4)], "poses": [np.eye(4, dtype=np.float32)],
            "projs": [np.eye(3, dtype=np.float32)]}
    n = 256 * 256 * 32
    pts = torch.arange(n, dtype=torch.float32).view(n, 1).expand(n, 3)
    for vis in (False, True):
        net = _RecordingNet()
        sig, seg, dino = sscbench.downsample_and_predict(data, net, pts, 1, "stego_kmeans", vis=vis)
        assert net.calls == [((1, n, 3), 0.2, "stego_kmeans")] and dino is None
        assert sig.dtype == np.float32 and seg.dtype == np.float64
        assert sig.shape == (256, 256, 32) and seg.shape == (256, 256, 32)
        rs, rg = net.predict_voxels(pts.reshape(1, -1, 3))
        assert np.array_equal(sig, _grow(rs.reshape(256, 256, 32)).numpy())
        assert np.array_equal(seg, rg.reshape(256, 256, 32).numpy().astype(np.float64))
    assert grown == [(256, 256, 32)] * 2
    # query_voxels itself, defaults untouched
    net = _RecordingNet()
    s1, g1 = sscbench.query_voxels(net, pts[:4 * 3 * 2], (4, 3, 2))
    assert net.calls == [((1, 24, 3), 0.2, "stego_kmeans")] and s1.shape == (4, 3, 2)


def _standin(f, dims):
    """predict(points = fine flat indices) with sigma >= 0 (30 % zeros) and labels 0..18."""
    sigma, label = PO.make_inputs(dims, f, 19, 11)
    sig, lab = torch.as_tensor(sigma).reshape(-1), torch.as_tensor(label).reshape(-1)
    lab = torch.where(sig > 0, lab, torch.zeros_like(lab))
    return (lambda p: (sig[p[:, 0].long()], lab[p[:, 0].long()])), sig, lab


def test_query_voxels_is_chunk_invariant():
    dims, f = (6, 5, 3), 2
    predict, sig, lab = _standin(f, dims)
    pts = _index_points(dims, f)
    plane = f ** 3 * dims[1] * dims[2]
    fine = tuple(f * d for d in dims)
    # unchunked statement: pool the whole fine grid, then grow
    ws, wg = sscbench.pool_voxels(sig.reshape(fine), lab.reshape(fine), f, 0.1)
    ws = _grow(ws)
    sizes = []

    def counting(p):
        sizes.append(p.shape[0])
        return predict(p)
    for max_points, want_sizes in ((plane, [plane] * 6), (3 * plane + 5, [3 * plane] * 2),
                                   (1, [plane] * 6), (None, [6 * plane])):
        sizes.clear()
        s, g = sscbench.query_voxels(None, pts, dims, factor=f, predict=counting, grow_fn=_grow,
                                     max_points=max_points)
        assert sizes == want_sizes, max_points
        assert torch.equal(s, ws) and torch.equal(g, wg) and g.dtype == torch.uint8
        # vis contract: per-point results, grow on the fine grid
        s, g = sscbench.query_voxels(None, pts, dims, factor=f, predict=predict, grow_fn=_grow,
                                     max_points=max_points, pooled=False)
        assert torch.equal(s, _grow(sig.reshape(fine))) and torch.equal(g, lab.reshape(fine))
    s, g = sscbench.query_voxels(None, pts, dims, factor=f, predict=predict, grow=False)
    assert torch.equal(g, wg) and not torch.equal(s, ws)


def test_default_point_budget_keeps_a_chunk_of_codes_well_under_1_gb():
    assert sscbench.MAX_POINTS * 64 * 2 <= (1 << 30) // 4
    assert sscbench.MAX_POINTS // (8 * 256 * 32) == 32   # coarse planes per chunk at factor 2
    assert sscbench.MAX_POINTS // (64 * 256 * 32) == 4   # ... at factor 4


# ------------------------------------------------------------------ slabs over gloo
def _slab_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dims, f = (16, 6, 5), 2
        predict, sig, lab = _standin(f, dims)
        pts = _index_points(dims, f)
        plane = f ** 3 * dims[1] * dims[2]
        s, g = sscbench.query_voxels_slab(predict, pts, dims, rank, world, grow_fn=_grow, factor=f,
                                          max_points=4 * plane)
        full_s, full_g = sscbench.gather_slabs(s, g, dims)
        fine = tuple(f * d for d in dims)
        ws, wg = sscbench.pool_voxels(sig.reshape(fine), lab.reshape(fine), f, 0.1)
        ok = torch.equal(full_s, _grow(ws)) and torch.equal(full_g, wg)
        dist.barrier()
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def test_supersampled_slabs_gloo_world2_equal_unsharded():
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_slab_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    assert dict(q.get(timeout=10) for _ in range(2)) == {0: True, 1: True}


def test_point_grid_dims_of_the_fine_voxel_sizes():
    rec = __import__("json").load(open(os.path.join(os.path.dirname(__file__), "golden",
                                                    "voxel_points_fine.json")))
    for vs, f in (("0.1", 2), ("0.05", 4)):
        assert list(sscbench.grid_dims(voxel_size=float(vs))) == rec[vs]["dims"] == [256 * f, 256 * f, 32 * f]
        assert int(0.2 // float(vs)) == f  # the evaluator's downsample_factor
