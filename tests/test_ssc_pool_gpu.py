"""sd_ssc_pool and the supersampled SSCBench query on the GPU.

What must agree (written here, before the first run):
  * sigma_out: bit-equal to F.max_pool3d(kernel f, stride f), NaN included.
  * labels: equal to the f64 oracle's (tests/_ssc_pool_oracle.py) wherever its top-two
    mean-scale scores differ by more than 2^-21: an f32 alpha carries at most about 2^-24 of
    absolute error (1 - expf(t) with t in [-1, 0]; measured 4.9e-8), the ascending f32 sum adds
    less, and 2^-21 is 8x that.  At most 0.5 % of a case's voxels may be excluded that way, and
    the oracle's own exclusions are asserted to stay inside that cap for the chosen seeds.
  * against the torch route (sscbench.pool_voxels on the CPU): the same two rules.
  * repeats, a side stream and a torch.cuda.graph replay: bit-equal.
  * the chunked driver on a small BTSNet: torch.equal to one un-chunked predict_voxels +
    torch-route pooling + max_pool3d grow, for two point budgets (the per-point kernels are
    point-wise), without a host synchronisation in the loop.
  * generate_point_grid(voxel_size=0.1): SHA-256 of the 512 x 512 x 64 centres equal to the
    numpy restatement's (tests/golden/voxel_points_fine.json), as at 0.2; the strided slice at
    0.05 bit-equal too.
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _ssc_pool_oracle as PO
from conftest import GOLDEN
from _helpers import load


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("dims,f,ncls,seed", PO.CASES)
def test_kernel_matches_torch_route_and_f64_oracle(gpu, dims, f, ncls, seed):
    from scenedino_amd import _lib, sscbench
    sigma, label = PO.make_inputs(dims, f, ncls, seed)
    vs = 0.2 / f
    sig, seg = _lib.ssc_pool(torch.from_numpy(sigma).to(gpu), torch.from_numpy(label).to(gpu), f, vs,
                             ncls)
    assert sig.shape == dims and seg.shape == dims and seg.dtype == torch.uint8
    ts, tg = sscbench.pool_voxels(torch.from_numpy(sigma), torch.from_numpy(label), f, vs, ncls)
    _, labels, margin, smax = PO.oracle(sigma, label, f, vs, ncls)
    clear = margin > PO.MARGIN
    excluded = 1.0 - clear.mean()
    got = seg.cpu().numpy()
    print(f"dims {dims} f {f} classes {ncls}: excluded {excluded:.5f}, "
          f"kernel != oracle on {(got != labels).sum()} voxels "
          f"({(got != labels)[clear].sum()} clear), kernel != torch route on "
          f"{(got != tg.numpy()).sum()}")
    assert excluded <= PO.MAX_EXCLUDED
    assert torch.equal(_bits(sig.cpu()), _bits(ts)) and np.array_equal(sig.cpu().numpy(), smax)
    assert (got == labels)[clear].all()
    assert (got == tg.numpy())[clear].all()
    # the routed public function takes the kernel for device tensors
    ps, pg = sscbench.pool_voxels(torch.from_numpy(sigma).to(gpu), torch.from_numpy(label).to(gpu),
                                  f, vs, ncls)
    assert torch.equal(_bits(ps), _bits(sig)) and torch.equal(pg, seg)


@pytest.mark.gpu
@pytest.mark.parametrize("f", [2, 4, 8])
def test_hand_built_voxels_on_the_device(gpu, f):
    from scenedino_amd import _lib
    sigma, label, ncls, want, want_sigma = PO.hand_built(f)
    sig, seg = _lib.ssc_pool(torch.from_numpy(sigma).to(gpu), torch.from_numpy(label).to(gpu), f, 0.1,
                             ncls)
    assert seg.cpu().reshape(-1).tolist() == want.tolist()
    np.testing.assert_array_equal(sig.cpu().reshape(-1).numpy(), want_sigma)


@pytest.mark.gpu
def test_repeat_side_stream_and_graph_replay_are_bit_equal(gpu):
    from scenedino_amd import _lib
    dims, f, ncls, seed = PO.CASES[2]
    sigma, label = PO.make_inputs(dims, f, ncls, seed)
    s_d, l_d = torch.from_numpy(sigma).to(gpu), torch.from_numpy(label).to(gpu)
    a_s, a_g = _lib.ssc_pool(s_d, l_d, f, 0.05, ncls)
    b_s, b_g = _lib.ssc_pool(s_d, l_d, f, 0.05, ncls)
    assert torch.equal(_bits(a_s), _bits(b_s)) and torch.equal(a_g, b_g)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c_s, c_g = _lib.ssc_pool(s_d, l_d, f, 0.05, ncls)
    side.synchronize()
    assert torch.equal(_bits(a_s), _bits(c_s)) and torch.equal(a_g, c_g)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d_s, d_g = _lib.ssc_pool(s_d, l_d, f, 0.05, ncls)
    for _ in range(2):
        d_s.fill_(-1.0)
        d_g.fill_(255)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(a_s), _bits(d_s)) and torch.equal(a_g, d_g)


@pytest.mark.gpu
def test_rejections_before_any_launch(gpu):
    from scenedino_amd import _lib
    lib = _lib.load()
    cx, cy, cz, f = 2, 3, 4, 2
    nf, nc = cx * cy * cz * f ** 3, cx * cy * cz
    s_f = torch.rand(nf + 64, device=gpu)
    g_f = torch.zeros(nf + 64, dtype=torch.uint8, device=gpu)
    s_o = torch.full((nc + 64,), -7.0, device=gpu)
    g_o = torch.full((nc + 64,), 99, dtype=torch.uint8, device=gpu)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(sf=p(s_f), gf=p(g_f), so=p(s_o), go=p(g_o), dims=(cx, cy, cz), factor=f, vs=0.1, ncls=19):
        return lib.sd_ssc_pool(sf, gf, dims[0], dims[1], dims[2], factor, vs, ncls, so, go, st)
    bad = {
        "factor 3": dict(factor=3), "factor 1": dict(factor=1), "factor 16": dict(factor=16),
        "n_classes 0": dict(ncls=0), "n_classes 33": dict(ncls=33),
        "zero dim": dict(dims=(cx, 0, cz)), "2^31 fine voxels": dict(dims=(1 << 10, 1 << 10, 1 << 8)),
        "voxel size": dict(vs=0.0),
        "misaligned sigma_f": dict(sf=p(s_f, 4)), "misaligned seg_f": dict(gf=p(g_f, 8)),
        "misaligned sigma_out": dict(so=p(s_o, 8)), "misaligned seg_out": dict(go=p(g_o, 1)),
        "sigma_out aliases sigma_f": dict(so=p(s_f)), "seg_out aliases seg_f": dict(go=p(g_f)),
        "sigma_out inside sigma_f": dict(so=p(s_f, 4 * (nf - 4))),
        "seg_out aliases sigma_out": dict(go=p(s_o, 16)),
        "null sigma_f": dict(sf=None), "null seg_out": dict(go=None),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert b"sd_ssc_pool" in lib.sd_last_error(), what
    torch.cuda.synchronize()
    assert bool((s_o == -7.0).all()) and bool((g_o == 99).all())  # nothing was launched
    assert call() == 0
    with pytest.raises(RuntimeError, match="sd_ssc_pool"):
        _lib.ssc_pool(s_f[:nf].view(2 * cx, 2 * cy, 2 * cz), g_f[:nf].view(2 * cx, 2 * cy, 2 * cz), 2,
                      0.1, 33)


def _small_net(gpu):
    from _helpers import build_net
    from test_seg import modules_from, seg_params
    from scenedino_amd.downstream_head import SemanticHead
    fq = load("field_query.npz")
    p = seg_params(load("seg_head.npz"), "_768")
    net = build_net(fq["grid"], fq["W_in"], fq["b_in"], fq["W_out"], fq["b_out"], "bf16", gpu)
    dr, st, cl = (m.to(gpu) for m in modules_from(p))
    head = SemanticHead(19, 19, 768, 64).to(gpu).eval()
    head.stego_head, head.stego_cluster_head = st, cl
    net.encoder.dim_reduction, net.downstream_head, net.gt_classes = dr, head, 19
    Tn = lambda k: torch.as_tensor(fq[k]).to(gpu)
    net.encode(Tn("images"), Tn("Ks"), Tn("poses"), ids_encoder=[0], ids_render=[0])
    return net


@pytest.mark.gpu
def test_chunked_query_equals_unchunked_statement(gpu):
    from scenedino_amd import _lib, sscbench
    net = _small_net(gpu)
    dims, f = (8, 8, 4), 2
    fine = tuple(f * d for d in dims)
    # fine voxel centres of a (16, 16, 8) block in front of the camera, 0.1 m voxels
    pts = _lib.voxel_points((2.0, -0.8, -0.4), 0.1, fine, sscbench.read_calib()["Tr"], gpu)
    plane = f ** 3 * dims[1] * dims[2]
    with torch.no_grad():
        sg, lb = net.predict_voxels(pts.reshape(1, -1, 3), voxel_size=0.1)
        ws, wg = sscbench.pool_voxels(sg.reshape(fine).cpu(), lb.reshape(fine).cpu(), f, 0.1)
        ws = F.max_pool3d(ws.unsqueeze(0), 3, 1, 1).squeeze(0)
        assert float(sg.max()) > 0 and lb.unique().numel() > 2  # a field worth pooling
        for max_points in (plane, 3 * plane):
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                s, g = sscbench.query_voxels(net, pts, dims, factor=f, max_points=max_points)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            assert torch.equal(_bits(s.cpu()), _bits(ws)), max_points
            assert torch.equal(g.cpu(), wg), max_points
        # vis contract: the fine grids, per-point seg, grow on the fine densities
        s, g = sscbench.query_voxels(net, pts, dims, factor=f, max_points=plane, pooled=False)
        assert torch.equal(g.cpu(), lb.reshape(fine).cpu())
        want = F.max_pool3d(sg.reshape(1, *fine).cpu(), 3, 1, 1).squeeze(0)
        assert torch.equal(_bits(s.cpu()), _bits(want))


@pytest.mark.gpu
def test_downsample_and_predict_factor_2(gpu):
    """The evaluator's entry point at VOXEL_SIZE 0.1: return types of the factor-1 path, and
    coarse x-planes [0, 2) equal to the unchunked statement of the fine planes under [0, 3)."""
    from scenedino_amd import sscbench
    net = _small_net(gpu)
    fq = load("field_query.npz")
    data = {"imgs": [torch.as_tensor(fq["images"])[0, 0]], "poses": [np.eye(4, dtype=np.float32)],
            "projs": [np.asarray(fq["Ks"])[0, 0]]}
    pts = sscbench.generate_point_grid(sscbench.read_calib()["Tr"], voxel_size=0.1, device=gpu)
    with torch.no_grad():
        sig, segs, dino = sscbench.downsample_and_predict(data, net, pts, 2, "stego_kmeans")
        assert dino is None and sig.shape == (256, 256, 32) and segs.shape == (256, 256, 32)
        assert sig.dtype == np.float32 and segs.dtype == np.float64
        n = 3 * 8 * 256 * 32
        sg, lb = net.predict_voxels(pts[:n].reshape(1, -1, 3), voxel_size=0.1)
        ws, wg = sscbench.pool_voxels(sg.reshape(6, 512, 64), lb.reshape(6, 512, 64), 2, 0.1)
        ws = F.max_pool3d(ws.unsqueeze(0), 3, 1, 1).squeeze(0)
    assert np.array_equal(sig[:2], ws[:2].cpu().numpy())
    assert np.array_equal(segs[:2], wg[:2].cpu().numpy().astype(np.float64))


@pytest.mark.gpu
def test_point_grid_at_fine_voxel_sizes_is_bit_exact(gpu):
    from scenedino_amd import sscbench
    rec = json.load(open(os.path.join(GOLDEN, "voxel_points_fine.json")))
    T = np.asarray(rec["T"])
    pts = sscbench.generate_point_grid(T, voxel_size=0.1, device=gpu)
    assert pts.shape == (512 * 512 * 64, 3) and pts.dtype == torch.float32
    assert hashlib.sha256(pts.cpu().numpy().tobytes()).hexdigest() == rec["0.1"]["sha256"]
    del pts
    fine = sscbench.generate_point_grid(T, voxel_size=0.05, device=gpu)
    assert fine.shape[0] == 1024 * 1024 * 128
    got = fine[::rec["0.05"]["slice_stride"]].cpu().numpy()
    want = np.asarray(rec["0.05"]["slice"], dtype=np.float32)
    assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))
