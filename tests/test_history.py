"""History independence: the same call on the same inputs returns the same bits, whatever
ran in between.

The project keeps state across calls in four places, each pinned here:
  1. the encoder's captured HIP graphs and the per-shape buffers they point into (the
     zero-padded K / V^T and the LayerNorm-tail ticket words on ``_Packed``): a graph replay
     after a pass at another shape on the shared encoder equals the eager pass;
  2. the projected grid P cached per frame: a K <= 64 render / a query never reads the
     hi + lo P that a K > 64 render projected, in either order;
  3. the packed head weights across an optimizer step (fused Adam bumps no version
     counter): forward/backward, query, step, query sees the stepped weights;
  4. the CU reservation (``sd_reserve_cus``): it sizes persistent grids only, the kernel /
     tile choices (and so the summation order) do not move with it.

Every comparison between two runs is bit-equality.  Each test also anchors one result to an
oracle, so "consistently wrong" cannot pass; the bounds are the ones the project already
asserts for the same path: encoder rel-L2 <= 3e-2 (test_vit._encoder_check), ViT -> DPT
<= 5e-2 (test_encoder), 16-bit renders rel-L2 < 1e-2 (test_wide_dino_head_vs_oracle), sd_gemm
max |d| <= 1e-4 scale + 1e-5 (f32) / 8e-3 scale (bf16) (test_gemm_epilogues), sd_attention
max |d| <= 2e-2 (test_qkv_scatter_and_attention).
"""
import math
from contextlib import contextmanager

import pytest
import torch
import torch.nn.functional as F

from _helpers import build_net, load, net_from_fixture, rel_l2
from oracle import dpt_oracle as DO
from oracle import vit_oracle as VO
from test_dpt import det_fill
from test_encoder import CONF
from test_vit import init_vit

pytestmark = pytest.mark.gpu

DEV = "cuda"
RESERVATIONS = (16, 128, 224)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()


@contextmanager
def _reserved(n):
    from scenedino_amd import _lib
    prev = _lib.reserve_cus(n)
    try:
        yield
    finally:
        _lib.reserve_cus(prev)


def _bf(t):
    return t.to(torch.bfloat16)


def _images(B, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, 64, 160, generator=g) * 2 - 1).to(DEV)


def _assert_same(a, b, what=""):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert not x.is_floating_point() or torch.isfinite(x).all(), (what, i)
        assert torch.equal(x, y), (what, i)


# --------------------------------------------------------------------------- 1. encoder graphs
def _small_vit(C, heads, depth, seed):
    """64 x 160 at patch 16: 41 tokens padded to 64, so 23 padding columns are live in the
    attention; C = 384 takes the fused LayerNorm GEMMs, C = 768 the separate launches."""
    from scenedino_amd.models.backbones.dino.vit import VisionTransformer
    return init_vit(VisionTransformer((64, 160), 16, C, depth, heads), seed)


def _shared_module(arch, C, heads, seed):
    """DINOv2Module (DPT decoder) whose gt_encoder IS its encoder, around a small ViT.  Three
    blocks, not two: the DPT takes four levels (three block outputs + the final grid)."""
    from scenedino_amd.models.backbones import make_backbone
    from scenedino_amd.models.backbones.dino.vit import _ViT
    m = make_backbone(dict(CONF, encoder_arch=arch, separate_gt_version=None)).eval()
    assert m.gt_encoder is m.encoder
    m.encoder.model = _ViT(_small_vit(C, heads, 3, seed), 16, intermediate_features=[0, 1, 2])
    det_fill(m.decoder, seed + 2)
    return m.to(DEV).eval()


def _poison(B, heads, n=8):
    """NaN-filled tensors with the byte size of the (B, heads, 64, 64) bf16 K and V^T buffers
    of a 41-token pass: had such a buffer been freed, the caching allocator would hand its
    block back here."""
    return [torch.full((B * heads * 64 * 64,), float("nan"), device=DEV, dtype=torch.bfloat16)
            for _ in range(n)]


@pytest.mark.parametrize("arch,C,heads", [("vit-s", 384, 6), ("vit-b", 768, 12)],
                         ids=["vit_s", "vit_b"])
def test_graph_replay_survives_other_shape_on_shared_encoder(arch, C, heads):
    """DINOv2Module._predict and _ViT.forward_grids each cache a graph over the same _Packed
    (gt_encoder is encoder).  A graph captured at B = 1 is replayed after the OTHER caller ran
    B = 2 on the shared encoder: bit-equal to the eager pass, in both directions."""
    m = _shared_module(arch, C, heads, 41)
    enc, vit = m.encoder, m.encoder.model
    A, A2, X2 = _images(1, 42), _images(1, 43), _images(2, 44)
    with torch.no_grad():
        m.use_graph = vit.use_graph = False
        e_pred = [m(x)[0].clone() for x in (A, A2)]
        e_pred2 = m(X2)[0].clone()
        e_vit = [[t.clone() for t in enc(x)] for x in (A, A2)]
        e_gt2 = m(X2, ground_truth=True)[0].clone()
        m.use_graph = vit.use_graph = True

        # the module's graph at B = 1, the shared encoder's own graph at B = 2 in between
        _assert_same([m(A)[0]], [e_pred[0]], "predict capture")
        graph = m._graph[1]
        _assert_same([m(X2, ground_truth=True)[0]], [e_gt2], "gt pass at B = 2")
        poison = _poison(1, heads)
        got_pred = m(A2)[0]
        assert m._graph[1] is graph  # a replay, not a re-capture
        torch.cuda.synchronize()
        _assert_same([got_pred], [e_pred[1]], "predict replay after the B = 2 gt pass")
        del poison

        # the mirror: the encoder's own graph at B = 1, the module's pass at B = 2 in between
        m._graph = vit._graph = None
        _assert_same(enc(A), e_vit[0], "vit capture")
        graph = vit._graph[1]
        _assert_same([m(X2)[0]], [e_pred2], "predict at B = 2")
        poison = _poison(1, heads)
        got_vit = enc(A2)
        assert vit._graph[1] is graph
        torch.cuda.synchronize()
        _assert_same(got_vit, e_vit[1], "vit replay after the B = 2 predict pass")
        del poison
    # oracle anchors of the two replays
    with torch.no_grad():
        feats = VO.encoder_forward(vit.vit.cpu(), A2.cpu(), [0, 1, 2])
        ref_pred = DO.dpt_forward(m.decoder.cpu(), feats)
    for i, (a, r) in enumerate(zip(got_vit, feats)):
        assert rel_l2(a, r) <= 3e-2, i
    assert rel_l2(got_pred, ref_pred) <= 5e-2


def test_vit_graph_b1_b2_b1_bit_equal_to_eager():
    """One _ViT going B = 1 -> B = 2 -> B = 1 (a re-capture at each change of shape, over
    buffers that other passes used in between): bit-equal to eager at every step."""
    from scenedino_amd.models.backbones.dino.vit import _ViT
    m = _ViT(_small_vit(384, 6, 2, 51), 16, intermediate_features=[0]).to(DEV).eval()
    xs = [_images(1, 52), _images(2, 53), _images(1, 54), _images(1, 55)]
    with torch.no_grad():
        m.use_graph = False
        eager = [[t.clone() for t in (lambda o: o[0] + [o[1]])(m.forward_grids(x))] for x in xs]
        m.use_graph = True
        poison = None
        for i, x in enumerate(xs):
            grids, final = m.forward_grids(x)  # the last step replays the third's graph
            torch.cuda.synchronize()
            _assert_same(grids + [final], eager[i], f"step {i}")
            poison = _poison(x.shape[0], 6, 4)  # held across the next step
    with torch.no_grad():
        ref = VO.encoder_forward(m.vit.cpu(), xs[-1].cpu(), [0])
    for a, r in zip(grids + [final], ref):
        assert rel_l2(a, r) <= 3e-2


# --------------------------------------------------------------------------- 2. projected grid
KEYS = ("depth", "dino_features", "rgb", "weights")


@pytest.fixture(scope="module")
def scene():
    """The 12 x 40 image / 6 x 20 grid / C = 256 frame of test_wide_dino_head_vs_oracle at
    D = 64: 480 rays, jitter for K = 32 / 64 / 128, and the oracle's render at each K."""
    from scenedino_amd.common.ray_sampler import ImageRaySampler
    g = torch.Generator().manual_seed(164)
    H, W, C, D = 12, 40, 256, 64
    s = {"images": torch.rand(1, 1, 3, H, W, generator=g) * 2 - 1,
         "grid": torch.randn(1, C, 6, 20, generator=g),
         "W_in": torch.randn(128, C + 39, generator=g) * 0.08,
         "b_in": torch.randn(128, generator=g) * 0.1,
         "W_out": torch.randn(1 + D, 128, generator=g) * 0.1,
         "b_out": torch.randn(1 + D, generator=g) * 0.1,
         "Kn": torch.tensor([[0.7849, 0.0, -0.0312], [0.0, 2.9391, 0.2701],
                             [0.0, 0.0, 1.0]]).view(1, 1, 3, 3),
         "pose": torch.eye(4).view(1, 1, 4, 4)}
    s["u"] = {K: torch.rand(H * W, K, generator=g) for K in (32, 64, 128)}
    rays, _ = ImageRaySampler(3, 80, H, W).sample(None, s["pose"].to(DEV), s["Kn"].to(DEV))
    s["rays"] = rays
    zz = 3 + 40 * torch.rand(H * W, 4, 1, generator=g)
    r = rays[0].cpu()
    s["xyz"] = (r[:, None, :3] + r[:, None, 3:6] * zz).reshape(1, -1, 3).contiguous().to(DEV)
    s["ref"] = {K: _oracle_render(s, K) for K in (32, 64, 128)}
    return s


def _oracle_render(s, K, W_in=None, W_out=None):
    from oracle import render_oracle as O
    w2c = torch.inverse(s["pose"])
    return O.render(s["rays"][0].cpu(), s["u"][K], s["grid"], w2c[:, 0], s["Kn"][:, 0],
                    s["images"] * 0.5 + 0.5, w2c, s["Kn"], s["W_in"] if W_in is None else W_in,
                    s["b_in"], s["W_out"] if W_out is None else W_out, s["b_out"], sb=1)


def _scene_net(s, precision, W_in=None, W_out=None):
    net = build_net(s["grid"], s["W_in"] if W_in is None else W_in, s["b_in"],
                    s["W_out"] if W_out is None else W_out, s["b_out"], precision, DEV)
    net.encode(s["images"].to(DEV), s["Kn"].to(DEV), s["pose"].to(DEV), ids_encoder=[0],
               ids_render=[0])
    return net


def _render(net, s, K):
    from scenedino_amd.renderer import NeRFRenderer
    r = NeRFRenderer(n_coarse=K, lindisp=True)
    r.z_jitter = s["u"][K].to(DEV)
    with torch.no_grad():
        c = r.bind_parallel(net).eval()(s["rays"], want_weights=True)["coarse"]
    torch.cuda.synchronize()
    return {k: c[k].clone() for k in KEYS}


def _query(net, xyz):
    with torch.no_grad():
        out = net.query(xyz)
    torch.cuda.synchronize()
    return [t.clone() for t in out]


def _same_render(a, b, what):
    for k in KEYS:
        assert torch.isfinite(a[k]).all(), (what, k)
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_render_and_query_independent_of_render_order(scene, precision):
    """K = 64 after K = 128 equals K = 64 on a fresh net, so does a query after K = 128, and
    K = 128 after K = 64 equals a fresh K = 128 -- which is the oracle's render within 1e-2."""
    s = scene
    n1 = _scene_net(s, precision)
    fresh64 = _render(n1, s, 64)
    after64_128 = _render(n1, s, 128)
    n2 = _scene_net(s, precision)
    fresh128 = _render(n2, s, 128)
    q_after128 = _query(n2, s["xyz"])
    after128_64 = _render(n2, s, 64)
    q_fresh = _query(_scene_net(s, precision), s["xyz"])
    _same_render(after128_64, fresh64, "K = 64 after K = 128")
    _same_render(after64_128, fresh128, "K = 128 after K = 64")
    assert float(q_fresh[0].sum()) > 0
    _assert_same(q_after128, q_fresh, "query after K = 128")
    assert fresh128["dino_features"].shape[-1] == 64
    for k in KEYS:
        assert rel_l2(fresh128[k], s["ref"][128][k]) < 1e-2, k


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_weight_change_reprojects_plain_and_exact_grid(scene, precision):
    """Both cached P variants follow the weights: after K = 64 and K = 128 renders, a
    training-path forward and an in-place update that bumps no version counter (the pattern
    of test_inference_after_inplace_optimizer_step_uses_new_weights), the K = 128 and the
    K = 64 render equal those of fresh nets built on the new weights."""
    s = scene
    net = _scene_net(s, precision)
    old = {K: _render(net, s, K) for K in (64, 128)}
    net.train()
    with torch.enable_grad():
        sig, dino, *_ = net._query_diff(s["xyz"])
        (sig.sum() + dino.sum()).backward()
    net.eval()
    head = net.heads["normal_head"]
    g = torch.Generator().manual_seed(7)
    v0 = head.lin_in.weight._version
    head.lin_in.weight.data.add_(0.05 * torch.randn(head.lin_in.weight.shape, generator=g).cuda())
    head.lin_out.weight.data.add_(0.05 * torch.randn(head.lin_out.weight.shape, generator=g).cuda())
    assert head.lin_in.weight._version == v0
    W_in, W_out = head.lin_in.weight.detach().cpu(), head.lin_out.weight.detach().cpu()
    for K in (128, 64):
        new = _render(net, s, K)
        _same_render(new, _render(_scene_net(s, precision, W_in, W_out), s, K), f"K = {K}")
        assert not torch.equal(new["depth"], old[K]["depth"])
        assert not torch.equal(new["dino_features"], old[K]["dino_features"])
    ref = _oracle_render(s, 128, W_in, W_out)
    new = _render(net, s, 128)
    for k in KEYS:
        assert rel_l2(new[k], ref[k]) < 1e-2, k


# --------------------------------------------------------------------------- 3. optimizer step
def _fresh_like(d, net, precision):
    head = net.heads["normal_head"]
    d2 = dict(d)
    for k, p in (("W_in", head.lin_in.weight), ("b_in", head.lin_in.bias),
                 ("W_out", head.lin_out.weight), ("b_out", head.lin_out.bias)):
        d2[k] = p.detach().cpu().numpy()
    return net_from_fixture(d2, precision)


def _assert_field_oracle(d, net, sigma, dino):
    """The 16-bit bounds of test_field_query_wide_head_vs_oracle (points with z_cam >= 1 m:
    sigma rel-L2 < 2e-2, dino < 1e-2) against the CPU oracle on the net's current weights."""
    from oracle import render_oracle as O
    Tc = torch.from_numpy
    head = net.heads["normal_head"]
    w2c = torch.inverse(Tc(d["poses"]))
    r = O.field_query(Tc(d["xyz"]), Tc(d["grid"]), w2c[:, 0], Tc(d["Ks"])[:, 0],
                      Tc(d["images"]) * 0.5 + 0.5, w2c, Tc(d["Ks"]),
                      *(p.detach().cpu() for p in (head.lin_in.weight, head.lin_in.bias,
                                                   head.lin_out.weight, head.lin_out.bias)))
    xyz = Tc(d["xyz"]).double().reshape(-1, 3)
    ok = xyz @ w2c[0, 0].double()[2, :3] + w2c[0, 0].double()[2, 3] >= 1.0
    D = dino.shape[-1]
    assert rel_l2(sigma.reshape(-1).cpu()[ok], r["sigma"].reshape(-1)[ok]) < 2e-2
    assert rel_l2(dino.reshape(-1, D).cpu()[ok], r["dino"].reshape(-1, D)[ok]) < 1e-2


def _train_forward_backward(net, xyz):
    net.train()
    with torch.enable_grad():
        sig, dino, *_ = net._query_diff(xyz)
        (sig.sum() + dino.sum()).backward()
    net.eval()


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_inference_query_between_backward_and_fused_adam_step(precision):
    """forward/backward -> no_grad query (re-packs the pre-step weights) -> fused Adam step
    (in place, no version bump) -> no_grad query: the last query runs on the stepped weights,
    bit-equal to a freshly built net carrying them."""
    d = load("field_query.npz")
    net = net_from_fixture(d, precision)
    xyz = torch.as_tensor(d["xyz"]).cuda()
    head = net.heads["normal_head"]
    opt = torch.optim.Adam(head.parameters(), lr=1e-2, fused=True)
    _train_forward_backward(net, xyz)
    s_pre, dn_pre = _query(net, xyz)[:2]
    w_pre = head.lin_in.weight.detach().clone()
    opt.step()
    assert not torch.equal(head.lin_in.weight.detach(), w_pre)
    s_post, dn_post = _query(net, xyz)[:2]
    s_ref, dn_ref = _query(_fresh_like(d, net, precision), xyz)[:2]
    assert torch.isfinite(s_post).all() and torch.isfinite(dn_post).all()
    assert torch.equal(s_post, s_ref) and torch.equal(dn_post, dn_ref)
    assert not torch.equal(s_post, s_pre) and not torch.equal(dn_post, dn_pre)
    # the query between backward and step ran on the untouched weights
    s0, dn0 = _query(net_from_fixture(d, precision), xyz)[:2]
    assert torch.equal(s_pre, s0) and torch.equal(dn_pre, dn0)
    _assert_field_oracle(d, net, s_post, dn_post)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_invalidate_packed_after_an_update_no_hook_sees(precision):
    """The same sequence with `.data` writes in place of the optimizer: nothing can see the
    update, net.invalidate_packed() is the documented call."""
    d = load("field_query.npz")
    net = net_from_fixture(d, precision)
    xyz = torch.as_tensor(d["xyz"]).cuda()
    head = net.heads["normal_head"]
    _train_forward_backward(net, xyz)
    s_pre, dn_pre = _query(net, xyz)[:2]
    g = torch.Generator().manual_seed(7)
    head.lin_in.weight.data.add_(0.05 * torch.randn(head.lin_in.weight.shape, generator=g).cuda())
    head.lin_out.weight.data.add_(0.05 * torch.randn(head.lin_out.weight.shape, generator=g).cuda())
    net.invalidate_packed()
    s_post, dn_post = _query(net, xyz)[:2]
    s_ref, dn_ref = _query(_fresh_like(d, net, precision), xyz)[:2]
    assert torch.equal(s_post, s_ref) and torch.equal(dn_post, dn_ref)
    assert not torch.equal(s_post, s_pre) and not torch.equal(dn_post, dn_pre)
    _assert_field_oracle(d, net, s_post, dn_post)


# --------------------------------------------------------------------------- 4. CU reservation
@pytest.mark.parametrize("M,N,K", [(481, 384, 1536), (97, 64, 2048)])
def test_gemm_independent_of_cu_reservation(M, N, K):
    """The split-K shapes of test_gemm_cross_workgroup_split_k (32 x 32 ring tiles when they
    fit the CUs): the tile choice compares with the device's CUs, not the unreserved ones."""
    from scenedino_amd import _lib
    g = torch.Generator().manual_seed(M + K)
    a = _bf(torch.randn(M, K, generator=g)).to(DEV)
    w = _bf(torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV)
    bias = (0.1 * torch.randn(N, generator=g)).to(DEV)
    res = torch.randn(M, N, generator=g).to(DEV)
    gam = torch.rand(N, generator=g).to(DEV)

    def run():
        out = torch.empty(M, N, device=DEV)
        _lib.gemm(a, w, bias, _lib.SD_EPI_F32, out=out)
        x = res.clone()
        _lib.gemm(a, w, bias, _lib.SD_EPI_RESID, out=x, gamma=gam)
        ob = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        _lib.gemm(a, w, bias, _lib.SD_EPI_GELU, out=ob)
        torch.cuda.synchronize()
        return out, x, ob

    with _reserved(0):
        base = run()
    for r in RESERVATIONS:
        with _reserved(r):
            _assert_same(run(), base, f"reserve {r}")
    ref = a.double() @ w.double().t() + bias.double()
    scale = ref.abs().max().item()
    out, x, ob = base
    assert (out - ref).abs().max().item() <= 1e-4 * scale + 1e-5
    assert (x - (res + gam * ref)).abs().max().item() <= 1e-4 * scale + 1e-5
    assert (ob - F.gelu(ref)).abs().max().item() <= 8e-3 * scale


@pytest.mark.parametrize("B,H,T", [(1, 6, 481), (2, 12, 77)])
def test_attention_independent_of_cu_reservation(B, H, T):
    """sd_attention picks one of three kernels by comparing its workgroup count with the
    CUs: (1, 6, 481) sits under half of 256 CUs and over half of 32."""
    from scenedino_amd import _lib
    g = torch.Generator().manual_seed(T)
    C = 64 * H
    xn = _bf(torch.randn(B * T, C, generator=g)).to(DEV)
    w = _bf(torch.randn(3 * C, C, generator=g) / math.sqrt(C)).to(DEV)
    b = (0.1 * torch.randn(3 * C, generator=g)).to(DEV)
    Tp = (T + 63) // 64 * 64
    q = torch.empty(B, H, T, 64, device=DEV, dtype=torch.bfloat16)
    k = torch.zeros(B, H, Tp, 64, device=DEV, dtype=torch.bfloat16)
    vt = torch.zeros(B, H, 64, Tp, device=DEV, dtype=torch.bfloat16)
    _lib.gemm(xn, w, b, _lib.SD_EPI_QKV, qkv=(q, k, vt), tokens=T, heads=H)

    def run():
        out = torch.empty(B * T, C, device=DEV, dtype=torch.bfloat16)
        _lib.attention(q, k, vt, 64 ** -0.5, out)
        torch.cuda.synchronize()
        return [out]

    with _reserved(0):
        base = run()
    for r in RESERVATIONS:
        with _reserved(r):
            _assert_same(run(), base, f"reserve {r}")
    kk, vv = k[:, :, :T].double(), vt[..., :T].double().transpose(-1, -2)
    att = ((q.double() * 64 ** -0.5) @ kk.transpose(-1, -2)).softmax(-1)
    ref = (att @ vv).transpose(1, 2).reshape(B * T, C)
    assert (base[0].double() - ref).abs().max().item() <= 2e-2


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 12, 40, 256, 256), (2, 7, 9, 64, 128)])
def test_conv3x3_independent_of_cu_reservation(B, H, W, Cin, Cout):
    """The DPT's low-resolution 3 x 3 convolution (a small-M, large-K GEMM: ring tiles or
    the big conv tiles by CU count) and an odd small one."""
    from scenedino_amd import _lib
    g = torch.Generator().manual_seed(H * W + Cin)
    x = _bf(torch.randn(B, H, W, Cin, generator=g)).to(DEV)
    w = _bf(torch.randn(Cout, 9 * Cin, generator=g) / math.sqrt(9 * Cin)).to(DEV)
    bias = (0.1 * torch.randn(Cout, generator=g)).to(DEV)

    def run():
        out = [_lib.conv3x3(x, w, bias), _lib.conv3x3(x, w, bias, relu_in=True, epi=_lib.SD_EPI_F32)]
        torch.cuda.synchronize()
        return out

    with _reserved(0):
        base = run()
    for r in RESERVATIONS:
        with _reserved(r):
            _assert_same(run(), base, f"reserve {r}")
    # anchor: F.conv2d in float64 on the same bf16 operands, test_dpt.test_conv3x3's bound for
    # the bf16 output (|d| <= 2e-2 max|ref|)
    wk = w.double().view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), wk, bias.double(), padding=1)
    ref = ref.permute(0, 2, 3, 1)
    assert (base[0].double() - ref).abs().max().item() <= 2e-2 * ref.abs().max().item()


def test_vit_independent_of_cu_reservation():
    """The small ViT end to end, eager: every GEMM / attention choice inside it.  B = 3: 18
    128-query attention workgroups, under half of 256 CUs and over half of the 32 that a
    reservation of 224 leaves -- the batch at which the attention choice used to flip."""
    from scenedino_amd.models.backbones.dino.vit import _ViT
    m = _ViT(_small_vit(384, 6, 2, 61), 16, intermediate_features=[0]).to(DEV).eval()
    m.use_graph = False
    x = _images(3, 62)

    def run():
        with torch.no_grad():
            grids, final = m.forward_grids(x)
        torch.cuda.synchronize()
        return grids + [final]

    with _reserved(0):
        base = run()
    for r in RESERVATIONS:
        with _reserved(r):
            _assert_same(run(), base, f"reserve {r}")
    with torch.no_grad():
        ref = VO.encoder_forward(m.vit.cpu(), x.cpu(), [0])
    for a, r in zip(base, ref):
        assert rel_l2(a, r) <= 3e-2


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("K", [32, 64])
def test_render_independent_of_cu_reservation(scene, precision, K):
    """The 480-ray render with the persistent grids (projection, tile kernel, overflow list)
    shrunk to 240, 128 and 32 workgroups: rays are independent, the same bits."""
    s = scene
    with _reserved(0):
        base = _render(_scene_net(s, precision), s, K)
    for r in RESERVATIONS:
        with _reserved(r):
            _same_render(_render(_scene_net(s, precision), s, K), base, f"reserve {r}")
    for k in KEYS:
        assert rel_l2(base[k], s["ref"][K][k]) < 1e-2, k
