"""sd_attention / sd_attention_bwd outside the near-uniform softmax: sharp logits, the key
padding mask, split-state merges and every key -> value index map.

tests/test_vit.py draws N(0, 1) logits (a near-uniform softmax whose output is about a mean
of V) and holds the forward to 2e-2 absolute, which is about the size of that output: a
kernel that does not mask the padded keys at all passes it at 481 tokens (the replay's
`nomask` mutant below: max error 0.019).  Here every reference is float64 on the CPU
from the same bf16-rounded operands the kernel gets, cached per (family, B, H, T).

Input families (scale 0.125, head_dim 64, u a fixed unit vector):
  random     q, k, v ~ N(0, 1)                      logits within +-5
  sharp      q, k ~ 3 N(0, 1)                       logit std about 9: large rescale steps
  sharp2     q, k ~ 2 N(0, 1)                       logit std about 4 (backward only)
  negbias    q - 16 u, k + 16 u                     every real logit in -46 .. -19: an
                                                    unmasked pad key (score 0) takes the row
  ramp_up /  q + 8 u, k_j + linspace(-+40, +-40)_j u
  ramp_down                                         the maximum moves in every block / never
                                                    after the first; split maxima ~100 apart
  onehot     k_j in {-1, +1}^64, q_i = 16 k_pi(i)   logit 128 at pi(i), >= 40 lower elsewhere:
                                                    the output is v[pi(i)] bit for bit

Forward tolerance, per element, from the kernel's roundings (A = softmax in float64):
    |out - A v| <= 2^-8 (A |v|) + 2^-8 |A v| + 1e-6
each P entry is rounded once to bf16 before the PV product, the row sum is taken over the
unrounded p, and the output is rounded once to bf16.  bf16 keeps 8 significant bits, so one
rounding is at most 2^-8 relative just above a power of two and 2^-9 just below the next:
the two terms are the worst case of the two roundings, with v_exp_f32 and the f32 score /
argument rounding (about 1e-5 relative here) far below them.  The CPU replay of that
arithmetic peaks at 0.89 of the bound and the kernels at the same 0.89 (sharp, T = 481).
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import vit_oracle as VO
from test_vit import init_vit
from test_vit_train import _attn_ref, _split_dqkv, check_gradients

BF = torch.bfloat16
SCALE = 0.125
B0, H0 = 2, 3  # bh / H with a head count that is no power of two
# one block; a 2split half with no block (<= 64); a ragged last block (65); an odd block
# count (129: one 2split half idles, two 128-query lds tiles); five blocks over four dir
# waves (300); two blocks per dir wave (481)
TS = [1, 40, 64, 65, 129, 300, 481]
MODES = ["auto", "lds", "dir", "2split"]
FAMILIES = ["random", "sharp", "negbias", "ramp_up", "ramp_down"]
PERMS = ["identity", "reverse", "last", "first", "stride37"]
_SEEDS = {n: i for i, n in enumerate(FAMILIES + ["sharp2"])}


def _q(t):
    return t.to(BF).float()


def ceil64(T):
    return (T + 63) // 64 * 64


def _unit():
    u = torch.randn(64, generator=torch.Generator().manual_seed(64))
    return u / u.norm()


def _operands(name, B, H, T):
    """bf16-rounded f32 q, k, v (B, H, T, 64) of a family."""
    g = torch.Generator().manual_seed(100003 * _SEEDS[name] + 1000 * B + 10 * T + H)
    q, k, v = (torch.randn(B, H, T, 64, generator=g) for _ in range(3))
    u = _unit()
    if name == "sharp":
        q, k = 3 * q, 3 * k
    elif name == "sharp2":
        q, k = 2 * q, 2 * k
    elif name == "negbias":
        q, k = q - 16 * u, k + 16 * u
    elif name in ("ramp_up", "ramp_down"):
        r = torch.linspace(-40, 40, T) * (1 if name == "ramp_up" else -1)
        q, k = q + 8 * u, k + r[:, None] * u
    return _q(q), _q(k), _q(v)


def _rows(x):
    """(B, H, T, 64) -> the kernel's output layout (B T, H 64)."""
    B, H, T, _ = x.shape
    return x.transpose(1, 2).reshape(B * T, H * 64)


def _bound(q, k, v):
    """float64 reference and the per-element bound of the module docstring, (B T, H 64)."""
    A = (SCALE * q.double() @ k.double().transpose(-1, -2)).softmax(-1)
    ref, mag = A @ v.double(), A @ v.double().abs()
    return _rows(ref), _rows(2.0 ** -8 * mag + 2.0 ** -8 * ref.abs() + 1e-6)


@functools.lru_cache(maxsize=None)
def fwd_case(name, B, H, T):
    q, k, v = _operands(name, B, H, T)
    return (q, k, v) + _bound(q, k, v)


def _perm(name, T):
    i = torch.arange(T)
    return {"identity": i, "reverse": T - 1 - i, "last": torch.full_like(i, T - 1),
            "first": torch.zeros_like(i), "stride37": (37 * i + 5) % T}[name]


@functools.lru_cache(maxsize=None)
def onehot_case(B, H, T, perm):
    """(q, k, v, pi, gap): logit 128 at key pi(i), every other logit at least gap lower.  All
    operands are exact in bf16."""
    g = torch.Generator().manual_seed(T)
    k = (torch.randint(0, 2, (B, H, T, 64), generator=g) * 2 - 1).float()
    v = _q(torch.randn(B, H, T, 64, generator=g))
    pi = _perm(perm, T)
    q = 16 * k[:, :, pi]
    logits = SCALE * q.double() @ k.double().transpose(-1, -2)
    idx = pi.view(1, 1, T, 1).expand(B, H, T, 1)
    assert (logits.gather(-1, idx) == 128).all()
    gap = (128 - logits.scatter(-1, idx, -math.inf).max()).item()
    assert torch.equal(_q(q), q) and torch.equal(_q(k), k)
    return q, k, v, pi, gap


def replay(q, k, v, mutant=None):
    """The kernel's arithmetic on the CPU: f32 scores, mask, exp2 in the log2 domain, bf16 P
    into the PV product, f32 row sum of the unrounded p, bf16 output.  Mutants: `nomask` (pad
    keys, score 0, take part), `droplast` (the last 64-key block is skipped), `drop8` (8 keys
    at Tp / 2 are skipped)."""
    B, H, T, _ = q.shape
    Tp = ceil64(T)
    kp, vp = torch.zeros(B, H, Tp, 64), torch.zeros(B, H, Tp, 64)
    kp[:, :, :T], vp[:, :, :T] = k, v
    keep = torch.ones(Tp, dtype=torch.bool)
    if mutant != "nomask":
        keep[T:] = False
    if mutant == "droplast":
        keep[Tp - 64:] = False
    if mutant == "drop8":
        keep[Tp // 2:Tp // 2 + 8] = False
    sl2e = torch.tensor(SCALE * 1.4426950408889634, dtype=torch.float32)
    s = (q @ kp.transpose(-1, -2)).masked_fill(~keep, -math.inf)
    m = s.amax(-1, keepdim=True) * sl2e
    p = torch.exp2(s * sl2e - m)
    o = p.to(BF).float() @ vp
    return _rows(_q(o * (1 / p.sum(-1, keepdim=True))))


def _ratio(out, ref, bound):
    return ((out.double() - ref).abs() / bound).max().item()


# ------------------------------------------------------------------------ CPU
def test_attention_rejects_bad_arguments_without_gpu():
    from scenedino_amd import _lib
    lib = _lib.load()

    def call(**kw):
        d = dict(q=16, k=16, vt=16, B=2, heads=3, tokens=65, tokens_pad=128, head_dim=64,
                 scale=0.125, out=16)
        d.update(kw)
        return lib.sd_attention(d["q"], d["k"], d["vt"], d["B"], d["heads"], d["tokens"],
                                d["tokens_pad"], d["head_dim"], d["scale"], d["out"], None)

    for bad in (dict(scale=0.0), dict(scale=-0.125), dict(scale=math.nan), dict(scale=math.inf),
                dict(tokens_pad=64), dict(tokens_pad=100), dict(head_dim=32), dict(head_dim=128),
                dict(B=256, heads=256), dict(q=None), dict(k=None), dict(vt=None),
                dict(out=None)):
        # another entry point's rejection first, so that the message below is this call's
        assert lib.sd_attention_bwd(None, None) == -1
        assert b"sd_attention:" not in lib.sd_last_error()
        assert call(**bad) == -1 and b"sd_attention:" in lib.sd_last_error(), bad


def test_replay_meets_the_bound_and_its_mutants_do_not():
    """A test of the tests: the arithmetic replay stays inside the derived bound on every
    family, and three subtly wrong kernels do not where they should not.  Measured (CPU),
    err / bound: replay at most 0.89 (sharp, T = 481); nomask 127 / 125 on negbias and 47 on
    random at T = 65 (3.2 at T = 481, which is 0.019 absolute: about the 2e-2 that
    tests/test_vit.py allows); droplast 3.7e3 .. 7.0e4 on sharp / ramp_up; drop8 4.2e4 on sharp at
    T = 481."""
    worst = {}
    for T in (65, 481):
        for name in FAMILIES:
            q, k, v, ref, bound = fwd_case(name, B0, H0, T)
            worst[name, T] = {m: _ratio(replay(q, k, v, m), ref, bound)
                              for m in (None, "nomask", "droplast", "drop8")}
            print(f"replay {name} T={T}: "
                  + " ".join(f"{m}={r:.3g}" for m, r in worst[name, T].items()))
            assert worst[name, T][None] <= 1.0, (name, T)
    for T in (65, 481):
        assert worst["negbias", T]["nomask"] > 1
        assert worst["sharp", T]["droplast"] > 1 and worst["ramp_up", T]["droplast"] > 1
    assert worst["random", 65]["nomask"] > 1
    assert worst["sharp", 481]["drop8"] > 1
    # what the 2e-2 absolute check lets through
    q, k, v, ref, _ = fwd_case("random", B0, H0, 481)
    err = (replay(q, k, v, "nomask").double() - ref).abs().max().item()
    # printed, not asserted against 2e-2: 0.019 here, and another randn or matmul order may
    # move it across.  What is asserted is that the derived bound does catch this mutant.
    print(f"nomask on random at T=481: max |err| {err:.4f} (tests/test_vit.py allows 2e-2)")
    assert worst["random", 481]["nomask"] > 1 and err > 5e-3


@pytest.mark.parametrize("T", TS)
def test_onehot_gap_precondition(T):
    for perm in PERMS:
        assert onehot_case(B0, H0, T, perm)[4] >= 40, perm


# ------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


def _pack(q, k, v, gpu, Tp=None):
    """The kernel operands: q, k zero-padded to Tp rows, v transposed and zero-padded."""
    B, H, T, _ = q.shape
    Tp = Tp or ceil64(T)
    kd = torch.zeros(B, H, Tp, 64, device=gpu, dtype=BF)
    vtd = torch.zeros(B, H, 64, Tp, device=gpu, dtype=BF)
    kd[:, :, :T] = k.to(BF).to(gpu)
    vtd[..., :T] = v.transpose(-1, -2).to(BF).to(gpu)
    return q.to(BF).to(gpu), kd, vtd


def _launch(qd, kd, vtd, guard=0):
    """sd_attention on packed operands into a buffer prefilled with 7.0 (+ guard rows)."""
    from scenedino_amd import _lib
    B, H, T, _ = qd.shape
    buf = torch.full((B * T + guard, H * 64), 7.0, device=qd.device, dtype=BF)
    _lib.attention(qd, kd, vtd, SCALE, buf[:B * T])
    return buf


def _forward(q, k, v, gpu, Tp=None):
    ops = _pack(q, k, v, gpu, Tp)
    return _launch(*ops), ops


def _set_mode(monkeypatch, mode):
    if mode != "auto":
        monkeypatch.setenv("SD_ATTN", mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", FAMILIES)
def test_attention_families(gpu, name, T, mode, monkeypatch):
    """Every family within the derived per-element bound, in every kernel.  Measured on
    MI355X, max err / bound over T and modes: random 0.52, sharp 0.89 (T = 481), negbias 0.65,
    ramp_up 0.77, ramp_down 0.80 (both T = 40); at each of these the modes agree to the digits
    shown, but for 2split at sharp, T = 481 (0.83)."""
    _set_mode(monkeypatch, mode)
    q, k, v, ref, bound = fwd_case(name, B0, H0, T)
    out = _forward(q, k, v, gpu)[0].float().cpu()
    assert torch.isfinite(out).all()
    r = _ratio(out, ref, bound)
    print(f"attention {name} T={T} {mode}: err / bound {r:.3f}")
    assert r <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("perm", PERMS)
@pytest.mark.parametrize("T", TS)
def test_attention_onehot_routes_bit_exact(gpu, T, perm, mode, monkeypatch):
    """Every other p is at most e^-40, so out[i] is v[pi(i)] to 1e-15 relative and must be
    bit-equal: at_perm, at_key, the V^T fragment layout, the LDS staging chunks and the
    buffer-load offsets with no tolerance at all."""
    _set_mode(monkeypatch, mode)
    q, k, v, pi, gap = onehot_case(B0, H0, T, perm)
    assert gap >= 40
    out = _forward(q, k, v, gpu)[0].float().cpu()
    assert torch.equal(out, _rows(v[:, :, pi]))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("extra", [64, 128])
@pytest.mark.parametrize("T", [1, 40, 65])
@pytest.mark.parametrize("name", ["random", "negbias"])
def test_attention_padded_key_blocks(gpu, name, T, extra, mode, monkeypatch):
    """tokens_pad beyond ceil64(tokens): wholly padded key blocks are never visited, so the
    result is the one of the tight call, bit for bit.  Measured on MI355X: err / bound at most
    0.65.  (While the key loops ran to tokens_pad, every case but T = 65 + 64 under 2split
    came back all NaN from k_attn_dir and k_attn_lds<2>: a wave or key half whose first block
    is wholly padded computed exp2(-inf - -inf).  k_attn_lds<1> was right.)"""
    _set_mode(monkeypatch, mode)
    q, k, v, ref, bound = fwd_case(name, B0, H0, T)
    tight = _forward(q, k, v, gpu)[0]
    out = _forward(q, k, v, gpu, Tp=ceil64(T) + extra)[0]
    assert torch.isfinite(out.float()).all()
    r = _ratio(out.float().cpu(), ref, bound)
    print(f"attention padded {name} T={T} +{extra} {mode}: err / bound {r:.3f}")
    assert r <= 1.0
    assert torch.equal(out, tight)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_attention_hygiene(gpu, mode, monkeypatch):
    _set_mode(monkeypatch, mode)
    q, k, v, _, _ = fwd_case("random", B0, H0, 65)
    n, guard = B0 * 65, 8
    ops = _pack(q, k, v, gpu)
    keep = [t.clone() for t in ops]  # before any launch
    buf = _launch(*ops, guard=guard)
    assert torch.equal(buf[n:], torch.full_like(buf[n:], 7.0))
    assert not (buf[:n] == 7.0).all(dim=1).any()  # every token row was written
    two = _launch(*ops, guard=guard)  # on the operands the first launch has seen
    assert torch.equal(buf, two)
    for a, b in zip(keep, ops):
        assert torch.equal(a, b)
    assert not ops[1][:, :, 65:].any() and not ops[2][..., 65:].any()


# ------------------------------------------------------------------------ backward
BWD_SHAPES = [(1, 2, 65), (2, 3, 129), (1, 2, 300)]


@functools.lru_cache(maxsize=None)
def bwd_case(name, B, H, T):
    """(q, k, v, dO, fp32 autograd gradients, autocast gradients), once."""
    q, k, v = _operands(name, B, H, T)
    g = torch.Generator().manual_seed(31 * T + H)
    do = _q(torch.randn(B, T, H * 64, generator=g))
    return q, k, v, do, _attn_ref(q, k, v, do, False), _attn_ref(q, k, v, do, True)


def _backward(q, k, v, do, gpu, Tp=None):
    """d_qkv of sd_attention_bwd with ao from sd_attention, as in training."""
    from scenedino_amd import _lib
    B, H, T, _ = q.shape
    ao = _forward(q, k, v, gpu)[0]
    qd, kd, vtd = _pack(q, k, v, gpu, Tp)
    return _lib.attention_bwd(qd, kd, vtd, ao, do.to(BF).to(gpu).view(B * T, H * 64), SCALE)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,T", BWD_SHAPES)
@pytest.mark.parametrize("name", ["sharp2", "negbias", "ramp_up", "ramp_down"])
def test_attention_bwd_families(gpu, name, B, H, T):
    """sd_attention_bwd with wide-range softmax statistics, under the project's gradient
    rule (at most 2 x the bf16-autocast yardstick, tests/test_vit_train.py).  The yardstick
    grows with the logit magnitude, since autocast rounds the logits to bf16.  Measured on
    MI355X, concatenated rel-L2 against fp32 over T = 65 / 129 / 300, native against yardstick:
    sharp2 0.0032 / 0.0031 / 0.0030 against 0.0090 / 0.0101 / 0.0109; negbias 0.0034 / 0.0031 /
    0.0028 against 0.0237 / 0.0272 / 0.0223; ramp_up 0.0083 / 0.0079 / 0.0078 against 0.0405 /
    0.0462 / 0.0509; ramp_down 0.0081 / 0.0077 / 0.0085 against 0.0396 / 0.0438 / 0.0413.
    Closest to its bound is always dq: at most 0.0213 (ramp_up, T = 65) against 2 x 0.0517."""
    q, k, v, do, g32, g16 = bwd_case(name, B, H, T)
    got = _split_dqkv(_backward(q, k, v, do, gpu), B, H, T)
    check_gradients(got, g32, g16, f"attention_bwd {name} {(B, H, T)}")


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,T", BWD_SHAPES)
def test_attention_bwd_padded_key_blocks(gpu, B, H, T):
    """The backward loops over ceil64(tokens) keys whatever tokens_pad is: the same bits."""
    q, k, v, do, _, _ = bwd_case("sharp2", B, H, T)
    tight = _backward(q, k, v, do, gpu)
    assert torch.equal(_backward(q, k, v, do, gpu, Tp=ceil64(T) + 64), tight)


@pytest.mark.gpu
@pytest.mark.parametrize("perm", PERMS)
@pytest.mark.parametrize("T", [1, 65, 129, 300])
def test_attention_bwd_onehot_analytic(gpu, T, perm):
    """P is the 0 / 1 routing matrix of pi up to e^-40, so dV[pi(i)] collects the dO rows
    routed to it: the float64 sum within 2^-8 sum |dO_i| per element (one bf16 rounding of
    the f32 sum, doubled), bit-equal to dO where pi is a bijection; a key no query routes to
    has dV below e^-40 sum_i |dO_i| (its float64 value is not zero either).  dq and dk are
    zero up to the f32 rounding of the two 64-term dot products dP_i,pi(i) and D_i that
    cancel in dS: with eps_i = 2^-17 sum_e |dO_ie v_pi(i),e|, |dq_i| <= 0.125 eps_i (k is
    +-1) and |dk_j| <= 0.125 * 16 * sum_{i -> j} eps_i.  Measured on MI355X:
    |dq| at most 0.013 of its bound (T = 300, last), |dk| at most 0.013 (T = 300, identity);
    the largest dV entry of an unrouted key is 1.3e-28, not zero."""
    B, H = B0, H0
    q, k, v, pi, gap = onehot_case(B, H, T, perm)
    assert gap >= 40
    do = _q(torch.randn(B, T, H * 64, generator=torch.Generator().manual_seed(T + 7)))
    got = _split_dqkv(_backward(q, k, v, do, gpu), B, H, T)
    dO = do.view(B, T, H, 64).permute(0, 2, 1, 3).double()  # (B, H, T, 64)
    zero = torch.zeros(B, H, T, 64, dtype=torch.float64)
    ref = zero.index_add(2, pi, dO)
    mag = zero.index_add(2, pi, dO.abs())
    hit = torch.zeros(T, dtype=torch.bool).index_fill(0, pi, True)
    dv = got["dv"].double()
    tail = math.exp(-40) * dO.abs().sum(2, keepdim=True)  # what the other keys' p can carry
    assert ((dv - ref).abs() <= 2.0 ** -8 * mag + tail).all()
    if bool(hit.all()):
        assert torch.equal(got["dv"][:, :, pi], dO.float())
    stray = dv[:, :, ~hit].abs().max().item() if not bool(hit.all()) else 0.0
    eps = 2.0 ** -17 * (dO * v[:, :, pi].double()).abs().sum(-1)  # (B, H, T)
    bq = (0.125 * eps)[..., None]
    bk = (2.0 * torch.zeros(B, H, T, dtype=torch.float64).index_add(2, pi, eps))[..., None]
    rq = (got["dq"].double().abs() / bq).max().item()
    rk = (got["dk"].double().abs()[:, :, hit] / bk[:, :, hit]).max().item()
    print(f"attention_bwd onehot T={T} {perm}: |dq| / bound {rq:.3g}, |dk| / bound {rk:.3g}, "
          f"unrouted dV max {stray:.3g}")
    assert (got["dq"].double().abs() <= bq).all()
    assert (got["dk"].double().abs() <= bk + 16 * tail.sum(3, keepdim=True)).all()


# ------------------------------------------------------------------------ encoder
QK_GAIN = 3.0


@functools.lru_cache(maxsize=None)
def sharp_encoder_case():
    """The c128 geometry of tests/test_vit_train.py with the q and k thirds of every qkv
    scaled by QK_GAIN: (vit, images, fp32 oracle outputs, autocast oracle outputs, the
    oracle's pre-softmax logit std per block)."""
    from scenedino_amd.models.backbones.dino.vit import VisionTransformer
    C, nh = 128, 2
    vit = init_vit(VisionTransformer((32, 48), 16, C, 2, nh, layer_scale=True), seed=128)
    with torch.no_grad():
        for b in vit.blocks:
            b.attn.qkv.weight[:2 * C] *= QK_GAIN
            b.attn.qkv.bias[:2 * C] *= QK_GAIN
    images = torch.rand(2, 3, 32, 48, generator=torch.Generator().manual_seed(129)) * 2 - 1
    with torch.no_grad():
        # VO.block's attention restated: the logits each block's softmax sees
        t = F.conv2d(VO.normalize_input(images), vit.patch_embed.proj.weight,
                     vit.patch_embed.proj.bias, stride=16).flatten(2).transpose(1, 2)
        t = torch.cat([vit.cls_token.expand(2, -1, -1), t], 1) + vit.pos_embed
        stds = []
        for b in vit.blocks:
            y = F.layer_norm(t, (C,), b.norm1.weight, b.norm1.bias, 1e-6)
            qkv = F.linear(y, b.attn.qkv.weight, b.attn.qkv.bias)
            qkv = qkv.reshape(2, -1, 3, nh, C // nh).permute(2, 0, 3, 1, 4)
            stds.append(((qkv[0] * (C // nh) ** -0.5) @ qkv[1].transpose(-2, -1)).std().item())
            t = VO.block(t, b, nh)
    ref = VO.encoder_forward(vit, images, [0, 1])
    with torch.autocast("cpu", dtype=BF):
        yard = [o.float() for o in VO.encoder_forward(vit, images, [0, 1])]
    return vit, images, ref, yard, stds


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_sharp_encoder_oracle_logits_and_yardstick():
    _, _, ref, yard, stds = sharp_encoder_case()
    print("sharp encoder: oracle logit std per block", [f"{s:.2f}" for s in stds])
    assert all(s >= 4 for s in stds)
    for r, y in zip(ref, yard):
        e = _rel(y, r)
        assert math.isfinite(e) and e > 0


@pytest.mark.gpu
def test_encoder_with_sharp_attention(gpu):
    """The only whole-encoder run whose attention leaves the near-uniform regime (oracle
    logit std >= 4 in both blocks): forward_grids against the fp32 oracle, per output at
    most 2 x the rel-L2 of the oracle under bf16 autocast.  Measured on MI355X (oracle logit
    std 8.5 and 9.6), native / yardstick per output: 0.0040 / 0.0052, 0.0065 / 0.0062,
    0.0067 / 0.0063."""
    import copy
    from scenedino_amd.models.backbones.dino.vit import _ViT
    vit, images, ref, yard, stds = sharp_encoder_case()
    assert all(s >= 4 for s in stds)
    m = _ViT(copy.deepcopy(vit), 16, intermediate_features=[0, 1]).to(gpu).eval()
    with torch.no_grad():
        grids, final = m.forward_grids(images.to(gpu))
    for i, (a, r, y) in enumerate(zip(grids + [final], ref, yard)):
        assert a.shape == r.shape
        e, n = _rel(y, r), _rel(a.float().cpu(), r)
        print(f"sharp encoder output {i}: native rel-L2 {n:.4f}, autocast yardstick {e:.4f}")
        assert math.isfinite(e) and e > 0
        assert n <= 2 * e, (i, n, e)
