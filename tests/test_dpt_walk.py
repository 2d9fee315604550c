"""DPTHead.forward_nhwc is one walk for inference and training (CPU, no kernels).

_lib.conv3x3 / linear_nhwc / upsample2x are replaced by recorders that return zero tensors of
the right shape and dtype, so what is compared is the sequence of kernel calls and the
identity of their packed operands: an eval pass under no_grad, two train passes with grad
enabled and another eval pass, all on one head with unchanged parameters.
"""
import pytest
import torch

from scenedino_amd import _lib
from scenedino_amd.models.backbones.dino import dpt_autograd as A
from scenedino_amd.models.backbones.dino.dpt_head import DPTHead

N_EVAL, N_TRAIN = 35, 37
FRONT_EVAL, FRONT_TRAIN = 4, 6  # calls of levels 0 and 1: folded GEMM + convs[i] / unfolded


class Recorder:
    def __init__(self):
        self.calls, self.dgrad3, self.dgrad1 = [], 0, 0

    def take(self):
        got = self.calls, self.dgrad3, self.dgrad1
        self.calls, self.dgrad3, self.dgrad1 = [], 0, 0
        return got

    def conv3x3(self, x, w, bias, stride=1, relu_in=False, epi=None, out=None, res=None, res2=None):
        assert out is None and x.dtype == torch.bfloat16 and w.shape[1] == 9 * x.shape[3]
        B, H, W, _ = x.shape
        shape = (B, (H - 1) // stride + 1, (W - 1) // stride + 1, w.shape[0])
        for r in (res, res2):
            assert r is None or tuple(r.shape) == shape
        self.calls.append(dict(op="conv3x3", w=w, bias=bias, stride=stride, relu_in=bool(relu_in),
                               res=res is not None, res2=res2 is not None, epi=epi))
        return torch.zeros(shape, dtype=torch.float32 if epi == _lib.SD_EPI_F32 else torch.bfloat16)

    def linear_nhwc(self, x, w, bias, epi=None, out=None, shuf=None, res=None):
        assert out is None and res is None and x.dtype == torch.bfloat16 and w.shape[1] == x.shape[3]
        B, H, W, _ = x.shape
        k = shuf or 1
        self.calls.append(dict(op="linear_nhwc", w=w, bias=bias, shuf=shuf, epi=epi))
        return torch.zeros(B, H * k, W * k, w.shape[0] // (k * k), dtype=torch.bfloat16)

    def upsample2x(self, x):
        B, H, W, C = x.shape
        self.calls.append(dict(op="upsample2x"))
        return torch.zeros(B, 2 * H, 2 * W, C, dtype=torch.bfloat16)


def same(a, b):
    """Two recorded calls: the same op on the same operand objects with the same options."""
    return a.keys() == b.keys() and all(
        a[k] is b[k] if k in ("w", "bias") else a[k] == b[k] for k in a)


@pytest.fixture(scope="module")
def walk():
    rec = Recorder()
    torch.manual_seed(0)
    head = DPTHead(embed_dims=64, post_process_channels=[32, 32, 64, 64], d_out=64)
    xs = [torch.zeros(1, 2, 4, 64, dtype=torch.bfloat16) for _ in range(4)]
    d3, d1 = A.pack_dgrad3, A.pack_dgrad1

    def pack_dgrad3(w):
        rec.dgrad3 += 1
        return d3(w)

    def pack_dgrad1(w):
        rec.dgrad1 += 1
        return d1(w)

    out = {"head": head}
    with pytest.MonkeyPatch.context() as mp:
        for name in ("conv3x3", "linear_nhwc", "upsample2x"):
            mp.setattr(_lib, name, getattr(rec, name))
        mp.setattr(A, "pack_dgrad3", pack_dgrad3)
        mp.setattr(A, "pack_dgrad1", pack_dgrad1)
        head.eval()
        with torch.no_grad():
            out["eval_out"] = head.forward_nhwc(xs)[0]
        out["eval"] = rec.take()
        head.train()
        out["train_out"] = head.forward_nhwc(xs)[0]
        out["train"] = rec.take()
        head.forward_nhwc(xs)
        out["train2"] = rec.take()
        head.eval()
        with torch.no_grad():
            head.forward_nhwc(xs)
        out["eval2"] = rec.take()
        out["rec"], out["xs"] = rec, xs
        yield out  # the recorders stay in place for the tests


def test_call_counts_and_outputs(walk):
    assert len(walk["eval"][0]) == N_EVAL and len(walk["train"][0]) == N_TRAIN
    assert walk["eval_out"].shape == (1, 64, 32, 64) and walk["eval_out"].dtype == torch.float32
    assert walk["eval_out"].grad_fn is None
    out = walk["train_out"]
    assert out.shape == (1, 64, 32, 64) and out.dtype == torch.float32 and out.grad_fn is not None


def test_both_modes_make_the_same_calls_from_level_2_on(walk):
    ev, tr = walk["eval"][0][FRONT_EVAL:], walk["train"][0][FRONT_TRAIN:]
    assert len(ev) == len(tr) == N_EVAL - FRONT_EVAL
    for i, (a, b) in enumerate(zip(ev, tr)):
        assert same(a, b), (i, a, b)
    assert ev[-1]["op"] == "conv3x3" and ev[-1]["epi"] == _lib.SD_EPI_F32


def test_levels_0_and_1(walk):
    """Inference: the folded GEMM, then convs[i]; training: projection, ConvTranspose, then
    convs[i] on the same operands as inference."""
    ev, tr = walk["eval"][0], walk["train"][0]
    head = walk["head"]
    for i in (0, 1):
        fold, conv_e = ev[2 * i], ev[2 * i + 1]
        proj, up, conv_t = tr[3 * i: 3 * i + 3]
        k = head.reassemble_blocks.resize_layers[i].kernel_size[0]
        assert [fold["op"], conv_e["op"]] == ["linear_nhwc", "conv3x3"] and fold["shuf"] == k
        assert [proj["op"], up["op"]] == ["linear_nhwc"] * 2
        assert proj["shuf"] is None and up["shuf"] == k
        assert fold["w"].shape == up["w"].shape[:1] + proj["w"].shape[1:]
        assert same(conv_e, conv_t)
        assert tuple(conv_e["w"].shape) == (64, 9 * 32) and conv_e["bias"] is None


def test_data_gradient_operands_come_with_the_first_train_pass_only(walk):
    assert walk["eval"][1:] == (0, 0)
    assert walk["train"][1:] == (22, 11)
    assert walk["train2"][1:] == (0, 0) and walk["eval2"][1:] == (0, 0)
    assert len(walk["train2"][0]) == N_TRAIN
    for a, b in zip(walk["train"][0], walk["train2"][0]):
        assert same(a, b)


def test_forward_operands_survive_the_train_pass(walk):
    assert len(walk["eval2"][0]) == N_EVAL
    for a, b in zip(walk["eval"][0], walk["eval2"][0]):
        assert same(a, b)


def test_train_mode_refuses_last_false(walk):
    head, rec = walk["head"], walk["rec"]
    head.train()
    try:
        with pytest.raises(NotImplementedError, match="last=False"):
            head.forward_nhwc(walk["xs"], last=False)
    finally:
        head.eval()
    assert rec.take() == ([], 0, 0)
