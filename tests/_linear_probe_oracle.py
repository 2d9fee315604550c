"""CPU formula of the linear probes, restated from the reference (LinearHead.forward,
scenedino/downstream_head/semantic_head.py:468-477, behind forward_training's ``_norm`` :37-38 and
its Dropout2d written as an explicit scale) for tests/test_linear_probe.py and
test_linear_probe_gpu.py, plus the seeded inputs the two share.

  xh = (normalize ? x / max(|x|, 1e-10) : x) o m        (normalised first, masked second)
  z  = W xh + b,  pred = argmax z,  loss = cross_entropy(z, target, ignore_index=-1)

Targets outside [0, C) are ignored; the tests only use -1 for them, which is what
F.cross_entropy's ignore_index takes.
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

import _stego_oracle as so
from _stego_oracle import check, dropout_scales, rel_l2  # noqa: F401  (shared with the tests)

BF = so.BF
RPG = 48  # rows per mask group: does not divide the kernel's 32-row tile


def xhat(x, m=None, rows_per_group=1, normalize=True):
    x = x.float()
    xh = F.normalize(x, dim=-1, eps=1e-10) if normalize else x
    if m is not None:
        xh = xh * so.rows_scale(m, rows_per_group, x.shape[0])
    return xh


def logits(xh, W, b):
    return F.linear(xh, W, b)


def logits_bf16(xh, W, b):
    """The CPU bf16 evaluation of the logits (tests/test_cluster_probe.py's convention: both
    operands rounded to bf16, the product returned in bf16)."""
    return (xh.to(BF) @ W.to(BF).t()).float() + b


def row_loss(z, target):
    """(N) per-row cross-entropy, 0 on ignored rows."""
    return F.cross_entropy(z, target.long(), ignore_index=-1, reduction="none")


def probe_eval(x, W, b, target, m=None, rows_per_group=1, normalize=True, autocast=False):
    """{"loss", "gW", "gb"}: the mean cross-entropy over the valid rows and its gradients by CPU
    autograd, in fp32 or under bf16 autocast."""
    Wl, bl = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=BF, enabled=autocast):
        z = F.linear(xhat(x, m, rows_per_group, normalize), Wl, bl).float()
        loss = F.cross_entropy(z, target.long(), ignore_index=-1)
    gW, gb = torch.autograd.grad(loss.float(), (Wl, bl))
    return {"loss": loss.detach().float().view(1), "gW": gW.float(), "gb": gb.float()}


# seed offset of the clustered family per shape (see inputs)
OFFSETS = {(4100, 64, 19): 4}


@functools.lru_cache(maxsize=None)
def inputs(family, N, d, C):
    """W (C, d) with rows of norm 4..8, b, x (N, d), m ((N + 47) // 48, d), target (N) with about
    20 % of -1 (row 0 always valid).  Family "a": clustered rows
    x = (W^_cls + 0.3 randn / sqrt(d)) U(0.01, 3); family "b": unstructured randn rows.

    Seed 31 N + 7 d + C + offset.  Family (a)'s precondition (the smallest fp32 top-2 margin over
    4 x the largest logit error of the CPU bf16 evaluation, asserted in the test) holds at
    offset 3 in every case of the grid but (4100, 64, 19), where one masked row has a margin of
    0.0018; that shape takes offset 4.  Offsets 3..14 were tried: 4..12 hold everywhere, 13
    fails at (4100, 64, 19) and 14 at (4100, 64, 32), each time at d = 64 with masks."""
    off = OFFSETS.get((N, d, C), 3) if family == "a" else 100000
    g = torch.Generator().manual_seed(31 * N + 7 * d + C + off)
    W = F.normalize(torch.randn(C, d, generator=g), dim=1) * (torch.rand(C, 1, generator=g) * 4 + 4)
    b = torch.randn(C, generator=g) * 0.1
    cls = torch.randint(C, (N,), generator=g)
    if family == "a":
        x = (F.normalize(W, dim=1)[cls] + 0.3 * torch.randn(N, d, generator=g) / d ** 0.5) \
            * (torch.rand(N, 1, generator=g) * 2.99 + 0.01)
    else:
        x = torch.randn(N, d, generator=g)
    m = dropout_scales((N + RPG - 1) // RPG, d, g)
    target = torch.where(torch.rand(N, generator=g) < 0.2, torch.full((N,), -1), cls)
    target[0] = cls[0]
    return W, b, x, m, target


# a ten-entry label table of the tests' own (ids, trainIds and colours are made up): one entry
# with id -1, one with trainId 255, one with trainId -1, a repeated id, gaps between the ids
class _Label:
    def __init__(self, name, id, trainId, color):
        self.name, self.id, self.trainId, self.color = name, id, trainId, color


def stub_label_module(n_train=19):
    import types
    rows = [("void", 0, 255, (0, 0, 0)), ("ground", 1, 0, (10, 20, 30)), ("wall", 2, 1, (40, 50, 60)),
            ("pole", 5, 2, (70, 80, 90)), ("sky", 6, 3, (1, 2, 3)), ("bike", 9, 4, (4, 5, 6)),
            ("far", 200, 5, (7, 8, 9)), ("last", 255, 6, (9, 9, 9)), ("plate", -1, -1, (0, 0, 1)),
            ("pole2", 5, 7, (3, 3, 3))]
    mod = types.ModuleType("datasets.kitti_360.labels")
    mod.labels = [_Label(*r) for r in rows]
    by_train = {lab.trainId: lab for lab in mod.labels}
    for i in range(n_train):  # SemanticHead._colors reads trainId2label[0 .. gt_classes)
        by_train.setdefault(i, _Label(f"pad{i}", 1000 + i, i, (i, i, i)))
    mod.trainId2label = by_train
    return mod


def install_stub_labels(monkeypatch, n_train=19):
    """Put the stub table where ``from datasets.kitti_360 import labels`` finds it."""
    import sys
    import types
    mod = stub_label_module(n_train)
    pkg, sub = types.ModuleType("datasets"), types.ModuleType("datasets.kitti_360")
    pkg.kitti_360, sub.labels = sub, mod
    pkg.__path__, sub.__path__ = [], []
    monkeypatch.setitem(sys.modules, "datasets", pkg)
    monkeypatch.setitem(sys.modules, "datasets.kitti_360", sub)
    monkeypatch.setitem(sys.modules, "datasets.kitti_360.labels", mod)
    return mod
