"""scenedino_amd/pack_cache.py: the one key format and the one optimizer-step hook (CPU)."""
import gc

import torch
from torch import nn
from torch.optim import optimizer

from scenedino_amd import pack_cache as PC


def _net():
    return nn.Sequential(nn.Linear(3, 4), nn.BatchNorm1d(4))  # parameters and buffers


def test_step_count_follows_its_own_modules_entries():
    a, b = _net(), _net()
    plain = PC.module_key(a, None, b)
    assert plain == PC.module_key(a) + PC.module_key(b)
    assert plain == PC.tensor_key(*a.parameters(), *a.buffers(), *b.parameters(), *b.buffers())
    b._step_gen = 2
    key = PC.module_key(a, None, b)
    assert key != plain and key.count(("step", 2)) == 1
    assert key == PC.module_key(a) + PC.tensor_key(*b.parameters(), *b.buffers()) + (("step", 2),)
    assert PC.steps(a) == 0 and PC.steps(b) == 2
    # the other order: the count sits between the two modules' entries
    assert PC.module_key(b, a) == PC.module_key(b) + PC.module_key(a)
    assert PC.module_key(b, a).index(("step", 2)) == len(PC.module_key(b)) - 1


def test_track_steps_is_idempotent_and_installs_one_hook():
    m, other = _net(), nn.Linear(2, 2)
    before = len(optimizer._global_optimizer_post_hooks)
    had_hook = PC._HOOK is not None
    PC.track_steps(m)
    hook = PC._HOOK
    assert len(optimizer._global_optimizer_post_hooks) == before + (0 if had_hook else 1)
    for p in list(m.parameters()) + list(other.parameters()):
        p.grad = torch.zeros_like(p)
    torch.optim.SGD(other.parameters(), lr=0.1).step()
    assert m._step_gen == 0
    torch.optim.SGD(m.parameters(), lr=0.1).step()
    assert m._step_gen == 1
    PC.track_steps(m)
    assert PC._HOOK is hook and m._step_gen == 1
    assert len(optimizer._global_optimizer_post_hooks) == before + (0 if had_hook else 1)
    torch.optim.SGD(m.parameters(), lr=0.1).step()
    assert m._step_gen == 2 and PC.steps(m) == 2  # one bump per step: one hook
    assert "_step_gen" not in m.state_dict()


def test_tracked_set_holds_modules_weakly():
    m = _net()
    PC.track_steps(m)
    ident = id(m)
    assert any(id(x) == ident for x in PC._TRACKED)
    del m
    gc.collect()
    assert not any(id(x) == ident for x in PC._TRACKED)


def test_buffer_edit_and_load_state_dict_change_the_key():
    m = _net()
    k0 = PC.module_key(m)
    m[1].running_mean.add_(1.0)
    k1 = PC.module_key(m)
    assert k1 != k0
    m.load_state_dict(_net().state_dict())
    k2 = PC.module_key(m)
    assert k2 != k1
    m[0].weight = nn.Parameter(torch.zeros(4, 3))  # Parameter replacement
    assert PC.module_key(m) != k2
