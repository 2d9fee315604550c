"""What a cached pack, a folded record or a captured graph is valid for: one key format and
one optimizer-step count for every module (host-only).

A key holds, per tensor, its storage pointer and version counter, so it changes on
load_state_dict, in-place edits, .to() and Parameter replacement.  Shape and device are not
in the entry: a move to another device or a resize changes the pointer, and the encoder's key
is built at every graph replay, where the two extra fields were measured to double the host
time of the walk (ViT-B/14 + DPT, 237 tensors: 61 -> 123 us).

torch's fused optimizers update parameters in place without bumping their version counters
(observed on torch 2.10 / ROCm 7.0: Adam's default and foreach=False steps take every
parameter's _version from 1 to 2, fused=True leaves it at 1), so the key of a module that
trains natively also carries the number of optimizer steps that touched it: its training
forward calls ``track_steps``, and one process-wide step post-hook then counts, per tracked
module, the steps of optimizers that hold one of its parameters.  Steps of other optimizers
(one for the field head alone, say) leave a module's packs and graphs alone.  An update that
neither shows -- a raw ``.data`` write, an optimizer that does not go through
``Optimizer.step``, the replay of a HIP graph that captured the step -- has to be followed by
dropping the cache by hand.
"""
from __future__ import annotations

import weakref

from torch.optim import optimizer

_TRACKED = weakref.WeakSet()
_HOOK = None


def tensor_key(*tensors):
    return tuple((t.data_ptr(), t._version) for t in tensors)


def steps(module) -> int:
    """Optimizer steps that touched a tracked module; 0 for one that never trained."""
    return module.__dict__.get("_step_gen", 0)


def module_key(*modules):
    """tensor_key over every parameter and buffer of the given modules (None entries are
    skipped), each module's entries followed by ("step", n) once its step count n is non-zero:
    a module that never trained keys as its raw tensors do.  The parameter and buffer dicts
    of the submodules that hold any are collected once per module (a recursive m.parameters()
    walk costs ~0.3 ms of host time per encode for ViT + DPT, enough to starve the launch
    queue); re-structuring a module after its first key is not tracked."""
    key = []
    for m in modules:
        if m is None:
            continue
        dicts = m.__dict__.get("_sd_tensor_dicts")
        if dicts is None:
            dicts = m.__dict__["_sd_tensor_dicts"] = [
                d for x in m.modules() for d in (x._parameters, x._buffers) if d]
        key += [(t.data_ptr(), t._version) for d in dicts for t in d.values() if t is not None]
        n = m.__dict__.get("_step_gen", 0)
        if n:
            key.append(("step", n))
    return tuple(key)


def track_steps(module):
    """Count, in ``module._step_gen`` (a plain attribute, never in the state dict), the steps
    of every optimizer that holds one of the module's parameters, from now on.  Idempotent."""
    global _HOOK
    module.__dict__.setdefault("_step_gen", 0)
    _TRACKED.add(module)
    if _HOOK is None:
        def _bump(optimizer, args, kwargs):
            ids = {id(p) for grp in optimizer.param_groups for p in grp["params"]}
            for m in list(_TRACKED):
                if any(id(p) in ids for p in m.parameters()):
                    m._step_gen += 1

        _HOOK = optimizer.register_optimizer_step_post_hook(_bump)
