"""Memory-hygiene harness: operands carved out of guard-banded allocations.

GPU AddressSanitizer and debuggers are not available to this project, so the only way the
suite can see where a kernel reads and writes is to own the memory around every operand:

    [front margin | payload | back margin]          one torch.uint8 allocation per operand

The payload start is 16-byte aligned; each margin is at least 4 KiB and at least `tile_rows`
rows of `ld` elements (a whole output tile of the widest tiling the entry point can pick: 256
rows for sd_gemm / convolution outputs, 64 for row-wise kernels), so that an overrun by a
whole tile still lands in memory the test owns.  Nothing here is meant to fault: every call
uses arguments inside the documented domain.

  outputs  margins, row gaps (ld > width) and payload are filled with a sentinel bit pattern
           (a quiet NaN with a fixed payload for float types, a fixed negative value for
           integers).  After the call the margins and gaps must be bit-identical to the
           sentinel, and, where the header says the kernel writes every element, the payload
           must hold no sentinel.  Accumulate-into outputs are pre-set (`preset=`) and only
           their margins and gaps are checked.
  inputs   margins and gaps are poisoned -- NaN in one run, a large finite value in the next --
           and the whole buffer must be bit-identical to a clone taken before the call.
  work     exactly the bytes the size function promises, NaN-filled (or zeroed where the
           header says the caller zeroes them), a guard behind them.

`run3(device, body)` runs `body(arena)` three times -- NaN poison, finite poison, and plain
tight tensors from torch.empty / torch.zeros -- collects every arena finding and compares the
outputs of the three runs bit for bit (or, for the float-atomics kernels listed below, within
the bound their existing test uses against its reference).

Kernels that accumulate with floating-point atomics (summation order varies from launch to
launch, so their three runs agree only within their existing test's bound):
  sd_field_gather_bwd   scenedino_amd/csrc/sdhip_train.hip:225  unsafeAtomicAdd into dgrid_nhwc
                        (bound: rel_l2 < 1e-5, test_field_gather_fwd_bwd_gpu)
  sd_mlp_train_bwd      scenedino_amd/csrc/sdhip_mlp.hip:298  unsafeAtomicAdd into dgrid, with
                        dgrid != NULL only (the fused scatter); with dgrid == NULL it is
                        deterministic.

REGISTRY maps every `int sd_*(..., void *stream)` entry point of include/sdhip.h that has a
hygiene case to that case's test id; EXEMPT holds the entry points that need none, PENDING the
ones whose case is still to be written (tests/test_hygiene_registry.py pins both lists, so a
kernel added later without a case fails there, on the CPU).
"""
from __future__ import annotations

import torch

MIN_MARGIN = 4096  # bytes

# sentinel bit patterns, by element size and kind (float: quiet NaN with a fixed payload)
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_SENTINEL_FLOAT = {torch.float32: 0x7FC5A5A5, torch.float16: 0x7E5A, torch.bfloat16: 0x7FC5,
                   torch.float64: 0x7FF85A5A5A5A5A5A}
_SENTINEL_INT = {torch.int32: -0x5A5A5A5B, torch.int64: -0x5A5A5A5A5A5A5A5B, torch.int16: -0x5A5B,
                 torch.uint8: 0xA5, torch.int8: -0x5B, torch.bool: 0xA5}
# the large finite poison of the second input run
_BIG = {torch.float32: 1e30, torch.bfloat16: 1e30, torch.float16: 60000.0, torch.float64: 1e30}


def _signed(v, bits):
    return v - (1 << bits) if v >= (1 << (bits - 1)) else v


def sentinel_bits(dtype):
    """The sentinel of `dtype` as a value of its integer view (_INT_VIEW[itemsize])."""
    if dtype in _SENTINEL_FLOAT:
        return _signed(_SENTINEL_FLOAT[dtype], 8 * torch.empty(0, dtype=dtype).element_size())
    return _SENTINEL_INT[dtype]


def _finite_bits(dtype):
    if dtype in _BIG:
        t = torch.tensor([_BIG[dtype]], dtype=dtype)
        return int(t.view(_INT_VIEW[t.element_size()])[0])
    return sentinel_bits(dtype)  # integer inputs: the same fixed negative value in both runs


class _Operand:
    __slots__ = ("name", "role", "dtype", "shape", "ld", "raw", "ints", "view", "mask", "before",
                 "full", "inplace", "off", "n_pay")


class Arena:
    """Hands out operand views; see the module docstring.  poison: "nan", "finite", or None
    (plain: tight tensors straight from torch.empty, nothing checked)."""

    def __init__(self, device, poison="nan"):
        assert poison in ("nan", "finite", None)
        self.device = torch.device(device)
        self.poison = poison
        self.ops = {}
        self._armed = False

    # ---- carving -------------------------------------------------------------------------
    def _carve(self, name, role, shape, dtype, ld, tile_rows):
        assert name not in self.ops, f"operand {name} declared twice"
        shape = tuple(int(s) for s in shape)
        width = shape[-1] if shape else 1
        rows = 1
        for s in shape[:-1]:
            rows *= s
        op = _Operand()
        op.name, op.role, op.dtype, op.shape = name, role, dtype, shape
        op.full, op.inplace = False, False
        if self.poison is None:
            op.ld = width
            op.raw = op.ints = op.mask = op.before = None
            op.view = torch.empty(shape, dtype=dtype, device=self.device)
            self.ops[name] = op
            return op
        ld = width if ld is None else int(ld)
        assert ld >= width
        op.ld = ld
        isz = torch.empty(0, dtype=dtype).element_size()
        n_pay = max(rows * ld, 1)                      # payload span, trailing row gap included
        margin = max(MIN_MARGIN, tile_rows * ld * isz)
        margin = (margin + 15) // 16 * 16              # payload start stays 16-byte aligned
        tail = (n_pay * isz + 15) // 16 * 16
        op.raw = torch.empty(margin + tail + margin, dtype=torch.uint8, device=self.device)
        assert op.raw.data_ptr() % 16 == 0
        op.ints = op.raw.view(_INT_VIEW[isz])
        op.off, op.n_pay = margin // isz, n_pay
        typed = op.raw.view(dtype) if dtype != torch.bool else op.raw.view(torch.bool)
        strides = []
        acc = ld
        for s in reversed(shape[:-1]):
            strides.append(acc)
            acc *= s
        strides = tuple(reversed(strides)) + ((1,) if shape else ())
        op.view = torch.as_strided(typed, shape, strides, op.off)
        op.mask = torch.zeros(op.ints.numel(), dtype=torch.bool, device=self.device)
        torch.as_strided(op.mask, shape, strides, op.off).fill_(True)
        self.ops[name] = op
        return op

    def input(self, name, data, ld=None, tile_rows=64, inplace=False):
        """A view holding a copy of `data`; margins and row gaps poisoned.  inplace: the header
        declares the payload in-place (only margins and gaps must survive)."""
        op = self._carve(name, "in", data.shape, data.dtype, ld, tile_rows)
        op.inplace = inplace
        if self.poison is not None:
            bits = sentinel_bits(op.dtype) if self.poison == "nan" else _finite_bits(op.dtype)
            op.ints.fill_(bits)
        op.view.copy_(data)
        return op.view

    def output(self, name, shape, dtype, ld=None, tile_rows=64, full=True, preset=None):
        """An output view.  full: the header says every payload element is written (checked:
        no sentinel left).  preset: the values an accumulate-into output starts from (its
        payload is then not checked for sentinels)."""
        op = self._carve(name, "out", shape, dtype, ld, tile_rows)
        op.full = bool(full) and preset is None
        if self.poison is not None:
            op.ints.fill_(sentinel_bits(op.dtype))
        else:  # so that elements the kernel leaves alone compare equal across the three runs
            op.view.view(_INT_VIEW[op.view.element_size()]).fill_(sentinel_bits(op.dtype))
        if preset is not None:
            op.view.copy_(preset)
        return op.view

    def work(self, name, numel, dtype=torch.float32, zero=False):
        """Scratch of exactly `numel` elements (what the size function promised), NaN-filled
        unless the header says the caller zeroes it; a guard behind and in front."""
        op = self._carve(name, "work", (int(numel),), dtype, None, 64)
        if self.poison is not None:
            op.ints.fill_(sentinel_bits(op.dtype))
        else:
            op.view.view(_INT_VIEW[op.view.element_size()]).fill_(sentinel_bits(op.dtype))
        if zero:
            op.view.zero_()
        return op.view

    def raw(self, name):
        """(integer view of the whole allocation, element offset of the payload): for the
        harness's own tests."""
        op = self.ops[name]
        return op.ints, op.off

    # ---- checking ------------------------------------------------------------------------
    def arm(self):
        """Snapshot every buffer; call right before the kernel."""
        if self.poison is not None:
            for op in self.ops.values():
                op.before = op.ints.clone()
        self._armed = True

    def check(self):
        """Findings (strings) of the call made since arm(); [] = clean."""
        assert self._armed, "Arena.arm() was not called before the kernel"
        out = []
        if self.poison is None:
            return out
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for op in self.ops.values():
            changed = op.ints != op.before
            outside = changed & ~op.mask
            n = int(outside.sum())
            if n:
                idx = outside.nonzero().flatten()
                first = int(idx[0]) - op.off
                last = int(idx[-1]) - op.off
                where = []
                if first < 0:
                    where.append("front margin")
                if last >= op.n_pay:
                    where.append("back margin")
                inner = idx[(idx >= op.off) & (idx < op.off + op.n_pay)]
                if inner.numel():
                    where.append(f"row gap (first at row {int(inner[0] - op.off) // op.ld}, "
                                 f"column {int(inner[0] - op.off) % op.ld})")
                out.append(f"{op.name} ({op.role}): {n} elements outside the payload were written: "
                           f"{', '.join(where)}; element offsets {first}..{last} from the payload "
                           f"start [{self.poison} run]")
            if op.role == "in" and not op.inplace:
                n = int((changed & op.mask).sum())
                if n:
                    out.append(f"{op.name} (in): {n} payload elements of a read-only input changed "
                               f"[{self.poison} run]")
            if op.role == "out" and op.full:
                left = (op.ints == sentinel_bits(op.dtype)) & op.mask
                n = int(left.sum())
                if n:
                    first = int(left.nonzero()[0]) - op.off
                    out.append(f"{op.name} (out): {n} payload elements were never written (first at "
                               f"row {first // op.ld}, column {first % op.ld}) [{self.poison} run]")
        return out

    def results(self):
        """Dense clones of every output payload."""
        return {n: op.view.clone().contiguous() for n, op in self.ops.items() if op.role == "out"}


def _bit_equal(a, b):
    isz = a.element_size()
    if a.dtype == torch.bool:
        return bool((a == b).all())
    return bool((a.contiguous().view(_INT_VIEW[isz]) == b.contiguous().view(_INT_VIEW[isz])).all())


def run3(device, body, atomic_rel_l2=None):
    """Run body(arena) with NaN poison, finite poison and plain tight tensors.  `body` declares
    its operands on the arena, calls arena.arm() and then the kernel.  Returns (findings,
    outputs of the plain run).  atomic_rel_l2: for the float-atomics kernels of the module
    docstring, the bound within which the three runs must agree (and every output be finite)."""
    findings, res = [], {}
    for mode in ("nan", "finite", None):
        a = Arena(device, mode)
        body(a)
        findings += a.check()
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize(device)
        res[mode] = a.results()
    plain = res[None]
    for mode in ("nan", "finite"):
        for name, ref in plain.items():
            got = res[mode][name]
            if atomic_rel_l2 is None or not ref.is_floating_point():
                if not _bit_equal(got, ref):
                    nbad = int((got != ref).sum()) if not ref.is_floating_point() else \
                        int(((got != ref) & ~(got.isnan() & ref.isnan())).sum())
                    findings.append(f"{name}: the {mode}-poisoned run differs from the plain run in "
                                    f"{nbad} elements (poison leaked into the result)")
            else:
                g, r = got.double(), ref.double()
                if not bool(torch.isfinite(g).all()):
                    findings.append(f"{name}: non-finite values in the {mode}-poisoned run")
                elif float((g - r).norm() / r.norm().clamp_min(1e-30)) >= atomic_rel_l2:
                    findings.append(f"{name}: the {mode}-poisoned run differs from the plain run by "
                                    f"rel-L2 >= {atomic_rel_l2}")
    return findings, plain


def assert_clean(findings):
    assert not findings, "memory hygiene:\n  " + "\n  ".join(findings)


# ---- registry -------------------------------------------------------------------------------
_V, _D, _R, _H = ("tests/test_hygiene_vit.py::", "tests/test_hygiene_dpt.py::",
                  "tests/test_hygiene_render.py::", "tests/test_hygiene_heads.py::")
REGISTRY = {
    # sdhip_vit.hip / sdhip_vit_bwd.hip
    "sd_gemm": _V + "test_hygiene_gemm",
    "sd_ln_gemm": _V + "test_hygiene_ln_gemm",
    "sd_attention": "tests/test_attention.py::test_attention_hygiene",
    "sd_layernorm": _V + "test_hygiene_layernorm",
    "sd_layernorm_nhwc": _V + "test_hygiene_layernorm_nhwc",
    "sd_tokens_to_nhwc": _V + "test_hygiene_tokens_to_nhwc",
    "sd_tokens_to_grid": _V + "test_hygiene_tokens_to_grid",
    "sd_patchify": _V + "test_hygiene_patchify",
    "sd_attention_bwd": _V + "test_hygiene_attention_bwd",
    "sd_layernorm_bwd": _V + "test_hygiene_layernorm_bwd",
    "sd_gelu_bwd": _V + "test_hygiene_gelu_bwd",
    # DPT decoder (sd_gemm's convolution routes: test_hygiene_conv3x3_*, test_hygiene_linear_nhwc)
    "sd_upsample2x": _D + "test_hygiene_upsample2x",
    "sd_upsample2x_bwd": _D + "test_hygiene_upsample2x_bwd",
    "sd_relu_bwd": _D + "test_hygiene_relu_bwd",
    "sd_conv_wgrad": _D + "test_hygiene_conv_wgrad",
    # render / field / training MLP
    "sd_render_proj": _R + "test_hygiene_render_proj",
    "sd_render_fused": _R + "test_hygiene_render_fused",
    "sd_field_query": _R + "test_hygiene_field_query",
    "sd_composite": _R + "test_hygiene_composite",
    "sd_composite_bwd": _R + "test_hygiene_composite_bwd",
    "sd_field_gather": _R + "test_hygiene_field_gather",
    "sd_field_gather_bwd": _R + "test_hygiene_field_gather_bwd",
    "sd_gen_rays": _R + "test_hygiene_gen_rays",
    "sd_sample_z": _R + "test_hygiene_sample_z",
    "sd_patch_rays": _R + "test_hygiene_patch_rays",
    "sd_pack_grid": _R + "test_hygiene_pack_grid",
    "sd_unpack_grid": _R + "test_hygiene_unpack_grid",
    "sd_cast_grid": _R + "test_hygiene_cast_grid",
    "sd_pack_image": _R + "test_hygiene_pack_image",
    "sd_cam_records": _R + "test_hygiene_cam_records",
    "sd_frame_inputs": _R + "test_hygiene_frame_inputs",
    "sd_project_grid": _R + "test_hygiene_project_grid",
    "sd_project_grid_nhwc": _R + "test_hygiene_project_grid",
    "sd_project_grid_nhwc_inputs": _R + "test_hygiene_project_grid",
    "sd_mlp_train_fwd": _R + "test_hygiene_mlp_train_fwd_bwd",
    "sd_mlp_train_bwd": _R + "test_hygiene_mlp_train_fwd_bwd",
    "sd_wgrad": _R + "test_hygiene_wgrad",
    "sd_mlp_train_wgrad": _R + "test_hygiene_mlp_train_wgrad",
    # heads, SSCBench, downstream stage, losses
    "sd_voxel_points": _H + "test_hygiene_voxel_points",
    "sd_grow3": _H + "test_hygiene_grow3",
    "sd_seg_query": _H + "test_hygiene_seg_query",
    "sd_voxel_fov": _H + "test_hygiene_voxel_fov",
    "sd_ssc_confusion": _H + "test_hygiene_ssc_confusion",
    "sd_expand_bwd": _H + "test_hygiene_expand_bwd",
    "sd_stego_train_fwd": _H + "test_hygiene_stego_train",
    "sd_stego_train_bwd": _H + "test_hygiene_stego_train",
    "sd_cluster_probe": _H + "test_hygiene_cluster_probe",
    "sd_linear_probe": "tests/test_linear_probe_gpu.py::test_edge_cases",
    "sd_stego_corr_fwd": _H + "test_hygiene_stego_corr",
    "sd_stego_corr_bwd": _H + "test_hygiene_stego_corr",
    "sd_recon_loss_fwd": _H + "test_hygiene_recon_loss",
    "sd_recon_loss_bwd": _H + "test_hygiene_recon_loss",
    "sd_msc_gt": _H + "test_hygiene_msc_gt",
    "sd_crop3d_centres": _H + "test_hygiene_crop3d_centres",
    "sd_crop3d_compact": _H + "test_hygiene_crop3d_compact",
    "sd_salience_fwd": _H + "test_hygiene_salience",
    "sd_salience_bwd": _H + "test_hygiene_salience",
}

# entry points with nothing to guard
EXEMPT = {
    "sd_spin": "writes no memory (diagnostic busy-wait)",
}

# entry points whose hygiene case is not written yet: this list may only shrink
PENDING = {}
