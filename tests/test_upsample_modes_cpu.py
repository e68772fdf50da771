"""nn.Upsample(scale_factor=2) in nearest and half-pixel trilinear mode (csrc/upsample.hip), what can be checked without a
GPU: the mode resolution of models/modular_unet.py:_run_upsample, the argument checks of the eight entry points and of
m355_upsample2x_plan (one fault and two faults; these calls return before any launch, the pointers are integers that are
never followed), the plan of dense, padded and misaligned calls, and the identity of torch's two nearest index maps at
factor 2.  Modelled on tests/test_resample_routes_cpu.py."""
import ctypes as C
import itertools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from segmentation_pipeline_amd import _lib, ops
from segmentation_pipeline_amd.models import ModularUNet
from segmentation_pipeline_amd.models.modular_unet import _run_upsample, _upsample_route

EINVALID = -1
SCALAR, VECTOR = 0, 1
NEAREST, HP = 0, 1
FWD, BWD = 0, 1
KEYS = sorted(_lib.UPSAMPLE2X_OPS)
IDS = [_lib.UPSAMPLE2X_OPS[k][0] for k in KEYS]
WORD = {"n": b"null", "d": b"non-positive", "c": b"compute", "a": b"aligned"}
BASE_PTR = (1 << 20, 2 << 20, 3 << 20, 4 << 20)


# ------------------------------------------------------------------------------------------------ mode resolution
ACCEPTED = [
    (dict(scale_factor=2), "upsample_nearest2x"),                                   # nn.Upsample's own default mode
    (dict(scale_factor=2, mode="nearest"), "upsample_nearest2x"),
    (dict(scale_factor=2.0, mode="nearest-exact"), "upsample_nearest2x"),
    (dict(scale_factor=(2, 2, 2), mode="nearest"), "upsample_nearest2x"),
    (dict(scale_factor=2, mode="trilinear", align_corners=True), "upsample_trilinear2x"),
    (dict(scale_factor=(2.0, 2.0, 2.0), mode="trilinear", align_corners=True), "upsample_trilinear2x"),
    (dict(scale_factor=2, mode="trilinear"), "upsample_trilinear2x_hp"),            # align_corners=None means False
    (dict(scale_factor=2, mode="trilinear", align_corners=False), "upsample_trilinear2x_hp"),
    (dict(scale_factor=(2.0, 2.0, 2.0), mode="trilinear", align_corners=False), "upsample_trilinear2x_hp"),
    (dict(scale_factor=2, mode="trilinear", recompute_scale_factor=False), "upsample_trilinear2x_hp"),
]
REJECTED = [
    dict(scale_factor=3), dict(scale_factor=1.5, mode="trilinear"), dict(scale_factor=(2, 2, 1)), dict(scale_factor=(2, 2)),
    dict(scale_factor=(2, 2, 2, 2)), dict(size=(8, 8, 8)), dict(size=8, mode="trilinear", align_corners=True),
    dict(scale_factor=2, recompute_scale_factor=True), dict(scale_factor=2, mode="trilinear", recompute_scale_factor=True),
    dict(scale_factor=2, mode="bilinear"), dict(scale_factor=2, mode="bicubic"), dict(scale_factor=2, mode="linear"),
    dict(scale_factor=2, mode="area"), dict(scale_factor=2, mode="nearest", align_corners=True),
    dict(scale_factor=2, mode="nearest", align_corners=False),
]


@pytest.mark.parametrize("params,route", ACCEPTED, ids=lambda v: str(v).replace(" ", "") if isinstance(v, dict) else v)
def test_accepted_spellings_resolve_to_their_route(params, route, monkeypatch):
    assert _upsample_route(nn.Upsample(**params)) is getattr(ops, route)
    # _run_upsample hands the tensor and the slot to that function (looked up when called)
    seen = []
    monkeypatch.setattr(ops, route, lambda x, out=None: seen.append((x, out)) or "y")
    assert _run_upsample(nn.Upsample(**params), "x", out="slot") == "y" and seen == [("x", "slot")]


@pytest.mark.parametrize("params", REJECTED, ids=lambda v: str(v).replace(" ", ""))
def test_other_spellings_are_refused_with_the_supported_list(params):
    with pytest.raises(NotImplementedError, match="nearest-exact") as e:
        _run_upsample(nn.Upsample(**params), None)
    msg = str(e.value)
    assert "align_corners=True" in msg and "align_corners=False" in msg and "size=" in msg and "recompute_scale_factor" in msg


def test_the_constructor_takes_the_stock_defaults():
    """upsample_params as a user writes them reach nn.Upsample untouched; no parameters, so a state_dict of the default
    model loads"""
    torch.manual_seed(0)
    ref = ModularUNet(2, 3, [8, 16, 16], 3)
    for params, route in (({'scale_factor': 2}, ops.upsample_nearest2x),
                          ({'scale_factor': 2, 'mode': 'trilinear'}, ops.upsample_trilinear2x_hp),
                          ({'scale_factor': 2, 'mode': 'trilinear', 'align_corners': False}, ops.upsample_trilinear2x_hp)):
        m = ModularUNet(2, 3, [8, 16, 16], 3, upsample_params=dict(params))
        assert all(_upsample_route(u) is route for u in m.upsampling) and len(m.upsampling) == 2
        m.load_state_dict(ref.state_dict())
    assert all(_upsample_route(u) is ops.upsample_trilinear2x for u in ref.upsampling)


def test_ops_mode_argument_defaults_to_align_corners():
    """ops.upsample_trilinear2x(x) is today's behaviour; an unknown mode and a CPU tensor fail loudly"""
    with pytest.raises(ValueError, match="mode"):
        ops.upsample_trilinear2x(torch.zeros(1, 1, 2, 2, 2), mode="bicubic")
    for fn in (ops.upsample_trilinear2x, ops.upsample_nearest2x, ops.upsample_trilinear2x_hp):
        with pytest.raises(_lib.M355Error, match="no CPU fallback"):
            fn(torch.zeros(1, 1, 2, 2, 2))


def test_nearest_equals_nearest_exact_at_factor_2():
    """torch's two nearest index maps, floor(o * 0.5) and floor((o + 0.5) * 0.5), coincide at scale factor 2 -- on odd
    sizes and size 1 too -- so one kernel serves both modes (forward bits and gradient)"""
    g = torch.Generator().manual_seed(0)
    for shape in [(1, 2, 1, 1, 1), (2, 3, 2, 3, 5), (1, 1, 7, 4, 9), (1, 2, 16, 16, 16)]:
        x = torch.randn(shape, generator=g)
        x.view(-1)[0] = float("nan")
        a = F.interpolate(x, scale_factor=2, mode="nearest")
        b = F.interpolate(x, scale_factor=2, mode="nearest-exact")
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        dy = torch.randn(a.shape, generator=g)
        grads = []
        for mode in ("nearest", "nearest-exact"):
            xr = torch.zeros(shape, requires_grad=True)
            grads.append(torch.autograd.grad(F.interpolate(xr, scale_factor=2, mode=mode), xr, dy)[0])
        assert torch.equal(*grads)
    for n in range(1, 64):
        o = torch.arange(2 * n)
        assert torch.equal(torch.floor(o * 0.5).long().clamp(max=n - 1), torch.floor((o + 0.5) * 0.5).long().clamp(max=n - 1))
        assert torch.equal(torch.floor(o * 0.5).long(), o // 2)


# ------------------------------------------------------------------------------------------------ bindings
def test_symbols_are_bound_with_their_counterparts_argument_lists():
    S = _lib.SIGNATURES
    assert len(_lib.RESAMPLE_OPS) == 17 and len(KEYS) == 8
    for (mode, direction, c8), (name, order, nstr, checks) in _lib.UPSAMPLE2X_OPS.items():
        twin = "m355_upsample_trilinear2x_" + ("bwd" if direction else "fwd") + ("_h16" if c8 else "")
        assert S["m355_" + name] == S[twin], name
        assert getattr(_lib.lib(), "m355_" + name) is not None
        assert (order, nstr, checks) == ((0, 1), 2, "ndca" if c8 else "dn")
        assert ("nearest" in name) == (mode == NEAREST) and ("_hp_" in name) == (mode == HP)
    assert sorted(IDS) == sorted([
        "upsample_nearest2x_fwd", "upsample_nearest2x_bwd", "upsample_nearest2x_fwd_h16", "upsample_nearest2x_bwd_h16",
        "upsample_trilinear2x_hp_fwd", "upsample_trilinear2x_hp_bwd", "upsample_trilinear2x_hp_fwd_h16",
        "upsample_trilinear2x_hp_bwd_h16"])


# ------------------------------------------------------------------------------------------------ plans
def plan(key, shape, bs, ptr, compute=_lib.COMPUTE_BF16):
    out = (C.c_int64 * 8)()
    rc = _lib.lib().m355_upsample2x_plan(*key, *shape, (C.c_int64 * 3)(*bs), (C.c_uint64 * 4)(*ptr), compute, out)
    return rc, tuple(out)


def dense_strides(key, C_, D, H, W):
    """(input-sized tensor, 2x tensor) in the entry point's order: forward x | y, backward dy | dx"""
    S, CB = D * H * W, (C_ + 7) // 8
    small, big = (CB * S * 8, CB * S * 64) if key[2] else (C_ * S, C_ * S * 8)
    return (big, small) if key[1] == BWD else (small, big)


def expected_code(key, shape, bs, ptr, compute):
    """the first failing check in the entry point's order: fp32 d, n; c8 n, d, c, a"""
    for check in _lib.UPSAMPLE2X_OPS[key][3]:
        if check == "n" and (ptr[0] == 0 or ptr[1] == 0):
            return EINVALID, check
        if check == "d" and min(shape) <= 0:
            return EINVALID, check
        if check == "c" and compute not in (_lib.COMPUTE_BF16, _lib.COMPUTE_F16):
            return EINVALID, check
        if check == "a":
            s = [b or d for b, d in zip(bs, dense_strides(key, *shape[1:]))]
            if ptr[0] % 16 or ptr[1] % 16 or s[0] % 8 or s[1] % 8:
                return EINVALID, check
    return 0, None


def expected_plan(key, shape, bs, ptr):
    """(variant, grid x, 1, 1, 0, strides): a thread per input voxel (c8: per input item), per x pair on the fp32 vector
    variant, per pair of output items in the c8 half-pixel forward; grid-stride, at most 65536 blocks of 256"""
    mode, direction, c8 = key
    N, C_, D, H, W = shape
    s = [b or d for b, d in zip(bs, dense_strides(key, C_, D, H, W))] + [0]
    big, small = (0, 1) if direction == BWD else (1, 0)        # index of the 2x tensor / the input-sized one
    variant = SCALAR
    if c8:
        total = N * ((C_ + 7) // 8) * D * H * W * (4 if (mode, direction) == (HP, FWD) else 1)
    else:
        vec = W % 2 == 0 and s[big] % 4 == 0 and ptr[big] % 16 == 0     # float4 rows of the 2x tensor
        if direction == BWD:
            vec = vec and s[small] % 2 == 0 and ptr[small] % 8 == 0     # float2 stores of dx
        variant = int(vec)
        total = N * C_ * D * H * (W // 2 if vec else W)
    return (variant, max(1, min(-(-total // 256), 65536)), 1, 1, 0) + tuple(s)


# (N, C, (D, H, W), pad of each batch stride in elements (0: passed as dense; c8: times 8), byte offset of each pointer)
CASES = [
    (1, 3, (1, 1, 1), (0, 0), (0, 0)), (2, 5, (2, 3, 5), (0, 0), (0, 0)), (1, 2, (3, 2, 4), (0, 0), (0, 0)),
    (1, 2, (2, 2, 3), (0, 0), (0, 0)), (2, 3, (4, 4, 8), (0, 0), (0, 0)),                       # dense
    (2, 3, (4, 4, 8), (4, 8), (0, 0)), (2, 3, (4, 4, 8), (8, 4), (0, 0)),                       # padded, still aligned
    (2, 3, (4, 4, 8), (2, 2), (0, 0)), (2, 3, (4, 4, 8), (1, 0), (0, 0)), (2, 3, (4, 4, 8), (0, 1), (0, 0)),   # padded off a row
    (2, 3, (4, 4, 8), (0, 0), (4, 0)), (2, 3, (4, 4, 8), (0, 0), (0, 4)), (2, 3, (4, 4, 8), (0, 0), (8, 0)),
    (2, 3, (4, 4, 8), (0, 0), (0, 8)), (2, 3, (4, 4, 8), (0, 0), (4, 4)),                       # shifted bases
    (1, 128, (32, 32, 32), (0, 0), (0, 0)), (1, 64, (64, 64, 64), (0, 0), (0, 0)),              # the decoder levels of cfg2
    (2, 32, (128, 128, 128), (0, 0), (0, 0)),                                                   # at the grid cap
]


def arguments(key, case):
    N, C_, vol, pads, offs = case
    if key[2]:
        pads, offs = [8 * p for p in pads], (0, 0)
    dense = dense_strides(key, C_, *vol)
    bs = [d + p if p else 0 for d, p in zip(dense, pads)] + [0]
    return (N, C_) + vol, bs, [BASE_PTR[0] + offs[0], BASE_PTR[1] + offs[1], 0, 0]


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_plans_agree_with_the_arguments(key):
    """variant, grid and strides of dense, padded and misaligned calls; nothing here is rejected -- odd sizes, size 1 and
    4-byte aligned fp32 tensors are served (the c8 cases are passed aligned: anything else is a code, below)"""
    variants = set()
    for case in CASES:
        shape, bs, ptr = arguments(key, case)
        rc, out = plan(key, shape, bs, ptr)
        assert rc == 0, (case, _lib.lib().m355_last_error())
        assert out == expected_plan(key, shape, bs, ptr), case
        variants.add(out[0])
    assert variants == ({SCALAR} if key[2] else {SCALAR, VECTOR})
    assert plan(key, *arguments(key, CASES[-1]))[1][1] == 65536


def test_each_term_of_the_vector_verdicts_decides():
    shape, zero = (2, 3, 4, 4, 8), [0, 0, 0]
    for key in KEYS:
        if key[2]:
            continue
        big, small = (0, 1) if key[1] == BWD else (1, 0)
        dense = dense_strides(key, *shape[1:])
        assert plan(key, shape, zero, BASE_PTR)[1][0] == VECTOR
        assert plan(key, (2, 3, 4, 4, 7), zero, BASE_PTR)[1][0] == SCALAR                      # odd W
        assert plan(key, (2, 3, 3, 5, 6), zero, BASE_PTR)[1][0] == VECTOR                      # odd D, H are no obstacle
        for pad, off, want in ((2, 8, SCALAR), (4, 16, VECTOR)):                               # the 2x tensor: 16 bytes
            bs, ptr = list(zero), list(BASE_PTR)
            bs[big] = dense[big] + pad
            assert plan(key, shape, bs, BASE_PTR)[1][0] == want
            ptr[big] += off
            assert plan(key, shape, zero, ptr)[1][0] == want
        # the input-sized tensor: read as scalars by the forward (any 4-byte alignment), stored as float2 by the backward
        for pad, off, want in ((1, 4, SCALAR if key[1] == BWD else VECTOR), (2, 8, VECTOR)):
            bs, ptr = list(zero), list(BASE_PTR)
            bs[small] = dense[small] + pad
            assert plan(key, shape, bs, BASE_PTR)[1][0] == want
            ptr[small] += off
            assert plan(key, shape, zero, ptr)[1][0] == want


# ------------------------------------------------------------------------------------------------ codes
VALID = dict(N=2, C=8, D=4, H=4, W=4, compute=_lib.COMPUTE_BF16, bs0=0, bs1=0, ptr0=BASE_PTR[0], ptr1=BASE_PTR[1])
# every way one argument can be wrong; whether it is a fault for a given entry point is the model's call (an odd size or
# a 4-byte offset of an fp32 tensor is served)
FAULTS = ([("ptr0", 0), ("ptr1", 0)] + [(k, 0) for k in "NCDHW"] + [("N", -1)] + [(k, 5) for k in "DHW"]
          + [("compute", 0), ("compute", 3)] + [(f"ptr{i}", BASE_PTR[i] + off) for i in range(2) for off in (4, 8)]
          + [(f"bs{i}", v) for i in range(2) for v in (8200, 8195)])


def fault_tuples():
    singles = [(f,) for f in FAULTS]
    pairs = [p for p in itertools.combinations(FAULTS, 2) if p[0][0] != p[1][0]]
    for faults in singles + pairs:
        a = dict(VALID)
        a.update(dict(faults))
        yield faults, tuple(a[k] for k in "NCDHW"), [a["bs0"], a["bs1"], 0], [a["ptr0"], a["ptr1"], 0, 0], a["compute"]


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_codes_of_one_and_two_faults(key):
    """every check on its own and every pair of two faults: the entry point answers in its counterpart's order (fp32:
    dimension, then null; c8: null, dimension, compute, alignment) with its own name and the check's word, and
    m355_upsample2x_plan answers the same code -- also where the call is valid"""
    L = _lib.lib()
    name, _, _, order = _lib.UPSAMPLE2X_OPS[key]
    fn = getattr(L, "m355_" + name)
    decided, rejected, served = set(), 0, 0
    for faults, shape, bs, ptr, compute in fault_tuples():
        code, check = expected_code(key, shape, bs, ptr, compute)
        assert plan(key, shape, bs, ptr, compute)[0] == code, (faults, L.m355_last_error())
        if code == 0:
            served += 1
            continue   # not a fault for this entry point: calling it would launch
        rc = fn(*_lib.resample_args(key, shape, bs, ptr, compute))
        msg = L.m355_last_error()
        assert rc == code, (faults, rc, msg)
        assert msg.startswith(name.encode() + b":") and WORD[check] in msg, (faults, msg)
        decided.add((check, len(faults)))
        rejected += 1
    assert decided == {(c, n) for c in order for n in (1, 2)}
    assert rejected >= 100 and served >= (1 if key[2] else 20)


def test_plan_query_rejects_its_own_bad_arguments():
    L = _lib.lib()
    bs, ptr, out = (C.c_int64 * 3)(), (C.c_uint64 * 4)(*BASE_PTR), (C.c_int64 * 8)()
    for key in ((-1, 0, 0), (2, 0, 0), (0, -1, 0), (0, 2, 0), (0, 0, -1), (0, 0, 2)):
        assert L.m355_upsample2x_plan(*key, 2, 8, 4, 4, 4, bs, ptr, 1, out) == EINVALID
        assert b"upsample2x_plan" in L.m355_last_error()
    assert L.m355_upsample2x_plan(0, 0, 0, 2, 8, 4, 4, 4, None, ptr, 1, out) == EINVALID
    assert L.m355_upsample2x_plan(0, 0, 0, 2, 8, 4, 4, 4, bs, None, 1, out) == EINVALID
    assert L.m355_upsample2x_plan(0, 0, 0, 2, 8, 4, 4, 4, bs, ptr, 1, None) == EINVALID
    for key in KEYS:
        assert L.m355_upsample2x_plan(*key, 2, 8, 4, 4, 4, bs, ptr, 1, out) == 0
    # the new rows stay behind their own query: m355_resample_plan still numbers 17 ops
    assert L.m355_resample_plan(17, 2, 8, 4, 4, 4, bs, ptr, 1, out) == EINVALID
