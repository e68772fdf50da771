"""The factor-2 resampling family (csrc/resample_host.hpp) resolves a call on the host: m355_resample_plan reports the batch
strides, the kernel variant and the grid an entry point uses, and returns the code that entry point returns.  Both are
recomputed here from the arguments, entry point by entry point.  Pure host code, no GPU: an entry point itself is only ever
called with arguments it rejects (the model below says so before the call), so nothing is launched; the pointers are
integers that are never followed.  tools/conv_routes.py --resample is the larger table."""
import ctypes as C
import itertools

import pytest

from segmentation_pipeline_amd import _lib

EINVALID, EUNSUPPORTED = -1, -2
OPS = [o[0] for o in _lib.RESAMPLE_OPS]
(AVG_FWD, AVG_BWD, AVG_BWD_ADD, TRI_FWD, TRI_BWD, S2D, D2S, MAX_FWD, MAX_BWD, AVG_FWD_H16, AVG_BWD_H16, TRI_FWD_H16, TRI_BWD_H16,
 S2D_H16, D2S_H16, MAX_FWD_H16, MAX_BWD_H16) = range(17)
SCALAR, VECTOR, QUADS, LDS = 0, 1, 1, 2

# The order of each entry point's argument checks: n null pointer, d dimension <= 0, o odd size (M355_EUNSUPPORTED),
# c compute mode, a alignment (M355_EINVALID_ARG for c8 tensors, M355_EUNSUPPORTED for the fp32 space / depth pair).
ORDER = {
    "avgpool3d_2x_fwd": "dno", "avgpool3d_2x_bwd": "dno", "avgpool3d_2x_bwd_add": "dno",
    "upsample_trilinear2x_fwd": "dn", "upsample_trilinear2x_bwd": "dn",
    "maxpool3d_2x_fwd": "ndo", "maxpool3d_2x_bwd": "ndo",
    "space_to_depth2": "ndoa", "depth_to_space2": "ndoa",
    "upsample_trilinear2x_fwd_h16": "ndca", "upsample_trilinear2x_bwd_h16": "ndca",
    "space_to_depth2_h16": "ondca", "depth_to_space2_h16": "ondca",
    "maxpool3d_2x_fwd_h16": "ndoca", "maxpool3d_2x_bwd_h16": "ndoca", "avgpool3d_2x_fwd_h16": "ndoca",
    "avgpool3d_2x_bwd_h16": "cndoa",
}
# pointers that may be null (index into tensor 0, 1, 2, route bytes): the skip gradients, the forward's route output
OPTIONAL = {MAX_FWD: {3}, MAX_FWD_H16: {3}, MAX_BWD: {1}, MAX_BWD_H16: {1}, AVG_BWD_H16: {1}}
ROUTES = {MAX_FWD, MAX_BWD, MAX_FWD_H16, MAX_BWD_H16}
WORD = {"n": b"null", "d": b"non-positive", "o": b"odd", "c": b"compute", "a": b"aligned"}


def is_c8(op):
    return op >= AVG_FWD_H16


def nstrides(op):
    return _lib.RESAMPLE_OPS[op][2]


def dense_strides(op, C_, D, H, W):
    """dense batch stride of each tensor, in the order of the entry point's batch strides"""
    S, OS, CB = D * H * W, (D // 2) * (H // 2) * (W // 2), (C_ + 7) // 8
    full, half, x8 = (CB * S * 8, CB * OS * 8, CB * S * 64) if is_c8(op) else (C_ * S, C_ * OS, C_ * S * 8)
    packed = C_ * OS * 8
    return {AVG_FWD: (full, half), AVG_BWD: (half, full), AVG_BWD_ADD: (half, full, full), TRI_FWD: (full, x8), TRI_BWD: (x8, full),
            S2D: (full, packed), D2S: (packed, full), MAX_FWD: (full, half), MAX_BWD: (half, full, full),
            AVG_FWD_H16: (full, half), AVG_BWD_H16: (half, full, full), TRI_FWD_H16: (full, x8), TRI_BWD_H16: (x8, full),
            S2D_H16: (full, packed), D2S_H16: (packed, full), MAX_FWD_H16: (full, half), MAX_BWD_H16: (half, full, full)}[op]


def expected_code(op, shape, bs, ptr, compute):
    """the first failing check in the entry point's order"""
    N, C_, D, H, W = shape
    for check in ORDER[OPS[op]]:
        if check == "n":
            need = set(range(nstrides(op))) | ({3} if op in ROUTES else set())
            if any(ptr[i] == 0 for i in need - OPTIONAL.get(op, set())):
                return EINVALID, check
        elif check == "d" and min(shape) <= 0:
            return EINVALID, check
        elif check == "o" and (D % 2 or H % 2 or W % 2):
            return EUNSUPPORTED, check
        elif check == "c" and compute not in (_lib.COMPUTE_BF16, _lib.COMPUTE_F16):
            return EINVALID, check
        elif check == "a":
            s = [b or d for b, d in zip(bs, dense_strides(op, C_, D, H, W))]
            if is_c8(op):
                if any(ptr[i] % 16 for i in range(nstrides(op))) or any(v % 8 for v in s) or (op in ROUTES and ptr[3] % 8):
                    return EINVALID, check
            else:   # the full-resolution side of the fp32 space / depth pair
                f = 0 if op == S2D else 1
                if ptr[f] % 8 or s[f] % 2:
                    return EUNSUPPORTED, check
    return 0, None


def grid_x(total, cap):
    return max(1, min(-(-total // 256), cap))


def expected_plan(op, shape, bs, ptr):
    """(variant, grid x, y, z, LDS bytes, strides) as each entry point has always computed them"""
    N, C_, D, H, W = shape
    S, CB = D * H * W, (C_ + 7) // 8
    s = [b or d for b, d in zip(bs, dense_strides(op, C_, D, H, W))]
    s += [0] * (3 - len(s))
    variant, lds, grid = SCALAR, 0, None
    if op in (AVG_FWD, MAX_FWD):
        vec = W % 4 == 0 and s[0] % 4 == 0 and s[1] % 2 == 0 and ptr[0] % 16 == 0 and ptr[1] % 8 == 0
        variant = int(vec and (op == AVG_FWD or ptr[3] % 2 == 0))
        total, cap = N * C_ * (D // 2) * (H // 2) * (W // 4 if variant else W // 2), 8192
    elif op == MAX_BWD:
        variant = int(W % 4 == 0 and s[2] % 4 == 0 and s[1] % 4 == 0 and s[0] % 2 == 0 and ptr[2] % 16 == 0 and ptr[1] % 16 == 0
                      and ptr[0] % 8 == 0 and ptr[3] % 2 == 0)
        total, cap = N * C_ * D * H * (W // 4 if variant else W // 2), 8192
    elif op in (AVG_BWD, AVG_BWD_ADD):
        total, cap = N * C_ * D * H * (W // 2), 8192
    elif op in (S2D, D2S):
        total, cap = N * C_ * D * H * (W // 2), 16384
    elif op == TRI_BWD:
        total, cap = N * C_ * S, 65536
    elif op == TRI_FWD:
        quads = W % 2 == 0 and s[1] % 4 == 0 and ptr[1] % 16 == 0
        patch = 4 * 10 * W * 4
        if quads and D >= 2 and H >= 2 and patch <= 48 * 1024 and N * C_ <= 65535 and -(-2 * D // 4) <= 65535:
            variant, lds, grid = LDS, patch, (-(-2 * H // 16), -(-2 * D // 4), N * C_)
        elif quads and N * C_ * D * H * 4 < 2 ** 31:
            variant, total, cap = QUADS, N * C_ * S * 8 // 4, 65536
        else:
            total, cap = N * C_ * S * 8, 16384
    elif op in (AVG_FWD_H16, MAX_FWD_H16):
        total, cap = N * CB * (S // 8), 8192
    elif op in (AVG_BWD_H16, MAX_BWD_H16):
        total, cap = N * CB * S, 16384
    elif op == TRI_FWD_H16:
        total, cap = N * CB * S * 8, 65536
    elif op == TRI_BWD_H16:
        total, cap = N * CB * S, 65536
    else:   # S2D_H16, D2S_H16
        total, cap = N * CB * (S // 8), 65536
    return (variant,) + (grid or (grid_x(total, cap), 1, 1)) + (lds,) + tuple(s)


def plan(op, shape, bs, ptr, compute=_lib.COMPUTE_BF16):
    out = (C.c_int64 * 8)()
    rc = _lib.lib().m355_resample_plan(op, *shape, (C.c_int64 * 3)(*bs), (C.c_uint64 * 4)(*ptr), compute, out)
    return rc, tuple(out)


BASE_PTR = (1 << 20, 2 << 20, 3 << 20, 4 << 20)
# (N, C, (D, H, W), pad of each batch stride (0: passed as dense), bytes each pointer is off a 16-byte boundary).  c8 entry
# points take pads * 8 and aligned pointers (anything else they reject: the codes below).
CASES = [
    (2, 3, (2, 4, 4), (0, 0, 0), (0, 0, 0, 0)), (2, 3, (2, 2, 6), (0, 0, 0), (0, 0, 0, 0)), (1, 9, (4, 6, 8), (4, 2, 4), (0, 8, 0, 2)),
    (2, 3, (2, 4, 4), (2, 0, 0), (0, 0, 0, 0)), (2, 3, (2, 4, 4), (0, 1, 0), (0, 0, 0, 0)), (2, 3, (2, 4, 4), (0, 0, 2), (0, 0, 0, 0)),
    (2, 3, (2, 4, 4), (0, 0, 0), (8, 0, 0, 0)), (2, 3, (2, 4, 4), (0, 0, 0), (0, 4, 0, 0)), (2, 3, (2, 4, 4), (0, 0, 0), (0, 0, 8, 0)),
    (2, 3, (2, 4, 4), (0, 0, 0), (0, 0, 0, 1)), (2, 8, (16, 16, 20), (8, 8, 8), (0, 0, 0, 0)), (1, 1, (2, 2, 2), (0, 0, 0), (4, 4, 4, 0)),
    (2, 32, (36, 10, 132), (0, 0, 0), (0, 0, 0, 0)), (1, 32, (64, 64, 64), (0, 0, 0), (0, 0, 0, 0)),
    (1, 32, (128, 128, 128), (0, 0, 0), (0, 0, 0, 0)),
]
# the trilinear ops also take odd sizes: lds; quads with D = 1 and with H = 1; scalar with odd W; each side of the 48 KiB patch
# with D = H = 2 (W = 308 is the smallest even W above it); a stride and a pointer that deny the quads
TRI_CASES = [
    (2, 3, (2, 2, 2), (0, 0, 0), (0, 0, 0, 0)), (2, 3, (1, 2, 2), (0, 0, 0), (0, 0, 0, 0)), (2, 3, (2, 1, 4), (0, 0, 0), (0, 0, 0, 0)),
    (2, 3, (2, 2, 3), (0, 0, 0), (0, 0, 0, 0)), (2, 3, (2, 2, 306), (0, 0, 0), (0, 0, 0, 0)), (2, 3, (2, 2, 308), (0, 0, 0), (0, 0, 0, 0)),
    (2, 3, (2, 2, 2), (0, 2, 0), (0, 0, 0, 0)), (2, 3, (2, 2, 2), (0, 0, 0), (0, 8, 0, 0)), (2, 3, (3, 5, 7), (1, 4, 0), (4, 0, 0, 0)),
]


def arguments(op, case):
    N, C_, vol, pads, offs = case
    if is_c8(op):
        pads, offs = [8 * p for p in pads], (0, 0, 0, 0)
    dense = dense_strides(op, C_, *vol)
    bs = [d + p if p else 0 for d, p in zip(dense, pads)] + [0] * (3 - len(dense))
    return (N, C_) + vol, bs, [b + o for b, o in zip(BASE_PTR, offs)]


@pytest.mark.parametrize("op", range(17), ids=OPS)
def test_plans_agree_with_the_arguments(op):
    """strides, variant, grid and LDS bytes over the cases; a call the entry point rejects is rejected here with its code"""
    tri = "o" not in ORDER[OPS[op]]
    served = 0
    for case in CASES + (TRI_CASES if tri else []):
        shape, bs, ptr = arguments(op, case)
        rc, out = plan(op, shape, bs, ptr)
        code, _ = expected_code(op, shape, bs, ptr, _lib.COMPUTE_BF16)
        assert rc == code, (case, rc, _lib.lib().m355_last_error())
        if rc == 0:
            assert out == expected_plan(op, shape, bs, ptr), case
            served += 1
    assert served >= 12


def test_each_term_of_the_pool_verdicts_decides():
    """the fp32 pools: one vector case, and one scalar case per term of the verdict -- W % 4, each stride, each pointer"""
    shape = (2, 3, 2, 4, 4)
    # tensor index -> (stride pad, pointer offset) that breaks that tensor's term: float4 rows of the full-resolution tensors
    # (stride % 4, 16 bytes), float2 rows of the pooled one (stride % 2, 8 bytes)
    full, half = (2, 8), (1, 4)
    for op, tensors, routes in ((AVG_FWD, (full, half), False), (MAX_FWD, (full, half), True), (MAX_BWD, (half, full, full), True)):
        dense = dense_strides(op, *shape[1:])
        zero = [0, 0, 0]
        assert plan(op, shape, zero, BASE_PTR)[1][0] == VECTOR
        assert plan(op, (2, 3, 2, 4, 6), zero, BASE_PTR)[1][0] == SCALAR
        assert plan(op, shape, [d + 4 for d in dense] + zero[len(dense):], BASE_PTR)[1][0] == VECTOR   # padded, still aligned
        for i, (pad, off) in enumerate(tensors):
            bs, ptr = list(zero), list(BASE_PTR)
            bs[i] = dense[i] + pad
            assert plan(op, shape, bs, BASE_PTR) == (0, expected_plan(op, shape, bs, BASE_PTR)) and plan(op, shape, bs, BASE_PTR)[1][0] == SCALAR
            ptr[i] += off
            assert plan(op, shape, zero, ptr) == (0, expected_plan(op, shape, zero, ptr)) and plan(op, shape, zero, ptr)[1][0] == SCALAR
        if routes:   # uchar2 route stores
            ptr = BASE_PTR[:3] + (BASE_PTR[3] + 1,)
            assert plan(op, shape, zero, ptr)[1][0] == SCALAR
        if op == MAX_BWD:   # without the skip gradient its terms hold
            assert plan(op, shape, zero, (BASE_PTR[0], 0, BASE_PTR[2], BASE_PTR[3]))[1][0] == VECTOR


def test_trilinear_forward_takes_each_of_its_three_kernels():
    zero = [0, 0, 0]
    variant = lambda *shape: plan(TRI_FWD, shape, zero, BASE_PTR)[1][0]   # noqa: E731
    assert variant(2, 3, 2, 2, 2) == LDS and variant(2, 3, 1, 2, 2) == QUADS and variant(2, 3, 2, 2, 3) == SCALAR
    assert variant(2, 3, 2, 2, 306) == LDS and variant(2, 3, 2, 2, 308) == QUADS   # 160 * W bytes <= 48 KiB: W <= 307
    assert plan(TRI_FWD, (2, 3, 2, 2, 306), zero, BASE_PTR)[1][1:5] == (1, 1, 6, 160 * 306)
    # the quad kernel's 32-bit row index: N * C * D * H * 4 < 2^31
    assert variant(1, 32, 4095, 4096, 308) == QUADS and variant(1, 32, 4096, 4096, 308) == SCALAR
    # the tiled kernel's grid.z = N * C
    assert variant(1, 65535, 2, 2, 2) == LDS and variant(1, 65536, 2, 2, 2) == QUADS


@pytest.mark.parametrize("op", range(17), ids=OPS)
def test_a_128_cubed_level_sits_at_the_grid_cap(op):
    cap = {AVG_FWD: 8192, AVG_BWD: 8192, AVG_BWD_ADD: 8192, TRI_FWD: None, TRI_BWD: 65536, S2D: 16384, D2S: 16384, MAX_FWD: 8192,
           MAX_BWD: 8192, AVG_FWD_H16: 8192, AVG_BWD_H16: 16384, TRI_FWD_H16: 65536, TRI_BWD_H16: 65536, S2D_H16: 65536,
           D2S_H16: 65536, MAX_FWD_H16: 8192, MAX_BWD_H16: 16384}[op]
    # N = 2 reaches every cap but the c8 space / depth pair's (one thread per pooled voxel and channel block, cap 65536): N = 16
    shape = (16 if op in (S2D_H16, D2S_H16) else 2, 32, 128, 128, 128)
    rc, out = plan(op, shape, [0, 0, 0], BASE_PTR)
    assert rc == 0 and out == expected_plan(op, shape, [0, 0, 0], BASE_PTR)
    if op == TRI_FWD:   # tiled: (y tiles, z tiles, N * C); the grid-stride kernels behind it at their caps
        assert out[:4] == (LDS, 16, 64, 64)
        assert plan(op, (2, 32, 128, 128, 127), [0, 0, 0], BASE_PTR)[1][:2] == (SCALAR, 16384)
        assert plan(op, (2, 32, 128, 128, 308), [0, 0, 0], BASE_PTR)[1][:2] == (QUADS, 65536)
    else:
        assert out[1:4] == (cap, 1, 1)


# ---- codes ----
VALID = dict(N=2, C=8, D=4, H=4, W=4, compute=_lib.COMPUTE_BF16, bs0=0, bs1=0, bs2=0, ptr0=BASE_PTR[0], ptr1=BASE_PTR[1],
             ptr2=BASE_PTR[2], ptr3=BASE_PTR[3])
# (field, value): every way one argument can be wrong.  Whether a fault is one for a given entry point is the model's call --
# a null skip gradient, an odd size on the trilinear ops or a 4-byte offset on an fp32 pool are served
FAULTS = ([(f"ptr{i}", 0) for i in range(4)] + [(k, 0) for k in "NCDHW"] + [("N", -1)] + [(k, 5) for k in "DHW"]
          + [("compute", 0), ("compute", 3)] + [(f"ptr{i}", BASE_PTR[i] + off) for i in range(4) for off in (4, 8)]
          + [(f"bs{i}", v) for i in range(3) for v in (4100, 4099)])


def fault_tuples(op):
    singles = [(f,) for f in FAULTS]
    pairs = [p for p in itertools.combinations(FAULTS, 2) if p[0][0] != p[1][0]]
    for faults in singles + pairs:
        if any(f[0] == f"bs{i}" for f in faults for i in range(nstrides(op), 3)):
            continue   # a stride the entry point does not take
        a = dict(VALID)
        a.update(dict(faults))
        yield faults, tuple(a[k] for k in "NCDHW"), [a["bs0"], a["bs1"], a["bs2"]], [a[f"ptr{i}"] for i in range(4)], a["compute"]


@pytest.mark.parametrize("op", range(17), ids=OPS)
def test_codes_of_one_and_two_faults(op):
    """every check on its own and every pair of two faults: the entry point answers as the order table says, with its own
    name and the check's word in the message, and m355_resample_plan answers the same -- also where the call is valid"""
    L = _lib.lib()
    name = OPS[op]
    assert _lib.RESAMPLE_OPS[op][3] == ORDER[name]
    fn = getattr(L, "m355_" + name)
    decided, rejected = set(), 0
    for faults, shape, bs, ptr, compute in fault_tuples(op):
        code, check = expected_code(op, shape, bs, ptr, compute)
        assert plan(op, shape, bs, ptr, compute)[0] == code, (faults, L.m355_last_error())
        if code == 0:
            continue   # not a fault for this entry point: calling it would launch
        rc = fn(*_lib.resample_args(op, shape, bs, ptr, compute))
        msg = L.m355_last_error()
        assert rc == code, (faults, rc, msg)
        assert msg.startswith(name.encode() + b":") and WORD[check] in msg, (faults, msg)
        decided.add((check, len(faults)))
        rejected += 1
    assert decided == {(c, n) for c in ORDER[name] for n in (1, 2)}
    assert rejected >= 150


def test_plan_query_rejects_its_own_bad_arguments():
    L = _lib.lib()
    bs, ptr, out = (C.c_int64 * 3)(), (C.c_uint64 * 4)(*BASE_PTR), (C.c_int64 * 8)()
    for op in (-1, 17):
        assert L.m355_resample_plan(op, 2, 8, 4, 4, 4, bs, ptr, 1, out) == EINVALID
    assert L.m355_resample_plan(0, 2, 8, 4, 4, 4, None, ptr, 1, out) == EINVALID
    assert L.m355_resample_plan(0, 2, 8, 4, 4, 4, bs, None, 1, out) == EINVALID
    assert L.m355_resample_plan(0, 2, 8, 4, 4, 4, bs, ptr, 1, None) == EINVALID
    assert L.m355_resample_plan(0, 2, 8, 4, 4, 4, bs, ptr, 1, out) == 0
