"""The 3x3x3 conv routes (csrc/conv3d_route.hpp) answer consistently: the workspace queries, packed_bytes, the statistics
slots, fuses_softmax, m355_conv3d_plan and m355_conv3d_launch_plan are numbers of the same route; the facts a call adds to
its descriptor -- alignment, strides, optional tensors -- move it between the kernel variants under exactly the conditions
the launchers used to test; and a rejected call gets its code from the checks alone, before anything is launched.  Pure
host code, no GPU (num_cus() is then 256); tools/conv_routes.py --launch is the exhaustive table."""
import ctypes as C

import pytest

from segmentation_pipeline_amd import _lib

FWD, FWD_STATS, BWD_DATA, BWD_WEIGHT, FWD_H16, FWD_H16_C8, BWD_DATA_H16, BWD_DATA_H16_C8, BWD_WEIGHT_H16, BWD_WEIGHT_C8 = range(10)
# forward / data-gradient variants, weight-gradient variants (include/m355seg.h)
DIRECT, MFMA, MFMA_QUEUE, SMALL_VALU, SMALL_TOEPLITZ, X3, H16_QUEUE, H16_QUEUE8, H16_ONESHOT, H16_C4, H16_COUT4 = range(11)
W_DIRECT, W_VEC, W_SCALAR, W_MFMA2, W_MFMA2C, W_SMALL, W_X3, W_X3C, W_C8, W_C8_SMALL = range(10)
PACK_W, PACK_IN, PACK_DY, TILE16, SPLITK, SPLITK_STATS, SLAB_T, SLAB_TAP, SLAB_PLAIN, DBIAS_F32, DBIAS_C8 = (1 << i for i in range(11))
EINVALID, EUNSUPPORTED, EWORKSPACE = -1, -2, -4
F32, BF16, F16, F32X3 = range(4)
IN, W, BIAS, ADD, OUT, STAT, WS = range(7)   # slots of the query's `pointers`


def desc(shape, compute=F32, k=3, stride=1, pad=1, flags=0, xbs=0, ybs=0):
    N, Cin, Cout, D, H, Wd = shape
    return _lib.ConvDesc(N, Cin, Cout, D, H, Wd, k, stride, pad, 0, xbs, ybs, compute, flags)


def pointers(present=(), offsets=None):
    """aligned dummies for the four mandatory pointers and those named in `present`; offsets: {slot: bytes} added on top"""
    p = [0] * 7
    for i in (IN, W, OUT, WS) + tuple(present):
        p[i] = (i + 1) << 20
    for i, off in (offsets or {}).items():
        p[i] += off
    return p


def launch_plan(entry, d, present=(), offsets=None, strides=(0, 0), ws_bytes=1 << 40, ptrs=None):
    """(return code, the twelve numbers)"""
    out = (C.c_int64 * 12)()
    ptrs = pointers(present, offsets) if ptrs is None else ptrs
    rc = _lib.lib().m355_conv3d_launch_plan(entry, C.byref(d), (C.c_int64 * 2)(*strides), (C.c_uint64 * 7)(*ptrs), ws_bytes, out)
    return rc, tuple(out)


def served(*a, **kw):
    rc, out = launch_plan(*a, **kw)
    assert rc == 0, _lib.lib().m355_last_error()
    return out


def family(d, which):
    out = (C.c_int32 * 4)()
    assert _lib.lib().m355_conv3d_plan(C.byref(d), which, out) == 0
    return tuple(out)


SHAPES = [(2, 3, 32, 6, 9, 36), (2, 32, 4, 6, 9, 36), (2, 40, 24, 5, 7, 33), (2, 32, 32, 6, 9, 36), (2, 8, 40, 5, 7, 33),
          (2, 32, 4, 8, 4, 32), (2, 8, 3, 8, 4, 32), (1, 32, 32, 64, 64, 64), (1, 40, 40, 96, 96, 96), (1, 4, 32, 128, 128, 128)]
# the kernel families of m355_conv3d_plan -> the variants that may stand behind them
FAMILY_VARIANTS = {0: {DIRECT}, 1: {MFMA}, 3: {MFMA_QUEUE}, 2: {SMALL_VALU, SMALL_TOEPLITZ}, 7: {X3},
                   4: {H16_QUEUE, H16_C4, H16_COUT4}, 5: {H16_QUEUE8}, 6: {H16_ONESHOT, H16_C4, H16_COUT4}}
W_FAMILY_VARIANTS = {0: {W_DIRECT}, 8: {W_X3, W_X3C}, 9: {W_VEC, W_SCALAR, W_MFMA2, W_MFMA2C}, 10: {W_SMALL}, 11: {W_C8}}


@pytest.mark.parametrize("compute", [F32, BF16, F16, F32X3])
@pytest.mark.parametrize("shape", SHAPES)
def test_queries_are_numbers_of_the_route(shape, compute):
    L = _lib.lib()
    d = desc(shape, compute)
    ref = C.byref(d)
    h16 = compute in (BF16, F16)
    for which, entry, entry16 in ((0, FWD, FWD_H16), (1, BWD_DATA, BWD_DATA_H16)):
        fam, ntw, gx, ksplit = family(d, which)
        out = served(entry, d)
        assert out[0] in FAMILY_VARIANTS[fam]
        assert out[8] == (L.m355_conv3d_fwd_workspace, L.m355_conv3d_bwd_data_workspace)[which](ref)
        assert bool(out[7] & SPLITK) == (ksplit > 1) and bool(out[7] & PACK_W) and bool(out[7] & PACK_IN) == h16
        packed = L.m355_conv3d_packed_bytes(ref, which)
        if out[0] not in (DIRECT, SMALL_VALU, SMALL_TOEPLITZ):
            assert out[10] == packed                                    # the slabs follow the packed weights
            assert out[11] == L.m355_conv3d_h16_workspace(ref, which) if h16 else out[11] == out[8]
        if h16:
            assert served(entry16, d)[8] == L.m355_conv3d_h16_workspace(ref, which)
            # exactly the workspace the query names is enough, one byte less is not
            assert launch_plan(entry16, d, ws_bytes=L.m355_conv3d_h16_workspace(ref, which) - 1)[0] == EWORKSPACE
        else:
            assert launch_plan(entry16, d)[0] == EUNSUPPORTED
        assert launch_plan(entry, d, ws_bytes=out[8])[0] == 0 and (out[8] == 0 or launch_plan(entry, d, ws_bytes=out[8] - 1)[0] == EWORKSPACE)
    # statistics: offered exactly where the slots query is non-zero; softmax: accepted exactly where fuses_softmax says so
    assert (launch_plan(FWD_STATS, d, present=(STAT,))[0] == 0) == (L.m355_conv3d_stats_slots(ref) > 0)
    if h16:
        assert (launch_plan(FWD_H16_C8, d, present=(STAT,))[0] == 0) == (L.m355_conv3d_stats_slots_c8(ref) > 0)
    ds = desc(shape, compute, flags=_lib.CONV_SOFTMAX)
    assert (launch_plan(FWD_H16 if h16 else FWD, ds)[0] == 0) == bool(L.m355_conv3d_fuses_softmax(ref))
    # weight gradients
    out = served(BWD_WEIGHT, d, present=(STAT,))
    assert out[0] in W_FAMILY_VARIANTS[family(d, 2)[0]] and out[8] == L.m355_conv3d_bwd_weight_workspace(ref)
    assert bool(out[7] & PACK_IN) == bool(out[7] & PACK_DY) == (family(d, 2)[0] == 11) and out[7] & DBIAS_F32
    if h16:
        o16, oc8 = served(BWD_WEIGHT_H16, d, present=(BIAS, STAT)), served(BWD_WEIGHT_C8, d, present=(STAT,))
        assert o16[8] == L.m355_conv3d_bwd_weight_h16_workspace(ref) and oc8[8] == L.m355_conv3d_bwd_weight_c8_workspace(ref)
        assert o16[0] == W_C8 and o16[7] & DBIAS_F32 and oc8[7] & DBIAS_C8 and o16[10] == oc8[10] > 0
        assert oc8[0] == (W_C8_SMALL if min(shape[1], shape[2]) <= 4 else W_C8)
        if out[0] == W_C8:   # behind the pack: the c8 kernel's own launch, the copies behind its workspace
            assert out[1:5] == o16[1:5] and out[9:11] == o16[9:11] and out[11] == o16[8]
    else:
        assert launch_plan(BWD_WEIGHT_H16, d, present=(BIAS,))[0] == launch_plan(BWD_WEIGHT_C8, d)[0] == EUNSUPPORTED


def test_every_variant_is_reached(tuning):
    conv, bww = set(), set()

    def sweep(shapes=SHAPES):
        for shape in shapes:
            for compute in (F32, BF16, F32X3):
                d = desc(shape, compute)
                for entry in (FWD, BWD_DATA, FWD_H16, FWD_H16_C8, BWD_DATA_H16_C8):
                    rc, out = launch_plan(entry, d)
                    if rc == 0:
                        conv.add(out[0])
                for entry in (BWD_WEIGHT, BWD_WEIGHT_H16, BWD_WEIGHT_C8):
                    for off in (0, 4):
                        rc, out = launch_plan(entry, d, offsets={IN: off} if entry == BWD_WEIGHT else None)
                        if rc == 0:
                            bww.add(out[0])
        for geom in ((1, 1, 0), (3, 2, 1)):
            d = desc(SHAPES[0], F32, *geom)
            conv.add(served(FWD, d)[0])
            bww.add(served(BWD_WEIGHT, d)[0])
    sweep()
    for env in (dict(M355_CONV_SLOTS=5), dict(M355_H16_ONESHOT=3), dict(M355_H16_ONESHOT=3, M355_H16_W8=2), dict(M355_SMALLCOUT_VALU=0),
                dict(M355_BWW_GEN=1)):
        tuning(**{k: 0 for k in ("M355_CONV_SLOTS", "M355_BWW_GEN")} | dict(M355_H16_ONESHOT=1, M355_H16_W8=1, M355_SMALLCOUT_VALU=1,
                                                                       M355_BWW_GEN=2) | env)
        sweep(SHAPES[:7])
    assert conv == set(range(11)) and bww == set(range(10))


def expected_bww_variant(shape, x, dy, xbs, gen):
    """the choice the launcher used to make from the pointers (bww_variant) for a descriptor on the fp32 MFMA kernels"""
    N, Cin, Cout, D, H, Wd = shape
    S = D * H * Wd
    vec = Wd % 4 == 0 and (xbs or Cin * S) % 4 == 0 and x % 16 == 0
    gen2 = vec and dy % 4 == 0 and Cin * S < 2 ** 29 and Cout * S < 2 ** 29 and gen == 2
    rem = lambda c: 1 <= c % 32 <= 16   # noqa: E731
    if gen2:
        return W_MFMA2C if (rem(Cin) or rem(Cout)) and Cin > 4 and Cout > 4 else W_MFMA2
    return W_VEC if vec else W_SCALAR


@pytest.mark.parametrize("gen", [2, 1])
@pytest.mark.parametrize("shape", [(2, 32, 32, 6, 9, 36), (2, 40, 24, 6, 9, 36), (2, 8, 40, 5, 7, 33), (2, 40, 24, 5, 7, 33),
                                   (1, 64, 64, 256, 256, 256)])
def test_alignment_and_strides_move_the_weight_gradient(shape, gen, tuning):
    tuning(M355_BWW_GEN=gen)
    N, Cin, Cout, D, H, Wd = shape
    seen = set()
    for x_off in (0, 4, 8, 16):
        for dy_off in (0, 2, 4):
            for pad in (0, 4, 1, 2):
                xbs = Cin * D * H * Wd + pad if pad else 0
                d = desc(shape, xbs=xbs)
                rc, out = launch_plan(BWD_WEIGHT, d, offsets={IN: x_off, W: dy_off})
                assert rc == 0
                want = expected_bww_variant(shape, (1 << 20) + x_off, (2 << 20) + dy_off, xbs, gen)
                assert out[0] == want, (x_off, dy_off, pad)
                seen.add(want)
                # the reduction follows the kernel: transposed slabs of the second-generation kernels, plain ones otherwise
                assert bool(out[7] & (SLAB_T | SLAB_TAP)) == (want in (W_MFMA2, W_MFMA2C)) and bool(out[7] & SLAB_PLAIN) == (want in (W_VEC, W_SCALAR))
    assert W_SCALAR in seen and (gen == 1 or Wd % 4 or len(seen) >= 3 or shape[3] == 256)


@pytest.mark.parametrize("compute", [BF16, F16])
def test_c8_forward_moves_among_generic_c4_and_cout4(compute, tuning):
    tuning(M355_CONV_KSPLIT=1, M355_CONV_NTW=4)
    first, last, wide = (2, 3, 32, 8, 8, 32), (2, 32, 3, 8, 8, 32), (2, 32, 32, 8, 8, 32)
    generic = (H16_QUEUE, H16_QUEUE8, H16_ONESHOT)
    # <= 4 K-channels into a c8 output: the c4 kernel; into an fp32 output, or with more channels: the generic one
    assert served(FWD_H16_C8, desc(first, compute))[0] == H16_C4
    assert served(FWD_H16, desc(first, compute))[0] in generic
    assert served(FWD_H16_C8, desc(wide, compute))[0] in generic
    assert served(BWD_DATA_H16_C8, desc(last, compute))[0] == H16_C4   # the data gradient of the output conv: K-channels = Cout
    # <= 4 M-channels into a plain fp32 output: the cout4 kernel, with or without softmax; not with add, statistics or c8 output
    assert served(FWD_H16, desc(last, compute))[0] == H16_COUT4
    assert served(FWD_H16, desc(last, compute, flags=_lib.CONV_SOFTMAX))[0] == H16_COUT4
    assert served(FWD_H16, desc(last, compute), present=(BIAS,))[0] == H16_COUT4
    assert served(FWD_H16, desc(last, compute), present=(ADD,))[0] in generic
    assert served(FWD_H16, desc(last, compute), present=(STAT,))[0] in generic
    assert served(FWD_H16_C8, desc(last, compute))[0] in generic
    assert served(BWD_DATA_H16, desc(first, compute))[0] == H16_COUT4
    # both need 32 lanes along x, an unsplit plan, 4 waves -- and cout4 the 4-row tile
    narrow = (2, 32, 3, 8, 8, 16)
    assert served(FWD_H16, desc(narrow, compute))[0] in generic and served(FWD_H16_C8, desc((2, 3, 32, 8, 8, 16), compute))[0] in generic
    tuning(M355_CONV_KSPLIT=1, M355_CONV_NTW=2)
    assert served(FWD_H16, desc(last, compute))[0] in generic and served(FWD_H16_C8, desc(first, compute))[0] == H16_C4
    tuning(M355_CONV_KSPLIT=1, M355_CONV_NTW=4, M355_NO_SMALL=1)
    assert served(FWD_H16, desc(last, compute))[0] in generic and served(FWD_H16_C8, desc(first, compute))[0] in generic
    tuning(M355_CONV_KSPLIT=2, M355_CONV_NTW=4, M355_NO_SMALL=0)
    assert served(FWD_H16, desc((2, 32, 3, 8, 8, 32), compute))[0] in generic


def call(entry, d, ptrs, strides=(0, 0), ws_bytes=1 << 40):
    fn = getattr(_lib.lib(), "m355_" + _lib.CONV_ENTRIES[entry][0])
    return fn(*_lib.conv_entry_args(entry, d, strides, ptrs, ws_bytes))


# (entry, descriptor, present, offsets, strides, workspace bytes, code, a word of the message): each call is REJECTED, so the
# entry point itself can be called on dummy pointers -- they are never followed.  The second block are the checks that used
# to sit behind a launch (pack_act16, the weight pack) or inside a launcher.
S26 = (1, 8, 8, 256, 256, 1024)
REJECTED = [
    (FWD, desc((0, 4, 8, 8, 8, 8)), (), None, (0, 0), 1 << 40, EINVALID, b"non-positive"),
    (FWD_STATS, desc((2, 8, 8, 8, 8, 8)), (), None, (0, 0), 1 << 40, EINVALID, b"null statistics"),
    (FWD, desc((2, 8, 8, 8, 8, 8), flags=_lib.CONV_SOFTMAX), (), None, (0, 0), 1 << 40, EUNSUPPORTED, b"SOFTMAX"),
    (FWD, desc((2, 8, 8, 8, 8, 8)), (), None, (0, 0), 16, EWORKSPACE, b"workspace too small"),
    (FWD, desc((2, 8, 8, 8, 8, 8)), (), {WS: 8}, (0, 0), 1 << 40, EINVALID, b"not 16B aligned"),
    (FWD, desc((2, 8, 8, 8, 8, 8), k=1, pad=0, flags=_lib.CONV_W_PACKED), (), None, (0, 0), 1 << 40, EINVALID, b"no packed weights"),
    (BWD_DATA, desc((2, 8, 8, 8, 8, 8)), (), {OUT: -(5 << 20)}, (0, 0), 1 << 40, EINVALID, b"conv3d_bwd_data: null"),
    (FWD_H16, desc((2, 8, 8, 8, 8, 8)), (), None, (0, 0), 1 << 40, EUNSUPPORTED, b"c8 input is only defined"),
    (BWD_WEIGHT, desc((2, 8, 8, 8, 8, 8)), (), None, (0, 0), 16, EWORKSPACE, b"conv3d_bwd_weight: workspace"),
    (BWD_WEIGHT_H16, desc((2, 8, 8, 8, 8, 8), BF16), (STAT,), None, (0, 0), 1 << 40, EINVALID, b"needs the fp32 dy"),
    (BWD_WEIGHT_C8, desc((2, 8, 8, 8, 8, 8), F16), (), {IN: 8}, (0, 0), 1 << 40, EINVALID, b"conv3d_bwd_weight_c8: c8 tensor"),
    (BWD_WEIGHT_C8, desc((2, 8, 8, 8, 8, 8), F16), (), None, (8 * 512 + 4, 0), 1 << 40, EINVALID, b"c8 tensor"),
    (BWD_WEIGHT_H16, desc(S26, BF16), (), None, (0, 0), 1 << 40, EUNSUPPORTED, b"volume too large"),
    # formerly behind a launch
    (FWD, desc(S26, BF16), (), None, (0, 0), 1 << 50, EUNSUPPORTED, b"32-bit offsets"),
    (BWD_DATA, desc(S26, F16), (), None, (0, 0), 1 << 50, EUNSUPPORTED, b"32-bit offsets"),
    (FWD_H16, desc((2, 8, 8, 8, 8, 8), BF16), (), {IN: 8}, (0, 0), 1 << 40, EINVALID, b"c8 input not 16B aligned"),
    (FWD_H16, desc((2, 8, 8, 8, 8, 8), BF16), (), None, (8 * 512 + 4, 0), 1 << 40, EINVALID, b"c8 input not 16B aligned"),
    (FWD_H16_C8, desc((2, 8, 8, 8, 8, 8), F16), (), {OUT: 8}, (0, 0), 1 << 40, EINVALID, b"c8 output"),
    (BWD_DATA_H16_C8, desc((2, 8, 8, 8, 8, 8), F16), (), None, (0, 8 * 512 + 2), 1 << 40, EINVALID, b"c8 output"),
    (BWD_WEIGHT, desc((2, 8, 8, 8, 8, 8), F32X3), (), {IN: 2}, (0, 0), 1 << 40, EINVALID, b"misaligned tensor"),
    (BWD_WEIGHT, desc((1, 2503, 2503, 7, 7, 7), k=7, pad=3), (), None, (0, 0), 1 << 40, EUNSUPPORTED, b"grid too large"),
    (BWD_WEIGHT, desc((2, 8, 8, 8, 8, 8), BF16), (), {WS: 8}, (0, 0), 1 << 40, EINVALID, b"conv3d_bwd_weight_h16: c8 tensor"),
]


@pytest.mark.parametrize("case", range(len(REJECTED)))
def test_a_rejected_call_gets_its_code_from_the_checks_alone(case):
    entry, d, present, offsets, strides, ws_bytes, code, word = REJECTED[case]
    ptrs = pointers(present, offsets)
    L = _lib.lib()
    assert launch_plan(entry, d, strides=strides, ws_bytes=ws_bytes, ptrs=ptrs)[0] == code
    assert word in L.m355_last_error()
    assert call(entry, d, ptrs, strides, ws_bytes) == code
    assert word in L.m355_last_error()


def test_a_call_wrong_in_two_ways_keeps_its_code():
    """the order of the checks is the entry points': unsupported softmax before a null pointer before the workspace"""
    d = desc((2, 8, 8, 8, 8, 8), flags=_lib.CONV_SOFTMAX)
    nothing = [0] * 7
    assert launch_plan(FWD, d, ptrs=nothing, ws_bytes=0)[0] == call(FWD, d, nothing, ws_bytes=0) == EUNSUPPORTED
    d = desc((2, 8, 8, 8, 8, 8))
    assert launch_plan(FWD, d, ptrs=nothing, ws_bytes=0)[0] == call(FWD, d, nothing, ws_bytes=0) == EINVALID
    d = desc((2, 8, 8, 8, 8, 8), BF16)
    misaligned = pointers((), {IN: 8})
    assert launch_plan(FWD_H16, d, ptrs=misaligned, ws_bytes=16)[0] == call(FWD_H16, d, misaligned, ws_bytes=16) == EWORKSPACE
    assert launch_plan(BWD_WEIGHT_C8, d, ptrs=misaligned, ws_bytes=16)[0] == call(BWD_WEIGHT_C8, d, misaligned, ws_bytes=16) == EWORKSPACE
    out = (C.c_int64 * 12)()
    assert _lib.lib().m355_conv3d_launch_plan(10, C.byref(d), (C.c_int64 * 2)(), (C.c_uint64 * 7)(), 0, out) == EINVALID
    assert _lib.lib().m355_conv3d_launch_plan(0, C.byref(d), None, (C.c_uint64 * 7)(), 0, out) == EINVALID
