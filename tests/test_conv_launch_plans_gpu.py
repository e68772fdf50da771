"""Every kernel variant a 3x3x3 conv route can name (csrc/conv3d_route.hpp) runs once from the plan the host resolved: each
case first asks m355_conv3d_launch_plan that the call it is about to make reports the variant it is meant to cover -- so it
cannot pass on another kernel --, then makes the call and compares with the CPU oracle at the tolerance tests/
test_kernels_gpu.py applies to that kernel and compute mode.  Shapes are the smallest at which a wrong grid, offset or
variant shows: N = 2; 6 x 9 x 36 and 5 x 7 x 33 (W % 4 != 0: a ragged tile on every axis); 8 x 4 x 32 for the 8-wave and
small-Cout kernels (D >= 8, W >= 32); channels 3 -> 32, 32 -> 4, 40 -> 24 (a <= 16 channel remainder on both sides: the
16-row tile alone, the pair classes), 32 -> 32, 8 -> 40."""
import pytest
import torch

from test_kernels_gpu import _c8_to_ncdhw, _rounded_close, close, rnd

pytestmark = pytest.mark.gpu

FWD, FWD_STATS, BWD_DATA, BWD_WEIGHT, FWD_H16, FWD_H16_C8, BWD_DATA_H16, BWD_DATA_H16_C8, BWD_WEIGHT_H16, BWD_WEIGHT_C8 = range(10)
DIRECT, MFMA, MFMA_QUEUE, SMALL_VALU, SMALL_TOEPLITZ, X3, H16_QUEUE, H16_QUEUE8, H16_ONESHOT, H16_C4, H16_COUT4 = range(11)
W_DIRECT, W_VEC, W_SCALAR, W_MFMA2, W_MFMA2C, W_SMALL, W_X3, W_X3C, W_C8, W_C8_SMALL = range(10)
TILE16, SPLITK = 8, 16
F32, BF16, F16, F32X3 = range(4)
V36, V33, V32 = (6, 9, 36), (5, 7, 33), (8, 4, 32)
PRESENT = 4096   # an aligned stand-in for an optional tensor in the plan query

_cache = {}


def data(ci, co, vol):
    """the operands of a shape, drawn once"""
    key = (ci, co, vol)
    if key not in _cache:
        x, w, b = rnd(2, ci, *vol, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * (1.0 / (27 * ci) ** 0.5), rnd(co, seed=3)
        _cache[key] = (x, w, b, rnd(2, co, *vol, seed=4), rnd(2, co, *vol, seed=5))
    return _cache[key]


def ref(oracle, what, ci, co, vol, compute=F32, stride=1):
    """the oracle's answers of a shape, computed once and shared (16-bit modes: on equally rounded operands)"""
    compute = compute if compute in (BF16, F16) else F32   # (the split kernels answer to the fp32 oracle)
    key = (what, ci, co, vol, compute, stride)
    if key not in _cache:
        x, w, b, add, dy = data(ci, co, vol)
        if what == "fwd":
            _cache[key] = oracle.conv3d_fwd(x, w, b, add if stride == 1 else None, stride, 1, compute=compute)
        elif what == "fwd_noadd":
            _cache[key] = oracle.conv3d_fwd(x, w, b, compute=compute)
        elif what == "bwd_data":
            _cache[key] = oracle.conv3d_bwd_data(dy, w, x.shape, compute=compute)
        else:
            _cache[key] = oracle.conv3d_bwd_weight(x, dy, 3, compute=compute)
    return _cache[key]


# (id, variant, auxiliary launches that must be in the plan, entry, (Cin, Cout), volume, compute, tuning)
CONV_CASES = [
    ("mfma", MFMA, 0, FWD, (32, 32), V36, F32, {}),
    ("mfma-ragged-tile16", MFMA, TILE16, FWD, (8, 40), V33, F32, {}),
    ("mfma-24-rows", MFMA, 0, FWD, (40, 24), V33, F32, {}),
    ("mfma-splitk", MFMA, SPLITK, FWD, (32, 32), V36, F32, {"M355_CONV_KSPLIT": 2}),
    ("mfma-bwd-data-tile16-alone", MFMA, TILE16, BWD_DATA, (3, 32), V33, F32, {}),   # 3 M-channels: no 32-row launch at all
    ("queue", MFMA_QUEUE, 0, FWD, (32, 32), V36, F32, {"M355_CONV_SLOTS": 5}),
    ("queue-tile16-splitk", MFMA_QUEUE, TILE16 | SPLITK, BWD_DATA, (40, 24), V33, F32, {"M355_CONV_SLOTS": 5, "M355_CONV_KSPLIT": 2}),
    ("queue-bwd-data", MFMA_QUEUE, TILE16, BWD_DATA, (40, 24), V36, F32, {"M355_CONV_SLOTS": 5}),
    ("small-valu", SMALL_VALU, 0, FWD, (32, 4), V32, F32, {}),
    ("small-toeplitz", SMALL_TOEPLITZ, 0, FWD, (32, 4), V32, F32, {"M355_SMALLCOUT_VALU": 0}),
    ("x3", X3, 0, FWD, (32, 32), V36, F32X3, {}),
    ("x3-tile16", X3, TILE16, FWD, (8, 40), V33, F32X3, {}),
    ("x3-bwd-data-tile16-splitk", X3, TILE16 | SPLITK, BWD_DATA, (40, 24), V33, F32X3, {"M355_CONV_KSPLIT": 2}),
    ("h16-queue", H16_QUEUE, 0, FWD_H16, (32, 32), V36, BF16, {"M355_H16_ONESHOT": 3, "M355_CONV_SLOTS": 5, "M355_CONV_KSPLIT": 1}),
    ("h16-queue-splitk", H16_QUEUE, SPLITK, FWD_H16, (40, 24), V33, F16, {"M355_H16_ONESHOT": 3, "M355_CONV_SLOTS": 5, "M355_CONV_KSPLIT": 2}),
    ("h16-queue-packed-input", H16_QUEUE, 2, FWD, (8, 40), V33, BF16, {"M355_H16_ONESHOT": 3, "M355_CONV_KSPLIT": 1}),
    ("h16-queue-bwd-data", H16_QUEUE, 0, BWD_DATA_H16, (8, 40), V33, F16, {"M355_H16_ONESHOT": 3, "M355_CONV_KSPLIT": 1}),
    ("h16-queue8", H16_QUEUE8, 0, FWD_H16, (32, 32), V32, BF16, {"M355_H16_ONESHOT": 3, "M355_H16_W8": 2, "M355_CONV_KSPLIT": 1}),
    ("h16-queue8-c8-out", H16_QUEUE8, 0, FWD_H16_C8, (8, 40), V32, F16, {"M355_H16_ONESHOT": 3, "M355_H16_W8": 2, "M355_CONV_KSPLIT": 1}),
    ("h16-oneshot", H16_ONESHOT, 0, FWD_H16, (40, 24), V33, BF16, {"M355_CONV_KSPLIT": 1}),
    ("h16-oneshot-c8-out-splitk", H16_ONESHOT, SPLITK, FWD_H16_C8, (32, 32), V36, F16, {"M355_CONV_KSPLIT": 2}),
    ("h16-oneshot-bwd-data-c8", H16_ONESHOT, 0, BWD_DATA_H16_C8, (40, 24), V36, BF16, {"M355_CONV_KSPLIT": 1}),
    ("h16-c4", H16_C4, 0, FWD_H16_C8, (3, 32), V32, BF16, {"M355_CONV_KSPLIT": 1}),
    ("h16-c4-bwd-data", H16_C4, 0, BWD_DATA_H16_C8, (32, 4), V32, F16, {"M355_CONV_KSPLIT": 1}),
    ("h16-cout4", H16_COUT4, 0, FWD_H16, (32, 4), V32, BF16, {"M355_CONV_KSPLIT": 1, "M355_CONV_NTW": 4}),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_forward_and_data_gradient_variants(hip, oracle, tuning, case):
    _, variant, aux, entry, (ci, co), vol, compute, env = case
    tuning(**env)
    x, w, b, add, dy = data(ci, co, vol)
    shape = (2, ci) + vol
    dt = torch.bfloat16 if compute == BF16 else torch.float16
    with_add = entry in (FWD, FWD_H16) and variant != H16_COUT4
    plan = hip.conv_launch_plan(entry, shape, co, compute, tensors=(None, None, PRESENT, PRESENT if with_add else None))
    assert plan[0] == variant and plan[7] & aux == aux, plan
    tol = (3e-5, 3e-5) if compute in (BF16, F16) else (2e-5, 2e-5)
    if entry == FWD:
        close(hip.conv3d_fwd(x, w, b, add, compute=compute), ref(oracle, "fwd", ci, co, vol, compute), *tol, "fwd")
    elif entry == BWD_DATA:
        close(hip.conv3d_bwd_data(dy, w, x.shape, compute=compute), ref(oracle, "bwd_data", ci, co, vol, compute), *tol, "bwd_data")
    elif entry == FWD_H16:
        x16 = hip.act16_pack(x, compute)
        if variant == H16_COUT4:   # (test_out_conv_tap_rows_on_the_m_side_16bit)
            r = ref(oracle, "fwd_noadd", ci, co, vol, compute)
            close(hip.conv3d_fwd_h16(x16, ci, vol, w, b, compute=compute), r, 3e-5, 3e-5 * r.abs().max().item(), "cout4 fwd")
        else:
            close(hip.conv3d_fwd_h16(x16, ci, vol, w, b, add, compute=compute), ref(oracle, "fwd", ci, co, vol, compute), *tol, "h16 fwd")
    elif entry == BWD_DATA_H16:
        close(hip.conv3d_bwd_data_h16(hip.act16_pack(dy, compute), co, w, x.shape, compute=compute),
              ref(oracle, "bwd_data", ci, co, vol, compute), *tol, "h16 bwd_data")
    else:
        # c8 output == the fp32 output of the same plan rounded once (test_conv3d_h16_c8_output_and_c8_norm, test_conv3d_bwd_data_
        # c8_output_and_weight_gradient_c8); the c4 kernel sums the same products in another order: one 16-bit ulp at most
        if entry == FWD_H16_C8:
            x16 = hip.act16_pack(x, compute)
            got = _c8_to_ncdhw(hip.conv3d_fwd_h16_c8(x16, ci, vol, w, b, compute=compute), co, vol)
            y32, r = hip.conv3d_fwd_h16(x16, ci, vol, w, b, compute=compute).cpu(), ref(oracle, "fwd_noadd", ci, co, vol, compute)
        else:
            dy16 = hip.act16_pack(dy, compute)
            got = _c8_to_ncdhw(hip.conv3d_bwd_data_h16_c8(dy16, co, w, shape, compute), ci, vol)
            y32, r = hip.conv3d_bwd_data_h16(dy16, co, w, shape, compute).cpu(), ref(oracle, "bwd_data", ci, co, vol, compute)
        close(y32, r, *tol, "the fp32 output of the plan")
        if variant == H16_C4:
            _rounded_close(got, y32, compute, 2e-5 * y32.abs().max().item(), "c4 output")
        else:
            assert torch.equal(got, y32.to(dt).float()), "c8 output == the fp32 output rounded once"


BWW_CASES = [
    ("vec", W_VEC, BWD_WEIGHT, (32, 32), V36, F32, {"M355_BWW_GEN": 1}),
    ("scalar", W_SCALAR, BWD_WEIGHT, (8, 40), V33, F32, {}),
    ("scalar-nsplit3", W_SCALAR, BWD_WEIGHT, (40, 24), V33, F32, {"M355_BWW_NSPLIT": 3}),
    ("mfma2", W_MFMA2, BWD_WEIGHT, (32, 32), V36, F32, {}),
    ("mfma2c", W_MFMA2C, BWD_WEIGHT, (40, 24), V36, F32, {}),
    ("mfma2c-nsplit3", W_MFMA2C, BWD_WEIGHT, (8, 40), V36, F32, {"M355_BWW_NSPLIT": 3}),
    ("small", W_SMALL, BWD_WEIGHT, (3, 32), V33, F32, {}),
    ("small-cout", W_SMALL, BWD_WEIGHT, (32, 4), V36, F32, {}),
    ("x3", W_X3, BWD_WEIGHT, (32, 32), V33, F32X3, {}),
    ("x3c", W_X3C, BWD_WEIGHT, (40, 24), V33, F32X3, {}),
    ("x3c-nsplit3", W_X3C, BWD_WEIGHT, (8, 40), V36, F32X3, {"M355_BWW_NSPLIT": 3}),
    ("c8-behind-the-pack", W_C8, BWD_WEIGHT, (40, 24), V33, BF16, {}),
    ("c8", W_C8, BWD_WEIGHT_H16, (32, 32), V36, F16, {}),
    ("c8-nsplit3", W_C8, BWD_WEIGHT_H16, (8, 40), V33, BF16, {"M355_BWW_NSPLIT": 3}),
    ("c8-flow", W_C8, BWD_WEIGHT_C8, (40, 24), V33, F16, {}),
    ("c8-small", W_C8_SMALL, BWD_WEIGHT_C8, (3, 32), V33, BF16, {}),
    ("c8-small-cout", W_C8_SMALL, BWD_WEIGHT_C8, (32, 4), V32, F16, {"M355_BWW_NSPLIT": 3}),
]


@pytest.mark.parametrize("case", BWW_CASES, ids=[c[0] for c in BWW_CASES])
def test_weight_gradient_variants(hip, oracle, tuning, case):
    _, variant, entry, (ci, co), vol, compute, env = case
    tuning(**env)
    x, w, b, add, dy = data(ci, co, vol)
    plan = hip.conv_launch_plan(entry, (2, ci) + vol, co, compute, tensors=(None, None, PRESENT, None, None, PRESENT))
    assert plan[0] == variant, plan
    assert bool(plan[7] & 6) == (entry == BWD_WEIGHT and compute in (BF16, F16)), "operand packs exactly behind the plain entry point"
    dt = torch.bfloat16 if compute == BF16 else torch.float16
    tol = 3e-5 * (2 * vol[0] * vol[1] * vol[2]) ** 0.5
    if entry == BWD_WEIGHT:
        dw, db = hip.conv3d_bwd_weight(x, dy, 3, compute=compute)
        dwo, dbo = ref(oracle, "bwd_weight", ci, co, vol, compute if variant == W_C8 else F32)
    elif entry == BWD_WEIGHT_H16:
        dw, db = hip.conv3d_bwd_weight_h16(hip.act16_pack(x, compute), hip.act16_pack(dy, compute), dy, ci, co, vol, compute)
        dwo, dbo = ref(oracle, "bwd_weight", ci, co, vol, compute)
    else:
        dw, db = hip.conv3d_bwd_weight_c8(hip.act16_pack(x, compute), hip.act16_pack(dy, compute), ci, co, vol, compute)
        dwo, _ = ref(oracle, "bwd_weight", ci, co, vol, compute)
        # (test_conv3d_bwd_data_c8_output_and_weight_gradient_c8: the bias gradient is reduced from the rounded dy)
        close(db, dy.to(dt).float().double().sum(dim=(0, 2, 3, 4)).float(), 1e-5, 1e-4, "dbias from c8")
        db = None
    close(dw, dwo, 3e-5, tol, "bwd_weight")
    if db is not None:
        close(db, dbo, 3e-5, tol, "dbias")


def test_direct_kernels(hip, oracle):
    """not 3x3x3 / stride 1 / pad 1: the direct kernels of all three fp32 entry points (test_conv3d_generic_direct's tolerances)"""
    ci, co, vol = 3, 32, V33
    x, w, b, _, _ = data(ci, co, vol)
    for entry, variant in ((FWD, DIRECT), (BWD_DATA, DIRECT), (BWD_WEIGHT, W_DIRECT)):
        assert hip.conv_launch_plan(entry, x.shape, co, stride=2)[0] == variant
    yo = ref(oracle, "fwd", ci, co, vol, stride=2)
    close(hip.conv3d_fwd(x, w, b, None, 2, 1), yo)
    dy = rnd(*yo.shape, seed=5)
    close(hip.conv3d_bwd_data(dy, w, x.shape, 2, 1), oracle.conv3d_bwd_data(dy, w, x.shape, 2, 1))
    (dw, db), (dwo, dbo) = hip.conv3d_bwd_weight(x, dy, 3, 2, 1), oracle.conv3d_bwd_weight(x, dy, 3, 2, 1)
    close(dw, dwo, 3e-5, 1e-4)
    close(db, dbo, 3e-5, 1e-4)


def test_split_k_statistics_come_from_the_reduction(hip, oracle, tuning):
    """fused statistics of a split plan: the reduction pass emits them (test_conv3d_fused_statistics' tolerances)"""
    tuning(M355_CONV_KSPLIT=2)
    ci, co, vol = 32, 32, V36
    x, w, b, _, _ = data(ci, co, vol)
    plan = hip.conv_launch_plan(FWD_STATS, x.shape, co, tensors=(None, None, PRESENT, None, None, PRESENT))
    assert plan[0] == MFMA and plan[7] & 48 == 48, plan
    y, mean, rstd = hip.conv3d_fwd_stats(x, w, b, groups=8)
    close(y, ref(oracle, "fwd_noadd", ci, co, vol), what="fwd")
    m2, r2 = hip.norm_stats(y, 8)[:2]
    close(mean, m2, 1e-5, 1e-6, "fused mean")
    close(rstd, r2, 1e-5, 1e-6, "fused rstd")
