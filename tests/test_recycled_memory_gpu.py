"""Every entry point on recycled memory: workspaces, outputs and auxiliary results that hold what a previous call left
there, 0xFF bytes, or NaN canaries instead of whatever torch.empty returns (raw_ops.Scratch / raw_ops.PoisonedEmpty, self-
tested in test_recycled_memory_cpu.py; the regions each entry point keeps in its workspace are listed in DESIGN.md, "Scratch
memory").  Each case runs raw_ops.assert_recycled: twice on zeroed scratch (bit-identical), then on "stale", "ones" and "nan"
scratch (bit-identical to the clean run in every returned tensor -- partials, statistics, dw / dbias, sums, c8 outputs with
their channel pads), the "nan" run also against the oracle / fp64 reference at the tolerance of the entry point's own parity
test, and with a count of what was dirtied.  The package-level cases do the same through torch.empty itself.  The last test
reads the work-queue pool after every queue-driven launch, in a process of its own."""
import functools
import os
import subprocess
import sys
import time

import pytest
import torch
from torch import nn

from raw_ops import PoisonedEmpty, assert_recycled, bit_equal
from test_kernels_gpu import _c8_to_ncdhw, _rounded_close, close, rnd

pytestmark = pytest.mark.gpu

X3 = 3
# cases whose two runs on zeroed scratch differ (atomics in a floating-point sum): (b) gives way to (c) in every mode
NOT_DETERMINISTIC = set()


def dt16(compute):
    return torch.bfloat16 if compute == 1 else torch.float16


def env_id(env):
    return ",".join(f"{k[5:]}={v}" for k, v in env.items()) or "default"


def recycled(hip, oracle, tuning, case_id, env, run, tol=None, check=None, oracle_run=None, has_workspace=True):
    """run(be, seed) -> {name: tensor}; tol {name: (rtol, atol)}: compared with oracle_run() (default run(oracle, 1)) through
    test_kernels_gpu.close; check(got): further assertions of the case against its reference"""
    tuning(**env)

    def reference(got):
        if tol:
            want = oracle_run() if oracle_run else run(oracle, 1)
            for name, (rtol, atol) in tol.items():
                if name in got:
                    close(got[name], want[name], rtol, atol, f"{case_id} {name}")
        if check:
            check(got)
    assert_recycled(hip, lambda: run(hip, 1), lambda: run(hip, 2), reference, has_workspace=has_workspace,
                    deterministic=case_id not in NOT_DETERMINISTIC)


# ======================================================================================== 3x3x3 convolutions, fp32 tensors
def conv_inputs(case, seed, k=3, stride=1, pad=1):
    N, Ci, Co, D, H, W = case
    o = 100 * (seed - 1)
    od = lambda n: (n + 2 * pad - k) // stride + 1   # noqa: E731
    x, w, b = rnd(N, Ci, D, H, W, seed=o + 1), rnd(Co, Ci, k, k, k, seed=o + 2) * (1.0 / (k ** 3 * Ci) ** 0.5), rnd(Co, seed=o + 3)
    yshape = (N, Co, od(D), od(H), od(W))
    return x, w, b, rnd(*yshape, seed=o + 4), rnd(*yshape, seed=o + 5)


def conv_run(case, compute, groups, k=3, stride=1, pad=1):
    """forward (bias + residual), data gradient and, groups != None, the forward with fused statistics"""
    def run(be, seed):
        x, w, b, add, dy = conv_inputs(case, seed, k, stride, pad)
        c = compute if be.backend == "hip" or compute in (1, 2) else 0     # (the oracle has no F32X3: exact fp32)
        out = {"y": be.conv3d_fwd(x, w, b, add if stride == 1 else None, stride, pad, compute=c),
               "dx": be.conv3d_bwd_data(dy, w, x.shape, stride, pad, compute=c)}
        if groups is not None:
            r = be.conv3d_fwd_stats(x, w, b, groups, compute=c, partials=True)
            assert r is not None, f"no fused statistics for {case} at compute {c}: the partials are the point of the case"
            out.update(y_stats=r[0], mean=r[1], rstd=r[2])
            if be.backend == "hip":
                out["partials"] = r[3]     # (every slot of every channel is written: compared whole)
        return out
    return run


@functools.lru_cache(maxsize=None)
def conv_oracle(oracle, case, compute, groups, k=3, stride=1, pad=1):
    return conv_run(case, compute, groups, k, stride, pad)(oracle, 1)


def conv_tol(compute):
    t = (3e-5, 3e-5) if compute in (1, 2) else (2e-5, 2e-5)
    return {"y": t, "dx": t, "y_stats": (2e-5, 2e-5), "mean": (1e-5, 1e-5), "rstd": (1e-5, 1e-5)}


CONV_CASES = [   # (shape, tuning, groups of the fused statistics)
    ((1, 320, 64, 4, 4, 4), {}, 8),                                                   # split-K slabs
    ((2, 5, 7, 9, 10, 33), {}, 0),                                                    # ragged, N = 2
    ((1, 32, 32, 8, 16, 64), {"M355_CONV_SLOTS": 5}, 8),                              # persistent kernel
    ((1, 32, 32, 8, 16, 64), {"M355_CONV_SLOTS": 5, "M355_CONV_KSPLIT": 2}, 8),       # ... with a slab reduction
]
# the cases and knobs of test_conv3d_fused_statistics (which runs them under M355_CONV_KSPLIT=1 unless the knob says otherwise)
STATS_SHAPES = [(2, 8, 16, 9, 10, 36, 4), (1, 5, 40, 6, 21, 16, 8), (2, 8, 24, 12, 9, 8, 0), (1, 16, 32, 16, 16, 32, 8)]
STATS_ENVS = [{}, {"M355_CONV_SLOTS": 5}, {"M355_CONV_KSPLIT": 2}, {"M355_CONV_KSPLIT": 0}]
CONV_CASES += [(s[:6], {"M355_CONV_KSPLIT": 1, **e}, s[6]) for s in STATS_SHAPES for e in STATS_ENVS]


@pytest.mark.parametrize("compute", [0, X3], ids=["f32", "f32x3"])
@pytest.mark.parametrize("case,env,groups", CONV_CASES, ids=[f"{c}-{env_id(e)}" for c, e, _ in CONV_CASES])
def test_conv3d_fp32(hip, oracle, tuning, case, env, groups, compute):
    """m355_conv3d_fwd / _fwd_stats / _bwd_data: split-K slabs, the persistent kernels' queue-driven slabs, the repacked
    weights at the head of the workspace, the statistics partials (epilogue and reduction pass)"""
    recycled(hip, oracle, tuning, f"conv{case}", env, conv_run(case, compute, groups), conv_tol(compute),
             oracle_run=lambda: conv_oracle(oracle, case, 0, groups))


@pytest.mark.parametrize("compute", [0, X3], ids=["f32", "f32x3"])
def test_conv3d_generic_direct(hip, oracle, tuning, compute):
    """(2,3,5,7,6,5) k3 s2 p1: the generic direct kernels (the tolerances of test_conv3d_generic_direct); they declare no
    workspace, and M355_COMPUTE_F32X3 is M355_COMPUTE_F32 for them"""
    case = (2, 3, 5, 7, 6, 5)
    recycled(hip, oracle, tuning, f"direct{case}", {}, conv_run(case, compute, None, 3, 2, 1), conv_tol(0), has_workspace=None)

    def run(be, seed):
        x, _, _, _, dy = conv_inputs(case, seed, 3, 2, 1)
        dw, db = be.conv3d_bwd_weight(x, dy, 3, 2, 1, compute=compute if be.backend == "hip" else 0)
        return {"dw": dw, "db": db}
    recycled(hip, oracle, tuning, f"direct-bww{case}", {}, run, {"dw": (3e-5, 1e-4), "db": (3e-5, 1e-4)}, has_workspace=None)


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", [(2, 5, 7, 9, 10, 33), (1, 320, 64, 4, 4, 4)], ids=repr)
def test_conv3d_plain_entry_points_in_the_16bit_modes(hip, oracle, tuning, case, compute):
    """fp32 NCDHW in, 16-bit arithmetic: the c8 staging copy the entry points make in the workspace (5 channels leave three
    pad channels of the one channel block there; a NaN pad times a zero weight would be NaN), then the slabs.  With the
    fused statistics where the library has them in these modes: m355_conv3d_stats_slots is 0 for the split-K plan of
    (1,320,64,4,4,4), so that shape runs forward and data gradient only.  Statistics against norm_stats of the call's own
    output, as test_conv3d_h16_c8_input_persistent_and_fused_statistics holds them."""
    groups = 0 if case[1] == 5 else None
    tol = {k: v for k, v in conv_tol(compute).items() if k not in ("mean", "rstd")}
    tol["y_stats"] = tol["y"]

    def check(got):
        if groups is not None:
            m2, r2 = oracle.norm_stats(got["y_stats"].cpu(), groups)[:2]
            close(got["mean"], m2, 1e-5, 1e-6, "fused mean")
            close(got["rstd"], r2, 1e-5, 1e-6, "fused rstd")
    recycled(hip, oracle, tuning, f"conv16{case}", {}, conv_run(case, compute, groups), tol, check=check,
             oracle_run=lambda: conv_oracle(oracle, case, compute, groups))


# ------------------------------------------------------------------------------------------------- 3x3x3 weight gradient
def bww_run(case, compute):
    def run(be, seed):
        x, _, _, _, dy = conv_inputs(case, seed)
        dw, db = be.conv3d_bwd_weight(x, dy, 3, compute=(compute if be.backend == "hip" or compute in (1, 2) else 0))
        return {"dw": dw, "db": db}
    return run


@functools.lru_cache(maxsize=None)
def bww_oracle(oracle, case, compute):
    return bww_run(case, compute)(oracle, 1)


def bww_tol(case):
    N, _, _, D, H, W = case
    t = (3e-5, 3e-5 * (N * D * H * W) ** 0.5)
    return {"dw": t, "db": t}


BWW_SHAPES = [(1, 40, 40, 8, 8, 32), (1, 64, 40, 8, 8, 16), (2, 12, 8, 9, 10, 36), (1, 33, 80, 5, 9, 8), (1, 80, 33, 6, 7, 20),
              (1, 120, 16, 4, 8, 8), (1, 48, 96, 4, 6, 12)]


@pytest.mark.parametrize("compute", [0, X3], ids=["f32", "f32x3"])
@pytest.mark.parametrize("env", [{}, {"M355_BWW_NSPLIT": 3}, {"M355_BWW_NSPLIT": 1}], ids=env_id)
@pytest.mark.parametrize("case", BWW_SHAPES, ids=repr)
def test_conv3d_bwd_weight_fp32(hip, oracle, tuning, case, env, compute):
    """m355_conv3d_bwd_weight with bias: the split slabs of the four pair classes and the bias-gradient scratch (the cases
    and knobs of test_conv3d_bwd_weight_remainder_pair_classes)"""
    recycled(hip, oracle, tuning, f"bww{case}", {"M355_TILE16": 1, **env}, bww_run(case, compute), bww_tol(case),
             oracle_run=lambda: bww_oracle(oracle, case, 0))


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_conv3d_bwd_weight_plain_entry_point_in_the_16bit_modes(hip, oracle, tuning, compute):
    """(1,96,64,4,4,32): both operands rounded into c8 copies in the workspace, then the c8 kernel's slabs"""
    case = (1, 96, 64, 4, 4, 32)
    recycled(hip, oracle, tuning, f"bww16{case}", {}, bww_run(case, compute), bww_tol(case),
             oracle_run=lambda: bww_oracle(oracle, case, compute))


# ======================================================================================================= c8 entry points
def pads_are_zero(x16, channels, what):
    if channels % 8:
        assert (x16[:, (channels + 7) // 8 - 1, :, channels % 8:].float() == 0).all(), f"{what}: channel pads of the c8 layout must read 0"


H16_ENVS = [{"M355_CONV_KSPLIT": 1}, {"M355_CONV_KSPLIT": 1, "M355_CONV_SLOTS": 5, "M355_H16_ONESHOT": 3},
            {"M355_CONV_KSPLIT": 3}]


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("env", H16_ENVS, ids=env_id)
def test_conv3d_fwd_h16_and_bwd_data_h16(hip, oracle, tuning, env, compute):
    """c8 in, fp32 out, with the fused statistics where the plan is unsplit ((1,8,8,12,9,8) BatchNorm geometry, the smallest
    case of test_conv3d_h16_c8_input_persistent_and_fused_statistics); one-shot, queue-driven and split-K"""
    N, ci, co, D, H, W, groups = 1, 8, 8, 12, 9, 8, 0
    fused = env["M355_CONV_KSPLIT"] == 1

    def run(be, seed):
        x, w, b, _, dy = conv_inputs((N, ci, co, D, H, W), seed)
        x16, dy16 = be.act16_pack(x, compute), be.act16_pack(dy, compute)
        out = {"x16": x16, "dy16": dy16, "dx": be.conv3d_bwd_data_h16(dy16, co, w, x.shape, compute=compute)}
        if fused:
            out["y"], out["mean"], out["rstd"], out["partials"] = be.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute,
                                                                                     groups=groups, partials=True)
        else:
            out["y"] = be.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute)
        return out

    def check(got):
        x, w, b, _, dy = conv_inputs((N, ci, co, D, H, W), 1)
        close(got["y"], oracle.conv3d_fwd(x, w, b, compute=compute), 3e-5, 3e-5, "h16 fwd")
        close(got["dx"], oracle.conv3d_bwd_data(dy, w, x.shape, compute=compute), 3e-5, 3e-5, "h16 bwd_data")
        if fused:
            m2, r2 = oracle.norm_stats(got["y"].cpu(), groups)[:2]
            close(got["mean"], m2, 1e-5, 1e-6, "fused mean")
            close(got["rstd"], r2, 1e-5, 1e-6, "fused rstd")
    recycled(hip, oracle, tuning, "h16", env, run, check=check)


C8_ENVS = [{"M355_CONV_KSPLIT": 1}, {"M355_CONV_KSPLIT": 2, "M355_CONV_SLOTS": 5, "M355_H16_ONESHOT": 3}]


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("env", C8_ENVS, ids=env_id)
def test_conv3d_fwd_h16_c8_with_statistics(hip, oracle, tuning, env, compute):
    """c8 in, c8 out, 13 output channels: three pad channels in the second channel block, which the wrapper no longer
    pre-fills with 0.0; partials from the epilogue (unsplit) and from the reduction pass (split-K); and the statistics taken
    from the finished c8 tensor: m355_act16_channel_partials -> m355_norm_stats_from_partials"""
    N, ci, co, D, H, W, groups = 1, 24, 13, 6, 21, 16, 0
    dt = dt16(compute)

    def run(be, seed):
        x, w, b, _, _ = conv_inputs((N, ci, co, D, H, W), seed)
        x16 = be.act16_pack(x, compute)
        y16, part = be.conv3d_fwd_h16_c8(x16, ci, (D, H, W), w, b, compute=compute, with_stats=True)
        cpart = be.act16_channel_partials(y16, co, compute)
        mean, rstd = be.norm_stats_from_partials(cpart, (N, co, D, H, W), groups)
        return {"x16": x16, "y16": y16, "partials": part, "c8_partials": cpart, "mean": mean, "rstd": rstd}

    def check(got):
        x, w, b, _, _ = conv_inputs((N, ci, co, D, H, W), 1)
        y32 = hip.conv3d_fwd_h16(got["x16"], ci, (D, H, W), w, b, compute=compute).cpu()
        close(y32, oracle.conv3d_fwd(x, w, b, compute=compute), 3e-5, 3e-5, "the fp32-output kernel")
        y = _c8_to_ncdhw(got["y16"], co, (D, H, W))
        assert torch.equal(y, y32.to(dt).float()), "c8 output == the fp32 output rounded once"
        pads_are_zero(got["y16"], co, "y16")
        for pp, src in ((got["partials"], y32), (got["c8_partials"], y)):
            torch.testing.assert_close(pp[..., 0].sum(dim=1).cpu().double(), src.double().sum(dim=(2, 3, 4)), rtol=1e-4, atol=1e-3)
            torch.testing.assert_close(pp[..., 1].sum(dim=1).cpu().double(), (src.double() ** 2).sum(dim=(2, 3, 4)), rtol=1e-4, atol=1e-3)
        m2, r2 = oracle.norm_stats(y, groups)[:2]
        close(got["mean"], m2, 1e-5, 1e-6, "mean from c8 partials")
        close(got["rstd"], r2, 1e-5, 1e-6, "rstd from c8 partials")
    recycled(hip, oracle, tuning, "h16_c8", env, run, check=check)


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("env", [{}, {"M355_CONV_KSPLIT": 2}, {"M355_CONV_SLOTS": 5, "M355_H16_ONESHOT": 3}], ids=env_id)
@pytest.mark.parametrize("case", [(1, 4, 4, 4, 4, 32), (1, 24, 13, 6, 9, 16)], ids=repr)
def test_conv3d_bwd_data_h16_c8_and_weight_gradients_from_c8(hip, oracle, tuning, case, env, compute):
    """m355_conv3d_bwd_data_h16_c8 (4 channels: four pad channels in dx16), m355_conv3d_bwd_weight_c8 and _bwd_weight_h16:
    the smallest edge-layer case and the smallest wide case of test_conv3d_bwd_data_c8_output_and_weight_gradient_c8"""
    N, ci, co, D, H, W = case
    dt = dt16(compute)

    def run(be, seed):
        x, w, _, _, dy = conv_inputs(case, seed)
        x16, dy16 = be.act16_pack(x, compute), be.act16_pack(dy, compute)
        dw, db = be.conv3d_bwd_weight_c8(x16, dy16, ci, co, (D, H, W), compute)
        dw0, db0 = be.conv3d_bwd_weight_h16(x16, dy16, dy, ci, co, (D, H, W), compute)
        return {"x16": x16, "dy16": dy16, "dx16": be.conv3d_bwd_data_h16_c8(dy16, co, w, x.shape, compute), "dw": dw, "db": db,
                "dw_h16": dw0, "db_h16": db0}

    def check(got):
        x, w, _, _, dy = conv_inputs(case, 1)
        dx32 = hip.conv3d_bwd_data_h16(got["dy16"], co, w, x.shape, compute).cpu()
        close(dx32, oracle.conv3d_bwd_data(dy, w, x.shape, compute=compute), 3e-5, 3e-5, "the fp32-output kernel")
        dx = _c8_to_ncdhw(got["dx16"], ci, (D, H, W))
        if co > 4:
            assert torch.equal(dx, dx32.to(dt).float())
        else:
            _rounded_close(dx, dx32, compute, 2e-5 * dx32.abs().max().item(), "edge-layer dx")
        pads_are_zero(got["dx16"], ci, "dx16")
        pads_are_zero(got["x16"], ci, "x16")
        pads_are_zero(got["dy16"], co, "dy16")
        dyr = dy.to(dt).float()
        ref_dw, _ = oracle.conv3d_bwd_weight(x.to(dt).float(), dyr, 3)
        close(got["dw"], ref_dw, 3e-5, 3e-5 * ref_dw.abs().max().item(), "dw vs oracle")
        close(got["db"], dyr.double().sum(dim=(0, 2, 3, 4)).float(), 1e-5, 1e-4, "dbias from c8")
        if min(ci, co) > 4:
            assert torch.equal(got["dw"], got["dw_h16"])
            dwo, dbo = oracle.conv3d_bwd_weight(x, dy, 3, compute=compute)
            tol = 3e-5 * (N * D * H * W) ** 0.5
            close(got["dw_h16"], dwo, 3e-5, tol, "bwd_weight_h16")
            close(got["db_h16"], dbo, 3e-5, tol, "bwd_weight_h16 dbias")
        else:
            close(got["dw"], got["dw_h16"], 2e-5, 2e-5 * got["dw_h16"].abs().max().item(), "edge-layer dw vs the padded-tile kernel")
    recycled(hip, oracle, tuning, f"c8grads{case}", env, run, check=check)


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("env", [{}, {"M355_BWW_NSPLIT": 5}], ids=env_id)
def test_conv3d_bwd_weight_h16(hip, oracle, tuning, env, compute):
    """(1,32,32,4,8,32), the smallest case of test_conv3d_bwd_weight_from_c8_operands, one split set and five"""
    case = (1, 32, 32, 4, 8, 32)
    N, ci, co, D, H, W = case

    def run(be, seed):
        x, _, _, _, dy = conv_inputs(case, seed)
        dw, db = be.conv3d_bwd_weight_h16(be.act16_pack(x, compute), be.act16_pack(dy, compute), dy, ci, co, (D, H, W), compute)
        return {"dw": dw, "db": db}

    def check(got):
        x, _, _, _, dy = conv_inputs(case, 1)
        dwo, dbo = oracle.conv3d_bwd_weight(x, dy, 3, compute=compute)
        tol = 3e-5 * (N * D * H * W) ** 0.5
        close(got["dw"], dwo, 3e-5, tol, "bwd_weight from c8")
        close(got["db"], dbo, 3e-5, tol, "dbias")
    recycled(hip, oracle, tuning, "bww_h16", env, run, check=check)


# ===================================================================================================== conv-transposes
CONVT_CASES = [(2, 5, 7, 3, 5, 6, 2, 2, 0, 0), (1, 320, 48, 2, 2, 2, 2, 2, 0, 0), (1, 8, 8, 4, 4, 4, 4, 2, 1, 0),
               (1, 3, 4, 3, 3, 3, 3, 2, 1, 1)]


@functools.lru_cache(maxsize=None)
def convt_oracle(oracle, case):
    return convt_run(case)(oracle, 1)


def convt_run(case):
    N, Ci, Co, D, H, W, k, s, p, op = case

    def run(be, seed):
        o = 100 * (seed - 1)
        x, w, b = rnd(N, Ci, D, H, W, seed=o + 1), rnd(Ci, Co, k, k, k, seed=o + 2) * (1.0 / Ci ** 0.5), rnd(Co, seed=o + 3)
        y = be.convt_fwd(x, w, b, s, p, op)
        dy = rnd(*y.shape, seed=o + 5)
        dw, db = be.convt_bwd_weight(x, dy, k, s, p, op)
        return {"y": y, "dx": be.convt_bwd_data(dy, w, x.shape, s, p, op), "dw": dw, "db": db}
    return run


@pytest.mark.parametrize("case", CONVT_CASES, ids=repr)
def test_conv_transpose3d_fp32(hip, oracle, tuning, case):
    """forward, data gradient (320 -> 48 on 8 voxels splits K into workspace slabs) and weight gradient, MFMA and direct
    kernels (the tolerances of test_conv_transpose3d_fwd_bwd); the direct routes declare no workspace"""
    recycled(hip, oracle, tuning, f"convt{case}", {}, convt_run(case),
             {"y": (2e-5, 2e-5), "dx": (2e-5, 2e-5), "dw": (3e-5, 1e-4), "db": (3e-5, 1e-4)},
             oracle_run=lambda: convt_oracle(oracle, case), has_workspace=True if case[1] == 320 else None)


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_conv_transpose3d_c8_gradients(hip, oracle, tuning, compute):
    """m355_conv_transpose3d_bwd_weight_h16 (slabs in the workspace) and _bwd_data_h16 on (1,8,13,4,4,4), the smallest case
    m355_conv_transpose3d_h16_bwd_supported accepts in test_conv_transpose3d_c8_backward; 13 channels: pads in dy16"""
    N, ci, co, D, H, W = 1, 8, 13, 4, 4, 4
    dt = dt16(compute)
    assert hip.convt_h16_bwd_supported((N, ci, D, H, W), co)

    def inputs(seed):
        o = 100 * (seed - 1)
        return rnd(N, ci, D, H, W, seed=o + 1), rnd(N, co, 2 * D, 2 * H, 2 * W, seed=o + 2), rnd(ci, co, 2, 2, 2, seed=o + 3) * 0.2

    def run(be, seed):
        x, dy, w = inputs(seed)
        x16, dy16 = be.act16_pack(x, compute), be.act16_pack(dy, compute)
        dw, db = be.convt_bwd_weight_h16(x16, dy16, (N, ci, D, H, W), co, compute)
        return {"dy16": dy16, "dx16": be.convt_bwd_data_h16(dy16, w, (N, ci, D, H, W), compute), "dw": dw, "db": db}

    def check(got):
        x, dy, w = inputs(1)
        xr, dyr, wr = x.to(dt).float(), dy.to(dt).float(), w.to(dt).float()
        ref_dx = oracle.convt_bwd_data(dyr, wr, (N, ci, D, H, W), 2, 0, 0)
        _rounded_close(_c8_to_ncdhw(got["dx16"], ci, (D, H, W)), ref_dx, compute, 3e-5 * ref_dx.abs().max().item(), "convT dx")
        pads_are_zero(got["dy16"], co, "dy16")
        ref_dw, ref_db = oracle.convt_bwd_weight(xr, dyr, 2, 2, 0, 0)
        close(got["dw"], ref_dw, 3e-5, 3e-5 * ref_dw.abs().max().item(), "convT dw")
        close(got["db"], ref_db, 1e-5, 1e-4, "convT dbias")
    recycled(hip, oracle, tuning, "convt_c8", {}, run, check=check)


def test_conv_transpose3d_weight_gradient_on_the_split_pipe(hip, oracle, tuning):
    """m355_conv_transpose3d_bwd_weight_x3 on (2,40,24,3,5,8), the smallest case of test_convt_x3_grad_gpu.py: eight
    voxel-range splits, so eight slabs and eight rows of bias partials in the workspace; its bound: 3e-5 of the sum of
    |terms| per element.  (The data gradient has no split kernel: m355_conv_transpose3d_bwd_data_x3 launches nothing.)"""
    import test_convt_x3_grad_gpu as T
    shape = T.SHAPES[0]
    N, Cin, Cout, D, H, W = shape

    def run(be, seed):
        x, dy = T.operands(shape) if seed == 1 else (rnd(N, Cin, D, H, W, seed=101), rnd(N, Cout, 2 * D, 2 * H, 2 * W, seed=105))
        dw, db, nsplit = be.convt_bwd_weight_x3(x, dy)
        assert nsplit > 1, nsplit
        return {"dw": dw, "db": db}

    def check(got):
        ref_dw, ref_db, t, tb = T.reference(oracle, shape)
        T.bounded(got["dw"], ref_dw, 3e-5 * t + T.TINY, f"{shape} dw")
        T.bounded(got["db"], ref_db, 3e-5 * tb + T.TINY, f"{shape} dbias")
    recycled(hip, oracle, tuning, "convt_x3", {"M355_F32X3_CONVT_BWD": 2}, run, check=check)


# ============================================================================================================== norm.hip
NORM_CASES = [   # N, C, D, H, W, groups, act, training
    (2, 16, 5, 6, 7, 4, 1, 1),       # S no multiple of 4: the scalar path
    (3, 6, 3, 3, 5, 0, 2, 1),        # batch norm, ragged
    (1, 40, 8, 8, 8, 8, 0, 1),
    (1, 8, 32, 32, 32, 1, 1, 1),     # one group of 262144 elements: multi-block partials
    (2, 13, 2, 6, 8, 0, 1, 0),       # eval mode
]


def norm_inputs(case, seed):
    N, Cc, D, H, W, groups, act, training = case
    o = 100 * (seed - 1)
    x = rnd(N, Cc, D, H, W, seed=o + 1) * 1.7 + 0.3
    running = None if groups else (rnd(Cc, seed=o + 5) * 0.1, torch.rand(Cc, generator=torch.Generator().manual_seed(o + 6)) + 0.5)
    return x, rnd(Cc, seed=o + 2), rnd(Cc, seed=o + 3), rnd(N, Cc, D, H, W, seed=o + 7), running


@functools.lru_cache(maxsize=None)
def norm_oracle(oracle, case, seed):
    """the oracle's statistics (the backward's inputs on both backends, as in test_norm_act_fwd_bwd) and results of one seed"""
    N, Cc, D, H, W, groups, act, training = case
    x, gamma, beta, dy, running = norm_inputs(case, seed)
    mean, rstd, rm, rv = oracle.norm_stats(x, groups, running=running)
    dx, dg, db = oracle.norm_act_bwd(x, dy, mean, rstd, gamma, beta, groups, act, training)
    return {"mean": mean, "rstd": rstd, "running_mean": rm, "running_var": rv, "dx": dx, "dgamma": dg, "dbeta": db}


@pytest.mark.parametrize("case", NORM_CASES, ids=repr)
def test_norm_fp32_entry_points(hip, oracle, tuning, case):
    """m355_norm_stats with (batch norm) and without running statistics, m355_norm_sums -> _stats_from_sums, m355_norm_act_bwd,
    _bwd_h16, the _reduce / _apply halves with stat_m, and on even volumes m355_norm_act_bwd_pool: block partials and stat_m in
    the workspace.  Tolerances of test_norm_act_fwd_bwd for every form of the backward; the split statistics and the pooled
    form are held to the values of the fused calls, as test_norm_halves_gpu.py and test_norm_bwd_fusion_gpu.py hold them."""
    N, Cc, D, H, W, groups, act, training = case
    even = D % 2 == 0 and H % 2 == 0 and W % 2 == 0

    def run(be, seed):
        x, gamma, beta, dy, running = norm_inputs(case, seed)
        o = norm_oracle(oracle, case, seed)
        out = dict(zip(("mean", "rstd", "running_mean", "running_var"), be.norm_stats(x, groups, running=running)))
        out["mean_plain"], out["rstd_plain"] = be.norm_stats(x, groups)[:2]
        if groups == 0:
            out["sums"] = be.norm_sums(x)
            out.update(zip(("mean_s", "rstd_s", "running_mean_s", "running_var_s"),
                           be.norm_stats_from_sums(out["sums"], x.shape, running=running)))
        a = (x, dy, o["mean"], o["rstd"], gamma, beta)
        out["dx"], out["dgamma"], out["dbeta"] = be.norm_act_bwd(*a, groups, act, training)
        out["dx_h"], out["dgamma_h"], out["dbeta_h"], out["dx16"] = be.norm_act_bwd_h16(*a, groups, act, 1, training)
        out["stat_m"], out["dgamma_r"], out["dbeta_r"] = be.norm_act_bwd_reduce(*a, groups, act, training)
        out["dx_a"], out["dx16_a"] = be.norm_act_bwd_apply(*a, out["stat_m"], groups, act, compute=1)
        if even:
            dp = rnd(N, Cc, D // 2, H // 2, W // 2, seed=100 * (seed - 1) + 8)
            out["dx_p"], out["dgamma_p"], out["dbeta_p"] = be.norm_act_bwd_pool(x, dy, dp, o["mean"], o["rstd"], gamma, beta, groups,
                                                                               act, training)
            out["two_step"] = be.norm_act_bwd(x, be.avgpool_bwd_add(dp, dy, x.shape), *a[2:], groups, act, training)[0]
        return out

    def check(got):
        o = norm_oracle(oracle, case, 1)
        close(got["mean"], o["mean"], 1e-6, 1e-6, "mean")
        close(got["rstd"], o["rstd"], 2e-6, 1e-6, "rstd")
        assert bit_equal(got["mean_plain"], got["mean"]) and bit_equal(got["rstd_plain"], got["rstd"])
        if groups == 0:
            close(got["running_mean"], o["running_mean"], 1e-6, 1e-6, "running_mean")
            close(got["running_var"], o["running_var"], 2e-6, 1e-6, "running_var")
            for k in ("mean", "rstd", "running_mean", "running_var"):
                assert bit_equal(got[k + "_s"], got[k]), f"{k}: sums + stats_from_sums == norm_stats"
        for sfx in ("", "_h", "_a"):      # the fused call, the call with the c8 twin, the second half
            close(got["dx" + sfx], o["dx"], 2e-5, 2e-5, "dx" + sfx)
        for sfx in ("", "_h", "_r"):      # ... and the first half
            close(got["dgamma" + sfx], o["dgamma"], 2e-5, 1e-4, "dgamma" + sfx)
            close(got["dbeta" + sfx], o["dbeta"], 2e-5, 1e-4, "dbeta" + sfx)
        for dx16, dx in ((got["dx16"], got["dx_h"]), (got["dx16_a"], got["dx_a"])):
            assert torch.equal(_c8_to_ncdhw(dx16, Cc, (D, H, W)), dx.cpu().to(torch.bfloat16).float()), "c8 twin == its dx rounded once"
            pads_are_zero(dx16, Cc, "dx16")
        if even:
            assert torch.equal(got["dx_p"], got["two_step"]), "pooled backward == the two-step form"
    recycled(hip, oracle, tuning, f"norm{case}", {}, run, check=check)


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", [c for c in NORM_CASES if c[2] % 2 == 0 and c[3] % 2 == 0 and c[4] % 2 == 0], ids=repr)
def test_norm_act_bwd_c8_and_its_halves(hip, oracle, tuning, case, compute):
    """m355_norm_act_bwd_c8 (dy16 + un-pooled dpool16) against the oracle on the 16-bit values at the bounds of
    test_norm_act_bwd_c8; m355_norm_act_bwd_c8_reduce / _apply hold its bits"""
    N, Cc, D, H, W, groups, act, training = case
    dt = dt16(compute)

    def inputs(seed):
        x, gamma, beta, dy, _ = norm_inputs(case, seed)
        return x, gamma * 0.5 + 1.0, beta * 0.1, dy, rnd(N, Cc, D // 2, H // 2, W // 2, seed=100 * (seed - 1) + 8)

    def stats(seed):
        return oracle.norm_stats(inputs(seed)[0].to(dt).float(), groups)[:2]

    def run(be, seed):
        x, gamma, beta, dy, dp = inputs(seed)
        mean, rstd = stats(seed)
        x16, dy16, dp16 = be.act16_pack(x, compute), be.act16_pack(dy, compute), be.act16_pack(dp, compute)
        a = (x16, dy16, dp16, Cc, (D, H, W), mean, rstd, gamma, beta)
        out = dict(zip(("dx16", "dgamma", "dbeta"), be.norm_act_bwd_c8(*a, groups, act, compute, training=training)))
        out["stat_m"], out["dgamma_r"], out["dbeta_r"] = be.norm_act_bwd_c8_reduce(*a, groups, act, compute, training=training)
        out["dx16_a"] = be.norm_act_bwd_c8_apply(*a, out["stat_m"], groups, act, compute)
        return out

    def check(got):
        x, gamma, beta, dy, dp = inputs(1)
        mean, rstd = stats(1)
        g = dy.to(dt).float() + 0.125 * dp.to(dt).float().repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)
        ref_dx, ref_dg, ref_db = oracle.norm_act_bwd(x.to(dt).float(), g, mean, rstd, gamma, beta, groups, act, training=training)
        _rounded_close(_c8_to_ncdhw(got["dx16"], Cc, (D, H, W)), ref_dx, compute, 2e-5 * ref_dx.abs().max().item(), "dx")
        close(got["dgamma"], ref_dg, 1e-4, 1e-4 * ref_dg.abs().max().item(), "dgamma")
        close(got["dbeta"], ref_db, 1e-4, 1e-4 * ref_db.abs().max().item(), "dbeta")
        pads_are_zero(got["dx16"], Cc, "dx16")
        assert bit_equal(got["dx16_a"], got["dx16"]) and bit_equal(got["dgamma_r"], got["dgamma"]) and bit_equal(got["dbeta_r"], got["dbeta"])
    recycled(hip, oracle, tuning, f"norm_c8{case}", {}, run, check=check)


def test_pooling_norm_forward_patch_accumulate_and_sums_from_partials(hip, oracle, tuning):
    """the remaining wrappers with a second output: m355_norm_act_pool_fwd (pooled output), m355_norm_act_fwd_h16 (c8 twin,
    13 channels: three pads), m355_maxpool3d_2x_fwd / _fwd_h16 with their route bytes and the backward through them,
    m355_patch_accumulate + _finalize (accumulator and count zeroed by the caller, never dirtied), and m355_norm_sums fed
    by a conv epilogue's partials.  Tolerances of test_norm_act_with_pooled_second_output, test_norm_act_and_avgpool_c8_outputs,
    test_maxpool_gpu.py (bit-exact against torch) and test_patches_roundtrip_and_confusion; the sums from fp32 partials
    against fp64 sums within n 2^-24 sum|terms| (n values per channel, each fp32 addition rounds once), the count exact."""
    import torch.nn.functional as F
    N, Cc, D, H, W, groups, act = 2, 13, 4, 6, 8, 0, 1
    vshape, pshape = (20, 18, 22), (8, 8, 8)
    from oracle import torch_ref as R
    loc = torch.tensor(R.grid_locations(vshape, pshape, (2, 2, 2)), dtype=torch.int32)
    ccase = (2, 8, 16, 9, 10, 36)

    def inputs(seed):
        o = 100 * (seed - 1)
        x = rnd(N, Cc, D, H, W, seed=o + 1)
        return (x, rnd(Cc, seed=o + 2) * 0.5 + 1.0, rnd(Cc, seed=o + 3) * 0.1, rnd(N, Cc, D // 2, H // 2, W // 2, seed=o + 4),
                rnd(N, Cc, D, H, W, seed=o + 5), rnd(loc.shape[0], 2, *pshape, seed=o + 6))

    def run(be, seed):
        x, gamma, beta, dp, dskip, pv = inputs(seed)
        mean, rstd = oracle.norm_stats(x, groups)[:2]
        out = {}
        out["y"], out["pooled"] = be.norm_act_pool_fwd(x, mean, rstd, gamma, beta, groups, act)
        out["y16"], out["y32"] = be.norm_act_fwd_h16(x, mean, rstd, gamma, beta, groups, act, 1, want_f32=True)
        out["max"], out["route"] = be.maxpool_fwd(x)
        out["max_dx"] = be.maxpool_bwd(dp, out["route"], dskip, x.shape)
        x16, dp16, dskip16 = be.act16_pack(x, 1), be.act16_pack(dp, 1), be.act16_pack(dskip, 1)
        out["max16"], out["route8"] = be.maxpool_fwd_h16(x16, Cc, (D, H, W), 1)
        out["max_dx16"] = be.maxpool_bwd_h16(dp16, out["route8"], dskip16, Cc, (D, H, W), 1)
        out["aggregated"], out["count"] = be.patch_aggregate(pv, loc, vshape)
        cx, cw, cb, _, _ = conv_inputs(ccase, seed)
        cy, _, _, part = be.conv3d_fwd_stats(cx, cw, cb, 4, partials=True)
        out["conv_y"], out["sums"] = cy, be.norm_sums(stat_partials=part, x_shape=cy.shape)
        return out

    def check(got):
        x, gamma, beta, dp, dskip, pv = inputs(1)
        mean, rstd = oracle.norm_stats(x, groups)[:2]
        ref = oracle.norm_act_fwd(x, mean, rstd, gamma, beta, groups, act)
        close(got["y"], ref, what="norm_act_pool_fwd y")
        close(got["pooled"], oracle.avgpool_fwd(ref), 1e-5, 1e-6, "pooled")
        close(got["y32"], ref, 1e-5, 1e-5, "fp32 twin")
        assert torch.equal(_c8_to_ncdhw(got["y16"], Cc, (D, H, W)), got["y32"].cpu().to(torch.bfloat16).float())
        pads_are_zero(got["y16"], Cc, "y16")
        xr = x.clone().requires_grad_()
        ymax = F.max_pool3d(xr, 2, 2)
        assert torch.equal(got["max"].cpu(), ymax.detach())
        assert torch.equal(got["max_dx"].cpu(), torch.autograd.grad(ymax, xr, dp)[0] + dskip)
        bf = lambda t: t.to(torch.bfloat16).float()   # noqa: E731
        xr = bf(x).requires_grad_()
        ymax = F.max_pool3d(xr, 2, 2)
        assert torch.equal(_c8_to_ncdhw(got["max16"], Cc, (D // 2, H // 2, W // 2)), ymax.detach())
        routed = torch.autograd.grad(ymax, xr, bf(dp))[0]
        assert torch.equal(_c8_to_ncdhw(got["max_dx16"], Cc, (D, H, W)), bf(bf(dskip) + routed))
        pads_are_zero(got["max16"], Cc, "max16")
        pads_are_zero(got["max_dx16"], Cc, "max_dx16")
        ao, co = oracle.patch_aggregate(pv, loc, vshape)
        assert torch.equal(got["count"].cpu(), co)
        close(got["aggregated"], ao, 1e-6, 1e-6, "patch_aggregate")
        y = got["conv_y"].cpu().double()
        n, C_ = y.shape[0] * y[0, 0].numel(), y.shape[1]
        sums = got["sums"].cpu()
        assert sums[2 * C_].item() == n
        for j, terms in enumerate((y, y * y)):
            want, scale = terms.sum(dim=(0, 2, 3, 4)), terms.abs().sum(dim=(0, 2, 3, 4))
            assert ((sums[:2 * C_].view(C_, 2)[:, j] - want).abs() <= n * 2.0 ** -24 * scale).all(), ("sum", "sum of squares")[j]
    recycled(hip, oracle, tuning, "pool_norm_fwd", {"M355_CONV_KSPLIT": 1}, run, check=check)


# =========================================================================================================== hybrid loss
@pytest.mark.parametrize("shape", [(2, 3, 9, 10, 11), (1, 2, 17, 33, 31)], ids=repr)
def test_hybrid_loss(hip, oracle, tuning, shape):
    """m355_hybrid_loss_fwd (block partials in the workspace) and _bwd at the tolerances of test_hybrid_loss_fwd_bwd"""
    N, Cc = shape[:2]

    def run(be, seed):
        p = torch.softmax(rnd(*shape, seed=10 * seed) * 2, dim=1)
        lab = torch.randint(0, Cc, (N,) + shape[2:], generator=torch.Generator().manual_seed(10 * seed + 1))
        t = torch.nn.functional.one_hot(lab, Cc).permute(0, 4, 1, 2, 3).float().contiguous()
        cw = torch.tensor([1.0, 2.0, 3.0][:Cc])
        out3, sums = be.loss_fwd(p, t, 0.3, cw, False)
        return {"out3": out3, "sums": sums, "dp": be.loss_bwd(p, t, sums, 0.7, 0.3, cw, False)}
    recycled(hip, oracle, tuning, f"loss{shape}", {}, run, {"out3": (2e-6, 1e-7), "sums": (2e-6, 1e-6), "dp": (1e-5, 1e-9)})


# =================================================================================== package level: through torch.empty
def package_recycled(monkeypatch, run, other, reference, deterministic=True):
    """assert_recycled for code that allocates through torch (ops.py): run() / other() -> {name: tensor} on the case's and on
    other inputs; "stale" is other() unpoisoned before each poisoned run"""
    def under(mode):
        with PoisonedEmpty(monkeypatch, mode) as p:
            out = run()
            torch.cuda.synchronize()
        return out, p.dirtied
    clean, again = under("zeros")[0], under("zeros")[0]
    if deterministic:
        diff = [k for k in clean if not bit_equal(clean[k], again[k])]
        assert not diff, f"(a) two runs on zeroed memory differ in {diff}"
    for mode in ("ones", "nan"):
        other()
        got, dirtied = under(mode)
        assert dirtied >= 1, f"(d) {mode}: no allocation went through the wrapped torch.empty family"
        if deterministic:
            diff = [k for k in clean if not bit_equal(clean[k], got[k])]
            assert not diff, f"(b) on {mode!r} memory {diff} differ from the run on zeroed memory"
        if mode == "nan" or not deterministic:
            reference(got)


# (one channel in logits mode: the focal Tversky criterion has no such kernel, as in its own test)
@pytest.mark.parametrize("which,case,from_logits", [(w, c, fl) for w in ("binary", "focal_tversky") for c in ("small", "c1")
                                                     for fl in (False, True) if (w, c, fl) != ("focal_tversky", "c1", True)],
                         ids=lambda v: {False: "prob", True: "logits"}.get(v, v) if isinstance(v, bool) else v)
def test_package_binary_and_focal_tversky_criteria(monkeypatch, which, case, from_logits):
    """the criteria forward and backward through ops.py, configuration 1 of their own tests, against the fp64 formulas at the
    bounds of test_fwd_bwd_against_fp64 (loss terms close(2e-6, 1e-7), gradient for dloss = 0.7 close(1e-5, 1e-9))"""
    if which == "binary":
        import test_binary_loss_gpu as T
        from segmentation_pipeline_amd.criterions import HybridBinaryLogisticDiceLoss as Crit
    else:
        import test_focal_tversky_gpu as T
        from segmentation_pipeline_amd.criterions import HybridFocalTverskyLoss as Crit
    x, t, kw, (out3_ref, _, dx_ref), _ = T.expected(case, 1, from_logits)
    order = (("dice_weight", "class_weights", "pos_weight", "square_dice") if which == "binary" else
             ("tversky_weight", "alpha", "beta", "tversky_power", "focal_gamma", "focal_class_weights", "tversky_class_weights"))
    crit = Crit(*[kw[k] for k in order], from_logits)

    def step(x, t):
        xd = x.cuda().requires_grad_(True)
        ld = crit(xd, t.cuda())
        (ld["loss"] * T.DLOSS).backward()
        return {"out3": torch.stack([v.detach() for v in ld.values()]), "dx": xd.grad}

    def reference(got):
        T.close(got["out3"], out3_ref, 2e-6, 1e-7, f"{which} {case} out3")
        T.close(got["dx"], dx_ref, 1e-5, 1e-9, f"{which} {case} dx")
    package_recycled(monkeypatch, lambda: step(x, t), lambda: step(x.flip(2) * 0.5 + (0 if from_logits else 0.25), t.flip(3)), reference)


def test_package_blob_loss(monkeypatch):
    """ops.blob_dice_loss: blob_zero_kernel clears the accumulators of the n components the call has, n read on the device --
    so the snake (1 component) runs after a call with MORE components (the checkerboard) and after one with fewer (an empty
    target) have been through the same recycled tables; bounds of test_loss_and_gradient_against_the_literal_definition"""
    import numpy as np

    import test_blob_loss_gpu as T
    from segmentation_pipeline_amd import ops

    def step(name, square, target=None):
        tgt = T.CASES[name][0] if target is None else target
        p = T.BR.prediction("uniform", tgt.shape).cuda().requires_grad_()
        _, weights, planes, conn = T.CASES[name]
        if planes is None:
            loss, count = ops.blob_dice_loss(p, tgt.cuda(), weights, square, conn)
        else:
            loss, count = ops.blob_dice_loss(p, tgt.cuda(), torch.tensor(weights, device="cuda"), square, conn, planes=planes)
        loss.backward(torch.tensor(T.DLOSS, device="cuda"))
        return {"loss": loss.detach(), "count": count, "grad": p.grad}

    for name in ("checkerboard_6conn", "snake_1x1x17x10x130"):
        for square in (False, True):
            ref, ref_grad, ref_count = T._reference(name, "uniform", square)

            def reference(got):
                assert got["count"].item() == ref_count
                assert abs(got["loss"].double().item() - ref.item()) <= 2.0 ** -31 + 2.0 ** -24 * abs(ref.item())
                g, w = got["grad"].double().cpu().numpy(), (ref_grad * T.DLOSS).numpy()
                tol = np.full(w.shape, 4.0 * T._ulp32(np.abs(w).max())) if square else np.maximum(4.0 * T._ulp32(w), 0)
                on = np.abs(w) > 0 if not square else np.ones(w.shape, bool)
                assert (np.abs(g - w)[on] <= tol[on]).all() and not g[(w == 0) & ~on].any()

            def other():
                step("checkerboard_6conn", square)                                             # more components
                step(name, square, target=torch.zeros_like(T.CASES[name][0]))                  # fewer: none
            package_recycled(monkeypatch, lambda: step(name, square), other, reference)


@pytest.mark.parametrize("name,prec", [("unet", "fp32"), ("unet", "bf16"), ("unet", "fp16"), ("nested", "fp32")])
def test_package_model_forward_and_backward(monkeypatch, name, prec):
    """one training step of the smallest ModularUNet (filters [8, 16]; all three activation flows) and NestedResUNet (fp32
    flow; its 16-bit flows: the next test) of test_binary_loss_gpu.py: probabilities, loss and every parameter gradient.
    Reference: the fp32 flow against the CPU formulation at the bounds of test_model_fp32_flow_matches_the_cpu (1e-4;
    gradients 1e-3 max |g| + 1e-7); the ModularUNet's 16-bit flows at the bound of test_unet_16bit_training_step (finite,
    cosine with the fp32-flow gradient >= 0.95)."""
    import copy

    import segmentation_pipeline_amd as sp
    import test_binary_loss_gpu as T
    from segmentation_pipeline_amd import ops
    make, cin, cout, cpu_logits, pw = T.MODELS[name]
    model = make(nn.Sigmoid).cuda().train()
    sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    crit = T._criterion(name, False)
    x, y = T._batch(cin, cout)
    x2, y2 = T._batch(cin, cout, seed=99)

    def step(x, y):
        m = copy.deepcopy(model).train()       # (BatchNorm running statistics start from the same state every time)
        with sp.precision(prec):
            if prec == "fp16":
                ops.fp16_overflow()
            out, loss, grads = T._train_step(m, crit, x.cuda(), y.cuda())
        return {"out": out, "loss": loss, **{"grad " + k: g for k, g in grads.items()}}

    with sp.precision("fp32"):
        grads32 = T._train_step(copy.deepcopy(model).train(), crit, x.cuda(), y.cuda())[2]

    def reference(got):
        if prec == "fp32":
            names = {k for k, _ in model.named_parameters()}
            sd = {k: v.clone().requires_grad_(k in names) for k, v in sd0.items()}
            logits_ref = cpu_logits(sd, x)
            p_ref = torch.sigmoid(logits_ref)
            loss_ref = T.B.binary_loss(p_ref, y, pos_weight=pw, from_logits=False)["loss"]
            loss_ref.backward()
            assert (got["out"].cpu() - p_ref.detach()).abs().max().item() <= 1e-4
            assert abs(got["loss"].item() - loss_ref.item()) <= 1e-4
            for k in sorted(names):
                g_ref = sd[k].grad
                assert (got["grad " + k].cpu() - g_ref).abs().max().item() <= 1e-3 * g_ref.abs().max().item() + 1e-7, k
        else:
            assert bool(torch.isfinite(got["loss"]))
            for k, g32 in grads32.items():
                a, b = got["grad " + k].double().flatten(), g32.double().flatten()
                assert torch.isfinite(a).all(), k
                assert float(a @ b / (a.norm() * b.norm() + 1e-300)) >= 0.95, k
    package_recycled(monkeypatch, lambda: step(x, y), lambda: step(x2, y2), reference)


def test_package_label_and_post_processing(monkeypatch, golden):
    """post_processing.label at connectivity 1 and 3 on the serpentine of test_label_serpentine_across_many_tiles (one
    component through every tile: long merge chains over the parent table in the workspace), keep_components and remove_holes
    on the golden lesion map (histograms, rank tables, the dilation's ping-pong buffer): exactly the reference's results"""
    import numpy as np

    from segmentation_pipeline_amd import post_processing as PP
    D, H, W = 20, 34, 150
    img = np.zeros((D, H, W), np.uint8)
    for z in range(0, D, 2):
        img[z, 0::2, :] = 1
        img[z, 1::4, W - 1] = 1
        img[z, 3::4, 0] = 1
        img[z + 1, 0, 0] = 1
    g = golden("postprocessing.npz")
    snake, lesion = torch.from_numpy(img).cuda(), torch.from_numpy(g["lesion/img"].copy()).cuda()

    def step(snake, lesion):
        out = {}
        for conn in (1, 3):
            lab, n = PP.label(snake, connectivity=conn, return_num=True)
            out[f"label{conn}"], out[f"n{conn}"] = lab, torch.tensor(n)
        kept, comps, elems = PP.keep_components(lesion, 5)
        filled, holes = PP.remove_holes(lesion, 64)
        out.update(kept=kept, kept_counts=torch.tensor([int(comps), int(elems)]), filled=filled, holes=torch.tensor(int(holes)))
        return out

    def reference(got):
        for conn in (1, 3):
            assert int(got[f"n{conn}"]) == 1
            np.testing.assert_array_equal(got[f"label{conn}"].cpu().numpy(), img.astype(np.int64))
        np.testing.assert_array_equal(got["kept"].cpu().numpy(), g["lesion/keep5/out"])
        assert got["kept_counts"].tolist() == g["lesion/keep5/counts"].tolist()
        np.testing.assert_array_equal(got["filled"].cpu().numpy(), g["lesion/holes64/out"])
        assert [int(got["holes"])] == g["lesion/holes64/counts"].tolist()
    package_recycled(monkeypatch, lambda: step(snake, lesion), lambda: step(snake.flip(1), lesion.flip(2)), reference)


def test_package_target_pyramid_and_sampler(monkeypatch):
    """ops.target_pyramid (deep supervision; one flat result buffer whose levels are returned as views: the bytes between
    the levels are don't-care and not compared -- the mask of this case is "the returned views") bit for bit against
    avg_pool3d, as test_area_pyramid_of_a_one_hot_target_is_avg_pool3d_bit_for_bit; ops.sampler_build / sampler_draw on the
    (37,41,45) map of the sampler's own test: the cumulative table (block sums scanned in place) and the drawn corners equal
    the float64 restatement"""
    import deep_supervision_ref as DS
    from oracle import torch_ref as R
    from segmentation_pipeline_amd import ops
    dims, levels = (2, 3, 8, 16, 24), 3
    y = DS.one_hot_target(dims, 11)
    g = torch.Generator().manual_seed(5)
    shape, patch = (37, 41, 45), (8, 6, 10)
    pm = torch.rand(shape, generator=g)
    pm[pm < 0.3] = 0.0
    pm[5:9, 7:11, 3:30] = -2.0
    pm[20, 20, 20] = 5000.0
    pm[0, 0, 0] = 1e9
    u = torch.rand(512, dtype=torch.float64, generator=g)
    u[:4] = torch.tensor([0.0, 1.0 - 2.0 ** -53, 0.5, 1e-300], dtype=torch.float64)
    ref_loc, weights = R.weighted_sample_locations(pm.numpy(), patch, u.numpy())

    def step(y, pm):
        out = {f"level{j}": t for j, t in enumerate(ops.target_pyramid(y.cuda(), levels, 'area'), 1)}
        out["table"] = ops.sampler_build(pm.cuda(), patch)
        out["loc"] = ops.sampler_draw(pm.cuda(), out["table"], patch, u.cuda())
        return out

    def reference(got):
        for j, ref in enumerate(DS.pyramid(y, levels, 'area'), 1):
            assert torch.equal(got[f"level{j}"].cpu(), ref), f"level {j}"
        assert torch.equal(got["loc"].cpu(), torch.from_numpy(ref_loc))
        assert float(got["table"][-1]) == pytest.approx(float(weights.sum()), rel=1e-12) and float(got["table"][0]) == 0.0
    package_recycled(monkeypatch, lambda: step(y, pm), lambda: step(y.flip(2), pm.flip(0) * 0.5), reference)


def test_package_score_and_multilabel_evaluators(monkeypatch):
    """ops.eval_scores (argmax through a label table under a mask map, label-map target; predicted maps written) as
    test_scores_with_mask_map_and_label_map_targets, and ops.eval_multilabel on two subjects of odd sizes with per-channel
    thresholds as test_counts_against_torch: count tables zeroed by the call, exact against torch on the CPU"""
    import numpy as np

    import test_evaluation_gpu as TE
    import test_multilabel_eval_gpu as TM
    from segmentation_pipeline_amd import ops
    g = torch.Generator().manual_seed(11)
    sh = (5, 9, 13)
    s = torch.randn((2,) + sh, generator=g)
    mask = (torch.rand(sh, generator=g) < 0.5).to(torch.uint8)[None]
    target = torch.randint(0, 3, sh, generator=g).to(torch.int64)[None]
    table = ([0, 1], [0, 2])
    subjects = [TM.make_subject(g, 5, size, torch.float32, torch.uint8) for size in TM.SIZES["odd"]]
    thresholds = [0.5, 0.25, float("inf"), float("-inf"), 0.75]

    def step(s, subjects):
        counts, preds, _ = ops.eval_scores([s.cuda()], table, [1, 2], targets=[target.cuda()], masks=[mask.cuda()],
                                           write_pred=True, one_hot_targets=False)
        ml = ops.eval_multilabel([a.cuda() for a, _ in subjects], [t.cuda() for _, t in subjects], thresholds)
        return {"counts": counts[0], "pred": preds[0], "multilabel": ml}

    def reference(got):
        lab, tl = TE._ref_scores(s, table, target, mask=mask, one_hot=False)
        assert torch.equal(got["pred"].cpu()[0], lab)
        np.testing.assert_array_equal(got["counts"].cpu().numpy(), TE.np_counts(lab, tl, [1, 2]))
        for i, (a, t) in enumerate(subjects):
            assert np.array_equal(got["multilabel"][i].cpu().numpy(), TM.torch_counts(a, t, thresholds)), i
    package_recycled(monkeypatch, lambda: step(s, subjects), lambda: step(-s, [(1 - a, t) for a, t in subjects]), reference)


def test_package_surface_distance_evaluator(monkeypatch):
    """SurfaceDistanceEvaluator on every case of its fixture in one call (test_evaluator_fixture): border masks into a
    recycled scratch, the EDT workspace, the pooled gather buffer and the statistics table are torch.empty; the border counts,
    the gather cursors and the cast flags are caller-zeroed (torch.zeros) and must stay so.  Bounds of that test: surface
    voxel counts exact, distances within 2e-6 relative"""
    import numpy as np

    import test_surface_distance_gpu as TS
    from segmentation_pipeline_amd.evaluators import SURFACE_STAT_NAMES, SurfaceDistanceEvaluator
    fx = dict(np.load(os.path.join(TS.ROOT, "tests", "golden", "surface_distance.npz")))
    labels = TS._labels(fx)
    ncases = int(fx["cases"])
    ev = SurfaceDistanceEvaluator("pred", "target", percentile=int(fx["percentile"]), tolerance=float(fx["tolerance"]),
                                  stats_to_output=SURFACE_STAT_NAMES)

    def step(swap):
        subjects = [TS._subject(f"case{c}", fx[f"{c}.target" if swap else f"{c}.pred"], fx[f"{c}.pred" if swap else f"{c}.target"],
                                labels, tuple(fx[f"{c}.spacing"])) for c in range(ncases)]
        df = ev(subjects)["subject_stats"]
        rows = [[float(TS._row(df, f"case{c}", name)[stat]) for stat in SURFACE_STAT_NAMES] for c in range(ncases) for name in labels]
        return {"stats": torch.tensor(rows, dtype=torch.float64)}

    def reference(got):
        k = 0
        for c in range(ncases):
            for name in labels:
                want, row = fx[f"{c}.{name}.stats"], got["stats"][k].numpy()
                k += 1
                for j, stat in enumerate(SURFACE_STAT_NAMES):
                    if np.isnan(want[j]):
                        assert np.isnan(row[j]), (c, name, stat)
                    elif stat.endswith("_surface"):
                        assert row[j] == want[j], (c, name, stat)
                    else:
                        assert abs(row[j] - want[j]) <= 2e-6 * abs(want[j]), (c, name, stat, row[j], want[j])
    package_recycled(monkeypatch, lambda: step(False), lambda: step(True), reference)


def test_package_contour_counts_rank_and_mosaic(monkeypatch):
    """ops.slice_counts (per-slice count tables zeroed by the call) on the int32 label maps of test_slice_counts_label_maps,
    ops.slice_rank over every subject's three segments against a sort on the host, and ops.slice_mosaic (pad cells
    included) as test_mosaic_planes_and_grids: exact"""
    import numpy as np

    import contour_ref
    import test_contour_gpu as TC
    from segmentation_pipeline_amd import ops
    g = torch.Generator().manual_seed(4)
    maps = [TC._label_map(g, sh, torch.int32) for sh in TC.SHAPES] + [torch.zeros((4, 9, 21), dtype=torch.int32),
                                                                     TC._label_map(g, (3, 50, 449), torch.int32, density=0.1)]
    plane, n, ncol = contour_ref.PLANES[1], 5, 2
    dim = TC.VOL[1]
    img, lab = TC._volumes(torch.float32, n, 1), TC._volumes(torch.int64, n, 2)
    img[1] = None
    ks = [0, dim - 1, 2, 0, dim - 1]
    shape = contour_ref.slice_shape(TC.VOL, plane)

    def step(maps, flip):
        counts, layout = ops.slice_counts([m.cuda() for m in maps])
        segs = [(off + o, ln) for off, size3 in layout for o, ln in zip((0, size3[0], size3[0] + size3[1]), size3)]
        ids, ranked, nums = ops.slice_rank(counts, segs)
        outs, _ = ops.slice_mosaic([
            ([(None if v is None else (v.flip(0) if flip else v).cuda(), plane, k) for v, k in zip(img, ks)], ncol, -1, shape),
            ([((v.flip(0) if flip else v).cuda(), plane, k) for v, k in zip(lab, ks)], ncol, 0, shape)])
        return {"counts": counts, "ids": ids, "ranked": ranked, "nums": nums, "mosaic_img": outs[0], "mosaic_lab": outs[1],
                "_segs": torch.tensor(segs)}

    def reference(got):
        want = TC._want_counts(maps)
        assert torch.equal(got["counts"].cpu().long(), want)
        ids, ranked, nums = got["ids"].cpu(), got["ranked"].cpu(), got["nums"].cpu()
        for q, (off, ln) in enumerate(got["_segs"].tolist()):
            c = want[off:off + ln]
            order = sorted((i for i in range(ln) if c[i] > 0), key=lambda i: (-int(c[i]), i))
            assert int(nums[q]) == len(order) and ids[off:off + len(order)].tolist() == order
            assert ranked[off:off + len(order)].tolist() == [int(c[i]) for i in order]
            assert (ids[off + len(order):off + ln] == -1).all() and (ranked[off + len(order):off + ln] == 0).all()
        np.testing.assert_array_equal(got["mosaic_img"].cpu().numpy(), TC._ref_mosaic(img, plane, ks, ncol, -1, np.float32))
        np.testing.assert_array_equal(got["mosaic_lab"].cpu().numpy(), TC._ref_mosaic(lab, plane, ks, ncol, 0, np.int64))
    package_recycled(monkeypatch, lambda: step(maps, False), lambda: step([m.flip(2) for m in maps], True), reference)


def test_package_augmentation_chain(monkeypatch):
    """the dmri training chain of test_production_chains_match_reference at seed 1 (elastic deformation with blur; the order
    statistics and channel min / max of the intensity transforms take m355_aug_workspace, cleared by a memset at the head of
    each call) against the replay of its history in fp64: images within 1e-4 away from interpolation ties, labels equal"""
    import numpy as np

    import test_augmentation_gpu as TA
    imgs, labs, sp = TA._subject("dmri")
    chain = TA.dmri_chain()
    subject = {k: TA.dev(v) for k, v in {**imgs, **labs}.items()}
    history = {}

    def step(seed):
        out = chain(subject, label_maps=tuple(labs), spacing=sp, generator=torch.Generator().manual_seed(seed))
        history[seed] = chain.last_history
        return {k: out[k] for k in list(imgs) + list(labs)}

    def reference(got):
        near = {}
        ref = TA.replay(chain, history[1], {k: v.astype(np.float64) if k in imgs else v for k, v in {**imgs, **labs}.items()},
                        set(labs), sp, near)
        for k in imgs:
            ok = ~near[k]
            assert ok.mean() > 0.99
            assert np.abs(TA.host(got[k]) - ref[k])[:, ok].max(initial=0) <= 1e-4, k
        for k in labs:
            y = TA.host(got[k])
            assert y.dtype == labs[k].dtype and np.array_equal(y[:, ~near[k]], ref[k][:, ~near[k]]), k
    package_recycled(monkeypatch, lambda: step(1), lambda: step(8), reference)


def test_package_preprocessing_chain(monkeypatch):
    """the dmri inference chain of test_production_chains_in_reference_order (crop / pad around the mask: the bounding box
    and the minimum tables are cleared by a memset at the head of the call; NaN replacement, remap, one-hot with its
    out-of-range flag) against the reference order on the host: labels equal, images within 1e-5"""
    import numpy as np

    import test_preprocessing_gpu as TP
    imgs, labs, sp, lv = TP.subject("dmri")
    chain = TP.chain_of("dmri", False)
    s = {k: TP.dev(v) for k, v in {**imgs, **labs}.items()}
    s2 = {k: TP.dev(np.ascontiguousarray(np.flip(v, 1))) for k, v in {**imgs, **labs}.items()}

    def step(s):
        out = TP._run(chain, s, tuple(labs), spacing=sp, label_values=lv, generator=torch.Generator().manual_seed(0))
        return {k: v for k, v in out.items() if torch.is_tensor(v)}

    def reference(got):
        ref, near = TP.reference("dmri", None, imgs, labs, sp, None)
        assert set(got) == set(ref), (set(got), set(ref))
        for k, v in ref.items():
            y = TP.host(got[k])
            ok = ~near[k]
            assert y.shape == v.shape and ok.mean() > 0.9, k
            if k in labs or k == "y":
                assert np.array_equal(y[:, ok], v[:, ok]), k
            else:
                assert np.abs(y.astype(np.float64) - v)[:, ok].max(initial=0) <= 1e-5 * max(1.0, np.abs(v).max()), k
    package_recycled(monkeypatch, lambda: step(s), lambda: step(s2), reference)


def test_package_ensemble_accumulate_and_finalize(monkeypatch, golden):
    """models.EnsembleFlips through ops.py as test_ensemble_flips_golden: flip / permute, the accumulator (overwritten by
    the first member) and the finalize pass, mean within 1e-4 of the golden and majority votes equal to it"""
    from functools import partial

    from segmentation_pipeline_amd.models import EnsembleFlips, ModularUNet
    g = golden("components.npz")
    model = ModularUNet(4, 3, [8, 16], 2, block_params={'normalization_class': partial(nn.GroupNorm, 8)},
                        upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2})
    model.load_state_dict(g.state_dict("flips.sd."))
    model = model.cuda().eval()
    x = g.t("flips.x").cuda()

    def step(x):
        with torch.no_grad():
            return {"mean": EnsembleFlips(model, "mean")(x), "majority": EnsembleFlips(model, "majority", spatial_dims=(3, 4))(x)}

    def reference(got):
        assert (got["mean"].cpu().double() - g.t("flips.mean").double()).abs().max().item() <= 1e-4
        assert torch.equal(got["majority"].cpu(), g.t("flips.majority34"))
    package_recycled(monkeypatch, lambda: step(x), lambda: step(x.flip(2) * 0.5), reference)


def test_package_grid_aggregation_and_confusion(monkeypatch, oracle):
    """ops.patch_aggregate_grid on the padded grid of test_hann_aggregate_gpu.py, plain (== the oracle, bit for bit, as
    test_patch_aggregate_grid_one_pass) and Hann-weighted (== aggregate_ref.aggregate_windowed, bit for bit); ops.eval_confusion
    on several int32 maps in one launch (its count table is zeroed by the call) == the numpy restatement"""
    import numpy as np

    import aggregate_ref as AR
    import test_evaluation_gpu as TE
    from segmentation_pipeline_amd import ops
    from segmentation_pipeline_amd.prediction import grid_axes, hann_window_axes
    vshape, ps, ov, border = (12, 12, 12), (8, 8, 8), (4, 4, 4), (2, 2, 2)
    axes = grid_axes(tuple(v + 2 * b for v, b in zip(vshape, border)), ps, ov)
    ntiles = len(axes[0]) * len(axes[1]) * len(axes[2])
    tiles, tiles2 = rnd(ntiles, 3, *ps, seed=4), rnd(ntiles, 3, *ps, seed=104)
    window = hann_window_axes(ps)
    g = torch.Generator().manual_seed(9 * 31)
    labels = list(range(-3, 5)) + [300]
    values = sorted(set(labels[:6] + [0, 1, 44, -1]))
    shapes = [(1, 1, 7), (2, 2, 4), (1, 16, 256), (3, 5, 277), (2, 33, 65), (1, 1, 1)]
    preds = [TE._rand_map(g, s, torch.int32, values) for s in shapes]
    targets = [TE._rand_map(g, s, torch.int32, values) for s in shapes]
    targets[1] = None

    def step(tiles, preds):
        return {"plain": ops.patch_aggregate_grid(tiles.cuda(), axes, vshape, border),
                "hann": ops.patch_aggregate_grid(tiles.cuda(), axes, vshape, border, window=window),
                "confusion": ops.eval_confusion([p.cuda() for p in preds], [None if t is None else t.cuda() for t in targets], labels)}

    def reference(got):
        assert torch.equal(got["plain"].cpu(), oracle.patch_aggregate_grid(tiles, axes, vshape, border))
        assert torch.equal(got["hann"].cpu(), AR.aggregate_windowed(tiles, axes, vshape, border))
        counts = got["confusion"].cpu().numpy()
        for i, (p, t) in enumerate(zip(preds, targets)):
            np.testing.assert_array_equal(counts[i], TE.np_counts(p, t, labels), err_msg=f"subject {i}")
    package_recycled(monkeypatch, lambda: step(tiles, preds), lambda: step(tiles2, [p.flip(-1) for p in preds]), reference)


@pytest.mark.parametrize("name", ["sgd-nesterov-wd-all", "adamw-wd-all"])
def test_package_fused_optimizer_steps(monkeypatch, name):
    """optim.FusedSGD / FusedAdam through the trajectory of test_optimizer_gpu.run_case (clipping: the fp64 norm partials
    in the optimizer's workspace; weight decay, EMA, schedule): run_case itself holds every parameter, state and EMA tensor
    to the fp64 reference at its own bound, here on dirty memory; the state record is zero-filled by the optimizer and
    stays so"""
    import test_optimizer_gpu as T

    def step(case_name):
        opt, ps = T.run_case(T.FULL[case_name])
        return {f"tensor{i}": t for i, t in enumerate(T.everything(opt, ps))}
    package_recycled(monkeypatch, lambda: step(name), lambda: step("adam-wd-all"), lambda got: None)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_package_nested_res_unet_16bit_flows(monkeypatch, golden, mode):
    """one c8-flow training step of NestedResUNet(3, 2, 8) on its golden, at the bounds of
    test_c8_training_flow_architectures_with_fallback_ops: probabilities within the mode's tolerance of the reference's, every
    parameter gradient finite and in the reference's direction (or no further from it than 2.5x the twin flow + 0.03), all
    parameters together as close to the reference as the twin flow"""
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd import ops
    from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss
    from test_model_gpu import BUILDERS
    name = "nested_res_unet.npz"
    g = golden(name)
    x, y = g.t("x"), g.t("y")

    def step(x, y):
        model = BUILDERS[name][0]()
        model.load_state_dict(g.state_dict("m.sd."))
        model = model.cuda().train()
        with sp.precision(mode):
            if mode == "fp16":
                ops.fp16_overflow()
            p = model(x.cuda())
            ld = HybridLogisticDiceLoss(logistic_class_weights=BUILDERS[name][1])(p, y.cuda())
            ld["loss"].backward()
        return {"p": p.detach(), "loss": ld["loss"].detach(),
                **{"grad " + k: v.grad for k, v in model.named_parameters() if v.grad is not None}}

    try:
        ops.H16_TRAIN_C8ONLY = False
        twin = {k[5:]: v.cpu().double().flatten() for k, v in step(x, y).items() if k.startswith("grad ")}
    finally:
        ops.H16_TRAIN_C8ONLY = True

    def reference(got):
        assert (got["p"].cpu() - g.t("m.probs_train")).abs().max().item() <= (2e-2 if mode == "bf16" else 5e-3)
        grads = {k[5:]: v.cpu().double().flatten() for k, v in got.items() if k.startswith("grad ")}
        assert set(grads) == set(twin)

        def all_cosine(gr, check):
            dot = na = nb = 0.0
            for k, a in gr.items():
                ref = g.t(f"m.grad.{k}").double().flatten()
                assert torch.isfinite(a).all(), k
                if ref.norm() < 1e-9 * max(r.norm() for r in gr.values()):
                    continue
                cos = float(a @ ref / (a.norm() * ref.norm() + 1e-300))
                if check and cos < (0.9 if mode == "bf16" else 0.97):
                    rel, rel_tw = float((a - ref).norm() / ref.norm()), float((twin[k] - ref).norm() / ref.norm())
                    assert rel <= 2.5 * rel_tw + 0.03, (k, cos, rel, rel_tw)
                dot, na, nb = dot + float(a @ ref), na + float(a @ a), nb + float(ref @ ref)
            return dot / (na * nb) ** 0.5
        c8, tw = all_cosine(grads, True), all_cosine(twin, False)
        assert c8 >= min(0.995 if mode == "bf16" else 0.9995, tw - (0.01 if mode == "bf16" else 0.001)), (c8, tw)
    package_recycled(monkeypatch, lambda: step(x, y), lambda: step(x.flip(2), y.flip(2)), reference)


# ==================================================================================== the remaining raw wrappers with outputs
def test_raw_wrappers_without_workspace(hip, oracle, tuning):
    """the wrappers whose outputs (main and auxiliary) alone go through the harness: weight transforms with their mean / std,
    softmax, flip / permute, ensembles with the accumulator, patch gather / one-pass aggregation / cropped finalize,
    arg-max with the confusion counts; at the tolerances of their tests in test_kernels_gpu.py"""
    import itertools

    from segmentation_pipeline_amd.prediction import grid_axes
    members = [(perm, fm) for perm in itertools.permutations((0, 1, 2)) for fm in (0, 5)]
    vshape, ps, ov, border = (12, 12, 12), (8, 8, 8), (4, 4, 4), (2, 2, 2)
    axes = grid_axes(tuple(v + 2 * b for v, b in zip(vshape, border)), ps, ov)
    ntiles = len(list(itertools.product(*axes)))

    def run(be, seed):
        o = 100 * (seed - 1)
        out = {}
        w = rnd(5, 6, 3, 3, 3, seed=o + 1) * 0.3 + 0.05
        scale = torch.full((6,), 0.37) + rnd(6, seed=o + 3) * 0.01
        out["wexp"], out["ms"] = be.blur_weight_fwd(w, scale, True, False)
        # (the backward passes take the oracle's mean / std and softmax on both backends, as their tests do)
        out["blur_dw"] = be.blur_weight_bwd(rnd(*out["wexp"].shape, seed=o + 2), w, scale,
                                            oracle.blur_weight_fwd(w, scale, True, False)[1], True, False)
        w2 = rnd(40, 24, 3, 3, 3, seed=o + 4)
        out["wn"], out["ms2"] = be.weight_standardize_fwd(w2)
        out["ws_dw"] = be.weight_standardize_bwd(rnd(40, 24, 3, 3, 3, seed=o + 5), w2, oracle.weight_standardize_fwd(w2)[1])
        x = rnd(2, 7, 4, 5, 6, seed=o + 6) * 3
        out["softmax"] = be.softmax_fwd(x)
        out["softmax_dx"] = be.softmax_bwd(oracle.softmax_fwd(x), rnd(*x.shape, seed=o + 7))
        xe = rnd(2, 4, 6, 5, 8, seed=o + 8)
        preds = []
        for perm, fm in members:
            xm = be.flip_permute(xe, perm, fm)
            out[f"flip{perm}{fm}"] = xm
            preds.append(torch.softmax(xm.cpu() * (1.0 + 0.03 * len(preds)), dim=1))
        for strategy in ("mean", "majority"):
            out["ens_" + strategy], out["acc_" + strategy] = be.ensemble(preds, members, xe.shape[2:], strategy)
        out["grid"] = be.patch_aggregate_grid(rnd(ntiles, 3, *ps, seed=o + 9), axes, vshape, border)
        vol = rnd(3, 9, 6, 11, seed=o + 10)
        locs = torch.tensor([(0, 0, 0), (10, 6, 13), (4, 3, 7), (2, 0, 1)], dtype=torch.int32)
        out["gather_padded"] = be.patch_gather_padded(vol, locs, (5, 4, 6), (3, 2, 4), 2, -2.0)
        out["gather"] = be.patch_gather(vol, torch.tensor([(0, 0, 0), (4, 2, 5)], dtype=torch.int32), (5, 4, 6))
        cnt = torch.rand(15, 10, 19, generator=torch.Generator().manual_seed(o + 11)) + 1.0
        out["crop"] = be.patch_finalize_crop(rnd(3, 15, 10, 19, seed=o + 12), cnt, (3, 2, 4))
        prob = torch.softmax(rnd(2, 4, 9, 9, 9, seed=o + 13), dim=1)
        tgt = torch.randint(0, 4, (2, 9, 9, 9), generator=torch.Generator().manual_seed(o + 14))
        out["argmax"], out["confusion"] = be.argmax_confusion(prob, tgt)
        return out
    exact = (0.0, 0.0)
    tol = {"wexp": (1e-5, 1e-6), "ms": (1e-5, 1e-7), "blur_dw": (2e-5, 1e-6), "wn": (1e-5, 1e-5), "ms2": (1e-5, 1e-6),
           "ws_dw": (1e-4, 1e-5), "softmax": (2e-6, 1e-7), "softmax_dx": (1e-5, 1e-6), "ens_mean": exact, "acc_mean": exact,
           "ens_majority": exact, "acc_majority": exact, "grid": exact, "gather_padded": exact, "gather": exact,
           "crop": (1e-6, 1e-7), "argmax": exact, "confusion": exact, **{f"flip{p}{f}": exact for p, f in members}}
    recycled(hip, oracle, tuning, "misc", {}, run, tol, has_workspace=False)


# ========================================================================= the work-queue pool reads zero after every launch
QUEUE_CASES = [   # (entry, shape, compute, tuning): the queue-driven cases above
    ("fp32", (1, 320, 64, 4, 4, 4), 0, {}),                                               # one-shot, split-K
    ("fp32", (1, 32, 32, 8, 16, 64), 0, {"M355_CONV_SLOTS": 5}),                          # persistent
    ("fp32", (1, 32, 32, 8, 16, 64), X3, {"M355_CONV_SLOTS": 5, "M355_CONV_KSPLIT": 2}),  # persistent + slab reduction
    ("fp32", (2, 5, 7, 9, 10, 33), 1, {}),                                                # plain entry point, 16-bit
    ("h16", (1, 8, 8, 12, 9, 8), 1, {"M355_CONV_KSPLIT": 1, "M355_CONV_SLOTS": 5, "M355_H16_ONESHOT": 3}),
    ("h16", (1, 8, 8, 12, 9, 8), 2, {"M355_CONV_KSPLIT": 3, "M355_H16_ONESHOT": 3}),
]


def queue_case(hip, entry, case, compute):
    x, w, b, add, dy = conv_inputs(case, 1)
    if entry == "fp32":
        hip.conv3d_fwd(x, w, b, add, compute=compute)
        hip.conv3d_bwd_data(dy, w, x.shape, compute=compute)
    else:
        N, ci, co, D, H, W = case
        hip.conv3d_fwd_h16(hip.act16_pack(x, compute), ci, (D, H, W), w, b, compute=compute)
        hip.conv3d_bwd_data_h16(hip.act16_pack(dy, compute), co, w, x.shape, compute=compute)


def queue_pool_child():
    """the child process of test_work_queue_pool_reads_zero_after_every_launch: hands the library a pool from torch BEFORE any
    launch, then reads (never writes) the whole pool after each case"""
    from raw_ops import RawOps
    from segmentation_pipeline_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    _lib.ensure_queue_pool(dev)
    pool = _lib._queue_pools[dev.index]
    assert pool is not None, "the library already had a pool"
    assert pool.numel() == _lib.lib().m355_queue_pool_bytes() and int(pool.count_nonzero()) == 0
    hip = RawOps("hip")
    for entry, case, compute, env in QUEUE_CASES:
        os.environ.update({k: str(v) for k, v in env.items()})
        _lib.reload_tuning()
        queue_case(hip, entry, case, compute)
        torch.cuda.synchronize()
        bad = int(pool.count_nonzero())
        assert bad == 0, f"{entry} {case} compute {compute} {env}: {bad} non-zero bytes in the work-queue pool after the launch"
        for k in env:
            del os.environ[k]
    print(f"queue pool zero after {len(QUEUE_CASES)} cases")


def test_work_queue_pool_reads_zero_after_every_launch(hip, tuning):
    """include/m355seg.h: the pool's ticket and exit counters are "all zero between launches".  The pool can only be read when
    it is torch's, i.e. handed over before the first launch of a process: hence one child process.  The same cases are
    timed here in the parent (printed); the child gets ten times that and no less than CHILD_FLOOR_S, a generous allowance
    for a process start with the import of torch, the library load and the first launch's code-object load.  Measured on an
    MI355X: the cases 0.01 s in the parent, the whole child 2.2 s; limit max(10 * 0.01, 60) = 60 s."""
    CHILD_FLOOR_S = 60.0
    t0 = time.perf_counter()
    for entry, case, compute, env in QUEUE_CASES:
        tuning(**env)
        queue_case(hip, entry, case, compute)
        torch.cuda.synchronize()
        for k in env:
            os.environ.pop(k, None)
    measured = time.perf_counter() - t0
    limit = max(10.0 * measured, CHILD_FLOOR_S)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-c", "import test_recycled_memory_gpu as t; t.queue_pool_child()"],
                       cwd=os.path.dirname(os.path.abspath(__file__)), capture_output=True, text=True, timeout=limit)
    print(f"queue pool: the cases took {measured:.2f} s in the parent, the child {time.perf_counter() - t0:.2f} s of {limit:.0f} s")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "queue pool zero after" in r.stdout
