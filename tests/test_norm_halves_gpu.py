"""The two halves of the normalisation passes that synchronised BatchNorm wraps around its all-reduces, run with the local
count and no all-reduce, equal the fused calls bit for bit: m355_norm_sums + _stats_from_sums == m355_norm_stats,
m355_norm_act_bwd_reduce + _apply == m355_norm_act_bwd (and _bwd_h16 with the c8 twin of dx), m355_norm_act_bwd_c8_reduce +
_c8_apply == m355_norm_act_bwd_c8.  BatchNorm only (the halves exist for it).  Both sides run the same kernels on the same
plan (csrc/norm_host.hpp) and every sum has a fixed order, so equality is exact.

Shapes: the smallest with two chunks in each layout of the backward partials, plus one with a single chunk --
fp32 chunks are 16384 elements of N * S (statistics) and of S (backward); c8 chunks 4096 voxels."""
import pytest
import torch

from test_kernels_gpu import rnd

pytestmark = pytest.mark.gpu

# id -> (N, C, (D, H, W), batch stride of x / dx beyond dense)
FP32 = {"vec-2chunks": (2, 8, (4, 50, 41), 0),      # N * S = 16400 > 16384, S % 4 == 0: float4 kernels
        "scalar-2chunks": (2, 8, (4, 50, 42), 1),   # N * S = 16800, batch stride dense + 1: scalar kernels
        "one-chunk": (2, 8, (8, 8, 8), 0)}
C8 = {"2chunks": (1, 8, (4, 26, 40)),               # S = 4160 > 4096, all even (pooled gradient)
      "one-chunk": (2, 8, (8, 8, 8))}


def _params(Cc):
    return rnd(Cc, seed=2) * 0.5 + 1.0, rnd(Cc, seed=3) * 0.1


@pytest.mark.parametrize("case", FP32, ids=list(FP32))
def test_fp32_halves_equal_the_fused_calls(hip, case):
    N, Cc, sp, extra = FP32[case]
    x, dy = rnd(N, Cc, *sp, seed=1), rnd(N, Cc, *sp, seed=6)
    gamma, beta = _params(Cc)
    lay = dict(c_pre=0, c_post=0, extra=extra)
    xs = hip.slot(x, **lay) if extra else hip.to(x)
    out = (lambda: hip.slot(x.shape, **lay)) if extra else (lambda: None)
    val = (lambda t: t.result()) if extra else (lambda t: t)
    running = (rnd(Cc, seed=4), rnd(Cc, seed=5).abs() + 0.5)

    mean, rstd, rm, rv = hip.norm_stats(xs, 0, running=running)
    sums = hip.norm_sums(xs)
    assert sums[2 * Cc].item() == N * sp[0] * sp[1] * sp[2]
    for a, b in zip((mean, rstd, rm, rv), hip.norm_stats_from_sums(sums, x.shape, running=running)):
        assert torch.equal(a, b)

    dx, dg, db = hip.norm_act_bwd(xs, dy, mean, rstd, gamma, beta, 0, 1, out=out())
    for count in (None, sums[2 * Cc:]):   # this rank's own count: implied, or read from the device as the ranks' total is
        stat_m, dg2, db2 = hip.norm_act_bwd_reduce(xs, dy, mean, rstd, gamma, beta, 0, 1, total_count=count)
        dx2, _ = hip.norm_act_bwd_apply(xs, dy, mean, rstd, gamma, beta, stat_m, 0, 1, out=out())
        assert torch.equal(val(dx2), val(dx)) and torch.equal(dg2, dg) and torch.equal(db2, db)
    for compute in (1, 2):   # the c8 twin of dx rides on the second half
        dxh, dgh, dbh, dx16 = hip.norm_act_bwd_h16(xs, dy, mean, rstd, gamma, beta, 0, 1, compute, out=out())
        dx3, dx16_3 = hip.norm_act_bwd_apply(xs, dy, mean, rstd, gamma, beta, stat_m, 0, 1, compute=compute, out=out())
        assert torch.equal(dgh, dg) and torch.equal(dbh, db)   # (the first half is the same kernel with or without the twin)
        assert torch.equal(val(dx3), val(dxh)) and torch.equal(dx16_3, dx16)


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", C8, ids=list(C8))
def test_c8_halves_equal_the_fused_call(hip, case, compute):
    N, Cc, sp = C8[case]
    D, H, W = sp
    x16 = hip.act16_pack(rnd(N, Cc, *sp, seed=1), compute)
    dy16 = hip.act16_pack(rnd(N, Cc, *sp, seed=6), compute)
    dp16 = hip.act16_pack(rnd(N, Cc, D // 2, H // 2, W // 2, seed=7), compute)
    gamma, beta = _params(Cc)
    mean, rstd = hip.norm_stats(rnd(N, Cc, *sp, seed=1), 0)[:2]
    for dy_, dp_ in ((dy16, None), (dy16, dp16), (None, dp16)):
        dx, dg, db = hip.norm_act_bwd_c8(x16, dy_, dp_, Cc, sp, mean, rstd, gamma, beta, 0, 1, compute, unscale=0.5)
        stat_m, dg2, db2 = hip.norm_act_bwd_c8_reduce(x16, dy_, dp_, Cc, sp, mean, rstd, gamma, beta, 0, 1, compute, unscale=0.5)
        dx2 = hip.norm_act_bwd_c8_apply(x16, dy_, dp_, Cc, sp, mean, rstd, gamma, beta, stat_m, 0, 1, compute)
        assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db)
