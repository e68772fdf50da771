"""Every kernel variant plan_resample (csrc/resample_host.hpp) can pick, run once at the smallest shape that picks it.  Each
case first asks m355_resample_plan that its slots select the variant it is meant to cover, then runs the entry point into a
canary slot (raw_ops.Slot: one guard channel on each side, everything around the slot must stay untouched and every element
of it must be written) and compares with the reference and tolerance of the op's test in test_kernels_gpu.py /
test_maxpool_gpu.py.  Misaligned cases are the ones the library serves on its scalar kernels; nothing here is rejected."""
import pytest
import torch
import torch.nn.functional as F

import maxpool_ref as M
from test_kernels_gpu import _c8_to_ncdhw, _dt, _rounded_close, _ulp, close, rnd

pytestmark = pytest.mark.gpu

(AVG_FWD, AVG_BWD, AVG_BWD_ADD, TRI_FWD, TRI_BWD, S2D, D2S, MAX_FWD, MAX_BWD, AVG_FWD_H16, AVG_BWD_H16, TRI_FWD_H16, TRI_BWD_H16,
 S2D_H16, D2S_H16, MAX_FWD_H16, MAX_BWD_H16) = range(17)
SCALAR, VECTOR, QUADS, LDS = 0, 1, 1, 2
N, C3, C9 = 2, 3, 9

# fp32 pools and space / depth: (D, H, W), elements the slots sit behind their aligned position, the pools' variant
POOL_CASES = [((2, 4, 4), 0, VECTOR), ((2, 2, 6), 0, SCALAR), ((2, 4, 4), 1, SCALAR)]
POOL_IDS = ["vector", "scalar-W6", "scalar-4B-base"]


def slots(hip, lead, ins, outs):
    """input slots holding `ins`, canary output slots of the shapes `outs`: a guard channel on each side"""
    return ([hip.slot(t, c_pre=1, c_post=1, lead=lead) for t in ins],
            [hip.slot(s, c_pre=1, c_post=1, lead=lead) for s in outs])


def done(ins, outs, what):
    torch.cuda.synchronize()
    for s in ins:
        s.assert_unchanged(what)
    return [s.check_output(what).cpu() for s in outs]


def pooled(shape):
    return shape[:2] + tuple(v // 2 for v in shape[2:])


@pytest.mark.parametrize("case", POOL_CASES, ids=POOL_IDS)
def test_avgpool_fp32(hip, oracle, case):
    vol, lead, variant = case
    shape = (N, C3) + vol
    x, dy, add = rnd(*shape, seed=1), rnd(*pooled(shape), seed=2), rnd(*shape, seed=3)
    (xs, dys, adds), (ys, dxs, dxa) = slots(hip, lead, [x, dy, add], [pooled(shape), shape, shape])
    assert hip.resample_plan(AVG_FWD, shape, [xs, ys])[0] == variant
    assert hip.resample_plan(AVG_BWD, shape, [dys, dxs])[0] == SCALAR
    assert hip.resample_plan(AVG_BWD_ADD, shape, [dys, adds, dxa])[0] == SCALAR
    hip.avgpool_fwd(xs, out=ys)
    hip.avgpool_bwd(dys, shape, out=dxs)
    hip.avgpool_bwd_add(dys, adds, shape, out=dxa)
    y, dx, dx_add = done([xs, dys, adds], [ys, dxs, dxa], "avgpool")
    close(y, oracle.avgpool_fwd(x), 1e-6, 1e-6, "pool fwd")
    close(dx, oracle.avgpool_bwd(dy, shape), 0, 0, "pool bwd")
    close(dx_add, oracle.avgpool_bwd_add(dy, add, shape), 0, 1e-7, "pool bwd + add")


@pytest.mark.parametrize("case", POOL_CASES, ids=POOL_IDS)
def test_maxpool_fp32(hip, case):
    vol, lead, variant = case
    shape = (N, C3) + vol
    x, _ = M.tie_heavy_input(shape, seed=11)
    y_ref, ind = F.max_pool3d(x, 2, 2, return_indices=True)
    g = torch.Generator().manual_seed(51)
    dy, add = torch.randn(y_ref.shape, generator=g), torch.randn(shape, generator=g)
    xr = x.clone().requires_grad_(True)
    routed = torch.autograd.grad(F.max_pool3d(xr, 2, 2), xr, dy)[0]
    (xs, dys, adds), (ys, dxs, dxa) = slots(hip, lead, [x, dy, add], [pooled(shape), shape, shape])
    route = torch.empty(pooled(shape), dtype=torch.uint8, device="cuda")
    assert hip.resample_plan(MAX_FWD, shape, [xs, ys], routes=route)[0] == variant
    assert hip.resample_plan(MAX_BWD, shape, [dys, None, dxs], routes=route)[0] == variant
    assert hip.resample_plan(MAX_BWD, shape, [dys, adds, dxa], routes=route)[0] == variant
    _, idx = hip.maxpool_fwd(xs, out=ys)
    hip.maxpool_bwd(dys, idx, None, shape, out=dxs)
    hip.maxpool_bwd(dys, idx, adds, shape, out=dxa)
    y, dx, dx_add = done([xs, dys, adds], [ys, dxs, dxa], "maxpool")
    assert torch.equal(y.isnan(), y_ref.isnan()) and torch.equal(y.contiguous().view(torch.int32), y_ref.view(torch.int32))
    assert torch.equal(idx.cpu(), M.window_position(ind, vol[1], vol[2]))
    assert torch.equal(dx, routed)
    assert torch.equal(dx_add, routed + add)


@pytest.mark.parametrize("vol", [(2, 4, 4), (2, 2, 6)], ids=["W4", "W6"])
def test_space_to_depth_fp32(hip, oracle, vol):
    """(one kernel each way; a 4-byte-aligned full tensor is refused, not served: no such case)"""
    shape = (N, C3) + vol
    packed = (N, 8 * C3) + tuple(v // 2 for v in vol)
    x = rnd(*shape, seed=1)
    ref = oracle.space_to_depth(x)
    (xs, ps), (ys, back) = slots(hip, 0, [x, ref], [packed, shape])
    assert hip.resample_plan(S2D, shape, [xs, ys])[0] == SCALAR
    assert hip.resample_plan(D2S, shape, [ps, back])[0] == SCALAR
    hip.space_to_depth(xs, out=ys)
    hip.depth_to_space(ps, out=back)
    y, b = done([xs, ps], [ys, back], "space / depth")
    assert torch.equal(y, ref), "s2d is a permutation: bit-exact"
    assert torch.equal(b, x)


# the first even W whose [4][10][W] float patch is past 48 KiB, with D = H = 2: the quad kernel where the tiled one would apply
@pytest.mark.parametrize("vol,variant", [((2, 2, 2), LDS), ((1, 2, 2), QUADS), ((2, 2, 3), SCALAR), ((2, 2, 308), QUADS)],
                         ids=["lds", "quads-D1", "scalar-W3", "quads-W308"])
def test_trilinear_fp32(hip, oracle, vol, variant):
    shape = (N, C3) + vol
    up = (N, C3) + tuple(2 * v for v in vol)
    x, dy = rnd(*shape, seed=3), rnd(*up, seed=4)
    (xs, dys), (ys, dxs) = slots(hip, 0, [x, dy], [up, shape])
    plan = hip.resample_plan(TRI_FWD, shape, [xs, ys])
    assert plan[0] == variant and (plan[4] > 0) == (variant == LDS)
    assert hip.resample_plan(TRI_BWD, shape, [dys, dxs])[0] == SCALAR
    hip.upsample_fwd(xs, out=ys)
    hip.upsample_bwd(dys, shape, out=dxs)
    y, dx = done([xs, dys], [ys, dxs], "trilinear")
    close(y, oracle.upsample_fwd(x), 2e-6, 2e-6, "up fwd")
    close(dx, oracle.upsample_bwd(dy, shape), 1e-5, 1e-5, "up bwd")


def c8_slots(hip, ins, outs, dt):
    return ([hip.slot(t, c_pre=1, c_post=1) for t in ins], [hip.slot(s, dtype=dt, c_pre=1, c_post=1) for s in outs])


C8_VOLUMES = [(2, 2, 2), (2, 4, 2)]
CB9 = (C9 + 7) // 8   # two channel blocks, the second with one channel


@pytest.mark.parametrize("vol", C8_VOLUMES, ids=["2x2x2", "2x4x2"])
@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_avgpool_c8(hip, compute, vol):
    dt = _dt(compute)
    D, H, W = vol
    S, shape = D * H * W, (N, C9) + vol
    x, dp, sk = rnd(*shape, seed=1), rnd(*pooled(shape), seed=2), rnd(*shape, seed=3)
    x16, dp16, sk16 = (hip.act16_pack(t, compute) for t in (x, dp, sk))
    (xs, dps, sks), (ps, dxs, dxk) = c8_slots(hip, [x16, dp16, sk16], [(N, CB9, S // 8, 8), (N, CB9, S, 8), (N, CB9, S, 8)], dt)
    assert hip.resample_plan(AVG_FWD_H16, shape, [xs, ps], compute=compute)[0] == SCALAR
    assert hip.resample_plan(AVG_BWD_H16, shape, [dps, None, dxs], compute=compute)[0] == SCALAR
    assert hip.resample_plan(AVG_BWD_H16, shape, [dps, sks, dxk], compute=compute)[0] == SCALAR
    hip.avgpool_fwd_h16(xs, C9, vol, compute, out=ps)
    hip.avgpool_bwd_h16(dps, None, C9, vol, compute, out=dxs)
    hip.avgpool_bwd_h16(dps, sks, C9, vol, compute, out=dxk)
    p16, dx16, dxk16 = done([xs, dps, sks], [ps, dxs, dxk], "avgpool c8")
    pref = F.avg_pool3d(x.to(dt).float(), 2, 2).to(dt).float()
    assert ((_c8_to_ncdhw(p16, C9, pooled(shape)[2:]) - pref).abs() <= _ulp(compute) * pref.abs() * 1.01 + 1e-6).all()
    up = 0.125 * dp.to(dt).float().repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)
    assert torch.equal(_c8_to_ncdhw(dx16, C9, vol), up.to(dt).float())
    _rounded_close(_c8_to_ncdhw(dxk16, C9, vol), up + sk.to(dt).float(), compute, 1e-7, "pool bwd + skip")


@pytest.mark.parametrize("vol", C8_VOLUMES, ids=["2x2x2", "2x4x2"])
@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_maxpool_c8(hip, compute, vol):
    dt = _dt(compute)
    D, H, W = vol
    S, shape = D * H * W, (N, C9) + vol
    x, _ = M.tie_heavy_input(shape, seed=16)
    x = x.to(dt).float()                       # (small integers, NaN, -inf and signed zeros are exact)
    y_ref = F.max_pool3d(x, 2, 2)
    g = torch.Generator().manual_seed(79)
    dp, sk = torch.randn(y_ref.shape, generator=g).to(dt).float(), torch.randn(shape, generator=g).to(dt).float()
    xr = x.clone().requires_grad_(True)
    routed = torch.autograd.grad(F.max_pool3d(xr, 2, 2), xr, dp)[0]
    x16, dp16, sk16 = (hip.act16_pack(t, compute) for t in (x, dp, sk))
    (xs, dps, sks), (ps, dxs, dxk) = c8_slots(hip, [x16, dp16, sk16], [(N, CB9, S // 8, 8), (N, CB9, S, 8), (N, CB9, S, 8)], dt)
    route = torch.empty((N, CB9, S // 8, 8), dtype=torch.uint8, device="cuda")
    assert hip.resample_plan(MAX_FWD_H16, shape, [xs, ps], routes=route, compute=compute)[0] == SCALAR
    assert hip.resample_plan(MAX_BWD_H16, shape, [dps, None, dxs], routes=route, compute=compute)[0] == SCALAR
    assert hip.resample_plan(MAX_BWD_H16, shape, [dps, sks, dxk], routes=route, compute=compute)[0] == SCALAR
    _, idx8 = hip.maxpool_fwd_h16(xs, C9, vol, compute, out=ps)
    hip.maxpool_bwd_h16(dps, idx8, None, C9, vol, compute, out=dxs)
    hip.maxpool_bwd_h16(dps, idx8, sks, C9, vol, compute, out=dxk)
    p16, dx16, dxk16 = done([xs, dps, sks], [ps, dxs, dxk], "maxpool c8")
    y = _c8_to_ncdhw(p16, C9, pooled(shape)[2:])
    assert torch.equal(y.isnan(), y_ref.isnan()) and torch.equal(y.contiguous().view(torch.int32), y_ref.view(torch.int32))
    assert torch.equal(_c8_to_ncdhw(dx16, C9, vol), routed)
    assert torch.equal(_c8_to_ncdhw(dxk16, C9, vol), (sk + routed).to(dt).float())       # rounded once
    for t in (p16, dx16, dxk16):
        assert not t.view(torch.int16)[:, -1, :, C9 % 8:].any(), "lanes past C must be zero"


@pytest.mark.parametrize("vol", C8_VOLUMES, ids=["2x2x2", "2x4x2"])
@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_trilinear_and_space_to_depth_c8(hip, oracle, compute, vol):
    dt = _dt(compute)
    D, H, W = vol
    S, shape = D * H * W, (N, C9) + vol
    x, du = rnd(*shape, seed=1), rnd(N, C9, 2 * D, 2 * H, 2 * W, seed=4)
    xr = x.to(dt).float()
    x16, du16 = hip.act16_pack(x, compute), hip.act16_pack(du, compute)
    (xs, dus), (us, dlo, ss) = c8_slots(hip, [x16, du16], [(N, CB9, 8 * S, 8), (N, CB9, S, 8), (N, C9, S // 8, 8)], dt)
    assert hip.resample_plan(TRI_FWD_H16, shape, [xs, us], compute=compute)[0] == SCALAR
    assert hip.resample_plan(TRI_BWD_H16, shape, [dus, dlo], compute=compute)[0] == SCALAR
    assert hip.resample_plan(S2D_H16, shape, [xs, ss], compute=compute)[0] == SCALAR
    hip.upsample_trilinear2x_fwd_h16(xs, C9, vol, compute, out=us)
    hip.upsample_trilinear2x_bwd_h16(dus, C9, vol, compute, out=dlo)
    hip.s2d_h16(xs, shape, compute, True, out=ss)
    u16, dlo16, s16 = done([xs, dus], [us, dlo, ss], "trilinear / s2d c8")
    xg = xr.clone().requires_grad_()
    uref = torch.nn.Upsample(scale_factor=2, mode='trilinear', align_corners=True)(xg)
    _rounded_close(_c8_to_ncdhw(u16, C9, (2 * D, 2 * H, 2 * W)), uref.detach(), compute, 2e-6, "trilinear fwd c8")
    uref.backward(du.to(dt).float())
    _rounded_close(_c8_to_ncdhw(dlo16, C9, vol), xg.grad, compute, 1e-5, "trilinear bwd c8")
    assert torch.equal(_c8_to_ncdhw(s16, 8 * C9, pooled(shape)[2:]), oracle.space_to_depth(xr))
    # the inverse, from a slot holding the packed result
    (s16s,), (back,) = c8_slots(hip, [s16.cuda()], [(N, CB9, S, 8)], dt)
    assert hip.resample_plan(D2S_H16, shape, [s16s, back], compute=compute)[0] == SCALAR
    hip.s2d_h16(s16s, shape, compute, False, out=back)
    (b16,) = done([s16s], [back], "d2s c8")
    assert torch.equal(b16, x16.cpu()), "depth-to-space is not the inverse (incl. the zero padding of the last block)"
