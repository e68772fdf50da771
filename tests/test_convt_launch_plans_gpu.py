"""Every kernel instantiation and persistent loop of csrc/convt.hip, run once from the table in tests/convt_cases.py
(tests/test_convt_plan_cases_cpu.py proves on the host that the table reaches all of them).  Each case first asks
m355_conv_transpose3d_plan for the plan of the very call it is about to make -- same descriptor, same knobs, same y side --
so that it cannot pass on another kernel, then runs the kernel and compares with the CPU oracle on the same operands.

fp32 families (fp32 MFMA, X3, direct): per element, |err| <= 2e-5 * T + TINY for the forward and the data gradient and
3e-5 * T + TINY for dw and dbias, where T is the same oracle operation on the absolute values of the operands, i.e. the sum
of |terms| of that output element (the bound of test_kernels_gpu.py's docstring, taken per element and not on the tensor's
maximum: a wrong value in a small-magnitude corner of a tile fails).  Each fp32 case also checks, with no oracle and b = 0,
<convt_fwd(x, w), dy> == <x, bwd_data(dy, w)> == <w, dw> in fp64 on the host to 1e-5 * sum|terms|.

16-bit families, on operands rounded to the 16-bit type first, with the forms and constants of test_kernels_gpu.py:
the ulp-scaled check of test_conv_transpose3d_c8 (+ 2e-5; + 1e-4 on the 16-bit MFMA, whose weights are rounded too, as in
test_conv_transpose3d_c8_large_levels_on_16bit_mfma), _rounded_close for dx16 with atol 3e-5 * max|ref|, and for the weight
gradient close(dw, ref, 3e-5, 3e-5 * max|ref|), close(dbias, ref, 1e-5, 1e-4).

Persistent and split cases (fp32 weight gradient, split-K data gradient, 16-bit MFMA forward, c8 gradients) are called twice
and must be bit-identical: their reductions have a fixed order.  The multi-tile c8 weight gradients run again under
M355_CONVT_WGS=8, where the plan gives every workgroup one tile, and must agree within the same tolerance.  (The knob cannot
flatten the other two walks at these sizes: the c8 data gradient keeps at least four voxel tiles per workgroup whatever the
knob says, and the 16-bit MFMA forward's grid does not read it.  Their tiles are disjoint pieces of the output, so the
comparison with the oracle at every voxel is what checks the walk.)

Worst measured err / bound per family on an MI355X (profiles/convt_plan_coverage.txt; set M355_CONVT_COVERAGE_OUT to a path
to write the table again):
  bwd_data_h16                    0.9696   c8dx-nks64-bf16
  bwd_data_mfma                   0.0165   dx-nvt256-mt4
  bwd_weight_mfma dbias           0.0000   dw-mt4-51-splits-60-tiles-n2
  bwd_weight_mfma dw              0.0007   dw-mt4-51-splits-60-tiles-n2
  bww_c8 dbias                    0.0062   c8dw-ct4-42-splits-90-tiles-bf16
  bww_c8 dw                       0.0017   c8dw-ct2-64-splits-120-tiles-f16
  bww_c8 dw, walk vs one tile     0.0017   c8dw-ct2-64-splits-120-tiles-bf16
  direct_bwd_data                 0.0113   direct-dx-k4s3p2o2
  direct_bwd_weight dbias         0.0005   direct-dw-k2s1p1o0
  direct_bwd_weight dw            0.0030   direct-dw-k4s1p2o0
  direct_fwd                      0.0112   direct-fwd-k5s2p0o0
  fwd_c8                          0.9827   c8fwd-nvt64-short-last-group-bf16
  fwd_h16                         0.9827   h16fwd-ks8-ng1-136-tiles-86-wgs-bf16
  fwd_mfma                        0.0133   fwd-nvt128-one-group-774-tiles
  fwd_x3                          0.0148   x3-nvt128
  identity                        0.0010   direct-fwd-k3s1p2o0
(a 16-bit row near 1 is one rounding to the 16-bit type: the bound is one ulp of the reference)
"""
import os

import pytest
import torch

import convt_cases as T
from test_kernels_gpu import _c8_to_ncdhw, _dt, _rounded_close, _ulp, rnd

pytestmark = pytest.mark.gpu

TINY = 1e-30
FP32_CASES = [c for c in T.CASES if c.which <= T.BWD_WEIGHT]
C8_CASES = [c for c in T.CASES if c.which >= T.FWD_C8]
WORST = {}     # family -> (err / bound, case id)


@pytest.fixture(scope="module", autouse=True)
def coverage_table():
    yield
    lines = [f"{fam:28s} {ratio:9.4f}   {cid}" for fam, (ratio, cid) in sorted(WORST.items())]
    print("\nworst err / bound per family\n" + "\n".join(lines))
    path = os.environ.get("M355_CONVT_COVERAGE_OUT")
    if path:
        with open(path, "w") as f:
            f.write("# tests/test_convt_launch_plans_gpu.py on an MI355X: worst err / bound per kernel family, and its case\n")
            f.write("\n".join(lines) + "\n")


def note(family, ratio, case):
    if ratio > WORST.get(family, (-1.0, None))[0]:
        WORST[family] = (ratio, case.id)


def bounded(got, ref, bound, family, case, what):
    """|got - ref| <= bound per element (fp64 on the host); the worst ratio goes into the table"""
    got, ref, bound = got.detach().cpu().double(), ref.detach().cpu().double(), bound.detach().cpu().double()
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    ratio = (got - ref).abs() / bound
    worst = float(ratio.max()) if not torch.isnan(ratio).any() else float("inf")
    print(f"{case.id}: {what} worst err / bound {worst:.4f}")
    note(family, worst, case)
    at = int(ratio.flatten().argmax())
    assert worst <= 1.0, (f"{case.id} {what}: {int((ratio > 1).sum())} of {ratio.numel()} elements over their bound, worst "
                          f"{worst:.3f}x at flat index {at}: got {got.flatten()[at]:.9g}, reference {ref.flatten()[at]:.9g}, "
                          f"bound {bound.flatten()[at]:.3e}")


def family_name(case):
    return min((n for n in T.instantiations(case) if ":" not in n and n != "dx_reduce"), key=len).split("<")[0]


def dot(a, b):
    return float((a.detach().cpu().double() * b.detach().cpu().double()).sum())


# ------------------------------------------------------------------------------------------------------------ fp32
class Fp32Call:
    """the three fp32 entry points on one case's descriptor and layout: y / dy in a slot of odd batch stride where the case
    asks for it (the oracle always gets the dense tensors)"""

    def __init__(self, hip, case):
        self.hip, self.case = hip, case
        N, Cin, Cout, D, H, W = case.shape
        self.k, self.s, self.p, self.op = case.geom
        self.x_shape = (N, Cin, D, H, W)
        self.geom = (self.s, self.p, self.op)

    def _y_side(self, data_or_shape):
        if not self.case.odd_ybs:
            return data_or_shape if isinstance(data_or_shape, torch.Tensor) else None
        slot = self.hip.slot(data_or_shape, c_pre=0, c_post=0, extra=1)
        assert slot.bs % 2 == 1 and slot.misalign(64) == 0
        return slot

    def assert_plan(self, which, y_side, expect):
        slot = y_side if self.case.odd_ybs else None
        plan = self.hip.convt_plan(self.x_shape, self.case.shape[2], self.k, self.s, self.p, self.op,
                                   compute=self.case.compute if which == T.FWD else 0, which=which,
                                   ybs=slot.bs if slot is not None else 0, y_side=slot)
        if expect is not None:
            assert plan == expect, (self.case.id, which, plan)
        return plan

    def fwd(self, x, w, b, expect=None):
        out = self._y_side(self.case.out_shape())
        self.assert_plan(T.FWD, out, expect)
        y = self.hip.convt_fwd(x, w, b, *self.geom, compute=self.case.compute, out=out)
        torch.cuda.synchronize()
        return out.check_output(self.case.id) if out is not None else y

    def bwd_data(self, dy, w, expect=None):
        dys = self._y_side(dy)
        self.assert_plan(T.BWD_DATA, dys, expect)
        dx = self.hip.convt_bwd_data(dys, w, self.x_shape, *self.geom)
        torch.cuda.synchronize()
        return dx

    def bwd_weight(self, x, dy, with_bias, expect=None):
        dys = self._y_side(dy)
        self.assert_plan(T.BWD_WEIGHT, dys, expect)
        dw, db = self.hip.convt_bwd_weight(x, dys, self.k, *self.geom, with_bias=with_bias)
        torch.cuda.synchronize()
        return dw, db


def fp32_operands(case):
    N, Cin, Cout, D, H, W = case.shape
    k = case.geom[0]
    return (rnd(N, Cin, D, H, W, seed=1), rnd(Cin, Cout, k, k, k, seed=2) * (1.0 / Cin ** 0.5), rnd(Cout, seed=3),
            rnd(*case.out_shape(), seed=5))


@pytest.mark.parametrize("case", FP32_CASES, ids=repr)
def test_fp32_case_on_its_plan(hip, oracle, case, tuning):
    tuning(**case.tuning)
    call, fam, geom = Fp32Call(hip, case), family_name(case), case.geom[1:]
    x, w, b, dy = fp32_operands(case)
    ax, aw, ab, ady = x.abs(), w.abs(), b.abs(), dy.abs()
    k = case.geom[0]
    twice = T.persistent_or_split(case)
    if case.which == T.FWD:
        y = call.fwd(x, w, b, expect=case.plan)
        t0 = oracle.convt_fwd(ax, aw, None, *geom)
        bounded(y, oracle.convt_fwd(x, w, b, *geom), 2e-5 * (t0 + ab.view(1, -1, 1, 1, 1)) + TINY, fam, case, "y")
        terms = dot(t0, ady)
    elif case.which == T.BWD_DATA:
        dx = call.bwd_data(dy, w, expect=case.plan)
        t = oracle.convt_bwd_data(ady, aw, call.x_shape, *geom)
        bounded(dx, oracle.convt_bwd_data(dy, w, call.x_shape, *geom), 2e-5 * t + TINY, fam, case, "dx")
        if twice:
            assert torch.equal(dx, call.bwd_data(dy, w, expect=case.plan)), "split-K data gradient: not bit-identical"
        terms = dot(ax, t)
    else:
        dw, db = call.bwd_weight(x, dy, case.dbias, expect=case.plan)
        ref_dw, ref_db = oracle.convt_bwd_weight(x, dy, k, *geom)
        t, tb = oracle.convt_bwd_weight(ax, ady, k, *geom)
        bounded(dw, ref_dw, 3e-5 * t + TINY, fam + " dw", case, "dw")
        assert (db is None) == (not case.dbias)
        if case.dbias:
            bounded(db, ref_db, 3e-5 * tb + TINY, fam + " dbias", case, "dbias")
        if twice:
            dw2, db2 = call.bwd_weight(x, dy, case.dbias, expect=case.plan)
            assert torch.equal(dw, dw2) and (db is None or torch.equal(db, db2)), "weight gradient: not bit-identical"
        terms = dot(aw, t)
    # the oracle-free identity: all three entry points on this case's descriptor, b = 0
    lhs = dot(call.fwd(x, w, None), dy)
    mid = dot(x, call.bwd_data(dy, w))
    rhs = dot(w, call.bwd_weight(x, dy, False)[0])
    worst = max(abs(lhs - mid), abs(mid - rhs), abs(lhs - rhs)) / (1e-5 * terms)
    print(f"{case.id}: <y, dy> {lhs:.9g}  <x, dx> {mid:.9g}  <w, dw> {rhs:.9g}  sum|terms| {terms:.6g}  err / bound {worst:.4f}")
    note("identity", worst, case)
    assert worst <= 1.0, (case.id, lhs, mid, rhs, terms)


# ------------------------------------------------------------------------------------------------------------ c8
def c8_plan(hip, case):
    N, Cin, Cout, D, H, W = case.shape
    return hip.convt_plan((N, Cin, D, H, W), Cout, which=case.which)


def ratio16(got, ref, compute, atol):
    return float(((got - ref).abs() / (_ulp(compute) * ref.abs() * 1.01 + atol)).max())


def close_ratio(got, ref, rtol, atol):
    """test_kernels_gpu.close() as a ratio: max err / (atol + rtol * max|ref|)"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape
    r = float((got - ref).abs().max() / (atol + rtol * ref.abs().max()))
    return float("inf") if r != r else r


@pytest.mark.parametrize("case", C8_CASES, ids=repr)
def test_c8_case_on_its_plan(hip, oracle, case, tuning):
    tuning(**case.tuning)
    N, Cin, Cout, D, H, W = case.shape
    x_shape, vol, compute, dt, fam = (N, Cin, D, H, W), (D, H, W), case.compute, _dt(case.compute), family_name(case)
    x, w, b = rnd(*x_shape, seed=1), rnd(Cin, Cout, 2, 2, 2, seed=2) * 0.2, rnd(Cout, seed=3)
    xr, wr = x.to(dt).float(), w.to(dt).float()
    if case.which != T.FWD_C8:
        dy = rnd(*case.out_shape(), seed=4)
        dyr = dy.to(dt).float()
    assert c8_plan(hip, case) == case.plan
    if case.which == T.FWD_C8:
        h16 = case.plan[0] == T.H16
        x16 = hip.act16_pack(x, compute)
        y16 = hip.conv_transpose3d_fwd_h16(x16, Cin, vol, w, b, compute)
        ref = oracle.convt_fwd(xr, wr if h16 else w, b, 2, 0, 0)
        got = _c8_to_ncdhw(y16, Cout, case.out_shape()[2:])
        atol = 1e-4 if h16 else 2e-5
        r = ratio16(got, ref, compute, atol)
        print(f"{case.id}: y16 worst err / bound {r:.4f}")
        note(fam, r, case)
        assert ((got - ref).abs() <= _ulp(compute) * ref.abs() * 1.01 + atol).all(), (case.id, r)
        if Cout % 8:
            assert (y16[:, -1, :, Cout % 8:].float() == 0).all(), "padding lanes of the last channel block"
        if h16:
            assert torch.equal(y16, hip.conv_transpose3d_fwd_h16(x16, Cin, vol, w, b, compute)), "not bit-identical"
    elif case.which == T.BWD_DATA_C8:
        dy16 = hip.act16_pack(dy, compute)
        ref = oracle.convt_bwd_data(dyr, wr, x_shape, 2, 0, 0)
        dx16 = hip.convt_bwd_data_h16(dy16, w, x_shape, compute)
        got, atol = _c8_to_ncdhw(dx16, Cin, vol), 3e-5 * ref.abs().max().item()
        r = ratio16(got, ref, compute, atol)
        print(f"{case.id}: dx16 worst err / bound {r:.4f}")
        note(fam, r, case)
        _rounded_close(got, ref, compute, atol, f"convT dx {case.id}")
        if Cin % 8:
            assert (dx16[:, -1, :, Cin % 8:].float() == 0).all(), "padding lanes of the last channel block"
        assert torch.equal(dx16, hip.convt_bwd_data_h16(dy16, w, x_shape, compute)), "not bit-identical"
    else:
        x16, dy16 = hip.act16_pack(x, compute), hip.act16_pack(dy, compute)
        ref_dw, ref_db = oracle.convt_bwd_weight(xr, dyr, 2, 2, 0, 0)
        ref_dw, ref_db = ref_dw * case.unscale, ref_db * case.unscale
        dw_atol = 3e-5 * ref_dw.abs().max().item()

        def check(dw, db, what):
            rw, rb = close_ratio(dw, ref_dw, 3e-5, dw_atol), close_ratio(db, ref_db, 1e-5, 1e-4 * case.unscale)
            print(f"{case.id} {what}: dw err / bound {rw:.4f}, dbias err / bound {rb:.4f}")
            note(fam + " dw", rw, case)
            note(fam + " dbias", rb, case)
            assert rw <= 1.0 and rb <= 1.0, (case.id, what, rw, rb)

        dw, db = hip.convt_bwd_weight_h16(x16, dy16, x_shape, Cout, compute, unscale=case.unscale)
        check(dw, db, "on its plan")
        dw2, db2 = hip.convt_bwd_weight_h16(x16, dy16, x_shape, Cout, compute, unscale=case.unscale)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "not bit-identical"
        # the same call with one tile per workgroup: a difference is the tile walk's
        tuning(M355_CONVT_WGS=8)
        flat = c8_plan(hip, case)
        assert flat[:2] == case.plan[:2] and flat[2] == T.counts(case)["tiles"] > case.plan[2], flat
        dw1, db1 = hip.convt_bwd_weight_h16(x16, dy16, x_shape, Cout, compute, unscale=case.unscale)
        check(dw1, db1, "one tile per workgroup")
        rw = close_ratio(dw, dw1, 3e-5, dw_atol)
        note(fam + " dw, walk vs one tile", rw, case)
        assert rw <= 1.0, (case.id, "tile walk against one tile per workgroup", rw)
