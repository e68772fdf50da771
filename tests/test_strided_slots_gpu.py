"""HIP kernels on strided, misaligned concat slots with guard canaries (raw_ops.Slot).

The first convention of the C ABI: a tensor may be a channel slice of a larger concat buffer -- spatial dims dense, batch
stride explicit.  Every entry point that takes a batch stride runs here on slots and must
  1. leave the guards around every slot intact, write every output element, leave its inputs alone;
  2. agree with the oracle's DENSE call on the same values at the tolerance of that entry point's dense test in
     test_kernels_gpu.py (the numbers are copied from there, none is new);
  3. in the layout class "aligned", give the very bits of the HIP library's own dense call (same kernel, same summation
     order, only the addresses differ), with the same m355_conv3d_plan where there is one.

Layout classes (N = 2; "n1" is N = 1 on an offset pointer, where only the pointer matters):
  aligned  pointer 16-byte aligned, every stride a multiple of 4 elements, all strides different and none dense
  odd      an odd number of foreign channels in front and a stride that is no multiple of 4 (odd S, or `extra` elements):
           sample 0 is 16-byte aligned, sample 1 is not
  offset1 / offset2   the pointer 1 / 2 elements behind a 16-byte boundary (4- / 8-byte aligned only), strides as "aligned"
The fp32 ABI states no alignment requirement, so all of them are legal -- except where a host function rejects a layout
with a status code (norm_act_pool_fwd and space-to-depth want 8 bytes; c8 tensors 16 bytes and strides % 8): there the
status is asserted and the output must still hold the canary.  ops.py does not pass those layouts: an `OutSlot` into an
allocator-aligned buffer has the pointer buf + c0 * S elements and the stride Ctot * S, with S a multiple of 8 for both
ops (all spatial sizes even), and a caller's view that is dense but sits at an odd element offset is compacted first
(ops._pairs_in / _pairs_out: test_ops_compacts_views_the_pair_kernels_reject); c8 slots (`Act16.slot`) sit at whole
channel blocks of 16-byte items in a 256-byte aligned allocation.

Host / kernel branches on a stride or a pointer (file:line, condition, who takes the fast | the slow side):
  conv3d.hip:792    per sample: row vector stores need yn, an 16-B aligned, W % 4 == 0   test_conv3d_small_cout[aligned W=40 | odd, offset*, W=33]
  conv3d.hip:1710   dbias VEC: S % 4, ybs % 4, dy 16-B aligned                           test_conv3d_bwd_weight[aligned S%4==0 cases | odd, offset*]
  conv3d.hip:2072   (the host side of the same choice, launch_dbias)                    as above
  conv3d_route.hpp:955   split weight gradient requires 4-byte aligned x / dy (check_bww)   every fp32 tensor is (no other side to take)
  conv3d_route.hpp:911   bww float4 rows (route_bww): W % 4, xbs % 4, x 16-B aligned (gen2 | gen1)   test_conv3d_bwd_weight[aligned W=36 family 9 | odd, offset* family 9]
  conv3d_route.hpp:912   gen2 needs dy 4-byte aligned                                   always true for fp32 tensors
  conv3d_host.hip:159/167, conv3d_route.hpp:967 (check_bww) / 741 / 747 (check_conv)   c8 REQUIREs (16 B, % 8): act16_pack / _unpack, conv3d_bwd_weight_h16 / _c8,
                    the conv3d h16 forward / data gradient                               test_c8_conv3d, test_act16_pack_unpack | test_c8_rejects_misaligned_slots (each by name)
  convt.hip convt_y_side_ok -> route_convt   k2 s2 forward: ConvtKind MfmaF32 / X3 needs ybs % 2 == 0, y 8-B aligned, else Direct
                                                                                        test_conv_transpose3d[aligned, offset2 | odd (ybs odd), offset1, n1]
                    ... data gradient (MfmaF32 | Direct), same condition on dy          test_conv_transpose3d (same ids)
                    ... weight gradient (MfmaF32 | Direct), same condition on dy        test_conv_transpose3d (same ids)
  convt.hip validate_convt_c8   c8 REQUIREs: conv-transpose fwd / bwd_data / bwd_weight h16  test_c8_conv_transpose | test_c8_rejects_misaligned_slots (each by name)
  norm_host.hpp norm_pass   the vector verdict of each pass (one function; keyed by pass, not by line):
    plan: vector verdict of the forward       S % 4, xbs / ybs / abs % 4, x / y / add 16-B aligned   test_norm[aligned S%4==0 | odd, offset*, S odd]
    plan: vector verdict of the statistics    len % 4, S % 4, xbs % 4, x aligned                    test_norm (same ids); m355_norm_sums (synchronised BN) launches the same
                    kernel from the same verdict: test_norm_halves_gpu.py runs it dense and on a batch stride of dense + 1
    plan: vector verdict of backward pass 1   S % 4, xbs / ybs % 4, x / dy aligned                  test_norm (same ids)
    plan: vector verdict of backward pass 2   S % 4, xbs / ybs % 4, x / dy / dx aligned             test_norm (same ids)
  norm.hip m355_norm_act_pool_fwd   REQUIREs x / y 8-B aligned, even strides                test_norm_act_pool[aligned, offset2] | [odd, offset1: status asserted]
  norm.hip m355_norm_act_bwd_h16    c8 twin of dx 16-B aligned, stride % 8 (dx16_ok)        test_c8_norm (strided twin) | test_c8_rejects_misaligned_slots
  norm.hip m355_norm_act_bwd_apply  the same REQUIRE (dx16_ok) in the second half alone     test_norm_halves_gpu.py (accepting side: the twin through the half ==
                    the twin of the fused call); the rejecting side is the one function test_c8_rejects_misaligned_slots reaches through _bwd_h16
  elementwise.hip:625  s2d REQUIREs the full-resolution tensor 8-B aligned, even stride  test_space_to_depth[aligned, offset2] | [odd, offset1: status asserted]
  elementwise.hip:660  avgpool vec: W % 4, xbs % 4, ybs % 2, x 16-B, y 8-B               test_pool[aligned W=8 | odd, offset*, W=6]
  elementwise.hip:712  trilinear quads: W even, ybs % 4, y 16-B                          test_upsample[aligned even W | odd, offset*, odd W]
  elementwise.hip:746  c8 REQUIRE shared by trilinear fwd / bwd, s2d / d2s, channel_scale  test_c8_pool_upsample_s2d_scale | test_c8_rejects_misaligned_slots (all five)
  elementwise.hip:865  copy_channels vec: C*S % 4, strides % 4, both 16-B               test_copy_channels[aligned | odd, offset*]
  elementwise.hip:890  m355_add: dense, no stride argument                              out of scope (no slot can be passed)
  dwi.hip:79        dwi_mean vec: S % 4, x / y 16-B aligned                              test_dwi_mean_on_an_offset_base[aligned | offset1, offset2, S odd]
  c8 REQUIREs (16 B, strides % 8) by entry point: act16.hip m355_norm_act_fwd_h16, m355_avgpool3d_2x_fwd_h16, m355_norm_act_fwd_c8,
                    m355_act16_channel_partials; train16.hip m355_act16_pack_scaled / _unpack_scaled, norm_bwd_c8_args (m355_norm_act_bwd_c8
                    and its halves), m355_avgpool3d_2x_bwd_h16
                                                                                        test_c8_*, test_act16_pack_unpack | test_c8_rejects_misaligned_slots (each by name;
                                                                                        act16_channel_partials: the rejecting side only, its accepting side is test_kernels_gpu.py's dense call)
  evaluate.hip:208,349  dense [N, C, S] tensors without a batch stride                   out of scope (test_evaluation_gpu.py covers its alignment fallbacks)
"""
import pytest
import torch

from raw_ops import Slot
from test_kernels_gpu import X3, _c8_to_ncdhw, _dt, _rounded_close, _ulp, close, rnd

pytestmark = pytest.mark.gpu

CLASSES = ["aligned", "odd", "offset1", "offset2", "n1"]


def layout(cls, Cc, unit, role):
    """Slot layout of class `cls` for a tensor of Cc channels of `unit` elements; `role` (0, 1, 2) makes the strides of
    the tensors of one call differ from each other (and from dense)."""
    if cls == "odd":
        c_pre, c_post = (1, 3, 1)[role], (1, 1, 4)[role]
        extra = 0 if ((c_pre + Cc + c_post) * unit) % 4 else (1, 3, 2)[role]
        return dict(c_pre=c_pre, c_post=c_post, lead=(-c_pre * unit) % 4, extra=extra)
    c_pre, c_post = (4, 8, 4)[role], (4, 4, 12)[role]
    lead = {"aligned": 0, "offset1": 1, "offset2": 2, "n1": 1}[cls]
    return dict(c_pre=c_pre, c_post=c_post, lead=lead, extra=(-(c_pre + Cc + c_post) * unit) % 4)


def stride_of(lay, Cc, unit):
    return (lay["c_pre"] + Cc + lay["c_post"]) * unit + lay["extra"]


class Layouts:
    """the layouts of one call: tensors of the same (channels, unit, role) share one (the ABI gives `add` y's stride,
    dx x's); otherwise a stride that is already taken is widened by four foreign channels"""

    def __init__(self, cls):
        self.cls, self.by_key, self.taken = cls, {}, set()

    def get(self, shape, role):
        Cc, unit = shape[1], unit_of(shape)
        key = (Cc, unit, role)
        if key not in self.by_key:
            lay = layout(self.cls, Cc, unit, role)
            while self.cls != "odd" and stride_of(lay, Cc, unit) in self.taken | {Cc * unit}:
                lay["c_post"] += 4
                lay["extra"] = (-(lay["c_pre"] + Cc + lay["c_post"]) * unit) % 4
            self.taken.add(stride_of(lay, Cc, unit))
            self.by_key[key] = lay
        return self.by_key[key]


def unit_of(shape):
    u = 1
    for v in shape[2:]:
        u *= v
    return u


def nb(cls, N=2):
    return 1 if cls == "n1" else N


def run(hip, cls, call, ins, outs, what, same_stride=()):
    """call(ops, inputs, outs) -> tuple of results.  Runs it on slots of class `cls` (ins: [(tensor, role)], outs:
    [(shape, role)]) and dense (outs = None), checks criterion 1 and, for "aligned", criterion 3; returns the slot
    results as dense tensors.  same_stride: pairs (input index, output index) that share one stride by the ABI."""
    lays = Layouts(cls)
    si = [hip.slot(t, **lays.get(t.shape, r)) for t, r in ins]
    so = [hip.slot(s, **lays.get(s, r)) for s, r in outs]
    for i, o in same_stride:
        assert si[i].bs == so[o].bs and si[i].ptr != so[o].ptr
    if cls == "aligned":
        assert all(s.misalign() == 0 and s.bs % 4 == 0 for s in si + so)
        assert len({s.bs for s in si + so}) + len(same_stride) == len(si + so), "strides must differ"
    elif cls == "odd":
        assert all(s.misalign() == 0 and s.bs % 4 != 0 for s in si + so)
    else:
        assert all(s.misalign() == 4 * layout(cls, 1, 1, 0)["lead"] for s in si + so)
    res = call(hip, si, so)
    torch.cuda.synchronize()
    res = res if isinstance(res, tuple) else (res,)
    assert all(any(r is o for r in res) for o in so)
    for s in si:
        s.assert_unchanged(what)
    got = tuple(r.check_output(what) if isinstance(r, Slot) else r for r in res if r is not None)
    if cls == "aligned":
        dense = call(hip, [t for t, _ in ins], [None] * len(outs))
        dense = dense if isinstance(dense, tuple) else (dense,)
        for k, (g, d) in enumerate(zip(got, (d for d in dense if d is not None))):
            assert torch.equal(g, d), f"{what}: result {k} on aligned slots is not bit-identical to the dense call"
    return got


def same_plan(hip, cls, x_shape, Cout, compute, which, xs, ys, family):
    """the plan of the strided descriptor is the dense descriptor's, and of the expected family"""
    dense = hip.conv_plan(x_shape, Cout, compute=compute, which=which)
    assert dense[0] == family, f"expected kernel family {family}, planner says {dense}"
    assert hip.conv_plan(x_shape, Cout, compute=compute, which=which, xbs=xs, ybs=ys) == dense


def conv_layout_strides(cls, x_shape, y_shape, y_first=False):
    lays = Layouts(cls)
    if y_first:     # (the order run() builds the slots in decides which of two colliding strides is widened)
        ly, lx = lays.get(y_shape, 1), lays.get(x_shape, 0)
    else:
        lx, ly = lays.get(x_shape, 0), lays.get(y_shape, 1)
    return stride_of(lx, x_shape[1], unit_of(x_shape)), stride_of(ly, y_shape[1], unit_of(y_shape))


# ------------------------------------------------------------------------------------------------ conv3d 3x3x3
CONV_FWD = [
    # id, (Cin, Cout, D, H, W), compute, tuning, family forward / data gradient
    ("mfma-oneshot", (12, 40, 9, 10, 36), 0, {}, 1, 1),
    ("mfma-persistent", (12, 40, 9, 10, 36), 0, {"M355_CONV_SLOTS": 5}, 3, None),
    ("mfma-persistent-ragged", (8, 40, 9, 7, 33), 0, {"M355_CONV_SLOTS": 5}, 3, None),
    ("mfma-ksplit-ntw", (8, 40, 9, 7, 33), 0, {"M355_CONV_KSPLIT": 2, "M355_CONV_NTW": 2}, 1, 1),
    ("m16-remainder", (12, 8, 9, 10, 36), 0, {"M355_TILE16": 1}, 1, 1),
    ("split-x3", (12, 40, 9, 10, 36), X3, {"M355_F32X3_EDGE": 1}, 7, 7),
    ("split-x3-m16-odd", (6, 33, 6, 7, 20), X3, {"M355_F32X3_EDGE": 1, "M355_TILE16": 1}, 7, 7),
]


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("case", CONV_FWD, ids=[c[0] for c in CONV_FWD])
def test_conv3d_fwd_bwd_data(hip, oracle, tuning, case, cls):
    """m355_conv3d_fwd (bias + residual `add`, which shares y's batch stride), pre-packed weights, m355_conv3d_bwd_data:
    MFMA one-shot / persistent kernels, the 16-row remainder tile, the split kernel of M355_COMPUTE_F32X3."""
    _, (ci, co, D, H, W), compute, env, fam_f, fam_b = case
    tuning(**env)
    N = nb(cls)
    xsh, ysh = (N, ci, D, H, W), (N, co, D, H, W)
    x, w, b = rnd(*xsh, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * (1.0 / (27 * ci) ** 0.5), rnd(co, seed=3)
    add, dy = rnd(*ysh, seed=4), rnd(*ysh, seed=5)
    xs, ys = conv_layout_strides(cls, xsh, ysh)
    same_plan(hip, cls, xsh, co, compute, 0, xs, ys, fam_f)
    (y,) = run(hip, cls, lambda o, i, out: o.conv3d_fwd(i[0], w, b, i[1], compute=compute, out=out[0]),
               [(x, 0), (add, 1)], [(ysh, 1)], "conv3d_fwd", same_stride=[(1, 0)])
    close(y, oracle.conv3d_fwd(x, w, b, add), what="fwd")
    packed = hip.pack_weights(w, xsh, 0, compute)
    (yp,) = run(hip, cls, lambda o, i, out: o.conv3d_fwd(i[0], w, b, compute=compute, packed=packed, out=out[0]),
                [(x, 0)], [(ysh, 1)], "conv3d_fwd(packed)")
    close(yp, oracle.conv3d_fwd(x, w, b), what="fwd packed")
    if fam_b is not None:
        same_plan(hip, cls, xsh, co, compute, 1, *conv_layout_strides(cls, xsh, ysh, y_first=True), fam_b)
        (dx,) = run(hip, cls, lambda o, i, out: o.conv3d_bwd_data(i[0], w, xsh, compute=compute, out=out[0]),
                    [(dy, 1)], [(xsh, 0)], "conv3d_bwd_data")
        close(dx, oracle.conv3d_bwd_data(dy, w, xsh), what="bwd_data")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("case", [(9, 2, 9, 10, 40), (16, 3, 8, 6, 33)], ids=["W40", "W33"])
def test_conv3d_small_cout(hip, oracle, case, cls):
    """the z-Toeplitz small-Cout forward kernel (family 2): its epilogue picks row vector stores per sample from the
    alignment of y + n * ybs (conv3d.hip:792); with and without the fused softmax"""
    ci, co, D, H, W = case
    N = nb(cls)
    xsh, ysh = (N, ci, D, H, W), (N, co, D, H, W)
    x, w, b, add = rnd(*xsh, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * 0.2, rnd(co, seed=3), rnd(*ysh, seed=4)
    same_plan(hip, cls, xsh, co, 0, 0, *conv_layout_strides(cls, xsh, ysh), 2)
    (y,) = run(hip, cls, lambda o, i, out: o.conv3d_fwd(i[0], w, b, i[1], out=out[0]), [(x, 0), (add, 1)], [(ysh, 1)],
               "conv3d_fwd small cout", same_stride=[(1, 0)])
    close(y, oracle.conv3d_fwd(x, w, b, add), what="fwd")
    (p,) = run(hip, cls, lambda o, i, out: o.conv3d_fwd(i[0], w, b, softmax=True, out=out[0]), [(x, 0)], [(ysh, 1)],
               "conv3d_fwd + softmax")
    close(p, oracle.softmax_fwd(oracle.conv3d_fwd(x, w, b)), 2e-5, 1e-6, "conv + softmax")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("env", [{}, {"M355_CONV_SLOTS": "5"}], ids=["oneshot", "persistent"])
def test_conv3d_fwd_stats(hip, oracle, tuning, env, cls):
    """m355_conv3d_fwd_stats: y in a slot, the statistics partials dense"""
    tuning(**{"M355_CONV_KSPLIT": 1, **env})
    N, ci, co, D, H, W, groups = nb(cls), 8, 24, 9, 10, 36, 4

    def call(o, i, out):
        y, mean, rstd = o.conv3d_fwd_stats(i[0], w, b, groups, out=out[0])
        return y, mean, rstd
    x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * 0.2, rnd(co, seed=3)
    same_plan(hip, cls, (N, ci, D, H, W), co, 0, 0, *conv_layout_strides(cls, (N, ci, D, H, W), (N, co, D, H, W)),
              3 if env else 1)
    y, mean, rstd = run(hip, cls, call, [(x, 0)], [((N, co, D, H, W), 1)], "conv3d_fwd_stats")
    yo, mo, ro = oracle.conv3d_fwd_stats(x, w, b, groups)
    close(y, yo, 2e-5, 2e-5, "y")
    close(mean, mo, 1e-5, 1e-5, "mean")
    close(rstd, ro, 1e-5, 1e-5, "rstd")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("case", [(4, 2, 1, 6, 6, 8, 8, 8), (3, 2, 1, 3, 5, 7, 6, 5), (1, 1, 0, 4, 4, 5, 5, 5)],
                         ids=["blur-k4s2p1", "k3s2p1", "k1"])
def test_conv3d_generic_direct(hip, oracle, case, cls):
    """the generic direct kernels (family 0), incl. the strided Blur geometry k4 s2 p1: forward, both gradients"""
    k, s, p, ci, co, D, H, W = case
    N = nb(cls)
    xsh = (N, ci, D, H, W)
    x, w, b = rnd(*xsh, seed=1), rnd(co, ci, k, k, k, seed=2) * 0.2, rnd(co, seed=3)
    yo = oracle.conv3d_fwd(x, w, b, None, s, p)
    dy = rnd(*yo.shape, seed=5)
    (y,) = run(hip, cls, lambda o, i, out: o.conv3d_fwd(i[0], w, b, None, s, p, out=out[0]), [(x, 0)],
               [(tuple(yo.shape), 1)], "direct fwd")
    close(y, yo)
    (dx,) = run(hip, cls, lambda o, i, out: o.conv3d_bwd_data(i[0], w, xsh, s, p, out=out[0]), [(dy, 1)], [(xsh, 0)],
                "direct bwd_data")
    close(dx, oracle.conv3d_bwd_data(dy, w, xsh, s, p))
    dw, db = run(hip, cls, lambda o, i, out: o.conv3d_bwd_weight(i[0], i[1], k, s, p), [(x, 0), (dy, 1)], [], "direct bwd_weight")
    dwo, dbo = oracle.conv3d_bwd_weight(x, dy, k, s, p)
    close(dw, dwo, 3e-5, 1e-4)
    close(db, dbo, 3e-5, 1e-4)


BWW = [
    # id, (Cin, Cout, D, H, W), compute, tuning, family
    ("x3-8", (12, 40, 9, 10, 36), X3, {}, 8),
    ("x3-8-nsplit", (8, 40, 9, 7, 33), X3, {"M355_BWW_NSPLIT": 3}, 8),
    ("mfma-9", (12, 40, 9, 10, 36), 0, {"M355_TILE16": 1}, 9),
    ("mfma-9-ragged", (6, 33, 6, 7, 20), 0, {"M355_BWW_NSPLIT": 3, "M355_TILE16": 0}, 9),
    ("edge-10", (3, 40, 9, 10, 36), 0, {}, 10),
    ("edge-10-cout", (40, 3, 6, 7, 33), 0, {"M355_BWW_NSPLIT": 1}, 10),
]


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("case", BWW, ids=[c[0] for c in BWW])
def test_conv3d_bwd_weight(hip, oracle, tuning, case, cls):
    """m355_conv3d_bwd_weight with dbias: both operands in slots (the results are dense): families 8, 9, 10"""
    _, (ci, co, D, H, W), compute, env, fam = case
    tuning(**env)
    N = nb(cls)
    xsh, ysh = (N, ci, D, H, W), (N, co, D, H, W)
    x, dy = rnd(*xsh, seed=1), rnd(*ysh, seed=5)
    same_plan(hip, cls, xsh, co, compute, 2, *conv_layout_strides(cls, xsh, ysh), fam)
    dw, db = run(hip, cls, lambda o, i, out: o.conv3d_bwd_weight(i[0], i[1], 3, compute=compute), [(x, 0), (dy, 1)], [],
                 "conv3d_bwd_weight")
    dwo, dbo = oracle.conv3d_bwd_weight(x, dy, 3)
    close(dw, dwo, 3e-5, 3e-5 * (N * D * H * W) ** 0.5, what="bwd_weight")
    close(db, dbo, 3e-5, 3e-5 * (N * D * H * W) ** 0.5, what="dbias")


# ------------------------------------------------------------------------------------------------ conv-transpose
CONVT = [
    # Cin, Cout, D, H, W, k, s, p, out_pad
    (17, 5, 3, 5, 7, 2, 2, 0, 0),
    (64, 33, 4, 4, 6, 2, 2, 0, 0),
    (8, 8, 4, 4, 4, 4, 2, 1, 0),
    (3, 4, 3, 3, 3, 3, 2, 1, 1),
]


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("case", CONVT, ids=["k2s2-ragged", "k2s2-64", "k4s2p1", "k3s2p1op1"])
def test_conv_transpose3d(hip, oracle, case, cls):
    """m355_conv_transpose3d_fwd (F32 and, k2 s2, F32X3) / _bwd_data / _bwd_weight.  k2 s2 runs on the MFMA kernels when
    ybs % 2 == 0 and the y-side pointer is 8-byte aligned (convt_y_side_ok, the one fact route_convt takes from the
    call): classes aligned, offset2; an odd ybs ("odd": the output's S is a multiple of 8, so the stride is made odd with
    `extra` elements) and a 4-byte aligned pointer ("offset1", "n1") push the same shapes onto the direct kernels -- same
    tolerance either way.  m355_conv_transpose3d_plan, given each call's own y / dy slot, must name that side for all
    three entry points: family 1 (MfmaF32) or 2 (X3) against 0 (Direct)."""
    ci, co, D, H, W, k, s, p, op = case
    N = nb(cls)
    xsh = (N, ci, D, H, W)
    x, w, b = rnd(*xsh, seed=1), rnd(ci, co, k, k, k, seed=2) * (1.0 / ci ** 0.5), rnd(co, seed=3)
    yo = oracle.convt_fwd(x, w, b, s, p, op)
    ysh = tuple(yo.shape)
    dy = rnd(*ysh, seed=5)
    if k == 2:
        ly = layout(cls, co, unit_of(ysh), 1)
        ybs = (ly["c_pre"] + co + ly["c_post"]) * unit_of(ysh) + ly["extra"]
        mfma = ybs % 2 == 0 and (4 * (ly["lead"] + ly["c_pre"] * unit_of(ysh))) % 8 == 0
        assert mfma == (cls in ("aligned", "offset2")), "which side of convt_y_side_ok this class takes"
    families = []

    def planned(o, which, y_side, compute=0):
        """notes the family the library plans for the call that gets the slot `y_side` (the dense repeat has none)"""
        if isinstance(y_side, Slot):
            families.append((which, compute, o.convt_plan(xsh, co, k, s, p, op, compute, which, ybs=y_side.bs, y_side=y_side)[0]))

    for compute in ((0, X3) if k == 2 else (0,)):
        (y,) = run(hip, cls, lambda o, i, out: (planned(o, 0, out[0], compute),
                                                o.convt_fwd(i[0], w, b, s, p, op, compute=compute, out=out[0]))[1],
                   [(x, 0)], [(ysh, 1)], f"convt_fwd compute {compute}")
        close(y, yo, what="fwd")
    (dx,) = run(hip, cls, lambda o, i, out: (planned(o, 1, i[0]), o.convt_bwd_data(i[0], w, xsh, s, p, op, out=out[0]))[1],
                [(dy, 1)], [(xsh, 0)], "convt_bwd_data")
    close(dx, oracle.convt_bwd_data(dy, w, xsh, s, p, op), what="bwd_data")
    dw, db = run(hip, cls, lambda o, i, out: (planned(o, 2, i[1]), o.convt_bwd_weight(i[0], i[1], k, s, p, op))[1],
                 [(x, 0), (dy, 1)], [], "convt_bwd_weight")
    assert sorted(f[:2] for f in families) == [(0, 0)] + [(0, X3)] * (k == 2) + [(1, 0), (2, 0)]
    for which, compute, family in families:
        assert (family in (1, 2)) == (k == 2 and mfma) and (family == 0) != (k == 2 and mfma), (which, compute, family)
        assert family != 2 or (which == 0 and compute == X3), (which, compute, family)
    dwo, dbo = oracle.convt_bwd_weight(x, dy, k, s, p, op)
    close(dw, dwo, 3e-5, 1e-4, what="bwd_weight")
    close(db, dbo, 3e-5, 1e-4, what="dbias")


# ------------------------------------------------------------------------------------------------ normalisation
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("case", [(16, 4, 6, 8, 4, 1), (8, 5, 7, 9, 0, 2), (6, 3, 3, 5, 0, 1), (40, 4, 4, 6, 8, 0)],
                         ids=["gn-S192", "bn-S315", "bn-S45", "gn-5-per-group"])
def test_norm(hip, oracle, case, cls):
    """m355_norm_stats (GroupNorm; BatchNorm with running statistics), m355_norm_act_fwd with x, y and add strides all
    different, m355_norm_act_bwd (x / dx on x_batch_stride, dy on y_batch_stride)"""
    Cc, D, H, W, groups, act = case
    N = nb(cls)
    sh = (N, Cc, D, H, W)
    x = rnd(*sh, seed=1) * 1.7 + 0.3
    gamma, beta, add, dy = rnd(Cc, seed=2), rnd(Cc, seed=3), rnd(*sh, seed=4), rnd(*sh, seed=7)
    running = None if groups else (rnd(Cc, seed=5) * 0.1, torch.rand(Cc) + 0.5)
    st = run(hip, cls, lambda o, i, out: o.norm_stats(i[0], groups, running=running), [(x, 0)], [], "norm_stats")
    mo, ro, rmo, rvo = oracle.norm_stats(x, groups, running=running)
    close(st[0], mo, 1e-6, 1e-6, "mean")
    close(st[1], ro, 2e-6, 1e-6, "rstd")
    if running is not None:
        close(st[2], rmo, 1e-6, 1e-6, "running_mean")
        close(st[3], rvo, 2e-6, 1e-6, "running_var")
    # (add has the widest stride of the three, so a kernel that read it with x's or y's stride would stay inside add's buffer)
    (y,) = run(hip, cls, lambda o, i, out: o.norm_act_fwd(i[0], mo, ro, gamma, beta, groups, act, i[1], out=out[0]),
               [(x, 0), (add, 2)], [(sh, 1)], "norm_act_fwd")
    close(y, oracle.norm_act_fwd(x, mo, ro, gamma, beta, groups, act, add), what="fwd")
    for training in ((1,) if groups else (1, 0)):
        dx, dg, db = run(hip, cls, lambda o, i, out: o.norm_act_bwd(i[0], i[1], mo, ro, gamma, beta, groups, act, training, out=out[0]),
                         [(x, 0), (dy, 1)], [(sh, 0)], "norm_act_bwd", same_stride=[(0, 0)])
        dxo, dgo, dbo = oracle.norm_act_bwd(x, dy, mo, ro, gamma, beta, groups, act, training)
        close(dx, dxo, 2e-5, 2e-5, "dx")
        close(dg, dgo, 2e-5, 1e-4, "dgamma")
        close(db, dbo, 2e-5, 1e-4, "dbeta")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("case", [(16, 4, 6, 8, 4, 1), (3, 6, 2, 2, 0, 2)], ids=["gn", "bn-tiny"])
def test_norm_act_pool(hip, oracle, case, cls):
    """m355_norm_act_pool_fwd: y and the pooled tensor each in a slot of its own stride.  The host function requires x / y
    8-byte aligned with even strides (norm.hip:687, stated in m355seg.h): classes odd, offset1, n1 are rejected with
    M355_EINVALID_ARG before anything is launched.  Reference as in the dense test: oracle norm_act_fwd -> avgpool."""
    Cc, D, H, W, groups, act = case
    N = nb(cls)
    sh, psh = (N, Cc, D, H, W), (N, Cc, D // 2, H // 2, W // 2)
    x, gamma, beta = rnd(*sh, seed=1), rnd(Cc, seed=2) * 0.5 + 1.0, rnd(Cc, seed=3) * 0.1
    mean, rstd = oracle.norm_stats(x, groups)[:2]
    call = lambda o, i, out: o.norm_act_pool_fwd(i[0], mean, rstd, gamma, beta, groups, act, out=out[0], out_pooled=out[1])
    lx = layout(cls, Cc, D * H * W, 0)
    if lx["lead"] % 2 or lx["extra"] % 2:
        xs = hip.slot(x, **lx)
        y, pooled = hip.slot(sh, **layout(cls, Cc, D * H * W, 1)), hip.slot(psh, **layout(cls, Cc, D * H * W // 8, 2))
        with pytest.raises(RuntimeError, match="-> -1 .*8B aligned"):
            call(hip, [xs], [y, pooled])
        torch.cuda.synchronize()
        y.assert_untouched("norm_act_pool_fwd")
        pooled.assert_untouched("norm_act_pool_fwd")
        return
    y, pooled = run(hip, cls, call, [(x, 0)], [(sh, 1), (psh, 2)], "norm_act_pool_fwd")
    yo = oracle.norm_act_fwd(x, mean, rstd, gamma, beta, groups, act)
    close(y, yo, what="y")
    close(pooled, oracle.avgpool_fwd(yo), 1e-5, 1e-6, "pooled")


# ------------------------------------------------------------------------------------------------ pool / upsample / moves
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", [(5, 4, 6, 8), (3, 2, 6, 6)], ids=["W8", "W6"])
def test_pool(hip, oracle, shape, cls):
    """m355_avgpool3d_2x_fwd / _bwd / _bwd_add (three strides)"""
    sh = (nb(cls),) + shape
    x = rnd(*sh, seed=1)
    yo = oracle.avgpool_fwd(x)
    dy, skip = rnd(*yo.shape, seed=2), rnd(*sh, seed=3)
    (y,) = run(hip, cls, lambda o, i, out: o.avgpool_fwd(i[0], out=out[0]), [(x, 0)], [(tuple(yo.shape), 1)], "avgpool_fwd")
    close(y, yo, 1e-6, 1e-6, "pool fwd")
    (dx,) = run(hip, cls, lambda o, i, out: o.avgpool_bwd(i[0], sh, out=out[0]), [(dy, 1)], [(sh, 0)], "avgpool_bwd")
    close(dx, oracle.avgpool_bwd(dy, sh), 0, 0, "pool bwd")
    (dx,) = run(hip, cls, lambda o, i, out: o.avgpool_bwd_add(i[0], i[1], sh, out=out[0]), [(dy, 1), (skip, 2)], [(sh, 0)],
                "avgpool_bwd_add")
    close(dx, oracle.avgpool_bwd_add(dy, skip, sh), 0, 1e-7, "pool bwd + add")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", [(3, 6, 11, 12), (2, 5, 3, 7), (5, 1, 2, 6)], ids=["W12", "W7-odd", "D1"])
def test_upsample(hip, oracle, shape, cls):
    """m355_upsample_trilinear2x_fwd (even W: LDS / quad kernels with float4 stores; odd W or a misaligned y: the
    one-output-per-thread kernel, elementwise.hip:712) and _bwd"""
    sh = (nb(cls),) + shape
    x = rnd(*sh, seed=3)
    yo = oracle.upsample_fwd(x)
    dy = rnd(*yo.shape, seed=4)
    (y,) = run(hip, cls, lambda o, i, out: o.upsample_fwd(i[0], out=out[0]), [(x, 0)], [(tuple(yo.shape), 1)], "upsample_fwd")
    close(y, yo, 2e-6, 2e-6, "up fwd")
    (dx,) = run(hip, cls, lambda o, i, out: o.upsample_bwd(i[0], sh, out=out[0]), [(dy, 1)], [(sh, 0)], "upsample_bwd")
    close(dx, oracle.upsample_bwd(dy, sh), 1e-5, 1e-5, "up bwd")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", [(3, 4, 6, 8), (5, 2, 2, 6)], ids=["S192", "S24"])
def test_space_to_depth(hip, oracle, shape, cls):
    """m355_space_to_depth2 / m355_depth_to_space2 (bit-exact permutations).  The full-resolution tensor must be 8-byte
    aligned with an even stride (elementwise.hip:625, stated in m355seg.h): M355_EUNSUPPORTED otherwise, nothing written."""
    sh = (nb(cls),) + shape
    x = rnd(*sh, seed=1)
    yo = oracle.space_to_depth(x)
    psh = tuple(yo.shape)
    lf = layout(cls, sh[1], unit_of(sh), 0)
    if lf["lead"] % 2 or lf["extra"] % 2:
        out = hip.slot(psh, **layout(cls, psh[1], unit_of(psh), 1))
        with pytest.raises(RuntimeError, match="-> -2 .*8-byte aligned"):
            hip.space_to_depth(hip.slot(x, **lf), out=out)
        back = hip.slot(sh, **lf)
        with pytest.raises(RuntimeError, match="-> -2 .*8-byte aligned"):
            hip.depth_to_space(hip.slot(yo, **layout(cls, psh[1], unit_of(psh), 1)), out=back)
        torch.cuda.synchronize()
        out.assert_untouched("space_to_depth2")
        back.assert_untouched("depth_to_space2")
        return
    (y,) = run(hip, cls, lambda o, i, out: o.space_to_depth(i[0], out=out[0]), [(x, 0)], [(psh, 1)], "space_to_depth2")
    assert torch.equal(y.cpu(), yo)
    (xb,) = run(hip, cls, lambda o, i, out: o.depth_to_space(i[0], out=out[0]), [(yo, 1)], [(sh, 0)], "depth_to_space2")
    assert torch.equal(xb.cpu(), x)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", [(5, 4, 6, 8), (3, 5, 7, 9)], ids=["S192", "S315"])
def test_copy_channels(hip, oracle, shape, cls):
    sh = (nb(cls),) + shape
    x = rnd(*sh, seed=1)
    (y,) = run(hip, cls, lambda o, i, out: o.copy_channels(i[0], out=out[0]), [(x, 0)], [(sh, 1)], "copy_channels")
    assert torch.equal(y.cpu(), oracle.copy_channels(x)) and torch.equal(y.cpu(), x)


@pytest.mark.parametrize("cls", ["aligned", "offset1", "offset2"])
@pytest.mark.parametrize("shape", [(4, 6, 8), (5, 7, 9)], ids=["S192", "S315"])
def test_dwi_mean_on_an_offset_base(hip, shape, cls):
    """m355_dwi_mean has no stride argument: the channel stack and the output sit on offset pointers (dwi.hip:79 drops
    to the scalar kernel).  Reference as in test_dwi_reconstruction_gpu.py: the fp32 sum in pick order, divided by k."""
    x = rnd(1, 7, *shape, seed=1)
    idx = [5, 0, 3, 3, 6]
    (y,) = run(hip, cls, lambda o, i, out: o.dwi_mean(i[0], idx, out=out[0]), [(x, 0)], [((1, 1) + shape, 1)], "dwi_mean")
    acc = x[0, idx[0]].clone()
    for c in idx[1:]:
        acc = acc + x[0, c]
    assert torch.equal(y.cpu()[0, 0], acc / len(idx))


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_act16_pack_unpack(hip, compute, cls):
    """m355_act16_pack / _unpack (+ _scaled): the fp32 side in a slot of any class, the c8 side in an aligned c8 slot"""
    dt = _dt(compute)
    N, Cc, sp = nb(cls), 13, (3, 5, 7)
    x = rnd(N, Cc, *sp, seed=1)
    S = 3 * 5 * 7
    for scale in (None, 2.0 ** 7):
        want = (x * (scale or 1.0)).to(dt).float()
        o16 = hip.slot((N, 2, S, 8), dtype=dt, c_pre=1, c_post=2)
        xs = hip.slot(x, **layout(cls, Cc, S, 0))
        if scale is None:
            hip.act16_pack(xs, compute, out=o16)
        else:
            hip.act16_pack_scaled(xs, compute, scale, out=o16)
        torch.cuda.synchronize()
        xs.assert_unchanged("act16_pack")
        x16 = o16.check_output("act16_pack")
        assert torch.equal(_c8_to_ncdhw(x16, Cc, sp), want)
        assert (x16[:, -1, :, Cc % 8:].float() == 0).all()
        assert torch.equal(x16, hip.act16_pack(x, compute) if scale is None else hip.act16_pack_scaled(x, compute, scale))
        back = hip.slot((N, Cc) + sp, **layout(cls, Cc, S, 1))
        i16 = hip.slot(x16, c_pre=2, c_post=1)
        if scale is None:
            hip.act16_unpack(i16, Cc, sp, compute, out=back)
        else:
            hip.act16_unpack_scaled(i16, Cc, sp, compute, 1.0 / scale, out=back)
        torch.cuda.synchronize()
        i16.assert_unchanged("act16_unpack")
        assert torch.equal(back.check_output("act16_unpack").cpu(), want / (scale or 1.0))


# ------------------------------------------------------------------------------------------------ c8 family
def c8_slots(hip, tensors, outs):
    """aligned c8 slots (the only legal class: whole channel blocks of 16-byte items), strides all different"""
    si = [hip.slot(t, c_pre=1 + k, c_post=2) for k, t in enumerate(tensors)]
    so = [hip.slot(s, dtype=dt, c_pre=2, c_post=3 + k) for k, (s, dt) in enumerate(outs)]
    return si, so


def c8_done(si, so, what):
    torch.cuda.synchronize()
    for s in si:
        s.assert_unchanged(what)
    return [s.check_output(what) for s in so]


@pytest.mark.parametrize("N", [2, 1])
@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_c8_conv3d(hip, oracle, compute, N, tuning):
    """m355_conv3d_fwd_h16 (c8 in, fp32 slot out, with `add`), _fwd_h16_c8, _bwd_data_h16, _bwd_data_h16_c8,
    _bwd_weight_h16 / _c8: slots on the input side and the output side, bit-identical to the dense calls and within the
    dense tests' tolerance of the oracle on the rounded operands"""
    tuning(M355_CONV_KSPLIT=1)
    dt = _dt(compute)
    ci, co, D, H, W = 16, 40, 5, 6, 36
    S, sp = D * H * W, (D, H, W)
    xsh, ysh = (N, ci, D, H, W), (N, co, D, H, W)
    x, w, b = rnd(*xsh, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * (1.0 / (27 * ci) ** 0.5), rnd(co, seed=3)
    add, dy = rnd(*ysh, seed=4), rnd(*ysh, seed=5)
    x16, dy16 = hip.act16_pack(x, compute), hip.act16_pack(dy, compute)
    xr, dyr = x.to(dt).float(), dy.to(dt).float()
    # forward, fp32 output in an fp32 slot of class "aligned" (the out conv / unfused consumers)
    (xs, ), _ = c8_slots(hip, [x16], [])
    ads = hip.slot(add, **layout("aligned", co, S, 1))
    out = hip.slot(ysh, **layout("aligned", co, S, 1))
    hip.conv3d_fwd_h16(xs, ci, sp, w, b, ads, compute=compute, out=out)
    torch.cuda.synchronize()
    xs.assert_unchanged("conv3d_fwd_h16")
    ads.assert_unchanged("conv3d_fwd_h16")
    y = out.check_output("conv3d_fwd_h16")
    assert torch.equal(y, hip.conv3d_fwd_h16(x16, ci, sp, w, b, add, compute=compute))
    ref = oracle.conv3d_fwd(x, w, b, add, compute=compute)
    close(y, ref, 3e-5, 3e-5, "conv3d_fwd_h16")
    # forward c8 -> c8
    (xs,), (o16,) = c8_slots(hip, [x16], [((N, 5, S, 8), dt)])
    hip.conv3d_fwd_h16_c8(xs, ci, sp, w, b, compute=compute, out=o16)
    (y16,) = c8_done([xs], [o16], "conv3d_fwd_h16_c8")
    assert torch.equal(y16, hip.conv3d_fwd_h16_c8(x16, ci, sp, w, b, compute=compute))
    refc = oracle.conv3d_fwd(xr, w.to(dt).float(), b)
    assert ((_c8_to_ncdhw(y16, co, sp) - refc).abs() <= _ulp(compute) * refc.abs() * 1.01 + 3e-5).all()
    # data gradient: fp32 slot out, and c8 slot out
    (dys,), (dx16s,) = c8_slots(hip, [dy16], [((N, 2, S, 8), dt)])
    dxs = hip.slot(xsh, **layout("aligned", ci, S, 0))
    hip.conv3d_bwd_data_h16(dys, co, w, xsh, compute, out=dxs)
    hip.conv3d_bwd_data_h16_c8(dys, co, w, xsh, compute, out=dx16s)
    (dx16,) = c8_done([dys], [dx16s], "conv3d_bwd_data_h16_c8")
    dx = dxs.check_output("conv3d_bwd_data_h16")
    assert torch.equal(dx, hip.conv3d_bwd_data_h16(dy16, co, w, xsh, compute))
    assert torch.equal(dx16, hip.conv3d_bwd_data_h16_c8(dy16, co, w, xsh, compute))
    refd = oracle.conv3d_bwd_data(dy, w, xsh, compute=compute)
    close(dx, refd, 3e-5, 3e-5, "conv3d_bwd_data_h16")
    assert torch.equal(_c8_to_ncdhw(dx16, ci, sp), dx.cpu().to(dt).float())
    # weight gradients: both c8 operands and the fp32 dy (bias gradient) in slots
    (xs, dys), _ = c8_slots(hip, [x16, dy16], [])
    dyf = hip.slot(dy, **layout("aligned", co, S, 2))
    dw, db = hip.conv3d_bwd_weight_h16(xs, dys, dyf, ci, co, sp, compute)
    dwc, dbc = hip.conv3d_bwd_weight_c8(xs, dys, ci, co, sp, compute)
    c8_done([xs, dys, dyf], [], "conv3d_bwd_weight_h16")
    dw0, db0 = hip.conv3d_bwd_weight_h16(x16, dy16, dy, ci, co, sp, compute)
    dwc0, dbc0 = hip.conv3d_bwd_weight_c8(x16, dy16, ci, co, sp, compute)
    assert torch.equal(dw, dw0) and torch.equal(db, db0) and torch.equal(dwc, dwc0) and torch.equal(dbc, dbc0)
    dwo, dbo = oracle.conv3d_bwd_weight(x, dy, 3, compute=compute)
    tol = 3e-5 * (N * S) ** 0.5
    close(dw, dwo, 3e-5, tol, "bwd_weight from c8")
    close(db, dbo, 3e-5, tol, "dbias")
    close(dwc, dwo, 3e-5, 3e-5 * dwo.abs().max().item(), "bwd_weight_c8 vs oracle")
    close(dbc, dyr.double().sum(dim=(0, 2, 3, 4)).float(), 1e-5, 1e-4, "dbias from c8")


@pytest.mark.parametrize("N", [2, 1])
@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_c8_conv_transpose(hip, oracle, compute, N):
    """m355_conv_transpose3d_fwd_h16 / _bwd_data_h16 / _bwd_weight_h16 on c8 slots"""
    dt = _dt(compute)
    ci, co, D, H, W = 24, 40, 3, 5, 6
    S, sp, xsh = D * H * W, (D, H, W), (N, 24, 3, 5, 6)
    x, dy = rnd(*xsh, seed=1), rnd(N, co, 2 * D, 2 * H, 2 * W, seed=2)
    w, b = rnd(ci, co, 2, 2, 2, seed=3) * 0.2, rnd(co, seed=4)
    x16, dy16 = hip.act16_pack(x, compute), hip.act16_pack(dy, compute)
    xr, dyr, wr = x.to(dt).float(), dy.to(dt).float(), w.to(dt).float()
    (xs, dys), (ys, dxs) = c8_slots(hip, [x16, dy16], [((N, 5, 8 * S, 8), dt), ((N, 3, S, 8), dt)])
    hip.conv_transpose3d_fwd_h16(xs, ci, sp, w, b, compute, out=ys)
    assert hip.convt_h16_bwd_supported(xsh, co)
    hip.convt_bwd_data_h16(dys, w, xsh, compute, out=dxs)
    dw, db = hip.convt_bwd_weight_h16(xs, dys, xsh, co, compute)
    y16, dx16 = c8_done([xs, dys], [ys, dxs], "conv_transpose3d c8")
    assert torch.equal(y16, hip.conv_transpose3d_fwd_h16(x16, ci, sp, w, b, compute))
    assert torch.equal(dx16, hip.convt_bwd_data_h16(dy16, w, xsh, compute))
    dw0, db0 = hip.convt_bwd_weight_h16(x16, dy16, xsh, co, compute)
    assert torch.equal(dw, dw0) and torch.equal(db, db0)
    ref = oracle.convt_fwd(xr, w, b, 2, 0, 0)
    assert ((_c8_to_ncdhw(y16, co, (2 * D, 2 * H, 2 * W)) - ref).abs() <= _ulp(compute) * ref.abs() * 1.01 + 2e-5).all()
    ref_dx = oracle.convt_bwd_data(dyr, wr, xsh, 2, 0, 0)
    _rounded_close(_c8_to_ncdhw(dx16, ci, sp), ref_dx, compute, 3e-5 * ref_dx.abs().max().item(), "convT dx")
    ref_dw, ref_db = oracle.convt_bwd_weight(xr, dyr, 2, 2, 0, 0)
    close(dw, ref_dw, 3e-5, 3e-5 * ref_dw.abs().max().item(), "convT dw")
    close(db, ref_db, 1e-5, 1e-4, "convT dbias")


@pytest.mark.parametrize("N", [2, 1])
@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_c8_norm(hip, oracle, compute, N):
    """m355_norm_act_fwd_h16 (fp32 slot in, c8 slot + fp32 slot out), m355_norm_act_fwd_c8 (x16, add16, y16 strides all
    different), m355_norm_act_bwd_c8 (dy16 + dpool16)"""
    dt = _dt(compute)
    Cc, D, H, W, groups, act = 13, 4, 6, 8, 0, 1
    S, sp, sh = D * H * W, (D, H, W), (N, 13, 4, 6, 8)
    x, res, dy = rnd(*sh, seed=1), rnd(*sh, seed=4), rnd(*sh, seed=6)
    dp = rnd(N, Cc, D // 2, H // 2, W // 2, seed=7)
    gamma, beta = rnd(Cc, seed=2) * 0.5 + 1.0, rnd(Cc, seed=3) * 0.1
    mean, rstd = oracle.norm_stats(x, groups)[:2]
    xs, ads = hip.slot(x, **layout("aligned", Cc, S, 0)), hip.slot(res, **layout("aligned", Cc, S, 2))
    y32s, y16s = hip.slot(sh, **layout("aligned", Cc, S, 1)), hip.slot((N, 2, S, 8), dtype=dt, c_pre=1, c_post=2)
    hip.norm_act_fwd_h16(xs, mean, rstd, gamma, beta, groups, act, compute, add=ads, out16=y16s, out=y32s)
    (y16,) = c8_done([xs, ads], [y16s], "norm_act_fwd_h16")
    y32 = y32s.check_output("norm_act_fwd_h16 fp32 twin")
    d16, d32 = hip.norm_act_fwd_h16(x, mean, rstd, gamma, beta, groups, act, compute, add=res, want_f32=True)
    assert torch.equal(y16, d16) and torch.equal(y32, d32)
    ref = oracle.norm_act_fwd(x, mean, rstd, gamma, beta, groups, act, res)
    close(y32, ref, 1e-5, 1e-5, "fp32 twin")
    assert ((_c8_to_ncdhw(y16, Cc, sp) - ref).abs() <= _ulp(compute) * ref.abs() * 1.01 + 2e-5).all()
    # c8 -> c8
    x16, r16 = hip.act16_pack(x, compute), hip.act16_pack(res, compute)
    xr = x.to(dt).float()
    m2, r2 = oracle.norm_stats(xr, groups)[:2]
    (xs, rs), (os_,) = c8_slots(hip, [x16, r16], [((N, 2, S, 8), dt)])
    hip.norm_act_fwd_c8(xs, Cc, m2, r2, gamma, beta, groups, act, compute, add16=rs, out=os_)
    (a16,) = c8_done([xs, rs], [os_], "norm_act_fwd_c8")
    assert torch.equal(a16, hip.norm_act_fwd_c8(x16, Cc, m2, r2, gamma, beta, groups, act, compute, add16=r16))
    ref = oracle.norm_act_fwd(xr, m2, r2, gamma, beta, groups, act, res.to(dt).float())
    assert ((_c8_to_ncdhw(a16, Cc, sp) - ref).abs() <= _ulp(compute) * ref.abs() * 1.01 + 2e-5).all()
    # backward
    dy16, dp16 = hip.act16_pack(dy, compute), hip.act16_pack(dp, compute)
    (xs, dys, dps), (dxs,) = c8_slots(hip, [x16, dy16, dp16], [((N, 2, S, 8), dt)])
    _, dg, db = hip.norm_act_bwd_c8(xs, dys, dps, Cc, sp, m2, r2, gamma, beta, groups, act, compute, out=dxs)
    (dx16,) = c8_done([xs, dys, dps], [dxs], "norm_act_bwd_c8")
    dx0, dg0, db0 = hip.norm_act_bwd_c8(x16, dy16, dp16, Cc, sp, m2, r2, gamma, beta, groups, act, compute)
    assert torch.equal(dx16, dx0) and torch.equal(dg, dg0) and torch.equal(db, db0)
    g = dy.to(dt).float() + 0.125 * dp.to(dt).float().repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)
    ref_dx, ref_dg, ref_db = oracle.norm_act_bwd(xr, g, m2, r2, gamma, beta, groups, act, training=1)
    _rounded_close(_c8_to_ncdhw(dx16, Cc, sp), ref_dx, compute, 2e-5 * ref_dx.abs().max().item(), "dx")
    close(dg, ref_dg, 1e-4, 1e-4 * ref_dg.abs().max().item(), "dgamma")
    close(db, ref_db, 1e-4, 1e-4 * ref_db.abs().max().item(), "dbeta")
    # the fp32 backward with the c8 twin of dx in a c8 slot (m355_norm_act_bwd_h16): x / dx, dy and the twin all strided
    lx, ly = layout("aligned", Cc, S, 0), layout("aligned", Cc, S, 1)
    xs, dys, dxs = hip.slot(x, **lx), hip.slot(dy, **ly), hip.slot(sh, **lx)
    tws = hip.slot((N, 2, S, 8), dtype=dt, c_pre=2, c_post=1)
    _, dg, db, _ = hip.norm_act_bwd_h16(xs, dys, mean, rstd, gamma, beta, groups, act, compute, out=dxs, out16=tws)
    (tw,) = c8_done([xs, dys], [tws], "norm_act_bwd_h16")
    dx = dxs.check_output("norm_act_bwd_h16 dx")
    dx0, dg0, db0, tw0 = hip.norm_act_bwd_h16(x, dy, mean, rstd, gamma, beta, groups, act, compute)
    assert torch.equal(dx, dx0) and torch.equal(dg, dg0) and torch.equal(db, db0) and torch.equal(tw, tw0)
    assert torch.equal(_c8_to_ncdhw(tw, Cc, sp), dx.cpu().to(dt).float())
    dxo, dgo, dbo = oracle.norm_act_bwd(x, dy, mean, rstd, gamma, beta, groups, act)
    close(dx, dxo, 2e-5, 2e-5, "dx")
    close(dg, dgo, 2e-5, 1e-4, "dgamma")
    close(db, dbo, 2e-5, 1e-4, "dbeta")


@pytest.mark.parametrize("N", [2, 1])
@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_c8_pool_upsample_s2d_scale(hip, oracle, compute, N):
    """pooling (fwd / bwd + skip), trilinear upsampling (fwd / bwd), space-to-depth / depth-to-space and
    act16_channel_scale on c8 slots: bit-identical to the dense calls, and the dense tests' references"""
    dt = _dt(compute)
    Cc, D, H, W = 13, 4, 6, 8
    S, sp, sh = D * H * W, (D, H, W), (N, 13, 4, 6, 8)
    x, dpool = rnd(*sh, seed=1), rnd(N, Cc, D // 2, H // 2, W // 2, seed=2)
    x16, dp16 = hip.act16_pack(x, compute), hip.act16_pack(dpool, compute)
    xr = x.to(dt).float()
    (xs, dps), (ps, dxs, us, ss, cs) = c8_slots(hip, [x16, dp16], [((N, 2, S // 8, 8), dt), ((N, 2, S, 8), dt), ((N, 2, 8 * S, 8), dt),
                                                                ((N, Cc, S // 8, 8), dt), ((N, 2, S, 8), dt)])
    scale = torch.where(rnd(N * Cc, seed=3) > 0, torch.tensor(2.0), torch.tensor(0.0))
    hip.avgpool_fwd_h16(xs, Cc, sp, compute, out=ps)
    hip.avgpool_bwd_h16(dps, xs, Cc, sp, compute, out=dxs)
    hip.upsample_trilinear2x_fwd_h16(xs, Cc, sp, compute, out=us)
    hip.s2d_h16(xs, sh, compute, True, out=ss)
    hip.act16_channel_scale(xs, scale, Cc, compute, out=cs)
    p16, dx16, u16, s16, c16 = c8_done([xs, dps], [ps, dxs, us, ss, cs], "c8 elementwise")
    assert torch.equal(p16, hip.avgpool_fwd_h16(x16, Cc, sp, compute))
    assert torch.equal(dx16, hip.avgpool_bwd_h16(dp16, x16, Cc, sp, compute))
    assert torch.equal(u16, hip.upsample_trilinear2x_fwd_h16(x16, Cc, sp, compute))
    assert torch.equal(s16, hip.s2d_h16(x16, sh, compute, True))
    assert torch.equal(c16, hip.act16_channel_scale(x16, scale, Cc, compute))
    pref = torch.nn.functional.avg_pool3d(xr, 2, 2).to(dt).float()
    assert ((_c8_to_ncdhw(p16, Cc, (D // 2, H // 2, W // 2)) - pref).abs() <= _ulp(compute) * pref.abs() * 1.01 + 1e-6).all()
    up8 = 0.125 * dpool.to(dt).float().repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)
    _rounded_close(_c8_to_ncdhw(dx16, Cc, sp), up8 + xr, compute, 1e-7, "pool bwd + skip")
    up = torch.nn.Upsample(scale_factor=2, mode='trilinear', align_corners=True)
    xg = xr.clone().requires_grad_()
    uref = up(xg)
    _rounded_close(_c8_to_ncdhw(u16, Cc, (2 * D, 2 * H, 2 * W)), uref.detach(), compute, 2e-6, "trilinear fwd c8")
    assert torch.equal(_c8_to_ncdhw(s16, 8 * Cc, (D // 2, H // 2, W // 2)), oracle.space_to_depth(xr))
    _rounded_close(_c8_to_ncdhw(c16, Cc, sp), xr * scale.view(N, Cc, 1, 1, 1), compute, 0.0, "channel scale c8")
    # the inverse directions, from slots holding the results above
    du = rnd(N, Cc, 2 * D, 2 * H, 2 * W, seed=4)
    du16 = hip.act16_pack(du, compute)
    (dus, s16s), (dlo, back) = c8_slots(hip, [du16, s16], [((N, 2, S, 8), dt), ((N, 2, S, 8), dt)])
    hip.upsample_trilinear2x_bwd_h16(dus, Cc, sp, compute, out=dlo)
    hip.s2d_h16(s16s, sh, compute, False, out=back)
    dlo16, b16 = c8_done([dus, s16s], [dlo, back], "c8 elementwise inverse")
    assert torch.equal(dlo16, hip.upsample_trilinear2x_bwd_h16(du16, Cc, sp, compute))
    assert torch.equal(b16, x16), "depth-to-space is not the inverse"
    uref.backward(du.to(dt).float())
    _rounded_close(_c8_to_ncdhw(dlo16, Cc, sp), xg.grad, compute, 1e-5, "trilinear bwd c8")


@pytest.mark.parametrize("bad", ["pointer+8B", "stride+4"])
@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_c8_rejects_misaligned_slots(hip, compute, bad):
    """The c8 entry points document 16-byte items: a pointer that is only 8-byte aligned, or a batch stride that is no
    multiple of 8 elements, is refused with M355_EINVALID_ARG by the host function -- on the input side and on the output
    side -- and the output slot still holds the canary.  (`ops.Act16.slot` cannot produce either: c8 slots start at whole
    channel blocks, S * 16 bytes each, of a [N, CB, S, 8] allocation, and the stride is CB_total * S * 8.)"""
    dt = _dt(compute)
    N, Cc, D, H, W = 2, 16, 2, 4, 6
    S, sp, sh = D * H * W, (D, H, W), (2, 16, 2, 4, 6)
    x, dy, up = rnd(*sh, seed=1), rnd(*sh, seed=5), rnd(N, Cc, 2 * D, 2 * H, 2 * W, seed=6)
    w, b = rnd(16, 16, 3, 3, 3, seed=2) * 0.1, rnd(16, seed=3)
    wt = rnd(16, 16, 2, 2, 2, seed=4) * 0.1
    x16, dy16, up16 = hip.act16_pack(x, compute), hip.act16_pack(dy, compute), hip.act16_pack(up, compute)
    pool16 = hip.act16_pack(rnd(N, Cc, D // 2, H // 2, W // 2, seed=7), compute)
    s2d16 = hip.s2d_h16(x16, sh, compute, True)
    assert hip.convt_h16_bwd_supported(sh, Cc)
    good = dict(c_pre=1, c_post=1)
    lay = dict(good, lead=4) if bad == "pointer+8B" else dict(good, extra=4)
    mean, rstd = torch.zeros(2 * 4), torch.ones(2 * 4)
    B, B8, Bp = (N, 2, S, 8), (N, 2, 8 * S, 8), (N, 2, S // 8, 8)
    # name: (call(c8 input slot, c8 output slot), the c8 input tensor or None, shape of the c8 output)
    calls = {
        "act16_pack": (lambda i, o: hip.act16_pack(x, compute, out=o), None, B),
        "act16_pack_scaled": (lambda i, o: hip.act16_pack_scaled(x, compute, 2.0, out=o), None, B),
        "norm_act_fwd_h16": (lambda i, o: hip.norm_act_fwd_h16(x, mean, rstd, None, None, 4, 1, compute, out16=o), None, B),
        "norm_act_bwd_h16": (lambda i, o: hip.norm_act_bwd_h16(x, dy, mean, rstd, None, None, 4, 1, compute, out16=o), None, B),
        "conv3d_fwd_h16_c8": (lambda i, o: hip.conv3d_fwd_h16_c8(i, Cc, sp, w, b, compute=compute, out=o), x16, B),
        "conv3d_bwd_data_h16_c8": (lambda i, o: hip.conv3d_bwd_data_h16_c8(i, Cc, w, sh, compute, out=o), dy16, B),
        "conv_transpose3d_fwd_h16": (lambda i, o: hip.conv_transpose3d_fwd_h16(i, Cc, sp, wt, b, compute, out=o), x16, B8),
        "conv_transpose3d_bwd_data_h16": (lambda i, o: hip.convt_bwd_data_h16(i, wt, sh, compute, out=o), up16, B),
        "norm_act_fwd_c8": (lambda i, o: hip.norm_act_fwd_c8(i, Cc, mean, rstd, None, None, 4, 1, compute, out=o), x16, B),
        "norm_act_fwd_c8 (add16)": (lambda i, o: hip.norm_act_fwd_c8(x16, Cc, mean, rstd, None, None, 4, 1, compute, add16=i, out=o),
                                    dy16, B),
        "norm_act_bwd_c8 (x16)": (lambda i, o: hip.norm_act_bwd_c8(i, dy16, None, Cc, sp, mean, rstd, None, None, 4, 1, compute,
                                                                   out=o), x16, B),
        "norm_act_bwd_c8 (dy16)": (lambda i, o: hip.norm_act_bwd_c8(x16, i, None, Cc, sp, mean, rstd, None, None, 4, 1, compute,
                                                                    out=o), dy16, B),
        "norm_act_bwd_c8 (dpool16)": (lambda i, o: hip.norm_act_bwd_c8(x16, None, i, Cc, sp, mean, rstd, None, None, 4, 1, compute,
                                                                       out=o), pool16, B),
        "avgpool3d_2x_fwd_h16": (lambda i, o: hip.avgpool_fwd_h16(i, Cc, sp, compute, out=o), x16, Bp),
        "avgpool3d_2x_bwd_h16 (dpool16)": (lambda i, o: hip.avgpool_bwd_h16(i, x16, Cc, sp, compute, out=o), pool16, B),
        "avgpool3d_2x_bwd_h16 (dskip16)": (lambda i, o: hip.avgpool_bwd_h16(pool16, i, Cc, sp, compute, out=o), x16, B),
        "upsample_trilinear2x_fwd_h16": (lambda i, o: hip.upsample_trilinear2x_fwd_h16(i, Cc, sp, compute, out=o), x16, B8),
        "upsample_trilinear2x_bwd_h16": (lambda i, o: hip.upsample_trilinear2x_bwd_h16(i, Cc, sp, compute, out=o), up16, B),
        "space_to_depth2_h16": (lambda i, o: hip.s2d_h16(i, sh, compute, True, out=o), x16, (N, Cc, S // 8, 8)),
        "depth_to_space2_h16": (lambda i, o: hip.s2d_h16(i, sh, compute, False, out=o), s2d16, B),
        "act16_channel_scale": (lambda i, o: hip.act16_channel_scale(i, torch.ones(N * Cc), Cc, compute, out=o), x16, B),
    }
    for name, (call, t16, osh) in calls.items():
        sides = [("output", good, lay)] + ([("input", lay, good)] if t16 is not None else [])
        for side, lay_in, lay_out in sides:
            i = None if t16 is None else hip.slot(t16, **lay_in)
            o = hip.slot(osh, dtype=dt, **lay_out)
            with pytest.raises(RuntimeError, match="-> -1 "):
                call(i, o)
            torch.cuda.synchronize()
            o.assert_untouched(f"{name} ({side} slot {bad})")
    # c8 input, fp32 output
    for name, call in {"conv3d_fwd_h16": lambda i, o: hip.conv3d_fwd_h16(i, Cc, sp, w, b, compute=compute, out=o),
                       "conv3d_bwd_data_h16": lambda i, o: hip.conv3d_bwd_data_h16(i, Cc, w, sh, compute, out=o),
                       "act16_unpack": lambda i, o: hip.act16_unpack(i, Cc, sp, compute, out=o),
                       "act16_unpack_scaled": lambda i, o: hip.act16_unpack_scaled(i, Cc, sp, compute, 0.5, out=o)}.items():
        o = hip.slot(sh, c_pre=4, c_post=4)
        with pytest.raises(RuntimeError, match="-> -1 "):
            call(hip.slot(x16, **lay), o)
        torch.cuda.synchronize()
        o.assert_untouched(name)
    # c8 operands, small dense fp32 results (weight gradients, statistics partials): the status, on either operand
    for name, call in {"conv3d_bwd_weight_h16": lambda a, g: hip.conv3d_bwd_weight_h16(a, g, dy, Cc, Cc, sp, compute),
                       "conv3d_bwd_weight_c8": lambda a, g: hip.conv3d_bwd_weight_c8(a, g, Cc, Cc, sp, compute),
                       "conv_transpose3d_bwd_weight_h16": lambda a, g: hip.convt_bwd_weight_h16(a, g, sh, Cc, compute)}.items():
        g16 = up16 if name.startswith("conv_transpose") else dy16
        for lay_a, lay_g in ((lay, good), (good, lay)):
            with pytest.raises(RuntimeError, match="-> -1 "):
                call(hip.slot(x16, **lay_a), hip.slot(g16, **lay_g))
    with pytest.raises(RuntimeError, match="-> -1 "):
        hip.act16_channel_partials(hip.slot(x16, **lay), Cc, compute)


def test_ops_compacts_views_the_pair_kernels_reject():
    """ops.space_to_depth2 / depth_to_space2 / norm_act_pool on a caller's view that is dense but starts at an odd element
    offset (4-byte aligned pointer: m355_space_to_depth2 and m355_norm_act_pool_fwd reject it) compute what they compute
    on an aligned copy, forward and backward, instead of failing; the same for a misaligned depth-to-space destination."""
    from segmentation_pipeline_amd import ops

    def odd_view(t):
        flat = torch.empty(t.numel() + 1, device="cuda")
        v = flat[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 8 == 4
        return v
    x = rnd(2, 3, 4, 6, 8, seed=1).cuda()
    xa, xo = x.clone().requires_grad_(), odd_view(x).requires_grad_()
    ya, yo = ops.space_to_depth2(xa), ops.space_to_depth2(xo)
    assert torch.equal(ya, yo)
    g = rnd(*ya.shape, seed=2).cuda()
    ya.backward(g)
    yo.backward(g)
    assert torch.equal(xa.grad, xo.grad)
    pa, po = ya.detach().clone().requires_grad_(), odd_view(ya.detach()).requires_grad_()
    buf = torch.zeros(2 * 7 * 192 + 1, device="cuda")
    slot_buf = buf[1:].view(2, 7, 4, 6, 8)
    assert slot_buf.data_ptr() % 8 == 4
    za, zo = ops.depth_to_space2(pa), ops.depth_to_space2(po, out=ops.OutSlot(slot_buf, 2, 5))
    assert torch.equal(za, x) and torch.equal(zo, x) and torch.equal(slot_buf[:, 2:5], x)
    assert torch.count_nonzero(slot_buf[:, :2]) == 0 and torch.count_nonzero(slot_buf[:, 5:]) == 0 and buf[0] == 0
    gx = odd_view(rnd(*x.shape, seed=3).cuda())       # (the gradient of d2s is s2d: its full-resolution side is the gradient)
    za.backward(gx)
    zo.backward(gx)
    assert torch.equal(pa.grad, po.grad)
    # norm + activation + pool: misaligned input and a misaligned destination
    gamma, beta = (rnd(3, seed=4) * 0.5 + 1.0).cuda(), (rnd(3, seed=5) * 0.1).cuda()
    cfg = ops.NormCfg(groups=3, eps=1e-5, act=1)
    ya, pa_ = ops.norm_act_pool(x, gamma, beta, cfg)
    buf.zero_()
    cfg_o = ops.NormCfg(groups=3, eps=1e-5, act=1, out=ops.OutSlot(slot_buf, 2, 5))
    yo, po_ = ops.norm_act_pool(odd_view(x), gamma, beta, cfg_o)
    assert torch.equal(ya, yo) and torch.equal(pa_, po_) and torch.equal(slot_buf[:, 2:5], ya)
    assert torch.count_nonzero(slot_buf[:, :2]) == 0 and torch.count_nonzero(slot_buf[:, 5:]) == 0 and buf[0] == 0
