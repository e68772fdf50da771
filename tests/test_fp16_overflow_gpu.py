"""The overflow word of the fp16 training flow, kernel by kernel (include/m355seg.h m355_overflow_flag_set, csrc/common.hpp).

Every kernel that writes a loss-scaled gradient as fp16 stores values past +-65504 as exactly +-65504 and ORs bit 0 into
the word; every epilogue that removes the loss scale from a parameter gradient ORs bit 1 when the result is not finite,
whatever the unscale factor (1.0 included).  Each case runs the kernel on small seeded inputs, N = 2 or ragged channel
counts, and compares with a float64 reference of the same operation on the 16-bit operand values, clamped to +-65504 and
rounded to fp16 in the test:

  in range   outputs == reference (one rounding), word == 0
  overflow   a few inputs are scaled so that a known set of outputs lands past 65504: those are exactly +-65504 (never
             inf), every other output still matches, word == 1 exactly
  NaN        a NaN input stays NaN in exactly the outputs it reaches (nowhere else).  A NaN is NOT a clamped value: it
             does not set bit 0 (it is reported as bit 1 where it reaches a parameter gradient, see the bit-1 tests).

bf16 (same inputs): the word stays 0 and nothing is clamped -- bf16 has fp32's exponent range.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F16_MAX = 65504.0
UNSCALES = [2.0 ** -7, 1.0, 2.0]


def rnd(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _dt(compute):
    return torch.bfloat16 if compute == 1 else torch.float16


def _ulp(compute):
    return 2.0 ** -8 if compute == 1 else 2.0 ** -11


def _c8_to_ncdhw(x16, Cc, spatial):
    N, CB, S, _ = x16.shape
    return x16.double().cpu().permute(0, 1, 3, 2).reshape(N, CB * 8, S)[:, :Cc].reshape(N, Cc, *spatial)


def _r(t, compute):
    """the 16-bit value of an fp32 operand, as float64 (fp16: inputs of the tests stay inside its range)"""
    return t.to(_dt(compute)).double()


def check(got, ref, compute, atol_rel, what, expect_over=None):
    """got: kernel output (float64, cpu); ref: float64 reference BEFORE clamping / rounding.
    atol_rel: absolute slack relative to the largest in-range reference value (the fp32 accumulation of the kernel)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nan_ref = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan_ref), \
        f"{what}: NaN in {int(torch.isnan(got).sum())} outputs, reference reaches {int(nan_ref.sum())}"
    assert not torch.isinf(got).any(), f"{what}: {int(torch.isinf(got).sum())} outputs are inf"
    fin = ~nan_ref
    lim = F16_MAX if compute == 2 else float("inf")
    over = fin & (ref.abs() > lim * 1.002)            # clearly past the range: the fp32 value was too
    if expect_over is not None:
        assert int(over.sum()) > 0 if expect_over else not over.any(), f"{what}: test inputs do not do what they should"
    if over.any():
        assert torch.equal(got[over], torch.sign(ref[over]) * F16_MAX), f"{what}: overflowed outputs not saturated"
    rest = fin & ~over
    want = ref[rest].clamp(-lim, lim)
    scale = ref[rest].abs().max().item() if rest.any() else 0.0
    bad = (got[rest] - want).abs() > _ulp(compute) * want.abs() * 1.01 + atol_rel * scale
    assert not bad.any(), f"{what}: {int(bad.sum())} outputs off, worst {(got[rest] - want).abs().max().item():.3e}"


# ------------------------------------------------------------------------------------------ kernels writing fp16 (bit 0)
# each: (hip, oracle, compute, mode) -> (got, ref, atol_rel); mode in {"in", "over", "nan"}.  The word is cleared right
# before the call under test (packing the inputs must not count).

def k_pack_scaled(hip, oracle, compute, mode, take):
    x = rnd(2, 13, 3, 5, 7, seed=1)
    if mode == "over":
        x[0, 0, 0, 0, 0], x[1, 12, 2, 4, 6], x[1, 5, 1, 1, 1] = 100.0, -100.0, 70.0
    elif mode == "nan":
        x[1, 3, 1, 2, 3] = float("nan")
    scale = 2.0 ** 10
    take()
    x16 = hip.act16_pack_scaled(x, compute, scale)
    return _c8_to_ncdhw(x16, 13, (3, 5, 7)), x.double() * scale, 0.0


def k_channel_scale(hip, oracle, compute, mode, take):
    N, Cc, S3 = 2, 13, (3, 5, 7)
    x = rnd(N, Cc, *S3, seed=1)
    if mode == "over":
        x[0, 0, 0, 0, 0], x[1, 6, 2, 4, 6] = 30000.0, -20000.0
    elif mode == "nan":
        x[0, 9, 1, 1, 1] = float("nan")
    scale = torch.where(rnd(N * Cc, seed=2) > -0.5, torch.tensor(4.0), torch.tensor(0.0))
    scale[0] = scale[Cc + 6] = 4.0
    scale[1] = 1.25
    if mode == "nan":
        scale[9] = 4.0
    x16 = hip.act16_pack(x, compute)
    take()
    y16 = hip.act16_channel_scale(x16, scale, Cc, compute)
    return _c8_to_ncdhw(y16, Cc, S3), _c8_to_ncdhw(x16, Cc, S3) * scale.double().view(N, Cc, 1, 1, 1), 0.0


def _unpool(t):
    return 0.125 * t.repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)


def k_avgpool_bwd(hip, oracle, compute, mode, take, skip=True):
    N, Cc, D, H, W = 2, 13, 4, 6, 8
    dp, sk = rnd(N, Cc, D // 2, H // 2, W // 2, seed=1), rnd(N, Cc, D, H, W, seed=2)
    if mode == "over":
        dp[0, 1, 0, 0, 0], sk[0, 1, 1, 0, 1] = 60000.0, 60000.0
        dp[1, 12, 1, 2, 3], sk[1, 12, 3, 5, 7] = -40000.0, -62000.0
    elif mode == "nan":
        dp[1, 4, 1, 1, 1] = float("nan")
        sk[0, 7, 2, 3, 4] = float("nan")
    dp16, sk16 = hip.act16_pack(dp, compute), hip.act16_pack(sk, compute)
    take()
    got = hip.avgpool_bwd_h16(dp16, sk16 if skip else None, Cc, (D, H, W), compute)
    ref = _unpool(_r(dp, compute)) + (_r(sk, compute) if skip else 0.0)
    return _c8_to_ncdhw(got, Cc, (D, H, W)), ref, 0.0


def k_upsample_bwd(hip, oracle, compute, mode, take):
    N, Cc, D, H, W = 2, 13, 3, 4, 5
    dy = rnd(N, Cc, 2 * D, 2 * H, 2 * W, seed=2)
    if mode == "over":
        dy[0, 2, 1:5, 2:6, 3:7] = 30000.0
        dy[1, 10, 0:2, 0:3, 0:2] = -30000.0
    elif mode == "nan":
        dy[1, 5, 3, 3, 3] = float("nan")
    dy16 = hip.act16_pack(dy, compute)
    take()
    dx16 = hip.upsample_trilinear2x_bwd_h16(dy16, Cc, (D, H, W), compute)
    x = torch.zeros(N, Cc, D, H, W, dtype=torch.float64, requires_grad=True)
    up = F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=True)
    up.backward(_r(dy, compute))
    return _c8_to_ncdhw(dx16, Cc, (D, H, W)), x.grad, 1e-6


NORM_CASES = [(2, 13, 4, 6, 8, 0, 1), (2, 16, 4, 6, 8, 4, 0)]     # (N, C, D, H, W, groups, act): BatchNorm / GroupNorm


def _norm_inputs(case, mode):
    N, Cc, D, H, W, groups, act = case
    x, dy = rnd(N, Cc, D, H, W, seed=1), rnd(N, Cc, D, H, W, seed=6)
    dp = rnd(N, Cc, D // 2, H // 2, W // 2, seed=7)
    gamma, beta = (rnd(Cc, seed=2) * 0.5 + 1.0) * 8.0, rnd(Cc, seed=3) * 0.1
    if mode == "over":                                    # |dx| ~ gamma * rstd * |g|: well past the range in places
        dy, dp, gamma = dy * 8000.0, dp * 15000.0, gamma * 4.0
    elif mode == "nan":
        act = 0                                           # (no activation mask: the NaN reaches its whole group)
        dy[1, 3, 1, 2, 3] = float("nan")
    return (N, Cc, D, H, W, groups, act), x, dy, dp, gamma, beta


def k_norm_act_bwd_c8(hip, oracle, compute, mode, take, case, src):
    (N, Cc, D, H, W, groups, act), x, dy, dp, gamma, beta = _norm_inputs(case, mode)
    x16 = hip.act16_pack(x, compute)
    dy16 = hip.act16_pack(dy, compute) if src in ("dy", "both") else None
    dp16 = hip.act16_pack(dp, compute) if src in ("pool", "both") else None
    xr = _r(x, compute).float()
    g = torch.zeros(N, Cc, D, H, W, dtype=torch.float64)
    if dy16 is not None:
        g = g + _r(dy, compute)
    if dp16 is not None:
        g = g + _unpool(_r(dp, compute))
    mean, rstd = oracle.norm_stats(xr, groups)[:2]
    ref = _norm_bwd_ref(xr.double(), g, mean.double(), rstd.double(), gamma.double(), beta.double(), groups, act)
    take()
    dx16, _, _ = hip.norm_act_bwd_c8(x16, dy16, dp16, Cc, (D, H, W), mean, rstd, gamma, beta, groups, act, compute)
    return _c8_to_ncdhw(dx16, Cc, (D, H, W)), ref, 2e-5


def k_norm_act_bwd_h16(hip, oracle, compute, mode, take, case):
    (N, Cc, D, H, W, groups, act), x, dy, dp, gamma, beta = _norm_inputs(case, mode)
    mean, rstd = oracle.norm_stats(x, groups)[:2]
    ref = _norm_bwd_ref(x.double(), dy.double(), mean.double(), rstd.double(), gamma.double(), beta.double(), groups, act)
    take()
    _, _, _, dx16 = hip.norm_act_bwd_h16(x, dy, mean, rstd, gamma, beta, groups, act, compute)
    return _c8_to_ncdhw(dx16, Cc, (D, H, W)), ref, 2e-5


def _norm_bwd_ref(x, g, mean, rstd, gamma, beta, groups, act, slope=0.01):
    """float64 data gradient of y = act(gamma * (x - mean) * rstd + beta) with training-mode statistics (BatchNorm:
    groups 0, per channel over (N, S); GroupNorm: per (n, group)); act 0 none, 1 ReLU, 2 LeakyReLU"""
    N, Cc = x.shape[:2]
    xs = x.reshape(N, Cc, -1)
    gs = g.reshape(N, Cc, -1)
    if groups == 0:
        m, r = mean.view(1, Cc, 1), rstd.view(1, Cc, 1)
    else:
        m = mean.view(N, groups, 1).repeat_interleave(Cc // groups, 1)
        r = rstd.view(N, groups, 1).repeat_interleave(Cc // groups, 1)
    xhat = (xs - m) * r
    pre = gamma.view(1, Cc, 1) * xhat + beta.view(1, Cc, 1)
    if act == 1:
        gs = torch.where(pre > 0, gs, torch.zeros_like(gs))
    elif act == 2:
        gs = torch.where(pre > 0, gs, gs * slope)
    gh = gs * gamma.view(1, Cc, 1)                        # dL/dxhat
    cg = Cc // groups if groups else 1

    def red(t):                                           # mean over the statistics' population, broadcast back
        if groups == 0:
            return t.mean(dim=(0, 2), keepdim=True)
        return t.reshape(N, groups, -1).mean(dim=2, keepdim=True).repeat_interleave(cg, 1)
    dx = r * (gh - red(gh) - xhat * red(gh * xhat))
    return dx.reshape(x.shape)


def k_conv_bwd_data(hip, oracle, compute, mode, take, case):
    N, ci, co, D, H, W = case
    dy = rnd(N, co, D, H, W, seed=2)
    w = rnd(co, ci, 3, 3, 3, seed=3) * 0.1
    w[0] += 3.0
    w[min(1, co - 1)] += 3.0
    if mode == "over":
        dy[N - 1, 0, D // 2, H // 2, W // 2] = 30000.0
        dy[0, min(1, co - 1), 0, H - 1, W - 2] = -30000.0
    elif mode == "nan":
        dy[N - 1, co - 1, D - 1, 1, W // 3] = float("nan")
    dy16 = hip.act16_pack(dy, compute)
    take()
    dx16 = hip.conv3d_bwd_data_h16_c8(dy16, co, w, (N, ci, D, H, W), compute)
    ref = F.conv_transpose3d(_r(dy, compute), _r(w, compute), padding=1)
    return _c8_to_ncdhw(dx16, ci, (D, H, W)), ref, 3e-5


def k_convt_bwd_data(hip, oracle, compute, mode, take, case):
    N, ci, co, D, H, W = case
    assert hip.convt_h16_bwd_supported((N, ci, D, H, W), co)
    dy = rnd(N, co, 2 * D, 2 * H, 2 * W, seed=2)
    w = rnd(ci, co, 2, 2, 2, seed=3) * 0.2
    w[:, 0] += 3.0
    w[:, 1] += 3.0
    if mode == "over":
        dy[N - 1, 0, 2:4, 4:6, 0:2] = 30000.0
        dy[0, 1, 0:2, 2:4, 2 * W - 2:] = -30000.0
    elif mode == "nan":
        dy[N - 1, co - 1, 3, 1, 2 * W - 1] = float("nan")
    dy16 = hip.act16_pack(dy, compute)
    take()
    dx16 = hip.convt_bwd_data_h16(dy16, w, (N, ci, D, H, W), compute)
    ref = F.conv3d(_r(dy, compute), _r(w, compute), stride=2)
    return _c8_to_ncdhw(dx16, ci, (D, H, W)), ref, 3e-5


CONV_CASES = [(2, 13, 16, 5, 6, 20),      # ragged dx channels, N = 2
              (1, 40, 24, 4, 8, 32),      # two channel tiles of dx
              (2, 11, 3, 4, 7, 33)]       # <= 4 K-channels: conv3_c4_h16_kernel
CONV_PLANS = {"default": {},
              "persistent": {"M355_CONV_SLOTS": "5", "M355_H16_ONESHOT": "3"},
              "oneshot": {"M355_H16_ONESHOT": "2", "M355_CONV_KSPLIT": "1"},
              "splitk": {"M355_CONV_KSPLIT": "2", "M355_CONV_SLOTS": "5", "M355_H16_ONESHOT": "3"},
              "ntw1": {"M355_CONV_NTW": "1"}}
CONVT_CASES = [(2, 13, 24, 3, 5, 6), (1, 64, 32, 4, 4, 18)]

BIT0 = {
    "act16_pack_scaled": k_pack_scaled,
    "act16_channel_scale": k_channel_scale,
    "avgpool3d_2x_bwd_h16": k_avgpool_bwd,
    "upsample_trilinear2x_bwd_h16": k_upsample_bwd,
}
for _i, _c in enumerate(NORM_CASES):
    for _src in ("dy", "pool", "both"):
        BIT0[f"norm_act_bwd_c8-{_i}-{_src}"] = (lambda c, s: lambda *a: k_norm_act_bwd_c8(*a, case=c, src=s))(_c, _src)
    BIT0[f"norm_act_bwd_h16-{_i}"] = (lambda c: lambda *a: k_norm_act_bwd_h16(*a, case=c))(_c)
for _i, _c in enumerate(CONVT_CASES):
    BIT0[f"conv_transpose3d_bwd_data_h16-{_i}"] = (lambda c: lambda *a: k_convt_bwd_data(*a, case=c))(_c)


def test_fp16_avgpool_bwd_without_skip(hip, oracle):
    """without the skip gradient the pool backward is 0.125 * dp: it cannot overflow (in range and NaN only)"""
    for mode in ("in", "nan"):
        _run_bit0(hip, oracle, 2, mode, lambda *a: k_avgpool_bwd(*a, skip=False), f"avgpool3d_2x_bwd_h16 no skip {mode}")


def _run_bit0(hip, oracle, compute, mode, fn, what):
    with hip.overflow_word() as take:
        got, ref, atol = fn(hip, oracle, compute, mode, take)
        word = take()
    if compute == 2 and mode == "over":
        check(got, ref, compute, atol, what, expect_over=True)
        assert word == 1, f"{what}: overflow word {word}, want 1 (a value was clamped)"
    elif mode == "nan":
        check(got, ref, compute, atol, what)
        assert word & 1 == 0, f"{what}: a NaN set bit 0 of the overflow word ({word})"
    else:
        check(got, ref, compute, atol, what, expect_over=False)
        assert word == 0, f"{what}: overflow word {word} on in-range values"


@pytest.mark.parametrize("mode", ["in", "over", "nan"])
@pytest.mark.parametrize("name", sorted(BIT0))
def test_fp16_gradient_kernels_saturate_and_report(hip, oracle, name, mode):
    _run_bit0(hip, oracle, 2, mode, BIT0[name], f"{name} fp16 {mode}")


@pytest.mark.parametrize("mode", ["in", "over", "nan"])
@pytest.mark.parametrize("plan", sorted(CONV_PLANS))
def test_fp16_conv_data_gradient_saturates_and_reports(hip, oracle, tuning, plan, mode):
    """m355_conv3d_bwd_data_h16_c8 runs the forward kernels (one-shot, persistent, split-K + c8 reduce, the <= 4
    K-channel kernel): every c8 store path saturates and reports"""
    tuning(**CONV_PLANS[plan])
    for case in CONV_CASES:
        _run_bit0(hip, oracle, 2, mode, lambda *a: k_conv_bwd_data(*a, case=case), f"conv3d_bwd_data_h16_c8 {case} {plan} {mode}")


@pytest.mark.parametrize("mode", ["in", "over"])
@pytest.mark.parametrize("name", sorted(BIT0) + ["conv3d_bwd_data_h16_c8"])
def test_bf16_same_inputs_keep_their_range_and_leave_the_word(hip, oracle, name, mode):
    """bf16 (compute = 1) on the inputs of the fp16 cases: nothing is clamped (values past 65504 come out as they are,
    rounded once) and the word stays 0"""
    fn = BIT0.get(name) or (lambda *a: k_conv_bwd_data(*a, case=CONV_CASES[0]))
    with hip.overflow_word() as take:
        got, ref, atol = fn(hip, oracle, 1, mode, take)
        word = take()
    check(got, ref, 1, atol, f"{name} bf16 {mode}")
    assert word == 0
    if mode == "over" and name.startswith(("conv", "act16_pack", "norm_act_bwd_c8-0-both")):
        assert (got.abs() > F16_MAX).any(), "bf16 clamped at the fp16 range"



# ------------------------------------------------------------------------------------ forward activations in fp16
def test_fp16_forward_activation_saturates_without_reporting(hip):
    """The c8 forward of a 3x3x3 conv shares the data gradient's epilogue: in fp16 a forward value past 65504 is stored
    as +-65504 (never inf, which would turn the next normalisation's statistics into NaN), and the word is NOT set --
    it reports loss-scaled gradients, and a lower loss scale would not bring a forward value back into range."""
    N, ci, co, D, H, W = 2, 13, 16, 5, 6, 20
    x = rnd(N, ci, D, H, W, seed=1)
    x[1, 0, 2, 3, 10], x[0, 5, 0, 0, 0] = 30000.0, -30000.0
    w = rnd(co, ci, 3, 3, 3, seed=3) * 0.1
    w[:, 0] += 3.0
    w[:, 5] += 3.0
    with hip.overflow_word() as take:
        x16 = hip.act16_pack(x, 2)
        take()
        y16 = hip.conv3d_fwd_h16_c8(x16, ci, (D, H, W), w, compute=2)
        word = take()
    ref = F.conv3d(_r(x, 2), _r(w, 2), padding=1)
    check(_c8_to_ncdhw(y16, co, (D, H, W)), ref, 2, 3e-5, "conv3d_fwd_h16_c8 fp16", expect_over=True)
    assert word == 0


# ------------------------------------------------------------------------- parameter gradients, loss scale removed (bit 1)
def _nan_in_x(x):
    x = x.clone()
    x[-1, x.shape[1] // 2, 1, 1, 1] = float("nan")
    return x


BW_CASES = [(2, 13, 16, 5, 6, 20), (1, 4, 32, 8, 8, 32), (1, 24, 40, 4, 4, 32)]


@pytest.mark.parametrize("compute", [2, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("unscale", UNSCALES)
def test_conv_weight_gradient_reports_nonfinite(hip, compute, unscale):
    """m355_conv3d_bwd_weight_c8: a NaN in x reaches dw (not the bias gradient) -> bit 1 at every unscale factor,
    1.0 included; finite operands leave the word at 0 and dw == unscale * dw(1) (the bias likewise)"""
    for (N, ci, co, D, H, W) in BW_CASES:
        x, dy = rnd(N, ci, D, H, W, seed=1), rnd(N, co, D, H, W, seed=2)
        with hip.overflow_word() as take:
            x16, dy16 = hip.act16_pack(x, compute), hip.act16_pack(dy, compute)
            take()
            dw1, db1 = hip.conv3d_bwd_weight_c8(x16, dy16, ci, co, (D, H, W), compute)
            dw, db = hip.conv3d_bwd_weight_c8(x16, dy16, ci, co, (D, H, W), compute, unscale=unscale)
            clean = take()
            xn16 = hip.act16_pack(_nan_in_x(x), compute)
            take()
            dwn, dbn = hip.conv3d_bwd_weight_c8(xn16, dy16, ci, co, (D, H, W), compute, unscale=unscale)
            hit = take()
        assert clean == 0, f"{(N, ci, co)}: word {clean} on finite gradients"
        assert torch.equal(dw, dw1 * unscale)
        assert torch.isfinite(dbn).all() and torch.isnan(dwn).any()
        assert hit == 2, f"{(N, ci, co)} unscale {unscale}: word {hit}, want 2 (non-finite weight gradient)"


@pytest.mark.parametrize("compute", [2, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("unscale", UNSCALES)
def test_convt_weight_gradient_reports_nonfinite(hip, compute, unscale):
    """m355_conv_transpose3d_bwd_weight_h16: the same contract as the 3x3x3 weight gradient"""
    for (N, ci, co, D, H, W) in CONVT_CASES:
        x, dy = rnd(N, ci, D, H, W, seed=1), rnd(N, co, 2 * D, 2 * H, 2 * W, seed=2)
        with hip.overflow_word() as take:
            x16, dy16 = hip.act16_pack(x, compute), hip.act16_pack(dy, compute)
            take()
            dw1, _ = hip.convt_bwd_weight_h16(x16, dy16, (N, ci, D, H, W), co, compute)
            dw, _ = hip.convt_bwd_weight_h16(x16, dy16, (N, ci, D, H, W), co, compute, unscale=unscale)
            clean = take()
            xn16 = hip.act16_pack(_nan_in_x(x), compute)
            take()
            dwn, dbn = hip.convt_bwd_weight_h16(xn16, dy16, (N, ci, D, H, W), co, compute, unscale=unscale)
            hit = take()
        assert clean == 0
        torch.testing.assert_close(dw, dw1 * unscale, rtol=1e-6, atol=1e-8)
        assert torch.isfinite(dbn).all() and torch.isnan(dwn).any()
        assert hit == 2, f"{(N, ci, co)} unscale {unscale}: word {hit}, want 2"


@pytest.mark.parametrize("compute", [2, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("unscale", UNSCALES)
def test_norm_parameter_gradients_report_nonfinite(hip, oracle, compute, unscale):
    """m355_norm_act_bwd_c8: a NaN in the pre-norm input reaches dgamma (dbeta stays finite) -> bit 1 at every unscale
    factor; finite operands leave the word at 0"""
    for case in NORM_CASES:
        (N, Cc, D, H, W, groups, act), x, dy, dp, gamma, beta = _norm_inputs(case, "in")
        mean, rstd = oracle.norm_stats(_r(x, compute).float(), groups)[:2]
        with hip.overflow_word() as take:
            x16, dy16 = hip.act16_pack(x, compute), hip.act16_pack(dy, compute)
            take()
            _, dg, db = hip.norm_act_bwd_c8(x16, dy16, None, Cc, (D, H, W), mean, rstd, gamma, beta, groups, 0, compute,
                                            unscale=unscale)
            clean = take()
            xn16 = hip.act16_pack(_nan_in_x(x), compute)
            take()
            _, dgn, dbn = hip.norm_act_bwd_c8(xn16, dy16, None, Cc, (D, H, W), mean, rstd, gamma, beta, groups, 0, compute,
                                              unscale=unscale)
            hit = take()
        assert clean == 0 and torch.isfinite(dg).all() and torch.isfinite(db).all()
        assert torch.isnan(dgn).any() and torch.isfinite(dbn).all()
        assert hit & 2, f"{case} unscale {unscale}: word {hit}, bit 1 not set by a NaN dgamma"
        assert hit & 1 == 0
