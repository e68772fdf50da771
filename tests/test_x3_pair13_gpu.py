"""The lone 27th tap of the split fp32 kernel (conv3_f32x3_kernel, M355_COMPUTE_F32X3).

K = 16 of one v_mfma_f32_32x32x16_bf16 is 8 channels x 2 taps, so the 27 taps run as 14 tap pairs and pair 13 holds
tap (2, 2, 2) alone.  Its second K-half carries a second plane product of the SAME tap: three MFMAs

    weights lo | hi   x  activations hi | lo       (lo, hi) + (hi, lo)
    weights hi | mid  x  activations mid | mid     (hi, mid) + (mid, mid)
    weights hi | mid  x  activations hi | hi       (hi, hi) + (mid, hi)

instead of six against a zero K-half.  These tests isolate that pair (a wrong plane in either K-half shows as an error
of 2^-8 or 2^-16 of a term, not 2^-24), run every instantiated <NTW, GX> on one-chunk / odd-chunk-count inputs, cubes and
ragged volumes with strided batches, check the epilogues behind the shorter pair step, and read the packed weights back.
The reference of every comparison is a float64 torch convolution (or its gradient) of the same inputs.

In the data gradient the logical filter is W'[m][k][t] = w[k][m][26 - t]: ITS tap 26 is tap (0, 0, 0) of w, its K
(chunked) channels are w's output channels and its rows w's input channels -- the data-gradient cases below are laid out
by those roles.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

X3 = 3   # M355_COMPUTE_F32X3
FAMILY_X3 = 7   # plan code of conv3_f32x3_kernel


def rnd(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def fwd64(x, w):
    return F.conv3d(x.double(), w.double(), padding=1)


def dgrad64(dy, w):
    return F.conv_transpose3d(dy.double(), w.double(), padding=1)


# ------------------------------------------------------------------------------------------- the pair in isolation
def hard_operands(kc, mc, D, H, W, seed):
    """test_conv3d_f32x3_split_is_exact_on_hard_operands' generator: all 24 significant bits in use, magnitudes
    2^-20 .. 2^20 per K-channel (the weights carry the inverse range), signed zeros.  -> (activations [1, kc, D, H, W],
    weights as [mc, kc, 3, 3, 3])"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(1, kc, D, H, W, generator=g) * (2.0 ** torch.randint(-20, 21, (1, kc, 1, 1, 1), generator=g).float())
    a[0, 3, 1, 2, 5] = 0.0
    a[0, 4, 1, 2, 5] = -0.0
    w = torch.randn(mc, kc, 3, 3, 3, generator=g) * (2.0 ** -torch.randint(-20, 21, (1, kc, 1, 1, 1), generator=g).float()) / 20
    return a, w


@pytest.mark.parametrize("form", ["fwd", "dgrad"])
@pytest.mark.parametrize("mode", ["tap26-alone", "tap26-zero"])
def test_lone_tap_in_isolation(hip, form, mode):
    """Weights that are zero except at the lone tap of the form (pair 13 only), and weights whose lone tap is zero (pairs
    0 .. 12 only), on operands a bf16 rounding would destroy: |err| < 1e-5 of the sum of |terms| of each output."""
    kc, mc, D, H, W = 32, 32, 4, 6, 32   # 32 rows either way: no 16-row remainder tile
    a, w = hard_operands(kc, mc, D, H, W, seed=7 if form == "fwd" else 8)
    lone = (2, 2, 2) if form == "fwd" else (0, 0, 0)
    keep = torch.zeros(3, 3, 3, dtype=torch.bool)
    keep[lone] = True
    if mode == "tap26-zero":
        keep = ~keep
    w = w * keep
    if form == "fwd":
        assert hip.conv_plan(tuple(a.shape), mc, compute=X3)[0] == FAMILY_X3
        got = hip.conv3d_fwd(a, w, compute=X3).cpu().double()
        ref, scale = fwd64(a, w), fwd64(a.abs(), w.abs())
    else:
        wt = w.transpose(0, 1).contiguous()   # [K = Cout_w, M = Cin_w, 3, 3, 3]
        xsh = (1, mc, D, H, W)
        assert hip.conv_plan(xsh, kc, compute=X3, which=1)[0] == FAMILY_X3
        got = hip.conv3d_bwd_data(a, wt, xsh, compute=X3).cpu().double()
        ref, scale = dgrad64(a, wt), dgrad64(a.abs(), wt.abs())
    assert float(ref.abs().max()) > 0
    rel = float(((got - ref).abs() / scale.clamp_min(1e-300)).max())
    print(f"{form} {mode}: max |err| / sum |terms| = {rel:.3e}")
    assert rel < 1e-5


# ------------------------------------------------------------------------------------ every instantiated <NTW, GX>
VOLUMES = {8: [(8, 8, 8), (5, 6, 7)], 16: [(8, 8, 16), (5, 6, 31)], 32: [(8, 8, 32), (5, 6, 62)]}   # the W that selects GX


def rel_err(a, ref):
    return float((a.cpu().double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("gx", [8, 16, 32])
@pytest.mark.parametrize("ntw", [1, 2, 4])
def test_every_tile_variant(hip, tuning, ntw, gx):
    """NTW 1 / 2 / 4 x GX 8 / 16 / 32; K-channels 8 (one chunk), 24 (odd chunk count: the chunk boundary inside the ring
    of weight slots) and 32; 32 and 64 rows; a cube and a ragged volume whose last tap reaches the zero padding on all
    three faces; N = 2 in strided slots with guard canaries.  Forward and data gradient: max |err| / max |result| within
    3x of the fp32 MFMA kernel's on the same inputs and below 3e-6."""
    tuning(M355_CONV_NTW=ntw)
    N = 2
    for (D, H, W) in VOLUMES[gx]:
        for kc in (8, 24, 32):
            for mc in (32, 64):
                ash, rsh = (N, kc, D, H, W), (N, mc, D, H, W)
                a = torch.relu(rnd(*ash, seed=1))
                w = rnd(mc, kc, 3, 3, 3, seed=2) * (1.0 / (27 * kc) ** 0.5)
                wt = w.transpose(0, 1).contiguous()
                refs = {"fwd": fwd64(a, w), "dgrad": dgrad64(a, wt)}
                for form in ("fwd", "dgrad"):
                    errs = {}
                    for compute in (X3, 0):
                        src = hip.slot(a, c_pre=1, c_post=2, extra=3)
                        out = hip.slot(rsh, c_pre=2, c_post=1, extra=5)
                        if form == "fwd":
                            plan = hip.conv_plan(ash, mc, compute=compute, xbs=src.bs, ybs=out.bs)
                            hip.conv3d_fwd(src, w, compute=compute, out=out)
                        else:
                            plan = hip.conv_plan(rsh, kc, compute=compute, which=1, xbs=out.bs, ybs=src.bs)
                            hip.conv3d_bwd_data(src, wt, rsh, compute=compute, out=out)
                        what = f"{form} <{ntw},{gx}> {kc}->{mc} @{D}x{H}x{W} compute {compute}"
                        if compute == X3:
                            assert plan[:3] == (FAMILY_X3, ntw, gx), (what, plan)
                        src.assert_unchanged(what)
                        errs[compute] = rel_err(out.check_output(what), refs[form])
                    e3, e0 = errs[X3], errs[0]
                    assert e3 <= max(3.0 * e0, 2e-6) and e3 < 3e-6, \
                        f"{what}: split kernel {e3:.2e} vs fp32 MFMA {e0:.2e} (relative to max |fp64 result|)"


# ------------------------------------------------------------------------------------------------------ epilogues
def test_split_k(hip, tuning):
    """three chunks over two splits (2 + 1): the slabs of both splits hold a lone-tap step"""
    tuning(M355_CONV_KSPLIT=2)
    N, kc, mc, D, H, W = 2, 24, 32, 5, 6, 31
    a, w = torch.relu(rnd(N, kc, D, H, W, seed=1)), rnd(mc, kc, 3, 3, 3, seed=2) * (1.0 / (27 * kc) ** 0.5)
    wt = w.transpose(0, 1).contiguous()
    assert hip.conv_plan((N, kc, D, H, W), mc, compute=X3)[::3] == (FAMILY_X3, 2)
    assert hip.conv_plan((N, mc, D, H, W), kc, compute=X3, which=1)[::3] == (FAMILY_X3, 2)
    for name, got, got0, ref in (
            ("fwd", hip.conv3d_fwd(a, w, compute=X3), hip.conv3d_fwd(a, w), fwd64(a, w)),
            ("dgrad", hip.conv3d_bwd_data(a, wt, (N, mc, D, H, W), compute=X3), hip.conv3d_bwd_data(a, wt, (N, mc, D, H, W)),
             dgrad64(a, wt))):
        e3, e0 = rel_err(got, ref), rel_err(got0, ref)
        assert e3 <= max(3.0 * e0, 2e-6) and e3 < 3e-6, f"{name}: split kernel {e3:.2e} vs fp32 MFMA {e0:.2e}"


def test_fused_statistics_partials(hip, tuning):
    """the GroupNorm statistics epilogue: the (sum, sum of squares) partials per channel add up to the sums of the
    float64 result (rtol 1e-4, atol 1e-3: the tolerance of the c8 kernels' partials test)"""
    tuning(M355_CONV_KSPLIT=1)
    N, kc, mc, D, H, W = 2, 24, 64, 5, 6, 31
    x, w, b = torch.relu(rnd(N, kc, D, H, W, seed=1)), rnd(mc, kc, 3, 3, 3, seed=2) * (1.0 / (27 * kc) ** 0.5), rnd(mc, seed=3)
    xg, wg, bg = hip.to(x), hip.to(w), hip.to(b)
    d = hip.conv_desc(x.shape, mc, 3, 1, 1, compute=X3)
    assert hip.conv_plan(tuple(x.shape), mc, compute=X3)[::3] == (FAMILY_X3, 1)
    slots = hip.fn("conv3d_stats_slots")(C.byref(d))
    assert slots > 0
    y, part = hip.empty(N, mc, D, H, W), hip.empty(N, slots, mc, 2)
    ws = hip._ws("conv3d_fwd_workspace", d)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    hip._chk(hip.fn("conv3d_fwd_stats")(C.byref(d), ptr(xg), ptr(wg), ptr(bg), None, ptr(y), ptr(part), ptr(ws), ws.numel(),
                                        hip._stream()), "conv3d_fwd_stats")
    ref = fwd64(x, w) + b.double().view(1, -1, 1, 1, 1)
    e3, e0 = rel_err(y, ref), rel_err(hip.conv3d_fwd(x, w, b), ref)
    assert e3 <= max(3.0 * e0, 2e-6) and e3 < 3e-6, f"y: split kernel {e3:.2e} vs fp32 MFMA {e0:.2e}"
    torch.testing.assert_close(part[..., 0].sum(dim=1).cpu().double(), ref.sum(dim=(2, 3, 4)), rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(part[..., 1].sum(dim=1).cpu().double(), (ref ** 2).sum(dim=(2, 3, 4)), rtol=1e-4, atol=1e-3)


# ------------------------------------------------------------------------------------------------- packed weights
def pair_tap(pair, half):
    if pair < 9:
        return pair * 3 + half
    if pair < 12:
        return (pair - 9) * 9 + half * 3 + 2
    return half * 9 + 8 if pair == 12 else 26


def split3(v):
    """hi = trunc16(v), mid = trunc16(v - hi), lo = v - hi - mid -> the three as bf16 bit patterns (int32 tensors)"""
    top = lambda t: t.contiguous().view(torch.int32) & -65536
    hi = top(v)
    r1 = v - hi.view(torch.float32)
    mid = top(r1)
    lo = (r1 - mid.view(torch.float32)).contiguous().view(torch.int32)
    assert bool(((lo & 0xFFFF) == 0).all()), "the remainder fits 8 bits"
    return [(t >> 16) & 0xFFFF for t in (hi, mid, lo)]


def expected_pack(w, transpose):
    """[tile][chunk][pair][item][lane][8 channels] bf16 bit patterns of the 32-row tiles"""
    wl = (w.transpose(0, 1).flip(2, 3, 4) if transpose else w).reshape(-1, w.shape[1 - int(transpose)], 27)   # [row][K][tap]
    M, K = wl.shape[:2]
    otiles, nchunks = (M + 31) // 32, (K + 7) // 8
    wp = torch.zeros(otiles * 32, nchunks * 8, 27)
    wp[:M, :K] = wl
    hi, mid, lo = [t.view(otiles, 32, nchunks, 8, 27) for t in split3(wp)]
    out = torch.zeros(otiles, nchunks, 14, 3, 64, 8, dtype=torch.int32)
    for pair in range(14):
        for half in (0, 1):
            t = pair_tap(pair, half)
            h, m, l = [p[..., t].permute(0, 2, 1, 3) for p in (hi, mid, lo)]   # [tile][chunk][row][8]
            items = (h, m, l) if pair < 13 else ((h, h, l) if half == 0 else (m, m, h))
            for i, v in enumerate(items):
                out[:, :, pair, i, 32 * half:32 * half + 32] = v
    return out


def test_packed_weights(hip, tuning):
    """m355_conv3d_pack read back: pairs 0 .. 12 are hi / mid / lo of their two taps, pair 13 is hi | mid, hi | mid, lo | hi of
    tap 26 (lower | upper lane half); forward and data-gradient forms; the batched pack writes the same bytes."""
    tuning(M355_TILE16=0)   # (8 rows in the data-gradient form of Cin 8: on a padded 32-row tile, the layout under test)
    cases = []
    for ci in (8, 24):
        w = rnd(32, ci, 3, 3, 3, seed=20 + ci)
        for which in (0, 1):
            cases.append((w, (1, ci, 8, 8, 8), which, X3))
    batch = hip.pack_weights_batch(cases)
    for (w, xsh, which, _), bbuf in zip(cases, batch):
        buf = hip.pack_weights(w, xsh, which, X3)
        torch.cuda.synchronize()
        assert torch.equal(bbuf, buf), ("batch pack", tuple(w.shape), which)
        exp = expected_pack(w, transpose=bool(which))
        got = buf[:exp.numel() * 2].cpu().view(torch.int16).to(torch.int32) & 0xFFFF
        got = got.view(exp.shape)
        for pair in range(14):
            assert torch.equal(got[:, :, pair], exp[:, :, pair]), (tuple(w.shape), "which", which, "pair", pair)
