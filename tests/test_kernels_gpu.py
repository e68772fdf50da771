"""HIP kernels vs the CPU oracle, called through the C ABI on the same seeded inputs.

fp32 tolerance: the oracle accumulates in double; the kernels in fp32 (MFMA = k-ordered
fma chain).  Per-element bound used here: |err| <= 2e-5 * sum|terms| scale, written as
rtol/atol on the output scale.  Edge cases: ragged sizes that do not divide the tiles,
channels not multiple of 32 (and odd, for the MFMA k-pair), N > 1, tiny volumes, the
split-K path.  Every call here hands over dense, allocator-aligned tensors (batch stride 0), except a
few c8 wrappers with a padded destination: concat-slot batch strides, misaligned pointers and writes
outside a slot are tested kernel by kernel in test_strided_slots_gpu.py (raw_ops.Slot).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def rnd(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def close(a, b, rtol=2e-5, atol=2e-5, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= atol + rtol * ref, f"{what}: max err {err:.3e} (ref scale {ref:.3e})"


CONV3 = [
    # N, Cin, Cout, D, H, W      -- all 3x3x3 / s1 / p1 (MFMA implicit GEMM)
    (1, 4, 32, 16, 16, 32),      # first-layer shape family (Cin=4)
    (1, 32, 32, 8, 16, 64),      # GX=32 tiles
    (2, 5, 7, 9, 10, 33),        # ragged everything, odd Cin (zero k-pair), N=2
    (1, 64, 40, 8, 8, 16),       # GX=16, Cout not multiple of 32
    (1, 96, 32, 8, 8, 8),        # GX=8, concat-sized Cin
    (1, 3, 3, 4, 4, 4),          # tiny: W < 8
    (1, 320, 64, 4, 4, 4),       # deep level: split-K over channel chunks
    (2, 16, 3, 6, 6, 40),        # out-conv family (Cout=3)
    (1, 32, 3, 16, 16, 32),      # out conv on the z-Toeplitz small-Cout forward kernel
    (2, 9, 2, 9, 10, 40),        # same kernel: odd Cin, ragged D/H/W, N=2
]


@pytest.mark.parametrize("case", CONV3)
def test_conv3d_3x3x3_fwd_bwd(hip, oracle, case):
    N, Ci, Co, D, H, W = case
    x, w, b = rnd(N, Ci, D, H, W, seed=1), rnd(Co, Ci, 3, 3, 3, seed=2) * (1.0 / (27 * Ci) ** 0.5), rnd(Co, seed=3)
    add = rnd(N, Co, D, H, W, seed=4)
    scale = 1.0
    close(hip.conv3d_fwd(x, w, b, add), oracle.conv3d_fwd(x, w, b, add), what="fwd")
    close(hip.conv3d_fwd(x, w), oracle.conv3d_fwd(x, w), what="fwd nobias")
    dy = rnd(N, Co, D, H, W, seed=5)
    close(hip.conv3d_bwd_data(dy, w, x.shape), oracle.conv3d_bwd_data(dy, w, x.shape), what="bwd_data")
    dw_h, db_h = hip.conv3d_bwd_weight(x, dy, 3)
    dw_o, db_o = oracle.conv3d_bwd_weight(x, dy, 3)
    close(dw_h, dw_o, 3e-5, 3e-5 * (N * D * H * W) ** 0.5, what="bwd_weight")
    close(db_h, db_o, 3e-5, 3e-5 * (N * D * H * W) ** 0.5, what="dbias")


X3 = 3   # M355_COMPUTE_F32X3: fp32 tensors, the products on the bf16 matrix pipe (exact 3-way split of both operands)
CONV3_X3 = [
    # N, Cin, Cout, D, H, W
    (1, 32, 32, 8, 16, 64),      # forward NTW 4 / GX 32; weight gradient TX 32
    (2, 8, 40, 9, 7, 33),        # ragged everything, N = 2, channel tiles with empty rows
    (1, 96, 32, 12, 16, 16),     # GX / TX 16, concat-sized Cin
    (1, 20, 64, 8, 24, 8),       # GX / TX 8, a chunk with 4 real channels
    (1, 320, 64, 4, 4, 4),       # deep level: split-K over channel chunks, W < 8
    (3, 40, 40, 3, 10, 12),      # the reference's widths (msseg2.py:87), D < 4, several columns per split
    (1, 33, 7, 5, 6, 40),        # Cout < 8
    (1, 32, 32, 1, 2, 32),       # a single z plane
    (1, 32, 32, 2, 2, 32),       # two: every tile opens or closes a column
    (1, 16, 16, 17, 5, 70),      # three x tiles, ragged rows
    (1, 4, 32, 8, 16, 64),       # the first layer's family: half of the one chunk is real
    (2, 5, 33, 6, 7, 20),        # odd channels on both sides
]


@pytest.mark.parametrize("case", CONV3_X3)
def test_conv3d_f32x3_fwd_bwd(hip, oracle, case, tuning):
    """M355_COMPUTE_F32X3 (what precision "fp32" runs on the wide layers): forward (bias + residual), data gradient and
    weight gradient against the C oracle at the fp32 kernels' tolerances, and -- measured against an fp64 convolution --
    as accurate as fp32 arithmetic is: max error within 3x of the fp32 MFMA kernels' and below 2e-6 of max |result| (both
    carry the error of an fp32 accumulation -- stock torch on the CPU sits at 2-6e-7 on these shapes; the dropped plane
    products are below 2^-24 of each product; the split kernels add six partial products per 16 k-values to the accumulator
    where the fp32 MFMA adds eight)."""
    N, Ci, Co, D, H, W = case
    tuning(M355_F32X3_EDGE=1)   # (3..7 K-channels on the split kernel too: opt-in, see x3_layer in conv3d_route.hpp)
    plan = hip.conv_plan((N, Ci, D, H, W), Co, compute=X3)
    assert plan[0] == 7, f"expected conv3_f32x3_kernel for {case}, got family {plan}"
    # (a single z plane has no ring to walk: the weight gradient stays on the fp32 MFMA kernel)
    assert hip.conv_plan((N, Ci, D, H, W), Co, compute=X3, which=2)[0] == ((8 if D >= 2 else 9) if Ci > 4 else 10), "weight-gradient kernel"
    x, w, b = torch.relu(rnd(N, Ci, D, H, W, seed=1)), rnd(Co, Ci, 3, 3, 3, seed=2) * (1.0 / (27 * Ci) ** 0.5), rnd(Co, seed=3)
    add, dy = rnd(N, Co, D, H, W, seed=4), rnd(N, Co, D, H, W, seed=5)
    y3, dx3 = hip.conv3d_fwd(x, w, b, add, compute=X3), hip.conv3d_bwd_data(dy, w, x.shape, compute=X3)
    dw3, db3 = hip.conv3d_bwd_weight(x, dy, 3, compute=X3)
    close(y3, oracle.conv3d_fwd(x, w, b, add), what="fwd")
    close(hip.conv3d_fwd(x, w, compute=X3), oracle.conv3d_fwd(x, w), what="fwd nobias")
    close(dx3, oracle.conv3d_bwd_data(dy, w, x.shape), what="bwd_data")
    dw_o, db_o = oracle.conv3d_bwd_weight(x, dy, 3)
    close(dw3, dw_o, 3e-5, 3e-5 * (N * D * H * W) ** 0.5, what="bwd_weight")
    close(db3, db_o, 3e-5, 3e-5 * (N * D * H * W) ** 0.5, what="dbias")
    # against fp64, next to the fp32 MFMA kernels
    import torch.nn.functional as F
    xd, wd = x.double(), w.double().requires_grad_(True)
    ref = F.conv3d(xd, wd, b.double(), padding=1) + add.double()
    refdx = F.conv_transpose3d(dy.double(), wd.detach(), padding=1)
    ref.backward(dy.double())
    err = lambda a, r: float((a.cpu().double() - r).abs().max() / r.abs().max())
    e3 = (err(y3, ref.detach()), err(dx3, refdx), err(dw3, wd.grad))
    e0 = (err(hip.conv3d_fwd(x, w, b, add), ref.detach()), err(hip.conv3d_bwd_data(dy, w, x.shape), refdx),
          err(hip.conv3d_bwd_weight(x, dy, 3)[0], wd.grad))
    for name, a, r in zip(("fwd", "bwd_data", "bwd_weight"), e3, e0):
        assert a <= max(3.0 * r, 2e-6) and a < 3e-6, f"{name}: split kernels {a:.2e} vs fp32 MFMA {r:.2e} (relative to max |fp64 result|)"


def test_conv3d_f32x3_channel_remainders_on_16_row_tiles(hip, oracle, tuning):
    """Channel counts that are no multiple of 32 (the reference's 40 / 80 / 120, research/msseg2/msseg2.py:87) on the split
    kernels: the 1..16 remaining output channels of forward / data gradient on conv3_f32x3_m16_kernel (v_mfma_f32_16x16x32_bf16),
    the weight gradient's remainder pairs on the 16-channel sub-tiles of conv3_bww_x3c_kernel -- against the oracle and
    against the padded 32-row plans (M355_TILE16=0), which must agree to summation-order noise; every lane width, fused
    statistics, split-K."""
    for (N, ci, co, D, H, W) in [(1, 64, 40, 8, 8, 16), (1, 40, 80, 8, 12, 32), (2, 12, 8, 9, 10, 36), (1, 33, 16, 5, 9, 8),
                                 (1, 48, 33, 6, 7, 20), (1, 20, 120, 4, 8, 8), (1, 80, 40, 6, 10, 24)]:
        x, w, b = torch.relu(rnd(N, ci, D, H, W, seed=1)), rnd(co, ci, 3, 3, 3, seed=2) * (1.0 / (27 * ci) ** 0.5), rnd(co, seed=3)
        add, dy = rnd(N, co, D, H, W, seed=4), rnd(N, co, D, H, W, seed=5)
        got = {}
        for t16 in (1, 0):
            tuning(M355_TILE16=t16)
            got[t16] = (hip.conv3d_fwd(x, w, b, add, compute=X3), hip.conv3d_bwd_data(dy, w, x.shape, compute=X3),
                        hip.conv3d_bwd_weight(x, dy, 3, compute=X3)[0])
        close(got[1][0], oracle.conv3d_fwd(x, w, b, add), what=f"fwd {ci}->{co}")
        close(got[1][1], oracle.conv3d_bwd_data(dy, w, x.shape), what=f"bwd_data {ci}->{co}")
        close(got[1][2], oracle.conv3d_bwd_weight(x, dy, 3)[0], 3e-5, 3e-5 * (N * D * H * W) ** 0.5, what=f"bwd_weight {ci}->{co}")
        for a, p_, name in zip(got[1], got[0], ("fwd", "bwd_data", "bwd_weight")):
            close(a, p_, 3e-6, 3e-6, f"{name} vs the padded plan {ci}->{co}")


def test_conv3d_f32x3_split_is_exact_on_hard_operands(hip):
    """The three-way split must reproduce values a bf16 rounding would destroy: operands with all 24 significant bits in
    use, mixed magnitudes (2^-20 .. 2^20 per channel), signed zeros; a non-finite operand makes exactly the outputs it
    touches non-finite (inf, or NaN where it meets a zero plane of the other operand) and nothing else."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(7)
    N, Ci, Co, D, H, W = 1, 16, 32, 4, 6, 32
    x = torch.randn(N, Ci, D, H, W, generator=g) * (2.0 ** torch.randint(-20, 21, (1, Ci, 1, 1, 1), generator=g).float())
    x[0, 3, 1, 2, 5] = 0.0
    x[0, 4, 1, 2, 5] = -0.0
    w = torch.randn(Co, Ci, 3, 3, 3, generator=g) * (2.0 ** -torch.randint(-20, 21, (1, Ci, 1, 1, 1), generator=g).float()) / 20
    ref = F.conv3d(x.double(), w.double(), padding=1)
    y = hip.conv3d_fwd(x, w, compute=X3).cpu().double()
    scale = F.conv3d(x.double().abs(), w.double().abs(), padding=1)   # sum of |terms| per output
    assert float(((y - ref).abs() / scale).max()) < 1e-5   # fp32 accumulation of 432 terms; a bf16 rounding of an operand: ~4e-3
    dy = torch.randn(N, Co, D, H, W, generator=g)
    wg = w.double().requires_grad_(True)
    F.conv3d(x.double(), wg, padding=1).backward(dy.double())
    dw = hip.conv3d_bwd_weight(x, dy, 3, with_bias=False, compute=X3)[0].cpu().double()
    ws = torch.zeros_like(wg)
    wsg = ws.requires_grad_(True)
    F.conv3d(x.double().abs(), wsg, padding=1).backward(dy.double().abs())
    assert float(((dw - wg.grad).abs() / wsg.grad.clamp_min(1e-300)).max()) < 2e-5
    xi = x.clone()
    xi[0, 2, 2, 3, 10] = float("inf")
    yi = hip.conv3d_fwd(xi, w.abs() + 1e-3, compute=X3).cpu()
    far = torch.ones_like(yi, dtype=torch.bool)
    far[0, :, 1:4, 2:5, 9:12] = False
    assert torch.isfinite(yi[far]).all() and not torch.isfinite(yi[~far]).any()


def test_conv3d_f32x3_fused_statistics_and_packed_weights(hip, oracle):
    """The split kernel shares the fp32 kernels' epilogue: fused GroupNorm statistics (m355_conv3d_fwd_stats) and the
    pre-packed weight form of the model path (m355_conv3d_pack + M355_CONV_W_PACKED), forward and data gradient."""
    N, Ci, Co, D, H, W = 2, 24, 40, 8, 12, 32
    x, w, b = rnd(N, Ci, D, H, W, seed=1), rnd(Co, Ci, 3, 3, 3, seed=2) * 0.05, rnd(Co, seed=3)
    y = hip.conv3d_fwd(x, w, b, compute=X3)
    packed = hip.pack_weights(w, x.shape, 0, compute=X3)
    assert torch.equal(hip.conv3d_fwd(x, w, b, compute=X3, packed=packed), y)
    close(y, oracle.conv3d_fwd(x, w, b), what="fwd")


@pytest.mark.parametrize("case", [(1, 6, 6, 8, 8, 8, 4, 2, 1), (2, 3, 5, 7, 6, 5, 3, 2, 1), (1, 4, 4, 5, 5, 5, 1, 1, 0)])
def test_conv3d_generic_direct(hip, oracle, case):
    N, Ci, Co, D, H, W, k, s, p = case
    x, w, b = rnd(N, Ci, D, H, W, seed=1), rnd(Co, Ci, k, k, k, seed=2) * 0.2, rnd(Co, seed=3)
    yo = oracle.conv3d_fwd(x, w, b, None, s, p)
    close(hip.conv3d_fwd(x, w, b, None, s, p), yo)
    dy = rnd(*yo.shape, seed=5)
    close(hip.conv3d_bwd_data(dy, w, x.shape, s, p), oracle.conv3d_bwd_data(dy, w, x.shape, s, p))
    dw_h, db_h = hip.conv3d_bwd_weight(x, dy, k, s, p)
    dw_o, db_o = oracle.conv3d_bwd_weight(x, dy, k, s, p)
    close(dw_h, dw_o, 3e-5, 1e-4)
    close(db_h, db_o, 3e-5, 1e-4)


@pytest.mark.parametrize("env", [{"M355_CONV_SLOTS": "7"}, {"M355_CONV_SLOTS": "5", "M355_CONV_KSPLIT": "2"},
                                 {"M355_CONV_SLOTS": "3", "M355_CONV_NTW": "8"}])
def test_conv3d_persistent_kernel_matches_oracle(hip, oracle, env, tuning):
    """The persistent forward kernel (workgroups walk several output tiles, prefetching across the
    tile boundary) on ragged volumes, N = 2, residual add, split-K and the one-per-CU NTW = 8 tile:
    a tiny residency forces every workgroup through many items."""
    tuning(**env)
    for (N, ci, co, D, H, W) in [(2, 12, 40, 9, 10, 36), (1, 5, 33, 6, 21, 16), (1, 8, 8, 12, 9, 8)]:
        x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * 0.2, rnd(co, seed=3)
        add = rnd(N, co, D, H, W, seed=4)
        close(hip.conv3d_fwd(x, w, b, add), oracle.conv3d_fwd(x, w, b, add), 2e-5, 2e-5, "persistent fwd")
        dy = rnd(N, co, D, H, W, seed=5)
        close(hip.conv3d_bwd_data(dy, w, x.shape), oracle.conv3d_bwd_data(dy, w, x.shape), 2e-5, 2e-5,
              "persistent bwd_data")


@pytest.mark.parametrize("env", [{}, {"M355_CONV_SLOTS": "5"}, {"M355_CONV_NTW": "1"}, {"M355_CONV_NTW": "2", "M355_CONV_KSPLIT": "3"},
                                 {"M355_CONV_NTW": "4", "M355_CONV_KSPLIT": "1"}])
def test_conv3d_16_row_remainder_tile(hip, oracle, env, tuning):
    """Channel counts that are no multiple of 32 (the reference's real widths 40 / 80 / 120, research/msseg2/
    msseg2.py:87): the last 1..16 output channels run as one 16-row tile on v_mfma_f32_16x16x4_f32.  Forward
    (bias + residual), data gradient (the remainder is then over Cin), every lane width (W = 8 / 16 / 32+), every
    voxel-tile height, split-K, a tiny residency; against the oracle and against the padded 32-row plan
    (M355_TILE16=0), which must agree to rounding."""
    for (N, ci, co, D, H, W) in [(1, 64, 40, 8, 8, 16), (1, 40, 80, 8, 12, 32), (2, 12, 8, 9, 10, 36), (1, 33, 16, 5, 9, 8),
                                 (1, 48, 33, 6, 7, 20), (1, 20, 120, 4, 8, 8)]:
        x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * (1.0 / (27 * ci) ** 0.5), rnd(co, seed=3)
        add = rnd(N, co, D, H, W, seed=4)
        dy = rnd(N, co, D, H, W, seed=5)
        tuning(M355_TILE16=1, **env)
        y16 = hip.conv3d_fwd(x, w, b, add)
        dx16 = hip.conv3d_bwd_data(dy, w, x.shape)
        close(y16, oracle.conv3d_fwd(x, w, b, add), what=f"fwd {ci}->{co}")
        close(dx16, oracle.conv3d_bwd_data(dy, w, x.shape), what=f"bwd_data {ci}->{co}")
        tuning(M355_TILE16=0, **env)
        close(y16, hip.conv3d_fwd(x, w, b, add), 2e-6, 2e-6, "vs padded 32-row plan")
        close(dx16, hip.conv3d_bwd_data(dy, w, x.shape), 2e-6, 2e-6, "bwd_data vs padded 32-row plan")


@pytest.mark.parametrize("env", [{}, {"M355_BWW_NSPLIT": "3"}, {"M355_BWW_NSPLIT": "1"}])
def test_conv3d_bwd_weight_remainder_pair_classes(hip, oracle, env, tuning):
    """Weight gradient with a 1..16 channel remainder on the output and / or the input side: the pairs touching a
    remainder run on 16-channel sub-tiles (v_mfma_f32_16x16x4_f32), all four pair classes in one launch with
    cost-proportional split counts (conv3_mfma_bww2c_kernel).  Both sides ragged, one side only, no full tile on a
    side at all, every lane width, N = 2, ragged volumes; vs the oracle and vs the padded 32 x 32 plan."""
    for (N, ci, co, D, H, W) in [(1, 40, 40, 8, 8, 32), (1, 64, 40, 8, 8, 16), (2, 12, 8, 9, 10, 36), (1, 33, 80, 5, 9, 8),
                                 (1, 80, 33, 6, 7, 20), (1, 120, 16, 4, 8, 8), (1, 48, 96, 4, 6, 12)]:
        x, dy = rnd(N, ci, D, H, W, seed=1), rnd(N, co, D, H, W, seed=5)
        tuning(M355_TILE16=1, **env)
        dw, db = hip.conv3d_bwd_weight(x, dy, 3)
        dwo, dbo = oracle.conv3d_bwd_weight(x, dy, 3)
        tol = 3e-5 * (N * D * H * W) ** 0.5
        close(dw, dwo, 3e-5, tol, f"bwd_weight {ci}->{co}")
        close(db, dbo, 3e-5, tol, "dbias")
        tuning(M355_TILE16=0, **env)
        close(dw, hip.conv3d_bwd_weight(x, dy, 3)[0], 1e-5, tol / 3, "vs padded 32 x 32 pairs")


@pytest.mark.parametrize("env", [{}, {"M355_CONV_SLOTS": "5"}, {"M355_CONV_KSPLIT": "2"}, {"M355_CONV_KSPLIT": "0"}])
def test_conv3d_fused_statistics(hip, oracle, env, tuning):
    """m355_conv3d_fwd_stats + m355_norm_stats_from_partials == statistics of the conv output (GroupNorm and
    BatchNorm geometry, ragged volumes with overhanging tiles, N = 2, one-shot and persistent kernels: partials from
    the conv epilogue; split-K plans -- forced, and whatever the planner picks for these small volumes: partials from
    the reduction pass)."""
    tuning(**{"M355_CONV_KSPLIT": 1, **env})
    for (N, ci, co, D, H, W, groups) in [(2, 8, 16, 9, 10, 36, 4), (1, 5, 40, 6, 21, 16, 8), (2, 8, 24, 12, 9, 8, 0),
                                        (1, 16, 32, 16, 16, 32, 8)]:
        x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * 0.2, rnd(co, seed=3)
        got = hip.conv3d_fwd_stats(x, w, b, groups)
        assert got is not None, "the fp32 3x3x3 MFMA path has fused statistics for these shapes"
        y, mean, rstd = got
        yo, mo, ro = oracle.conv3d_fwd_stats(x, w, b, groups)
        close(y, yo, 2e-5, 2e-5, "y")
        close(mean, mo, 1e-5, 1e-5, "mean")
        close(rstd, ro, 1e-5, 1e-5, "rstd")
        # and against the unfused statistics pass over the same y
        m2, r2 = hip.norm_stats(y, groups)[:2]
        close(mean, m2, 1e-5, 1e-6, "mean vs norm_stats")
        close(rstd, r2, 1e-5, 1e-6, "rstd vs norm_stats")


@pytest.mark.parametrize("compute", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("env", [{}, {"M355_CONV_SLOTS": "5"}])
def test_conv3d_packed_weights_reused_across_launches(hip, compute, env, tuning):
    """M355_CONV_W_PACKED: weights packed once by m355_conv3d_pack and reused launch after launch give the very bits
    of the repack-per-launch path; the work-queue state inside the packed buffer is reset by the draining kernel,
    so the 2nd, 3rd ... launch on the same buffer see fresh queues (persistent kernels, tiny residency, small-Cout
    VALU kernel, data gradient)."""
    tuning(**env)
    for (N, ci, co, D, H, W) in [(2, 12, 40, 9, 10, 36), (1, 16, 3, 8, 8, 32), (1, 32, 32, 8, 16, 64)]:
        x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * 0.2, rnd(co, seed=3)
        ref = hip.conv3d_fwd(x, w, b, compute=compute)
        pk = hip.pack_weights(w, x.shape, 0, compute)
        for _ in range(3):
            assert torch.equal(hip.conv3d_fwd(x, w, b, compute=compute, packed=pk), ref)
        dy = rnd(N, co, D, H, W, seed=5)
        refd = hip.conv3d_bwd_data(dy, w, x.shape, compute=compute)
        pkd = hip.pack_weights(w, x.shape, 1, compute)
        for _ in range(3):
            assert torch.equal(hip.conv3d_bwd_data(dy, w, x.shape, compute=compute, packed=pkd), refd)


def test_conv3d_pack_batch_matches_single_packs(hip):
    """m355_conv3d_pack_batch writes the very bytes of one m355_conv3d_pack per item: fp32 / bf16 / fp16 / split (compute 3)
    layouts, forward and data-gradient forms, ragged channel counts, the Cout <= 4 forward layout, and more items than one launch holds
    (64 per launch)."""
    cases = []
    for i, (ci, co, D, H, W) in enumerate([(12, 40, 9, 10, 36), (16, 3, 8, 8, 32), (32, 32, 8, 16, 64), (4, 32, 8, 8, 32),
                                           (96, 32, 8, 8, 32), (40, 80, 6, 6, 12), (320, 320, 4, 4, 8)]):
        w = rnd(co, ci, 3, 3, 3, seed=10 + i)
        for compute in (0, 1, 2, 3):
            for which in (0, 1):
                if ci <= 4 and which == 1 and compute in (1, 2):
                    continue
                cases.append((w, (1 + i % 2, ci, D, H, W), which, compute))
    assert len(cases) > 32
    got = hip.pack_weights_batch(cases)
    for (w, shp, which, compute), buf in zip(cases, got):
        ref = hip.pack_weights(w, shp, which, compute)
        assert torch.equal(buf, ref), (tuple(w.shape), shp, which, compute)   # (incl. the zeroed work-queue tail)


def test_model_batched_repack_after_optimizer_step(golden):
    """After optimizer.step the first conv re-packs every stale cached form of every parameter with one launch
    (ops._repack_stale); the SGD trajectory is bit-identical to per-conv packing (M355_PACK_BATCH=0 path)."""
    from functools import partial
    from torch import nn
    from segmentation_pipeline_amd import ops
    from segmentation_pipeline_amd.models import ModularUNet
    g = golden("unet_gn_convt.npz")
    outs = []
    for batch in (True, False):
        model = ModularUNet(4, 3, [8, 16, 32], 3, block_params={'normalization_class': partial(nn.GroupNorm, 8)},
                            upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2})
        model.load_state_dict(g.state_dict("m.sd."))
        model = model.cuda().train()
        opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
        x = g.t("x").cuda()
        ops.PACK_BATCH = batch
        try:
            for _ in range(3):
                opt.zero_grad()
                p = model(x)
                (p * p).sum().backward()
                opt.step()
            w = model.down_blocks[1].layers.conv0.weight
            stale_before = w._m355_packed[0] != w._version
            with torch.no_grad():
                outs.append(model(x))
            assert stale_before and w._m355_packed[0] == w._version
            if batch:   # every registered parameter was refreshed by that one pass, not only the first conv's
                for q in model.parameters():
                    c = getattr(q, "_m355_packed", None)
                    assert c is None or c[0] == q._version
        finally:
            ops.PACK_BATCH = True
    assert torch.equal(outs[0], outs[1])


def test_model_packed_weight_cache_follows_parameter_versions(golden):
    """ops caches the packed weights per parameter version: same results as with the cache off, re-packed after an
    optimizer step (SGD trajectory golden stays green in test_model_gpu.py), and keyed by the data pointer."""
    from functools import partial
    from torch import nn
    from segmentation_pipeline_amd import ops
    from segmentation_pipeline_amd.models import ModularUNet
    g = golden("unet_gn_convt.npz")
    model = ModularUNet(4, 3, [8, 16, 32], 3, block_params={'normalization_class': partial(nn.GroupNorm, 8)},
                        upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2})
    model.load_state_dict(g.state_dict("m.sd."))
    model = model.cuda().train()
    x = g.t("x").cuda()
    w = model.down_blocks[1].layers.conv0.weight
    p1 = model(x)
    assert w._m355_packed[0] == w._version and len(w._m355_packed[2]) >= 1
    p1.sum().backward()
    assert any(k[0] == 1 for k in w._m355_packed[2]), "data-gradient packing cached on the parameter"
    try:
        ops.PACK_CACHE = False
        p2 = model(x)
    finally:
        ops.PACK_CACHE = True
    assert torch.equal(p1, p2)
    with torch.no_grad():
        w.mul_(0.5)
    p3 = model(x)
    assert w._m355_packed[0] == w._version and not torch.equal(p3, p1)


def test_out_conv_softmax_fused_epilogue(hip, oracle):
    """M355_CONV_SOFTMAX on the Cout <= 4 fp32 kernel (out conv + hypothesis, models/modular_unet.py:99-100) gives the
    very bits of m355_conv3d_fwd followed by m355_softmax_fwd, and matches the oracle's conv -> softmax."""
    for (N, ci, co, D, H, W) in [(1, 32, 3, 8, 16, 64), (2, 8, 2, 9, 10, 36), (1, 16, 4, 8, 8, 32)]:
        x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * 0.2, rnd(co, seed=3)
        fused = hip.conv3d_fwd(x, w, b, softmax=True)
        assert torch.equal(fused, hip.softmax_fwd(hip.conv3d_fwd(x, w, b)))
        close(fused, oracle.softmax_fwd(oracle.conv3d_fwd(x, w, b)), 2e-5, 1e-6, "conv + softmax")
        assert (fused.sum(dim=1) - 1).abs().max().item() <= 1e-5


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_out_conv_softmax_fused_epilogue_16bit(hip, oracle, compute, tuning):
    """M355_CONV_SOFTMAX on m355_conv3d_fwd_h16 (c8 input, Cout <= 4: the out conv of the 16-bit inference flow): the
    softmax is the kernel's epilogue (all channels of a voxel are registers of one lane) == the same conv followed
    by m355_softmax_fwd, bit for bit; 4-wave and 8-wave kernel variants, ragged volumes, N = 2."""
    for w8, one in ((0, 3), (2, 3), (0, 1)):   # queue-driven 4-wave / 8-wave kernels, and the default one-shot variant
        tuning(M355_H16_W8=w8, M355_H16_ONESHOT=one, M355_CONV_KSPLIT=1)
        for (N, ci, co, D, H, W) in [(1, 32, 3, 8, 16, 64), (2, 8, 2, 9, 10, 36), (1, 16, 4, 8, 8, 32)]:
            x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * 0.2, rnd(co, seed=3)
            x16 = hip.act16_pack(x, compute)
            fused = hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute, softmax=True)
            assert torch.equal(fused, hip.softmax_fwd(hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute)))
            close(fused, oracle.softmax_fwd(oracle.conv3d_fwd(x, w, b, compute=compute)), 1e-4, 1e-5, "conv + softmax")
            assert (fused.sum(dim=1) - 1).abs().max().item() <= 1e-5


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_out_conv_tap_rows_on_the_m_side_16bit(hip, oracle, compute, tuning):
    """conv3_cout4_h16_kernel (round 4: <= 4 output channels, c8 input, fp32 output -- the out conv of cfg2 / cfg4): the tap
    row dy sits on the MFMA's M side, an output row is the in-lane sum of three accumulator registers.  Against the oracle
    on equally rounded operands (1..4 output channels, channel counts that are no multiples of 16, ragged D / H, N = 2,
    bias, with and without the softmax epilogue) and against the generic 32-row kernel (M355_NO_SMALL=1)."""
    from segmentation_pipeline_amd import _lib
    for (N, ci, co, D, H, W) in [(1, 32, 3, 8, 16, 64), (2, 40, 1, 5, 7, 64), (1, 24, 4, 9, 10, 32), (1, 8, 2, 4, 4, 96)]:
        x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * 0.2, rnd(co, seed=3)
        x16 = hip.act16_pack(x, compute)
        tuning(M355_NO_SMALL=0, M355_CONV_KSPLIT=1, M355_CONV_NTW=4)   # (the planner takes a lower tile for these small volumes)
        plan = hip.conv_plan((N, ci, D, H, W), co, compute=compute)
        assert plan[1] == 4 and plan[2] == 32, plan        # (the geometry the kernel is instantiated for)
        y = hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute)
        ysm = hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute, softmax=True)
        ref = oracle.conv3d_fwd(x, w, b, compute=compute)
        close(y, ref, 3e-5, 3e-5 * ref.abs().max().item(), f"logits {(N, ci, co)}")
        assert torch.equal(ysm, hip.softmax_fwd(y))
        close(ysm, oracle.softmax_fwd(ref), 1e-4, 1e-5, "softmax")
        assert torch.equal(y, hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute))     # deterministic
        tuning(M355_NO_SMALL=1, M355_CONV_KSPLIT=1, M355_CONV_NTW=4)
        y_generic = hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute)
        close(y, y_generic, 3e-5, 3e-5 * ref.abs().max().item(), "vs the 32-row kernel")
    tuning(M355_NO_SMALL=0)


def test_conv3d_deterministic(hip):
    x, w = rnd(1, 32, 8, 16, 32, seed=1), rnd(32, 32, 3, 3, 3, seed=2) * 0.05
    dy = rnd(1, 32, 8, 16, 32, seed=3)
    a, b = hip.conv3d_fwd(x, w), hip.conv3d_fwd(x, w)
    assert torch.equal(a, b)
    (d1, _), (d2, _) = hip.conv3d_bwd_weight(x, dy, 3), hip.conv3d_bwd_weight(x, dy, 3)
    assert torch.equal(d1, d2)


CONVT = [
    # N, Cin, Cout, D, H, W, k, s, p, out_pad
    (1, 64, 64, 4, 4, 8, 2, 2, 0, 0),
    (2, 5, 7, 3, 5, 6, 2, 2, 0, 0),     # ragged channel tiles
    (1, 320, 48, 2, 2, 2, 2, 2, 0, 0),  # 8 voxels: the data gradient splits K = 8 * Cout
    (1, 8, 8, 4, 4, 4, 4, 2, 1, 0),     # BlurConvTranspose3d geometry
    (1, 3, 4, 3, 3, 3, 3, 2, 1, 1),
    (1, 520, 8, 2, 2, 2, 2, 2, 0, 0),   # Cin > 512: no forward x tile fits 64 KB of LDS; the gradients keep none there
]
# kernel family of fwd / bwd_data / bwd_weight (m355_conv_transpose3d_plan: 1 fp32 MFMA, 0 direct), in the order of CONVT
CONVT_FAMILIES = [(1, 1, 1), (1, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), (0, 1, 1)]


@pytest.mark.parametrize("case", CONVT)
def test_conv_transpose3d_fwd_bwd(hip, oracle, case):
    N, Ci, Co, D, H, W, k, s, p, op = case
    plans = [hip.convt_plan((N, Ci, D, H, W), Co, k, s, p, op, which=which) for which in (0, 1, 2)]
    assert tuple(pl[0] for pl in plans) == CONVT_FAMILIES[CONVT.index(case)], plans
    assert Ci != 320 or plans[1][3] > 1, f"splits of the data gradient's K: {plans[1]}"
    x, w, b = rnd(N, Ci, D, H, W, seed=1), rnd(Ci, Co, k, k, k, seed=2) * (1.0 / Ci ** 0.5), rnd(Co, seed=3)
    yo = oracle.convt_fwd(x, w, b, s, p, op)
    close(hip.convt_fwd(x, w, b, s, p, op), yo, what="fwd")
    dy = rnd(*yo.shape, seed=5)
    close(hip.convt_bwd_data(dy, w, x.shape, s, p, op), oracle.convt_bwd_data(dy, w, x.shape, s, p, op), what="bwd_data")
    dw_h, db_h = hip.convt_bwd_weight(x, dy, k, s, p, op)
    dw_o, db_o = oracle.convt_bwd_weight(x, dy, k, s, p, op)
    close(dw_h, dw_o, 3e-5, 1e-4, what="bwd_weight")
    close(db_h, db_o, 3e-5, 1e-4, what="dbias")


def test_conv_transpose3d_k2s2_forward_on_the_split_kernel(hip, oracle):
    """M355_COMPUTE_F32X3 on the fp32 conv-transpose entry point: the k2 s2 forward as six bf16 MFMAs per product group
    on the exact three-way operand split (convt_k2s2_fwd_x3_kernel) -- every voxel-tile width (Cin 64 / 130 / 320),
    ragged channel counts and voxel tiles, N = 2, a concat-slot output stride; against the oracle at the fp32 kernel's
    tolerance and against fp64 next to the fp32 MFMA kernel."""
    import torch.nn.functional as F
    for (N, ci, co, D, H, W) in [(1, 64, 64, 8, 8, 16), (2, 17, 5, 3, 5, 7), (1, 320, 320, 4, 4, 4), (1, 130, 70, 2, 9, 20),
                                 (1, 8, 8, 1, 1, 1), (2, 32, 33, 6, 6, 6)]:
        x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(ci, co, 2, 2, 2, seed=2) * (1.0 / ci ** 0.5), rnd(co, seed=3)
        y3 = hip.convt_fwd(x, w, b, compute=X3)
        close(y3, oracle.convt_fwd(x, w, b, 2, 0, 0), what=f"fwd {ci}->{co}")
        close(hip.convt_fwd(x, w, None, compute=X3), oracle.convt_fwd(x, w, None, 2, 0, 0), what="fwd nobias")
        ref = F.conv_transpose3d(x.double(), w.double(), b.double(), stride=2)
        e3 = float((y3.cpu().double() - ref).abs().max() / ref.abs().max())
        e0 = float((hip.convt_fwd(x, w, b).cpu().double() - ref).abs().max() / ref.abs().max())
        assert e3 <= max(3.0 * e0, 2e-6) and e3 < 3e-6, (ci, co, e3, e0)


NORM = [
    # N, C, D, H, W, groups, act
    (1, 32, 16, 16, 16, 8, 1),
    (2, 16, 5, 6, 7, 4, 1),      # S not multiple of 4 -> scalar path
    (2, 8, 8, 8, 8, 0, 1),       # batch norm
    (3, 6, 3, 3, 5, 0, 2),       # BN, leaky, ragged
    (1, 40, 8, 8, 8, 8, 0),      # 5 channels per group, no activation
    (1, 8, 32, 32, 32, 1, 1),    # one group of 262144 elements: multi-block partials
]


@pytest.mark.parametrize("case", NORM)
def test_norm_act_fwd_bwd(hip, oracle, case):
    N, Cc, D, H, W, groups, act = case
    x = rnd(N, Cc, D, H, W, seed=1) * 1.7 + 0.3
    gamma, beta = rnd(Cc, seed=2), rnd(Cc, seed=3)
    add = rnd(N, Cc, D, H, W, seed=4)
    running = None if groups else (rnd(Cc, seed=5) * 0.1, torch.rand(Cc) + 0.5)
    mh, rh, rmh, rvh = hip.norm_stats(x, groups, running=running)
    mo, ro, rmo, rvo = oracle.norm_stats(x, groups, running=running)
    close(mh, mo, 1e-6, 1e-6, "mean")
    close(rh, ro, 2e-6, 1e-6, "rstd")
    if running is not None:
        close(rmh, rmo, 1e-6, 1e-6, "running_mean")
        close(rvh, rvo, 2e-6, 1e-6, "running_var")
    close(hip.norm_act_fwd(x, mo, ro, gamma, beta, groups, act, add), oracle.norm_act_fwd(x, mo, ro, gamma, beta, groups, act, add),
          what="fwd")
    dy = rnd(N, Cc, D, H, W, seed=7)
    for training in ((1,) if groups else (1, 0)):
        dxh, dgh, dbh = hip.norm_act_bwd(x, dy, mo, ro, gamma, beta, groups, act, training)
        dxo, dgo, dbo = oracle.norm_act_bwd(x, dy, mo, ro, gamma, beta, groups, act, training)
        close(dxh, dxo, 2e-5, 2e-5, "dx")
        close(dgh, dgo, 2e-5, 1e-4, "dgamma")
        close(dbh, dbo, 2e-5, 1e-4, "dbeta")


def test_pool_upsample_softmax(hip, oracle):
    for shape in [(1, 3, 4, 6, 8), (2, 5, 2, 2, 6), (1, 2, 16, 16, 32)]:
        x = rnd(*shape, seed=1)
        yo = oracle.avgpool_fwd(x)
        close(hip.avgpool_fwd(x), yo, 1e-6, 1e-6, "pool fwd")
        dy = rnd(*yo.shape, seed=2)
        close(hip.avgpool_bwd(dy, x.shape), oracle.avgpool_bwd(dy, x.shape), 0, 0, "pool bwd")
    # (even W: four outputs per thread + float4 stores; odd W: the one-output-per-thread kernel)
    for shape in [(1, 2, 3, 4, 5), (2, 1, 1, 2, 2), (1, 3, 8, 8, 8), (1, 1, 2, 2, 2), (2, 3, 6, 11, 12), (1, 2, 5, 3, 7),
                  (2, 5, 12, 22, 6), (1, 2, 9, 17, 40), (2, 1, 5, 8, 33), (1, 1, 2, 3, 70)]:   # (several backward tiles per axis)
        x = rnd(*shape, seed=3)
        yo = oracle.upsample_fwd(x)
        close(hip.upsample_fwd(x), yo, 2e-6, 2e-6, "up fwd")
        dy = rnd(*yo.shape, seed=4)
        close(hip.upsample_bwd(dy, x.shape), oracle.upsample_bwd(dy, x.shape), 1e-5, 1e-5, "up bwd")
    for C_, inner, bias in [(3, 1, 0.0), (7, 1, 0.0), (2, 2, 5.0)]:
        x = rnd(2, C_ * inner, 4, 5, 6, seed=5) * 3
        yo = oracle.softmax_fwd(x, inner, bias)
        yh = hip.softmax_fwd(x, inner, bias)
        close(yh, yo, 2e-6, 1e-7, "softmax fwd")
        dy = rnd(*x.shape, seed=6)
        close(hip.softmax_bwd(yo, dy, inner), oracle.softmax_bwd(yo, dy, inner), 1e-5, 1e-6, "softmax bwd")


def test_avgpool_bwd_fused_with_skip_gradient(hip, oracle):
    dy, add = rnd(2, 5, 3, 4, 6, seed=1), rnd(2, 5, 6, 8, 12, seed=2)
    close(hip.avgpool_bwd_add(dy, add, add.shape), oracle.avgpool_bwd_add(dy, add, add.shape), 0, 1e-7, "pool bwd + add")
    close(hip.avgpool_bwd_add(dy, add, add.shape), hip.avgpool_bwd(dy, add.shape).cpu() + add, 0, 1e-7, "== separate ops")


def test_space_to_depth_roundtrip(hip, oracle):
    for shape in [(1, 3, 4, 6, 8), (2, 5, 2, 2, 6), (1, 2, 16, 16, 32)]:
        x = rnd(*shape, seed=1)
        yo = oracle.space_to_depth(x)
        yh = hip.space_to_depth(x)
        assert torch.equal(yh.cpu(), yo), "s2d is a permutation: bit-exact"
        assert torch.equal(hip.depth_to_space(yh).cpu(), x)
        assert torch.equal(hip.depth_to_space(yo).cpu(), oracle.depth_to_space(yo))
    # odd sizes are refused, not silently truncated
    with pytest.raises(RuntimeError):
        hip.space_to_depth(rnd(1, 1, 3, 4, 4, seed=2))


@pytest.mark.parametrize("standardize", [False, True])
@pytest.mark.parametrize("transposed", [False, True])
def test_blur_weight_transform(hip, oracle, standardize, transposed):
    for A, B in [(5, 6), (40, 40), (3, 130)]:
        w = rnd(A, B, 3, 3, 3, seed=1) * 0.3 + 0.05
        scale = torch.full((B,), 0.37) + rnd(B, seed=3) * 0.01
        eo, mso = oracle.blur_weight_fwd(w, scale, standardize, transposed)
        eh, msh = hip.blur_weight_fwd(w, scale, standardize, transposed)
        close(eh, eo, 1e-5, 1e-6, "wexp")
        if standardize:
            close(msh, mso, 1e-5, 1e-7, "mean/std")
        g = rnd(*eo.shape, seed=2)
        close(hip.blur_weight_bwd(g, w, scale, mso, standardize, transposed),
              oracle.blur_weight_bwd(g, w, scale, mso, standardize, transposed), 2e-5, 1e-6, "dw")


def test_weight_standardize_fwd_bwd(hip, oracle):
    w, g = rnd(40, 24, 3, 3, 3, seed=1), rnd(40, 24, 3, 3, 3, seed=2)
    wn_h, ms_h = hip.weight_standardize_fwd(w)
    wn_o, ms_o = oracle.weight_standardize_fwd(w)
    close(wn_h, wn_o, 1e-5, 1e-5, "standardize fwd")
    close(ms_h, ms_o, 1e-5, 1e-6, "mean/std")
    close(hip.weight_standardize_bwd(g, w, ms_o), oracle.weight_standardize_bwd(g, w, ms_o), 1e-4, 1e-5, "standardize bwd")


def test_blur_convs_mfma_path_matches_direct_kernels():
    """BlurConv3d / BlurConvTranspose3d route through s2d + 3x3x3 MFMA conv; compare values and all
    gradients with the generic direct stride-2 kernels on the same effective filter, and check that
    the transposed conv writes straight into a concat slot."""
    import segmentation_pipeline_amd.ops as ops
    from segmentation_pipeline_amd.models import BlurConv3d, BlurConvTranspose3d
    torch.manual_seed(0)
    bc = BlurConv3d(12, 12, 3, stride=2, padding=1).cuda()
    x = torch.randn(2, 12, 8, 12, 16, device="cuda", requires_grad=True)
    dy = torch.randn(2, 12, 4, 6, 8, device="cuda")
    y = bc(x)
    y.backward(dy)
    got = (y.detach().clone(), x.grad.clone(), bc.weight.grad.clone())
    x.grad = None
    bc.weight.grad = None
    w4, _ = bc.effective()
    y2 = ops.conv3d(x, w4, None, stride=2, padding=1)
    y2.backward(dy)
    for a, b, what in zip(got, (y2, x.grad, bc.weight.grad), ("y", "dx", "dw")):
        assert (a - b).abs().max().item() <= 2e-5 * max(1.0, b.abs().max().item()), what

    bt = BlurConvTranspose3d(12, 12, 3, stride=2, padding=1, output_padding=0).cuda()
    x = torch.randn(2, 12, 4, 6, 8, device="cuda", requires_grad=True)
    dy = torch.randn(2, 12, 8, 12, 16, device="cuda")
    buf = torch.zeros(2, 20, 8, 12, 16, device="cuda")
    y = bt(x, out=ops.OutSlot(buf, 8, 20))
    assert y.data_ptr() == buf[:, 8:].data_ptr() and torch.count_nonzero(buf[:, :8]) == 0
    y.backward(dy)
    got = (y.detach().clone(), x.grad.clone(), bt.weight.grad.clone())
    x.grad = None
    bt.weight.grad = None
    from segmentation_pipeline_amd.models.components import _box_blur
    y2 = ops.conv_transpose3d(x, _box_blur(bt.weight, bt.kernel), None, stride=2, padding=1, output_padding=0)
    y2.backward(dy)
    for a, b, what in zip(got, (y2, x.grad, bt.weight.grad), ("y", "dx", "dw")):
        assert (a - b).abs().max().item() <= 2e-5 * max(1.0, b.abs().max().item()), "T " + what


@pytest.mark.parametrize("cfg", [(0.5, None, True), (0.3, [1.0, 2.0, 3.0], False), (0.5, [1.0, 100.0, 1.0], True)])
def test_hybrid_loss_fwd_bwd(hip, oracle, cfg):
    dw, cw, sq = cfg
    p = torch.softmax(rnd(2, 3, 9, 10, 11, seed=1) * 2, dim=1)
    lab = torch.randint(0, 3, (2, 9, 10, 11), generator=torch.Generator().manual_seed(2))
    t = torch.nn.functional.one_hot(lab, 3).permute(0, 4, 1, 2, 3).float().contiguous()
    cwt = None if cw is None else torch.tensor(cw)
    oh, sh = hip.loss_fwd(p, t, dw, cwt, sq)
    oo, so = oracle.loss_fwd(p, t, dw, cwt, sq)
    close(oh, oo, 2e-6, 1e-7, "loss")
    close(sh, so, 2e-6, 1e-6, "sums")
    close(hip.loss_bwd(p, t, so, 0.7, dw, cwt, sq), oracle.loss_bwd(p, t, so, 0.7, dw, cwt, sq), 1e-5, 1e-9, "dp")


def test_loss_golden(hip, golden):
    g = golden("hybrid_loss.npz")
    p, t = g.t("p"), g.t("t")
    for i in range(3):
        cfg = g[f"case{i}.cfg"]
        dw, sq = float(cfg[0]), bool(cfg[1])
        cw = torch.tensor(cfg[2:], dtype=torch.float32) if len(cfg) > 2 else None
        out3, sums = hip.loss_fwd(p, t, dw, cw, sq)
        close(out3, g.t(f"case{i}.out"), 2e-6, 1e-7)
        close(hip.loss_bwd(p, t, sums, 1.0, dw, cw, sq), g.t(f"case{i}.dp"), 1e-5, 1e-8)


def test_patches_roundtrip_and_confusion(hip, oracle):
    from oracle import torch_ref as R
    vol = rnd(2, 20, 18, 22, seed=1)
    locs = R.grid_locations((20, 18, 22), (8, 8, 8), (2, 2, 2))
    loc = torch.tensor(locs, dtype=torch.int32)
    ph = hip.patch_gather(vol, loc, (8, 8, 8))
    po = oracle.patch_gather(vol, loc, (8, 8, 8))
    assert torch.equal(ph.cpu(), po)
    outh, cnth = hip.patch_aggregate(ph, loc, (20, 18, 22))
    outo, cnto = oracle.patch_aggregate(po, loc, (20, 18, 22))
    assert torch.equal(cnth.cpu(), cnto)
    close(outh, outo, 1e-6, 1e-6)
    close(outh, vol, 1e-6, 1e-6)  # tiling a pointwise model reproduces the volume
    # non-trivial patch values (aggregation order == patch order)
    pv = rnd(*po.shape, seed=9)
    a, _ = hip.patch_aggregate(pv, loc, (20, 18, 22))
    b, _ = oracle.patch_aggregate(pv, loc, (20, 18, 22))
    close(a, b, 1e-6, 1e-6)

    prob = torch.softmax(rnd(2, 4, 9, 9, 9, seed=2), dim=1)
    prob[0, 1, 0, 0, 0] = prob[0, 2, 0, 0, 0] = 0.4  # tie: first maximum wins
    prob[0, 0, 0, 0, 0] = prob[0, 3, 0, 0, 0] = 0.1
    tgt = torch.randint(0, 4, (2, 9, 9, 9), generator=torch.Generator().manual_seed(3))
    amh, ch = hip.argmax_confusion(prob, tgt)
    amo, co = oracle.argmax_confusion(prob, tgt)
    assert torch.equal(amh.cpu(), amo) and torch.equal(ch.cpu(), co)
    assert torch.equal(amo.long(), prob.argmax(dim=1))


def test_ensemble_kernels_match_oracle(hip, oracle):
    """flip/permute gather, accumulate through the inverse transform, finalize (mean / majority): bit-exact for the
    index and vote arithmetic, fp32 running sums in member order."""
    import itertools
    g = torch.Generator().manual_seed(9)
    x = torch.randn((2, 4, 6, 5, 8), generator=g)
    members = [(perm, fm) for perm in itertools.permutations((0, 1, 2)) for fm in range(8)]
    preds = []
    for perm, fm in members:
        xm = hip.flip_permute(x, perm, fm)
        assert torch.equal(xm.cpu(), oracle.flip_permute(x, perm, fm))
        preds.append(torch.softmax(xm.cpu() * (1.0 + 0.03 * len(preds)), dim=1))
    for strategy in ("mean", "majority"):
        out_h, acc_h = hip.ensemble(preds, members, x.shape[2:], strategy)
        out_o, acc_o = oracle.ensemble(preds, members, x.shape[2:], strategy)
        assert torch.equal(out_h.cpu(), out_o) and torch.equal(acc_h.cpu(), acc_o)


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4], ids=["constant", "edge", "reflect", "symmetric", "wrap"])
def test_padded_gather_and_cropped_finalize(hip, oracle, mode):
    vol = rnd(3, 9, 6, 11, seed=1)
    border, ps = (3, 2, 4), (5, 4, 6)
    locs = torch.tensor([(0, 0, 0), (10, 6, 13), (4, 3, 7), (2, 0, 1)], dtype=torch.int32)
    assert torch.equal(hip.patch_gather_padded(vol, locs, ps, border, mode, -2.0).cpu(),
                       oracle.patch_gather_padded(vol, locs, ps, border, mode, -2.0))
    acc, cnt = rnd(3, 15, 10, 19, seed=2), torch.rand(15, 10, 19) + 1.0
    close(hip.patch_finalize_crop(acc, cnt, border), oracle.patch_finalize_crop(acc, cnt, border), 1e-6, 1e-7, "crop")


def test_error_paths_gpu(hip):
    from segmentation_pipeline_amd import _lib
    L = hip.lib
    x = torch.zeros(1, 2, 3, 4, 4, device="cuda")
    rc = L.m355_avgpool3d_2x_fwd(C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), 1, 2, 3, 4, 4, 0, 0, None)
    assert rc == _lib.M355_OK - 2
    d = _lib.ConvDesc(1, 4, 4, 4, 4, 4, 3, 1, 1, 0, 0, 0)
    w = torch.zeros(4, 4, 3, 3, 3, device="cuda")
    rc = L.m355_conv3d_fwd(C.byref(d), C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), None, None,
                           C.c_void_p(x.data_ptr()), None, 0, None)
    assert rc == -4 and b"workspace" in L.m355_last_error()


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CONV3)
def test_conv3d_bf16_compute_mode(hip, oracle, case, compute):
    """M355_COMPUTE_BF16 / M355_COMPUTE_F16: operands rounded to bf16 / fp16 (RNE), fp32 accumulate.
    Against the oracle run in the same mode only the accumulation order differs (tolerance 3e-5 of the
    output scale); against exact fp32 the operand rounding shows up at the 2^-8 / 2^-11 level (bounded
    loosely here)."""
    N, Ci, Co, D, H, W = case
    x, w, b = rnd(N, Ci, D, H, W, seed=1), rnd(Co, Ci, 3, 3, 3, seed=2) * (1.0 / (27 * Ci) ** 0.5), rnd(Co, seed=3)
    add = rnd(N, Co, D, H, W, seed=4)
    yb = hip.conv3d_fwd(x, w, b, add, compute=compute)
    close(yb, oracle.conv3d_fwd(x, w, b, add, compute=compute), 3e-5, 3e-5, "bf16 fwd vs bf16 oracle")
    y32 = oracle.conv3d_fwd(x, w, b, add)
    rel = (yb.cpu().double() - y32.double()).abs().max().item() / y32.abs().max().item()
    assert rel < (2e-2 if compute == 1 else 3e-3), rel
    dy = rnd(N, Co, D, H, W, seed=5)
    close(hip.conv3d_bwd_data(dy, w, x.shape, compute=compute), oracle.conv3d_bwd_data(dy, w, x.shape, compute=compute), 3e-5, 3e-5,
          "bf16 bwd_data vs bf16 oracle")


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_act16_pack_unpack_roundtrip(hip, compute):
    """fp32 NCDHW <-> c8 ([N][C/8][voxel][8] 16-bit): rounding == torch's cast (RNE, pinned for the oracle in
    test_c_operand_rounding_matches_torch_casts), channel counts that are no multiple of 8 are zero-padded,
    a non-dense batch stride leaves the gap untouched."""
    dt = torch.bfloat16 if compute == 1 else torch.float16
    for (N, Cc, D, H, W, pad) in [(1, 8, 3, 4, 5, 0), (2, 13, 4, 6, 7, 2), (1, 3, 2, 2, 33, 0)]:
        x = rnd(N, Cc, D, H, W, seed=N + Cc) * 3.0
        x16 = hip.act16_pack(x, compute, pad_batch=pad)
        S, CB = D * H * W, (Cc + 7) // 8
        ref = torch.zeros(N, CB * 8, S)
        ref[:, :Cc] = x.reshape(N, Cc, S).to(dt).float()
        got = x16[:, :CB].float().cpu().permute(0, 1, 3, 2).reshape(N, CB * 8, S)
        assert torch.equal(got, ref)
        if pad:
            assert (x16[:, CB:].float() == 7.0).all()
        assert torch.equal(hip.act16_unpack(x16, Cc, (D, H, W), compute).cpu(), x.to(dt).float())


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("env", [{}, {"M355_CONV_SLOTS": "5", "M355_H16_ONESHOT": "3"},
                                 {"M355_CONV_SLOTS": "3", "M355_CONV_KSPLIT": "2", "M355_H16_ONESHOT": "3"},
                                 {"M355_CONV_NTW": "1"}, {"M355_CONV_NTW": "2", "M355_CONV_SLOTS": "7", "M355_H16_ONESHOT": "3"},
                                 {"M355_CONV_KSPLIT": "3"}])
def test_conv3d_h16_c8_input_persistent_and_fused_statistics(hip, oracle, compute, env, tuning):
    """m355_conv3d_fwd_h16 / m355_conv3d_bwd_data_h16 on c8 tensors (the model path of the 16-bit modes): equal to
    the oracle run with operands rounded to the same 16-bit type (only the fp32 accumulation order differs);
    ragged volumes, N = 2, odd channel-block counts, strided batches, tiny residencies (every workgroup walks
    many queue items: M355_H16_ONESHOT=3 selects the queue-driven kernels, the default is one item per workgroup),
    split-K, and the statistics of the following normalisation fused into the epilogue."""
    tuning(**{"M355_CONV_KSPLIT": 1, **env})  # the planner would split K on volumes this small: no fused statistics
    for (N, ci, co, D, H, W, groups) in [(2, 12, 40, 9, 10, 36, 8), (1, 24, 33, 6, 21, 16, None), (1, 8, 8, 12, 9, 8, 0),
                                        (1, 40, 16, 8, 8, 32, 4)]:
        x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * (1.0 / (27 * ci) ** 0.5), rnd(co, seed=3)
        x16 = hip.act16_pack(x, compute, pad_batch=1)
        yo = oracle.conv3d_fwd(x, w, b, compute=compute)
        split = "M355_CONV_KSPLIT" in env
        if groups is None or split:
            close(hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute), yo, 3e-5, 3e-5, "h16 fwd")
        else:
            y, mean, rstd = hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute, groups=groups)
            close(y, yo, 3e-5, 3e-5, "h16 fwd (stats variant)")
            m2, r2 = hip.norm_stats(y, groups)[:2]
            close(mean, m2, 1e-5, 1e-6, "fused mean")
            close(rstd, r2, 1e-5, 1e-6, "fused rstd")
        dy = rnd(N, co, D, H, W, seed=5)
        dy16 = hip.act16_pack(dy, compute)
        close(hip.conv3d_bwd_data_h16(dy16, co, w, x.shape, compute=compute),
              oracle.conv3d_bwd_data(dy, w, x.shape, compute=compute), 3e-5, 3e-5, "h16 bwd_data")
    # bit-reproducible regardless of which workgroup takes which item
    a = hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute)
    assert torch.equal(a, hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute))


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("env", [{}, {"M355_CONV_SLOTS": "3"}, {"M355_CONV_KSPLIT": "2", "M355_CONV_SLOTS": "5"}])
def test_conv3d_h16_eight_wave_double_buffered_variant(hip, oracle, compute, env, tuning):
    """The 8-wave variant of the 16-bit conv kernel (tile 8 x 2 x 32, one workgroup per CU, double-buffered LDS, one
    barrier per chunk) forced on small volumes (M355_H16_W8=2): forward with bias + residual, fused statistics,
    c8 output, data gradient; ragged D / H / W, odd channel-block counts, N = 2, tiny residency (every workgroup
    walks many items), split-K; == the oracle on rounded operands and == the 4-wave kernel bit for bit."""
    dt = torch.bfloat16 if compute == 1 else torch.float16
    for (N, ci, co, D, H, W, groups) in [(1, 32, 32, 8, 6, 32, 8), (2, 24, 40, 9, 5, 64, 8), (1, 96, 32, 17, 4, 62, 0),
                                        (1, 8, 13, 8, 2, 32, None)]:
        x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * (1.0 / (27 * ci) ** 0.5), rnd(co, seed=3)
        dy = rnd(N, co, D, H, W, seed=5)
        x16, dy16 = hip.act16_pack(x, compute), hip.act16_pack(dy, compute)
        out = {}
        for w8 in (2, 0):
            # queue-driven plans (M355_H16_ONESHOT=3); the planner would split K on these volumes
            tuning(**{"M355_H16_W8": w8, "M355_H16_ONESHOT": 3, "M355_CONV_KSPLIT": 1, **env})
            fused = groups is not None and "M355_CONV_KSPLIT" not in env
            if fused:
                y, mean, rstd = hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute, groups=groups)
            else:
                y, mean, rstd = hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute), None, None
            y16 = hip.conv3d_fwd_h16_c8(x16, ci, (D, H, W), w, b, compute=compute)
            dx = hip.conv3d_bwd_data_h16(dy16, co, w, x.shape, compute=compute)
            out[w8] = (y, y16, dx)
            if w8 == 2:
                assert hip.conv_plan((N, ci, D, H, W), co, compute)[0] == 5, "the 8-wave variant was not selected"
                close(y, oracle.conv3d_fwd(x, w, b, compute=compute), 3e-5, 3e-5, "8-wave fwd")
                close(dx, oracle.conv3d_bwd_data(dy, w, x.shape, compute=compute), 3e-5, 3e-5, "8-wave bwd_data")
                assert torch.equal(_c8_to_ncdhw(y16, co, (D, H, W)), y.cpu().to(dt).float())
                if fused:
                    m2, r2 = hip.norm_stats(y, groups)[:2]
                    close(mean, m2, 1e-5, 1e-6, "fused mean")
                    close(rstd, r2, 1e-5, 1e-6, "fused rstd")
        for a, bb, what in zip(out[2], out[0], ("fwd", "c8 out", "bwd_data")):
            assert torch.equal(a, bb), f"8-wave {what} != 4-wave {what} (same k order: must be bit-identical)"
        # and the default one-item-per-workgroup variant of the same kernel
        tuning(**{"M355_H16_ONESHOT": 2, "M355_CONV_KSPLIT": 1, **{k: v for k, v in env.items() if k != "M355_CONV_SLOTS"}})
        assert hip.conv_plan((N, ci, D, H, W), co, compute)[0] == 6
        one = (hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute),
               hip.conv3d_fwd_h16_c8(x16, ci, (D, H, W), w, b, compute=compute),
               hip.conv3d_bwd_data_h16(dy16, co, w, x.shape, compute=compute))
        if "M355_CONV_KSPLIT" not in env:
            for a, bb, what in zip(one, out[0], ("fwd", "c8 out", "bwd_data")):
                assert torch.equal(a, bb), f"one-shot {what} != queue-driven {what}"


def _c8_to_ncdhw(x16, Cc, spatial):
    N, CB, S, _ = x16.shape
    return x16.float().cpu().permute(0, 1, 3, 2).reshape(N, CB * 8, S)[:, :Cc].reshape(N, Cc, *spatial)


def test_norm_act_with_pooled_second_output(hip, oracle):
    """m355_norm_act_pool_fwd: the encoder block's last normalise + activation pass also emits AvgPool3d(2, 2) of its
    result == m355_norm_act_fwd followed by m355_avgpool3d_2x_fwd, bit for bit (GroupNorm / BatchNorm geometry,
    ReLU / LeakyReLU, N = 2, non-cubic even sizes), and == the oracle."""
    for (N, Cc, D, H, W, groups, act) in [(2, 16, 4, 6, 8, 4, 1), (1, 12, 2, 4, 6, 0, 2), (1, 40, 8, 4, 32, 8, 1), (1, 3, 6, 2, 2, 0, 0)]:
        x = rnd(N, Cc, D, H, W, seed=1)
        gamma, beta = rnd(Cc, seed=2) * 0.5 + 1.0, rnd(Cc, seed=3) * 0.1
        mean, rstd = oracle.norm_stats(x, groups)[:2]
        y, pooled = hip.norm_act_pool_fwd(x, mean, rstd, gamma, beta, groups, act)
        y2 = hip.norm_act_fwd(x, mean, rstd, gamma, beta, groups, act)
        assert torch.equal(y, y2) and torch.equal(pooled, hip.avgpool_fwd(y2))
        close(pooled, oracle.avgpool_fwd(oracle.norm_act_fwd(x, mean, rstd, gamma, beta, groups, act)), 1e-5, 1e-6, "pooled")


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_norm_act_bwd_with_c8_twin(hip, oracle, compute):
    """m355_norm_act_bwd_h16: dx / dgamma / dbeta bit-identical to m355_norm_act_bwd, and the c8 twin of dx == dx
    rounded once (GroupNorm and BatchNorm geometry, channel counts that are no multiple of 8, N = 2, eval mode)."""
    dt = torch.bfloat16 if compute == 1 else torch.float16
    for (N, Cc, D, H, W, groups, act, training) in [(2, 16, 4, 6, 8, 4, 1, 1), (1, 12, 2, 4, 6, 0, 2, 1), (1, 40, 4, 4, 32, 8, 1, 1),
                                                    (2, 13, 3, 5, 7, 0, 1, 0)]:
        x, dy = rnd(N, Cc, D, H, W, seed=1), rnd(N, Cc, D, H, W, seed=6)
        gamma, beta = rnd(Cc, seed=2) * 0.5 + 1.0, rnd(Cc, seed=3) * 0.1
        mean, rstd = oracle.norm_stats(x, groups)[:2]
        dx0, dg0, db0 = hip.norm_act_bwd(x, dy, mean, rstd, gamma, beta, groups, act, training=training)
        dx, dg, db, dx16 = hip.norm_act_bwd_h16(x, dy, mean, rstd, gamma, beta, groups, act, compute, training=training)
        assert torch.equal(dx, dx0) and torch.equal(dg, dg0) and torch.equal(db, db0)
        assert torch.equal(_c8_to_ncdhw(dx16, Cc, (D, H, W)), dx.cpu().to(dt).float())
        if Cc % 8:
            assert (dx16[:, -1, :, Cc % 8:].float() == 0).all()


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_norm_act_and_avgpool_c8_outputs(hip, oracle, compute):
    """m355_norm_act_fwd_h16 == the fp32 pass followed by one rounding to the 16-bit type (GroupNorm and BatchNorm
    geometry, residual add, channel counts that are no multiple of 8, optional fp32 twin output);
    m355_avgpool3d_2x_fwd_h16 == the fp32 pool of the 16-bit values followed by one rounding."""
    dt = torch.bfloat16 if compute == 1 else torch.float16
    for (N, Cc, D, H, W, groups, act, with_add) in [(2, 16, 4, 6, 8, 4, 1, False), (1, 12, 2, 4, 6, 0, 2, True),
                                                    (1, 40, 4, 4, 32, 8, 1, True)]:
        x = rnd(N, Cc, D, H, W, seed=1)
        gamma, beta = rnd(Cc, seed=2) * 0.5 + 1.0, rnd(Cc, seed=3) * 0.1
        add = rnd(N, Cc, D, H, W, seed=4) if with_add else None
        mean, rstd = oracle.norm_stats(x, groups)[:2]
        ref = oracle.norm_act_fwd(x, mean, rstd, gamma, beta, groups, act, add)
        y16, y32 = hip.norm_act_fwd_h16(x, mean, rstd, gamma, beta, groups, act, compute, add=add, want_f32=True)
        close(y32, ref, 1e-5, 1e-5, "fp32 twin")
        got = _c8_to_ncdhw(y16, Cc, (D, H, W))
        # one rounding of (a value within 1e-5 of) the fp32 result: at most one 16-bit ulp apart
        ulp = (2.0 ** -8 if compute == 1 else 2.0 ** -11)
        assert ((got - ref).abs() <= ulp * ref.abs() * 1.01 + 2e-5).all()
        assert torch.equal(got, y32.cpu().to(dt).float()), "c8 output must be the rounding of the fp32 output"
        if Cc % 8:
            assert (y16[:, -1, :, Cc % 8:].float() == 0).all(), "padded channels of the last block must be zero"
        p16 = hip.avgpool_fwd_h16(y16, Cc, (D, H, W), compute)
        pref = torch.nn.functional.avg_pool3d(got, 2, 2).to(dt).float()
        pg = _c8_to_ncdhw(p16, Cc, (D // 2, H // 2, W // 2))
        assert ((pg - pref).abs() <= ulp * pref.abs() * 1.01 + 1e-6).all()


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("env", [{"M355_CONV_KSPLIT": "1"}, {"M355_CONV_KSPLIT": "2", "M355_CONV_SLOTS": "5", "M355_H16_ONESHOT": "3"},
                                 {"M355_CONV_KSPLIT": "1", "M355_CONV_NTW": "1"}, {"M355_CONV_KSPLIT": "2"}])
def test_conv3d_h16_c8_output_and_c8_norm(hip, oracle, compute, env, tuning):
    """m355_conv3d_fwd_h16_c8: the epilogue writes c8 (lanes exchange channel halves with v_permlane32_swap) ==
    the fp32-output kernel's result rounded once; statistics fused (fp32, before rounding: conv epilogue, or the
    reduction pass of a split-K plan) and taken from the c8 tensor (m355_act16_channel_partials);
    m355_norm_act_fwd_c8 (c8 -> c8, residual in c8)."""
    tuning(**env)
    dt = torch.bfloat16 if compute == 1 else torch.float16
    ulp = 2.0 ** -8 if compute == 1 else 2.0 ** -11
    for (N, ci, co, D, H, W, groups) in [(2, 16, 40, 9, 10, 36, 8), (1, 24, 13, 6, 21, 16, 0), (1, 32, 64, 8, 8, 32, 8),
                                         (2, 4, 40, 9, 10, 36, 8), (1, 3, 32, 5, 7, 64, 4)]:
        x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * (1.0 / (27 * ci) ** 0.5), rnd(co, seed=3)
        x16 = hip.act16_pack(x, compute)
        y32 = hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute).cpu()
        if ci <= 4:
            # the first conv of a network: conv3_c4_h16_kernel (four taps x 4 channels per k-step) where the plan allows --
            # the same products, another fp32 summation order than the fp32-output kernel: one 16-bit ulp at most
            y16, part = hip.conv3d_fwd_h16_c8(x16, ci, (D, H, W), w, b, compute=compute, with_stats=True)
            got = _c8_to_ncdhw(y16, co, (D, H, W))
            assert ((got - y32).abs() <= ulp * y32.abs() * 1.01 + 2e-5).all()
            assert (y16[:, -1, :, co % 8:].float() == 0).all() if co % 8 else True
            s1 = part[..., 0].sum(dim=1).cpu().double()
            torch.testing.assert_close(s1, y32.double().sum(dim=(2, 3, 4)), rtol=1e-4, atol=1e-3)
            s2 = part[..., 1].sum(dim=1).cpu().double()
            torch.testing.assert_close(s2, (y32.double() ** 2).sum(dim=(2, 3, 4)), rtol=1e-4, atol=1e-3)
            ref = oracle.conv3d_fwd(x.to(dt).float(), w.to(dt).float(), b)
            assert ((got - ref).abs() <= ulp * ref.abs() * 1.01 + 3e-5).all()
            continue
        # statistics partials: from the conv epilogue (unsplit plans) or from the split-K reduction pass -- of the fp32
        # values either way; and m355_act16_channel_partials over the finished c8 tensor (the rounded values)
        y16, part = hip.conv3d_fwd_h16_c8(x16, ci, (D, H, W), w, b, compute=compute, with_stats=True)
        assert torch.equal(y16, hip.conv3d_fwd_h16_c8(x16, ci, (D, H, W), w, b, compute=compute)), "same output without stats"
        got = _c8_to_ncdhw(y16, co, (D, H, W))
        assert torch.equal(got, y32.to(dt).float()), "c8 output == the fp32 output rounded once"
        if co % 8:
            assert (y16[:, -1, :, co % 8:].float() == 0).all()
        for pp, src in ((part, y32), (hip.act16_channel_partials(y16, co, compute), got)):
            s1 = pp[..., 0].sum(dim=1).cpu().double()
            s2 = pp[..., 1].sum(dim=1).cpu().double()
            torch.testing.assert_close(s1, src.double().sum(dim=(2, 3, 4)), rtol=1e-4, atol=1e-3)
            torch.testing.assert_close(s2, (src.double() ** 2).sum(dim=(2, 3, 4)), rtol=1e-4, atol=1e-3)
        # c8 -> c8 normalise + activation + residual
        gamma, beta = rnd(co, seed=4) * 0.5 + 1.0, rnd(co, seed=5) * 0.1
        mean, rstd = oracle.norm_stats(got, groups)[:2]
        res = rnd(N, co, D, H, W, seed=6)
        res16 = hip.act16_pack(res, compute)
        a16 = hip.norm_act_fwd_c8(y16, co, mean, rstd, gamma, beta, groups, 1, compute, add16=res16)
        ref = oracle.norm_act_fwd(got, mean, rstd, gamma, beta, groups, 1, res.to(dt).float())
        ga = _c8_to_ncdhw(a16, co, (D, H, W))
        assert ((ga - ref).abs() <= ulp * ref.abs() * 1.01 + 2e-5).all()


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_conv_transpose3d_c8(hip, oracle, compute):
    """m355_conv_transpose3d_fwd_h16 (k2 s2, c8 -> c8, exact fp32 arithmetic inside) == the oracle on the 16-bit
    input values, rounded once to the 16-bit type; ragged channel counts and voxel tiles."""
    dt = torch.bfloat16 if compute == 1 else torch.float16
    ulp = 2.0 ** -8 if compute == 1 else 2.0 ** -11
    for (N, ci, co, D, H, W) in [(1, 64, 64, 4, 4, 8), (2, 24, 40, 3, 5, 6), (1, 320, 48, 2, 2, 2), (1, 8, 13, 4, 4, 4)]:
        x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(ci, co, 2, 2, 2, seed=2) * 0.2, rnd(co, seed=3)
        x16 = hip.act16_pack(x, compute)
        ref = oracle.convt_fwd(x.to(dt).float(), w, b, 2, 0, 0)
        y16 = hip.conv_transpose3d_fwd_h16(x16, ci, (D, H, W), w, b, compute)
        got = _c8_to_ncdhw(y16, co, (2 * D, 2 * H, 2 * W))
        assert ((got - ref).abs() <= ulp * ref.abs() * 1.01 + 2e-5).all()
        if co % 8:
            assert (y16[:, -1, :, co % 8:].float() == 0).all()


@pytest.mark.parametrize("compute", [1, 2])
def test_conv_transpose3d_c8_large_levels_on_16bit_mfma(hip, oracle, compute, tuning):
    """From 16k voxels per sample the c8 conv-transpose runs on v_mfma_f32_32x32x16_{bf16,f16}
    (convt_k2s2_fwd_h16_kernel): weights rounded to the 16-bit type like every other operand of the mode, fp32
    accumulation, 64 consecutive 16-byte items per store.  == the oracle on the rounded operands (output rounded
    once); ragged channel counts (odd number of input channel blocks, Cout not a multiple of 8), ragged voxel
    tiles, N = 2, both k-step widths; and == the fp32-MFMA c8 kernel (M355_CONVT_H16=0) to operand rounding."""
    dt = torch.bfloat16 if compute == 1 else torch.float16
    ulp = 2.0 ** -8 if compute == 1 else 2.0 ** -11
    for (N, ci, co, D, H, W) in [(1, 64, 32, 16, 32, 32), (1, 128, 64, 16, 32, 32), (1, 24, 40, 17, 31, 33), (2, 16, 8, 16, 32, 32),
                                 (1, 72, 13, 8, 64, 32)]:
        x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(ci, co, 2, 2, 2, seed=2) * 0.2, rnd(co, seed=3)
        x16 = hip.act16_pack(x, compute)
        ref = oracle.convt_fwd(x.to(dt).float(), w.to(dt).float(), b, 2, 0, 0)
        tuning(M355_CONVT_H16=1)
        y16 = hip.conv_transpose3d_fwd_h16(x16, ci, (D, H, W), w, b, compute)
        got = _c8_to_ncdhw(y16, co, (2 * D, 2 * H, 2 * W))
        assert ((got - ref).abs() <= ulp * ref.abs() * 1.01 + 1e-4).all(), (ci, co, (got - ref).abs().max().item())
        if co % 8:
            assert (y16[:, -1, :, co % 8:].float() == 0).all()
        tuning(M355_CONVT_H16=0)
        old = _c8_to_ncdhw(hip.conv_transpose3d_fwd_h16(x16, ci, (D, H, W), w, b, compute), co, (2 * D, 2 * H, 2 * W))
        close(got, old, 4 * ulp, 4 * ulp * (ci ** 0.5) * 0.2, "vs the fp32-weight c8 kernel")


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["unet_gn_convt.npz", "unet_default_bn.npz", "unet_res_blur.npz"])
def test_c8_inference_flow_matches_fp32_golden_and_autograd_path(golden, mode, name):
    """Under no_grad in a 16-bit precision mode the activations between conv -> norm/act -> conv -> pool flow only
    in c8 (ops.Act16; trilinear / conv-transpose / Blur convs through their fp32 fallbacks): the result stays within
    the mode's tolerance of the fp32 reference golden and close to the same mode's autograd-recording path."""
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd import ops
    from test_model_gpu import BUILDERS
    g = golden(name)
    model = BUILDERS[name][0]()
    model.load_state_dict(g.state_dict("m.sd."))
    model = model.cuda().eval()
    x = g.t("x").cuda()
    tol = 2e-2 if mode == "bf16" else 5e-3
    with sp.precision(mode):
        with torch.no_grad():
            assert ops.h16_flow() != 0
            p_flow = model(x)
        assert ops.h16_flow() != 0           # autograd on: the c8-only TRAINING flow (round 3), same forward kernels
        p_grad = model(x).detach()
        try:                                 # ... and the round-2 twin flow (fp32 tensors beside the c8 operands)
            ops.H16_TRAIN_C8ONLY = False
            assert ops.h16_flow() == 0
            p_twin = model(x).detach()
        finally:
            ops.H16_TRAIN_C8ONLY = True
    with torch.no_grad():
        p32 = model(x)                       # exact fp32 mode (itself pinned to the golden by test_model_gpu.py)
    if name == "unet_gn_convt.npz":          # BatchNorm goldens were taken after a training step moved the statistics
        assert (p32.cpu() - g.t("m.probs_eval")).abs().max().item() <= 1e-4
        assert torch.equal(p_flow, p_grad), "the c8 training flow's forward is the no-grad c8 flow, bit for bit"
    assert (p_flow - p32).abs().max().item() <= 2 * tol
    assert (p_flow - p_grad).abs().max().item() <= tol
    assert (p_flow - p_twin).abs().max().item() <= tol
    assert (p_flow.sum(dim=1) - 1).abs().max().item() <= 1e-5
    assert (p_flow - p_twin).abs().max().item() > 0 or name != "unet_gn_convt.npz"   # really a different data path


def _grads_as_accurate_as_the_rounded_oracle(g, model, mode, x, y, all_cos_min, cos_min):
    """The composed c8 training flow on the small north-star golden: its parameter gradients against the REFERENCE's
    fp32 gradients (the golden) must be as accurate as those of the rounding-matched oracle (oracle.torch_ref with
    `rounding=mode`: same operand / activation / gradient roundings, fp32 everything else): per parameter the relative L2
    distance to the golden at most 3x the oracle's (+ 0.03), plus bounds on direction and size.  (See
    tests/test_fullsize_gpu.py::_composed_16bit_training_check for why a deep network cannot match the rounded oracle
    element by element.)"""
    from oracle import torch_ref as R
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in g.state_dict("m.sd.").items()}
    spec = R.UNetSpec(4, 3, [8, 16, 32], 3, norm="group", groups=8, up="convT", rounding=mode)
    ld = R.hybrid_logistic_dice_loss(R.unet_forward(sd, spec, x, training=True), y)
    ld["loss"].backward()
    dot = na = nb = 0.0
    for k, v in model.named_parameters():
        ref = g.t(f"m.grad.{k}").double().flatten()
        got, orc = v.grad.cpu().double().flatten(), sd[k].grad.double().flatten()
        assert torch.isfinite(got).all()
        cos = float(got @ ref / (got.norm() * ref.norm() + 1e-30))
        rel, rel_o = float((got - ref).norm() / ref.norm()), float((orc - ref).norm() / ref.norm())
        assert cos >= cos_min, (k, cos)
        assert rel <= 3.0 * rel_o + 0.03, (k, rel, rel_o)      # (bounds the size of the gradient as well)
        dot, na, nb = dot + float(got @ ref), na + float(got @ got), nb + float(ref @ ref)
    assert dot / (na * nb) ** 0.5 >= all_cos_min, dot / (na * nb) ** 0.5


def test_fp16_precision_mode_end_to_end(golden):
    """cfg5-family precision mode ("mixed fp16 with MFMA channel-GEMM path"): fp16 operands, fp32 accumulate,
    on the small north-star model: 10 mantissa bits, so closer to the fp32 golden than bf16 (5e-3 / 2e-4)."""
    from functools import partial
    from torch import nn
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss
    from segmentation_pipeline_amd.models import ModularUNet
    g = golden("unet_gn_convt.npz")
    model = ModularUNet(4, 3, [8, 16, 32], 3, block_params={'normalization_class': partial(nn.GroupNorm, 8)},
                        upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2})
    model.load_state_dict(g.state_dict("m.sd."))
    model = model.cuda().train()
    x, y = g.t("x").cuda(), g.t("y").cuda()
    with sp.precision("fp16"):
        p = model(x)
        ld = HybridLogisticDiceLoss()(p, y)
        ld["loss"].backward()
    assert sp.get_precision() == "fp32"
    err = (p.detach().cpu() - g.t("m.probs_train")).abs().max().item()
    assert 1e-7 < err <= 5e-3, err
    assert abs(ld["dice_loss"].item() - float(g["m.dice_loss"])) <= 2e-4
    _grads_as_accurate_as_the_rounded_oracle(g, model, "fp16", x.cpu(), y.cpu(), all_cos_min=0.9995, cos_min=0.98)


def test_c8_twin_of_the_training_flow_is_voided_by_in_place_modification():
    """16-bit training flow: norm_act attaches the c8 twin of its fp32 result for the convolution that follows
    (ops._c8_twin).  The convolution must use it (same bits as packing the tensor itself) and must NOT use it after the
    fp32 tensor was modified in place (the twin is recorded with the tensor's version)."""
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd import ops, _lib
    with sp.precision("bf16"):
        x = rnd(1, 16, 8, 8, 32, seed=1).cuda().requires_grad_()
        gamma, beta = torch.ones(16, device="cuda"), torch.zeros(16, device="cuda")
        w = (rnd(8, 16, 3, 3, 3, seed=2) * 0.1).cuda().requires_grad_()
        y = ops.norm_act(x, gamma, beta, ops.NormCfg(groups=4, eps=1e-5, act=_lib.ACT_RELU))
        assert ops._c8_twin(y, _lib.COMPUTE_BF16) is not None, "norm_act did not attach a twin in the 16-bit training flow"
        assert torch.equal(ops.conv3d(y, w), ops.conv3d(y.detach().clone(), w)), "conv from the twin != conv from the packed tensor"
        with torch.no_grad():
            y.mul_(2.0)
        assert ops._c8_twin(y, _lib.COMPUTE_BF16) is None, "a stale twin survived an in-place modification"
        assert torch.equal(ops.conv3d(y, w), ops.conv3d(y.detach().clone(), w))


def test_bf16_precision_mode_end_to_end(golden):
    """cfg3-family precision mode on the small north-star model: probabilities within 2e-2 and soft
    Dice within 1e-3 of the fp32 reference golden (tolerances stated for the bf16 configs in SURVEY §8d);
    gradients flow; fp32 mode is restored afterwards."""
    from functools import partial
    from torch import nn
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss
    from segmentation_pipeline_amd.models import ModularUNet
    g = golden("unet_gn_convt.npz")
    model = ModularUNet(4, 3, [8, 16, 32], 3, block_params={'normalization_class': partial(nn.GroupNorm, 8)},
                        upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2})
    model.load_state_dict(g.state_dict("m.sd."))
    model = model.cuda().train()
    x, y = g.t("x").cuda(), g.t("y").cuda()
    with sp.precision("bf16"):
        assert sp.get_precision() == "bf16"
        p = model(x)
        ld = HybridLogisticDiceLoss()(p, y)
        ld["loss"].backward()
    assert sp.get_precision() == "fp32"
    err = (p.detach().cpu() - g.t("m.probs_train")).abs().max().item()
    assert 1e-6 < err <= 2e-2, err                     # really a different arithmetic, within the stated tolerance
    assert abs(ld["dice_loss"].item() - float(g["m.dice_loss"])) <= 1e-3
    _grads_as_accurate_as_the_rounded_oracle(g, model, "bf16", x.cpu(), y.cpu(), all_cos_min=0.999, cos_min=0.95)
    with pytest.raises(ValueError):
        sp.set_precision("fp8")


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", [(1, 32, 32, 8, 16, 64), (2, 40, 33, 5, 6, 32), (1, 96, 64, 4, 4, 32), (1, 16, 16, 8, 8, 16),
                                  (2, 24, 9, 3, 7, 21)])
def test_conv3d_bwd_weight_bf16_mode(hip, oracle, case, compute):
    """The plain entry point (fp32 NCDHW operands) in a 16-bit compute mode, both channel counts > 4: the operands are
    rounded into c8 copies and the c8 weight-gradient kernel runs (any W since round 4: the round-1 kernel of this entry
    needed W % 32 == 0); checked against the oracle with equally rounded operands."""
    N, Ci, Co, D, H, W = case
    x, dy = rnd(N, Ci, D, H, W, seed=1), rnd(N, Co, D, H, W, seed=5)
    dw_h, db_h = hip.conv3d_bwd_weight(x, dy, 3, compute=compute)
    dw_o, db_o = oracle.conv3d_bwd_weight(x, dy, 3, compute=compute)
    close(dw_h, dw_o, 3e-5, 3e-5 * (N * D * H * W) ** 0.5, "bf16 bwd_weight vs bf16 oracle")
    close(db_h, db_o, 3e-5, 3e-5 * (N * D * H * W) ** 0.5, "dbias")
    (d1, _), (d2, _) = hip.conv3d_bwd_weight(x, dy, 3, compute=compute), hip.conv3d_bwd_weight(x, dy, 3, compute=compute)
    assert torch.equal(d1, d2)


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("env", [{}, {"M355_BWW_NSPLIT": "1"}, {"M355_BWW_NSPLIT": "5"}])
def test_conv3d_bwd_weight_from_c8_operands(hip, oracle, compute, env, tuning):
    """m355_conv3d_bwd_weight_h16: x and dy handed over as c8 (what the 16-bit training flow holds anyway), voxel-major
    LDS tiles read through ds_read_b64_tr_b16.  == the oracle on the operands rounded to the 16-bit type (products
    exact in fp32, fp32 accumulation); ragged volumes (W no multiple of 32, odd D / H), ragged channel counts (odd
    number of c8 blocks, partial 32-channel tiles), N = 2, one split and several; bit-reproducible."""
    tuning(**env)
    for (N, ci, co, D, H, W) in [(1, 32, 32, 4, 8, 32), (1, 96, 32, 6, 8, 64), (2, 24, 40, 5, 7, 33), (1, 72, 8, 3, 9, 20),
                                 (1, 16, 100, 4, 4, 16)]:
        x, dy = rnd(N, ci, D, H, W, seed=1), rnd(N, co, D, H, W, seed=5)
        x16, dy16 = hip.act16_pack(x, compute), hip.act16_pack(dy, compute)
        dw, db = hip.conv3d_bwd_weight_h16(x16, dy16, dy, ci, co, (D, H, W), compute)
        dwo, dbo = oracle.conv3d_bwd_weight(x, dy, 3, compute=compute)
        tol = 3e-5 * (N * D * H * W) ** 0.5
        close(dw, dwo, 3e-5, tol, f"bwd_weight from c8 {ci}->{co}")
        close(db, dbo, 3e-5, tol, "dbias")
        assert torch.equal(dw, hip.conv3d_bwd_weight_h16(x16, dy16, dy, ci, co, (D, H, W), compute)[0])


def test_conv3d_bwd_weight_bf16_mode_falls_back_to_exact_fp32(hip, oracle):
    """The edge layers (<= 4 channels on one side) of the plain entry point stay exact fp32."""
    for (N, Ci, Co, D, H, W) in [(1, 32, 3, 8, 8, 16), (1, 4, 32, 8, 8, 32)]:
        x, dy = rnd(N, Ci, D, H, W, seed=1), rnd(N, Co, D, H, W, seed=5)
        dw_h, _ = hip.conv3d_bwd_weight(x, dy, 3, compute=1)
        dw_o, _ = oracle.conv3d_bwd_weight(x, dy, 3, compute=0)
        close(dw_h, dw_o, 3e-5, 3e-5 * (N * D * H * W) ** 0.5, "fallback")


# ----------------------------------------------------------------- c8-only training flow (round 3)
def _ulp(compute):
    return 2.0 ** -8 if compute == 1 else 2.0 ** -11


def _dt(compute):
    return torch.bfloat16 if compute == 1 else torch.float16


def _rounded_close(got, ref, compute, atol, what):
    """`got` = one rounding to the 16-bit type of (a value within atol of) `ref`"""
    bad = (got - ref).abs() > _ulp(compute) * ref.abs() * 1.01 + atol
    assert not bad.any(), f"{what}: {int(bad.sum())} elements off, worst {(got - ref).abs().max().item():.3e}"


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_act16_pack_unpack_scaled(hip, compute):
    """the loss scale enters where a gradient becomes c8: pack == round(x * scale), saturating at the fp16 range
    (an inf would poison every downstream sum); unpack removes it"""
    dt = _dt(compute)
    x = rnd(2, 13, 3, 5, 7, seed=1) * 1e-3
    x[0, 0, 0, 0, 0], x[1, 2, 1, 1, 1] = 3.0, -5.0
    scale = 2.0 ** 15
    x16 = hip.act16_pack_scaled(x, compute, scale)
    want = (x * scale)
    if compute == 2:
        want = want.clamp(-65504.0, 65504.0)
    assert torch.equal(_c8_to_ncdhw(x16, 13, (3, 5, 7)), want.to(dt).float())
    assert (x16[:, -1, :, 13 % 8:].float() == 0).all()
    back = hip.act16_unpack_scaled(x16, 13, (3, 5, 7), compute, 1.0 / scale)
    assert torch.equal(back.cpu(), want.to(dt).float() / scale)


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("env", [{}, {"M355_CONV_KSPLIT": "2"}])
def test_conv3d_bwd_data_c8_output_and_weight_gradient_c8(hip, oracle, compute, env, tuning):
    """m355_conv3d_bwd_data_h16_c8 == m355_conv3d_bwd_data_h16 rounded once; m355_conv3d_bwd_weight_c8: dw bit-identical to
    m355_conv3d_bwd_weight_h16 (same kernel, unscale 1), the bias gradient reduced from the c8 gradient itself, and
    grad_unscale applied to both in the fp32 epilogue"""
    tuning(**env)
    dt = _dt(compute)
    for (N, ci, co, D, H, W) in [(2, 16, 40, 5, 6, 36), (1, 24, 13, 6, 9, 16), (1, 4, 32, 8, 8, 32), (1, 32, 3, 4, 8, 32),
                                 (2, 3, 40, 5, 7, 33), (1, 72, 2, 3, 6, 20), (1, 4, 4, 4, 4, 32)]:
        x, dy = rnd(N, ci, D, H, W, seed=1), rnd(N, co, D, H, W, seed=2)
        w = rnd(co, ci, 3, 3, 3, seed=3) * (1.0 / (27 * co) ** 0.5)
        x16, dy16 = hip.act16_pack(x, compute), hip.act16_pack(dy, compute)
        dx32 = hip.conv3d_bwd_data_h16(dy16, co, w, (N, ci, D, H, W), compute).cpu()
        dx16 = hip.conv3d_bwd_data_h16_c8(dy16, co, w, (N, ci, D, H, W), compute)
        if co > 4:
            assert torch.equal(_c8_to_ncdhw(dx16, ci, (D, H, W)), dx32.to(dt).float())
        else:    # <= 4 K-channels: conv3_c4_h16_kernel (four taps per k-step): the same products in another fp32 order
            _rounded_close(_c8_to_ncdhw(dx16, ci, (D, H, W)), dx32, compute, 2e-5 * dx32.abs().max().item(), "edge-layer dx")
        if ci % 8:
            assert (dx16[:, -1, :, ci % 8:].float() == 0).all()
        dw0, _ = hip.conv3d_bwd_weight_h16(x16, dy16, dy, ci, co, (D, H, W), compute)
        dw, db = hip.conv3d_bwd_weight_c8(x16, dy16, ci, co, (D, H, W), compute)
        if min(ci, co) > 4:
            assert torch.equal(dw, dw0)
        else:   # edge layers: conv3_bww_c8_small_kernel (tap and narrow channel share the MFMA column), another sum order
            close(dw, dw0, 2e-5, 2e-5 * dw0.abs().max().item(), "edge-layer dw vs the padded-tile kernel")
        dyr = dy.to(dt).float()
        close(db, dyr.double().sum(dim=(0, 2, 3, 4)).float(), 1e-5, 1e-4, "dbias from c8")
        dws, dbs = hip.conv3d_bwd_weight_c8(x16, dy16, ci, co, (D, H, W), compute, unscale=2.0 ** -7)
        assert torch.equal(dws, dw * 2.0 ** -7)
        close(dbs, db * 2.0 ** -7, 1e-6, 1e-7, "dbias unscale")
        # and against the oracle on the rounded operands
        ref_dw, _ = oracle.conv3d_bwd_weight(x.to(dt).float(), dyr, 3)
        close(dw, ref_dw, 3e-5, 3e-5 * ref_dw.abs().max().item(), "dw vs oracle")


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_norm_act_bwd_c8(hip, oracle, compute):
    """m355_norm_act_bwd_c8 == the oracle's backward on the 16-bit values (x16 = pre-norm tensor; incoming gradient =
    dy16 + un-pooled dpool16, either alone or both), dx rounded once; dgamma / dbeta fp32 with grad_unscale.
    GroupNorm / BatchNorm geometry, ReLU / LeakyReLU / none, N = 2, ragged channel counts, eval mode."""
    dt = _dt(compute)
    cases = [(2, 16, 4, 6, 8, 4, 1, 1, "both"), (1, 12, 2, 4, 6, 0, 2, 1, "dy"), (1, 40, 4, 4, 32, 8, 1, 1, "pool"),
             (2, 13, 2, 6, 8, 0, 1, 0, "both"), (1, 8, 34, 32, 32, 2, 0, 1, "dy"), (2, 120, 3, 3, 3, 0, 1, 1, "dy")]
    for (N, Cc, D, H, W, groups, act, training, src) in cases:
        x, dy = rnd(N, Cc, D, H, W, seed=1), rnd(N, Cc, D, H, W, seed=6)
        dp = rnd(N, Cc, D // 2, H // 2, W // 2, seed=7)
        gamma, beta = rnd(Cc, seed=2) * 0.5 + 1.0, rnd(Cc, seed=3) * 0.1
        x16 = hip.act16_pack(x, compute)
        dy16 = hip.act16_pack(dy, compute) if src in ("dy", "both") else None
        dp16 = hip.act16_pack(dp, compute) if src in ("pool", "both") else None
        xr = x.to(dt).float()
        g = torch.zeros_like(x)
        if dy16 is not None:
            g = g + dy.to(dt).float()
        if dp16 is not None:
            g = g + 0.125 * dp.to(dt).float().repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)
        mean, rstd = oracle.norm_stats(xr, groups)[:2]
        ref_dx, ref_dg, ref_db = oracle.norm_act_bwd(xr, g, mean, rstd, gamma, beta, groups, act, training=training)
        dx16, dg, db = hip.norm_act_bwd_c8(x16, dy16, dp16, Cc, (D, H, W), mean, rstd, gamma, beta, groups, act, compute,
                                           training=training)
        scale = ref_dx.abs().max().item()
        _rounded_close(_c8_to_ncdhw(dx16, Cc, (D, H, W)), ref_dx, compute, 2e-5 * scale, f"dx {(N, Cc, groups, act, src)}")
        close(dg, ref_dg, 1e-4, 1e-4 * ref_dg.abs().max().item(), "dgamma")
        close(db, ref_db, 1e-4, 1e-4 * ref_db.abs().max().item(), "dbeta")
        if Cc % 8:
            assert (dx16[:, -1, :, Cc % 8:].float() == 0).all()
        _, dg2, db2 = hip.norm_act_bwd_c8(x16, dy16, dp16, Cc, (D, H, W), mean, rstd, gamma, beta, groups, act, compute,
                                          training=training, unscale=0.25)
        close(dg2, dg * 0.25, 1e-6, 1e-7, "dgamma unscale")
        close(db2, db * 0.25, 1e-6, 1e-7, "dbeta unscale")


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_avgpool_bwd_c8(hip, compute):
    dt = _dt(compute)
    for (N, Cc, D, H, W) in [(2, 16, 4, 6, 8), (1, 13, 2, 4, 34)]:
        dp, sk = rnd(N, Cc, D // 2, H // 2, W // 2, seed=1), rnd(N, Cc, D, H, W, seed=2)
        dp16, sk16 = hip.act16_pack(dp, compute), hip.act16_pack(sk, compute)
        up = 0.125 * dp.to(dt).float().repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)
        got = _c8_to_ncdhw(hip.avgpool_bwd_h16(dp16, None, Cc, (D, H, W), compute), Cc, (D, H, W))
        assert torch.equal(got, up.to(dt).float())
        got = _c8_to_ncdhw(hip.avgpool_bwd_h16(dp16, sk16, Cc, (D, H, W), compute), Cc, (D, H, W))
        _rounded_close(got, up + sk.to(dt).float(), compute, 1e-7, "pool bwd + skip")


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_trilinear_upsample_c8(hip, compute):
    """m355_upsample_trilinear2x_{fwd,bwd}_h16 == nn.Upsample(scale_factor=2, mode='trilinear', align_corners=True) of
    the 16-bit operand values evaluated in fp32 (torch CPU) and rounded once -- forward and its autograd; ragged channel
    counts, sizes of 1 along an axis, N = 2, a padded destination (concat slot)."""
    dt = _dt(compute)
    up = torch.nn.Upsample(scale_factor=2, mode='trilinear', align_corners=True)
    for (N, Cc, D, H, W, pad) in [(2, 16, 3, 4, 5, 0), (1, 13, 6, 11, 3, 2), (1, 40, 1, 2, 7, 0), (1, 8, 12, 22, 6, 1)]:
        x = rnd(N, Cc, D, H, W, seed=1)
        xr = x.to(dt).float().requires_grad_()
        ref = up(xr)
        y16 = hip.upsample_trilinear2x_fwd_h16(hip.act16_pack(x, compute), Cc, (D, H, W), compute, pad_batch=pad)
        got = _c8_to_ncdhw(y16[:, :(Cc + 7) // 8], Cc, (2 * D, 2 * H, 2 * W))
        _rounded_close(got, ref.detach(), compute, 2e-6, f"trilinear fwd c8 {(N, Cc, D, H, W)}")
        if pad:
            assert (y16[:, (Cc + 7) // 8:] == 7.0).all(), "wrote outside its channel blocks"
        dy = rnd(N, Cc, 2 * D, 2 * H, 2 * W, seed=2)
        ref.backward(dy.to(dt).float())
        dx16 = hip.upsample_trilinear2x_bwd_h16(hip.act16_pack(dy, compute), Cc, (D, H, W), compute)
        _rounded_close(_c8_to_ncdhw(dx16, Cc, (D, H, W)), xr.grad, compute, 1e-5, f"trilinear bwd c8 {(N, Cc, D, H, W)}")
        assert torch.equal(dx16, hip.upsample_trilinear2x_bwd_h16(hip.act16_pack(dy, compute), Cc, (D, H, W), compute))


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_space_to_depth_c8(hip, oracle, compute):
    """m355_space_to_depth2_h16 / m355_depth_to_space2_h16 == the fp32 rearrangement of the 16-bit values (pure data
    movement: bit-exact), each the inverse of the other; channel counts that are no multiple of 8 (zero padding of the
    last block is kept), N = 2, a padded destination."""
    dt = _dt(compute)
    for (N, Cc, D, H, W, pad) in [(2, 16, 4, 6, 8, 0), (1, 13, 2, 4, 6, 1), (1, 40, 6, 2, 10, 0), (1, 3, 2, 2, 2, 2)]:
        x = rnd(N, Cc, D, H, W, seed=1)
        xr = x.to(dt).float()
        ref = oracle.space_to_depth(xr)                                   # [N, 8C, D/2, H/2, W/2]
        x16 = hip.act16_pack(x, compute)
        p16 = hip.s2d_h16(x16, (N, Cc, D, H, W), compute, True, pad_batch=pad)
        got = _c8_to_ncdhw(p16[:, :Cc], 8 * Cc, (D // 2, H // 2, W // 2))
        assert torch.equal(got, ref)
        if pad:
            assert (p16[:, Cc:] == 7.0).all(), "wrote outside its channel blocks"
        back = hip.s2d_h16(p16[:, :Cc].contiguous(), (N, Cc, D, H, W), compute, False, pad_batch=pad)
        CB = (Cc + 7) // 8
        assert torch.equal(back[:, :CB], x16), "depth-to-space is not the inverse (incl. the zero padding of the last block)"
        if pad:
            assert (back[:, CB:] == 7.0).all()


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_channel_scale_c8(hip, compute):
    """m355_act16_channel_scale (Dropout3d mask on a c8 activation): one rounding of x16 * scale[n, c]; channels past C
    stay zero; fp16 saturates instead of overflowing"""
    dt = _dt(compute)
    for (N, Cc, S3) in [(2, 13, (3, 5, 7)), (1, 40, (2, 4, 4))]:
        x = rnd(N, Cc, *S3, seed=1)
        scale = torch.where(rnd(N * Cc, seed=2) > 0, torch.tensor(2.0), torch.tensor(0.0))
        scale[1] = 1.25
        y16 = hip.act16_channel_scale(hip.act16_pack(x, compute), scale, Cc, compute)
        ref = x.to(dt).float() * scale.view(N, Cc, 1, 1, 1)
        _rounded_close(_c8_to_ncdhw(y16, Cc, S3), ref, compute, 0.0, "channel scale c8")
        if Cc % 8:
            assert (y16[:, -1, :, Cc % 8:] == 0).all()
    if compute == 2:
        big = torch.full((1, 8, 1, 1, 2), 60000.0)
        y16 = hip.act16_channel_scale(hip.act16_pack(big, compute), torch.full((8,), 4.0), 8, compute)
        assert torch.isfinite(y16.float()).all() and (y16.float() == 65504.0).all()


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_conv_transpose3d_c8_backward(hip, oracle, compute):
    """m355_conv_transpose3d_bwd_data_h16 / _bwd_weight_h16 (k2 s2, c8 operands, 16-bit MFMA) == the oracle on the
    16-bit operand values (weights rounded too in the data gradient), dx rounded once; ragged channel counts, voxel
    tiles that overhang, N = 2, grad_unscale; unsupported geometries are reported by the query."""
    dt = _dt(compute)
    assert not hip.convt_h16_bwd_supported((1, 320, 8, 8, 8), 256)
    for (N, ci, co, D, H, W) in [(1, 64, 32, 4, 4, 32), (2, 24, 40, 3, 5, 6), (1, 128, 64, 2, 2, 34), (1, 8, 13, 4, 4, 4),
                                 (1, 160, 16, 2, 3, 33)]:
        assert hip.convt_h16_bwd_supported((N, ci, D, H, W), co)
        x, dy = rnd(N, ci, D, H, W, seed=1), rnd(N, co, 2 * D, 2 * H, 2 * W, seed=2)
        w = rnd(ci, co, 2, 2, 2, seed=3) * 0.2
        x16, dy16 = hip.act16_pack(x, compute), hip.act16_pack(dy, compute)
        xr, dyr, wr = x.to(dt).float(), dy.to(dt).float(), w.to(dt).float()
        ref_dx = oracle.convt_bwd_data(dyr, wr, (N, ci, D, H, W), 2, 0, 0)
        dx16 = hip.convt_bwd_data_h16(dy16, w, (N, ci, D, H, W), compute)
        _rounded_close(_c8_to_ncdhw(dx16, ci, (D, H, W)), ref_dx, compute, 3e-5 * ref_dx.abs().max().item(),
                       f"convT dx {(N, ci, co, D, H, W)}")
        if ci % 8:
            assert (dx16[:, -1, :, ci % 8:].float() == 0).all()
        ref_dw, ref_db = oracle.convt_bwd_weight(xr, dyr, 2, 2, 0, 0)
        dw, db = hip.convt_bwd_weight_h16(x16, dy16, (N, ci, D, H, W), co, compute)
        close(dw, ref_dw, 3e-5, 3e-5 * ref_dw.abs().max().item(), f"convT dw {(N, ci, co, D, H, W)}")
        close(db, ref_db, 1e-5, 1e-4, "convT dbias")
        dw2, db2 = hip.convt_bwd_weight_h16(x16, dy16, (N, ci, D, H, W), co, compute, unscale=0.5)
        close(dw2, dw * 0.5, 1e-6, 1e-8, "convT dw unscale")
        close(db2, db * 0.5, 1e-6, 1e-8, "convT dbias unscale")


def test_patch_aggregate_grid_one_pass(hip, oracle):
    """m355_patch_aggregate_grid == the oracle (bit-exact: same fp32 sums in tile order, same division) == the batch-by-batch
    accumulate + finalize it replaces in PatchPredict (bit-exact), ragged grids with a short last step, several channels,
    and the cropped (padded-volume) form."""
    import itertools
    from segmentation_pipeline_amd.prediction import grid_axes
    for vshape, ps, ov, border in [((20, 17, 23), (8, 6, 10), (2, 2, 4), (0, 0, 0)), ((12, 12, 12), (8, 8, 8), (4, 4, 4), (2, 2, 2)),
                                   ((9, 30, 11), (9, 7, 5), (0, 3, 1), (0, 1, 0))]:
        pshape = tuple(v + 2 * b for v, b in zip(vshape, border))
        axes = grid_axes(pshape, ps, ov)
        locs = list(itertools.product(*axes))
        tiles = rnd(len(locs), 3, *ps, seed=4)
        got = hip.patch_aggregate_grid(tiles, axes, vshape, border)
        ref = oracle.patch_aggregate_grid(tiles, axes, vshape, border)
        assert torch.equal(got.cpu(), ref)
        # the accumulate + finalize path it replaces (padded volume, then the crop)
        old, _ = hip.patch_aggregate(tiles, torch.tensor(locs, dtype=torch.int32), pshape)
        sl = (slice(None),) + tuple(slice(b, b + v) for b, v in zip(border, vshape))
        assert torch.equal(got, old[sl])


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["unet_res_blur.npz", "unet_default_bn.npz", "nested_res_unet.npz"])
def test_c8_training_flow_architectures_with_fallback_ops(golden, mode, name):
    """Architectures whose ops have no c8 kernel, through the c8-only training flow: the msseg2 family (residual blocks,
    BatchNorm, BlurConv3d / BlurConvTranspose3d, class weights [1, 100]; odd voxel counts on the deep levels) and the
    reference's DEFAULT ModularUNet (BatchNorm, AvgPool, trilinear upsampling) -- Blur convs and the trilinear upsampling
    join through the differentiable unpack / pack functions (trilinear has a c8 kernel since) -- and NestedResUNet (residual
    blocks, 2-/3-way concats, AvgPool + trilinear, tensors with three consumers).  Against the reference's fp32 golden: probabilities within the
    mode's tolerance, every parameter gradient in the reference's direction, and close to the round-2 twin flow."""
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd import ops
    from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss
    from test_model_gpu import BUILDERS
    g = golden(name)

    def run():
        model = BUILDERS[name][0]()
        model.load_state_dict(g.state_dict("m.sd."))
        model = model.cuda().train()
        with sp.precision(mode):
            p = model(g.t("x").cuda())
            ld = HybridLogisticDiceLoss(logistic_class_weights=BUILDERS[name][1])(p, g.t("y").cuda())
            ld["loss"].backward()
        return p.detach().cpu(), {k: v.grad.cpu().double().flatten() for k, v in model.named_parameters() if v.grad is not None}
    p, grads = run()
    try:
        ops.H16_TRAIN_C8ONLY = False
        p_twin, grads_twin = run()
    finally:
        ops.H16_TRAIN_C8ONLY = True
    tol = 2e-2 if mode == "bf16" else 5e-3
    assert (p - g.t("m.probs_train")).abs().max().item() <= tol
    assert (p - p_twin).abs().max().item() <= tol
    assert set(grads) == set(grads_twin)
    def all_cosine(gr, check):
        dot = na = nb = 0.0
        for k, got in gr.items():
            ref = g.t(f"m.grad.{k}").double().flatten()
            assert torch.isfinite(got).all(), k
            if ref.norm() < 1e-9 * max(r.norm() for r in gr.values()):
                continue      # (a conv bias in front of BatchNorm: analytically zero)
            cos = float(got @ ref / (got.norm() * ref.norm() + 1e-300))
            if check and cos < (0.9 if mode == "bf16" else 0.97):
                # a parameter whose gradient is small against the rounding noise BatchNorm over few voxels amplifies
                # (8-element BN weights on the deep levels): no further from the reference than 2.5x the twin flow
                rel, rel_tw = float((got - ref).norm() / ref.norm()), float((grads_twin[k] - ref).norm() / ref.norm())
                assert rel <= 2.5 * rel_tw + 0.03, (k, cos, rel, rel_tw)
            dot, na, nb = dot + float(got @ ref), na + float(got @ got), nb + float(ref @ ref)
        return dot / (na * nb) ** 0.5
    # all parameters together: as close to the reference as the twin flow (whose activations are rounded at fewer
    # points; BatchNorm over a batch of 2 x 16^3 amplifies the rounding noise of both)
    c8, twin = all_cosine(grads, True), all_cosine(grads_twin, False)
    assert c8 >= min(0.995 if mode == "bf16" else 0.9995, twin - (0.01 if mode == "bf16" else 0.001)), (c8, twin)


SHORT_WS_CASES = [   # (Cin, Cout, compute, tuning): one descriptor per route kind the defaults reach, and a split-K plan
    *[(ci, co, comp, {}) for comp in (0, X3) for ci, co in ((4, 32), (32, 3), (32, 32), (24, 40))],
    (32, 32, 1, {}), (32, 3, 1, {}), (32, 32, 0, {"M355_CONV_KSPLIT": 2})]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHORT_WS_CASES, ids=lambda c: f"{c[0]}-{c[1]}-c{c[2]}" + ("-ks2" if c[3] else ""))
def test_conv3d_short_workspace_is_refused_and_writes_nothing(hip, tuning, case):
    """Every launching conv entry point, handed the full-size workspace buffer but a byte count one below what its
    query returned, answers M355_EWORKSPACE and leaves its outputs (canary slots) unwritten: the launch checks the very
    number the query reports.  (The buffer really is full-size, so a broken check cannot write out of bounds.)"""
    from raw_ops import Slot, _p
    EWORKSPACE = -4
    Cin, Cout, compute, env = case
    tuning(**env)
    N, D, H, W = 1, 8, 8, 32
    S = D * H * W
    L, dev, st = hip.lib, hip.device, hip._stream()
    x, dy, w = hip.to(rnd(N, Cin, D, H, W, seed=1)), hip.to(rnd(N, Cout, D, H, W, seed=2)), hip.to(rnd(Cout, Cin, 3, 3, 3, seed=3))
    bias = hip.to(rnd(Cout, seed=4))
    d = hip.conv_desc(x.shape, Cout, 3, 1, 1, compute=compute)
    ref = C.byref(d)
    y, dx = (lambda: Slot(dev, (N, Cout, D, H, W))), (lambda: Slot(dev, (N, Cin, D, H, W)))
    dw, db = (lambda: Slot(dev, (1, Cout * Cin * 27))), (lambda: Slot(dev, (1, Cout)))
    calls = [   # (entry point, workspace query result, outputs, arguments around (workspace, bytes, stream))
        ("conv3d_fwd", L.m355_conv3d_fwd_workspace(ref), lambda o: (ref, _p(x), _p(w), _p(bias), None, _p(o[0])), (y,)),
        ("conv3d_bwd_data", L.m355_conv3d_bwd_data_workspace(ref), lambda o: (ref, _p(dy), _p(w), _p(o[0])), (dx,)),
        ("conv3d_bwd_weight", L.m355_conv3d_bwd_weight_workspace(ref), lambda o: (ref, _p(x), _p(dy), _p(o[0]), _p(o[1])), (dw, db)),
    ]
    if compute in (1, 2):
        x16, dy16 = hip.act16_pack(x, compute), hip.act16_pack(dy, compute)
        y16 = lambda: Slot(dev, (N, (Cout + 7) // 8, S, 8), dtype=hip.dt16(compute))
        calls += [
            ("conv3d_fwd_h16", L.m355_conv3d_h16_workspace(ref, 0),
             lambda o: (ref, _p(x16), 0, _p(w), _p(bias), None, _p(o[0]), None), (y,)),
            ("conv3d_fwd_h16_c8", L.m355_conv3d_h16_workspace(ref, 0),
             lambda o: (ref, _p(x16), 0, _p(w), _p(bias), _p(o[0]), o[0].bs_arg, None), (y16,)),
            ("conv3d_bwd_data_h16", L.m355_conv3d_h16_workspace(ref, 1), lambda o: (ref, _p(dy16), 0, _p(w), _p(o[0])), (dx,)),
            ("conv3d_bwd_weight_h16", L.m355_conv3d_bwd_weight_h16_workspace(ref),
             lambda o: (ref, _p(x16), 0, _p(dy16), 0, _p(dy), _p(o[0]), _p(o[1])), (dw, db)),
            ("conv3d_bwd_weight_c8", L.m355_conv3d_bwd_weight_c8_workspace(ref),
             lambda o: (ref, _p(x16), 0, _p(dy16), 0, _p(o[0]), _p(o[1]), 1.0), (dw, db)),
        ]
    ran = 0
    for name, need, args, outs in calls:
        if need == 0:
            continue      # (no workspace to be short of: the c8 entry points in an fp32 mode)
        ws = torch.empty(int(need), dtype=torch.uint8, device=dev)
        o = [mk() for mk in outs]
        rc = hip.fn(name)(*args(o), _p(ws), int(need) - 1, st)
        torch.cuda.synchronize()
        assert rc == EWORKSPACE, f"{name}: {need - 1} of {need} workspace bytes -> {rc} {L.m355_last_error().decode()}"
        for s in o:
            s.assert_untouched(name)
        ran += 1
    assert ran >= (8 if compute in (1, 2) else 3)
