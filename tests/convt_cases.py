"""TEST HELPER -- the table of conv-transpose calls that tests/test_convt_plan_cases_cpu.py checks against the host-side
plan query and tests/test_convt_launch_plans_gpu.py runs on the device.  No GPU imports.

A `Case` is one call of one entry point:
  id        name of the case
  which     entry point, as m355_conv_transpose3d_plan counts them: FWD, BWD_DATA, BWD_WEIGHT (fp32 tensors) and FWD_C8,
            BWD_DATA_C8, BWD_WEIGHT_C8 (c8 tensors of a 16-bit mode)
  shape     (N, Cin, Cout, D, H, W) of the descriptor
  compute   FP32, BF16, F16 or F32X3
  geom      (k, stride, pad, out_pad)
  tuning    M355_* knobs the call is made under
  plan      the four numbers m355_conv_transpose3d_plan must report: the kernel family and that family's out[1..3], on
            256 compute units (an MI355X, and what the library counts with when there is no device)
  features  names from FEATURES: what the case is in the table for.  Each is an inequality over counts(case), the tile counts
            that follow from the shape and the plan, so the CPU test can hold the case to it
  odd_ybs   the y / dy tensor gets an odd batch stride (fp32 entry points: the direct kernels serve it)
  dbias     the weight gradient is asked for the bias gradient too
  unscale   grad_unscale of the c8 weight gradient

instantiations(case) names the kernel template instantiation the plan selects, in the spelling of REQUIRED in the CPU
test, and "<instantiation>:<feature>" for each feature of the case."""

FWD, BWD_DATA, BWD_WEIGHT, FWD_C8, BWD_DATA_C8, BWD_WEIGHT_C8 = range(6)
DIRECT, MFMA, X3, C8, H16, UNSUPPORTED = range(6)
FP32, BF16, F16, F32X3 = range(4)
K2S2 = (2, 2, 0, 0)
HT = {BF16: "bf16", F16: "f16"}


def ceil_div(a, b):
    return -(-a // b)


def round_up(a, b):
    return ceil_div(a, b) * b


class Case:
    def __init__(self, id, which, shape, plan, compute=FP32, geom=K2S2, tuning=None, features=(), odd_ybs=False, dbias=True,
                 unscale=1.0):
        self.id, self.which, self.shape, self.plan, self.compute, self.geom = id, which, tuple(shape), tuple(plan), compute, geom
        self.tuning, self.features, self.odd_ybs, self.dbias, self.unscale = tuning or {}, tuple(features), odd_ybs, dbias, unscale

    def __repr__(self):
        return self.id

    def out_shape(self):
        N, _, Cout, D, H, W = self.shape
        k, s, p, op = self.geom
        return (N, Cout) + tuple((v - 1) * s - 2 * p + k + op for v in (D, H, W))


def counts(case, plan=None):
    """the numbers a case's features speak of: the shape, the plan's own numbers under their names, and the tile counts of
    the kernel the plan selects (csrc/convt.hip: one tile of the fp32 weight gradient is 64 voxels of the batch, of the c8
    weight gradient 2 rows x 32 voxels, of the c8 data gradient 128 voxels, of the 16-bit MFMA forward 128 * NG voxels)"""
    N, Cin, Cout, D, H, W = case.shape
    S = D * H * W
    family, a, b, c = plan or case.plan
    v = dict(N=N, Cin=Cin, Cout=Cout, D=D, H=H, W=W, S=S, family=family, compute=case.compute, k2s2=case.geom == K2S2,
             odd_ybs=case.odd_ybs, dbias=case.dbias, unscale=case.unscale, min=min, max=max)
    if family == DIRECT:
        return v
    if case.which == FWD or (case.which == FWD_C8 and family == C8):
        rows = ceil_div(Cout, 4) if case.which == FWD else ceil_div(ceil_div(Cout, 4), 2)
        v.update(nvt=a, mt_per_wg=b, rows=rows, vox_tiles=ceil_div(S, a) * N, grid_y=ceil_div(rows, b))
    elif case.which == BWD_DATA:
        cblocks = ceil_div(Cin, 32 * b)
        wgs = ceil_div(S, a) * cblocks * N
        ks = min(8, ceil_div(512, wgs), max(1, Cout // 16)) if wgs < 256 else 1     # the router's first choice of parts
        o_per_split = round_up(ceil_div(Cout, ks), 4)
        v.update(nvt=a, mt=b, split=c, wgs=wgs, ks=ks, o_per_split=o_per_split, last_part=Cout - (c - 1) * o_per_split)
    elif case.which == BWD_WEIGHT:
        v.update(mt=a, split=b, tiles=ceil_div(N * S, 64))
    elif case.which == FWD_C8:
        mtiles = 2 * ceil_div(Cout, 8)
        groups = ceil_div(mtiles, c)
        v.update(ks=a, ng=b, mt_per_wg=c, mtiles=mtiles, groups=groups, vox_tiles=ceil_div(S, 128 * b),
                 grid_x_cap=ceil_div(512, groups * N))
    elif case.which == BWD_DATA_C8:
        v.update(mtw=a, grid_x=b, vox_tiles=ceil_div(S, 128), nks=8 * ceil_div(ceil_div(Cout, 8), 2), mtiles=ceil_div(Cin, 32))
    else:
        v.update(ct=a, split=b, tiles=N * D * ceil_div(H, 2) * ceil_div(W, 32))
    return v


FEATURES = {
    # forward (fp32 MFMA, X3, c8): m-tile groups along grid.y
    "short_last_group": "grid_y > 1 and rows % mt_per_wg != 0",
    "one_group_overhang": "vox_tiles >= 768 and grid_y == 1 and mt_per_wg > rows",
    "x3_fallback": "compute == 3 and 337 <= Cin <= 512 and family == 1",
    "x3_cin_over_512": "compute == 3 and Cin > 512 and family == 0 and k2s2",
    # fp32 data gradient: the split of the K = 8 * Cout contraction
    "split_1": "split == 1",
    "even_split": "split > 1 and o_per_split * split == Cout",
    "partial_final_step": "split > 1 and last_part > 0 and last_part % 4 != 0",
    "split_below_ks": "1 < split < ks",
    "reduce_n2": "split > 1 and N == 2",
    # weight gradients: persistent workgroups
    "second_trip": "split < tiles and tiles % split != 0",
    "tile_straddles_samples": "N == 2 and S % 64 != 0",
    "ragged_channels": "Cout % 16 != 0 and Cin % (32 * mt) != 0",
    "dbias": "dbias",
    "no_dbias": "not dbias",
    "odd_h_ragged_w": "H % 2 == 1 and W % 32 != 0",
    "unscale": "unscale != 1",
    # c8 forward and data gradient
    "cout_pad_lanes": "Cout % 8 != 0",
    "second_voxel_tile": "vox_tiles > grid_x_cap",     # grid.x = min(vox_tiles, grid_x_cap): the plan does not carry it
    "rule_3_to_2": "65 <= Cin <= 96 and min(mtiles, 64 // nks, 4) == 3 and mtw == 2",
    "nks_64": "nks == 64 and 121 <= Cout <= 128",
    "ragged_share": "grid_x > 1 and vox_tiles % grid_x != 0",
    "cin_pad_lanes": "Cin % 8 != 0",
    # direct kernels
    "non_cubic": "D != H and H != W and D != W",
    "k2s2_forced_direct": "k2s2 and odd_ybs and family == 0",
}


def instantiations(case, plan=None):
    family, a, b, c = plan or case.plan
    if family == DIRECT:
        name = ("direct_fwd", "direct_bwd_data", "direct_bwd_weight")[case.which]
    elif case.which == FWD:
        name = f"fwd_x3<{a}>" if family == X3 else f"fwd_mfma<{a}>"
    elif case.which == BWD_DATA:
        name = f"bwd_data_mfma<{a},{b}>"
    elif case.which == BWD_WEIGHT:
        name = f"bwd_weight_mfma<{a}>"
    elif case.which == FWD_C8:
        name = f"fwd_c8<{a},{HT[case.compute]}>" if family == C8 else f"fwd_h16<{HT[case.compute]},{a},{b}>"
    elif case.which == BWD_DATA_C8:
        name = f"bwd_data_h16<{HT[case.compute]},{a}>"
    else:
        name = f"bww_c8<{HT[case.compute]},{a}>"
    names = {name} | {f"{name}:{f}" for f in case.features}
    if case.which == BWD_DATA and family == MFMA and c > 1:
        names.add("dx_reduce")
    return names


def persistent_or_split(case):
    """the cases whose result is a fixed-order reduction over workgroups or a walk over several tiles: called twice"""
    return (case.which in (BWD_DATA_C8, BWD_WEIGHT_C8) or (case.which == BWD_WEIGHT and case.plan[0] == MFMA)
            or (case.which == FWD_C8 and case.plan[0] == H16) or (case.which == BWD_DATA and case.plan[3] > 1))


BIG = (17, 60, 65)      # 66300 voxels: 259 tiles of 256
CASES = [
    # ---------------------------------------------------------------- forward, fp32 MFMA: convt_k2s2_fwd_mfma_kernel<NVT>
    Case("fwd-nvt128-short-last-group", FWD, (2, 17, 37, 3, 5, 7), (MFMA, 128, 4, 0), features=["short_last_group"]),
    Case("fwd-nvt64-short-last-group", FWD, (2, 200, 37, 3, 5, 7), (MFMA, 64, 4, 0), features=["short_last_group"]),
    Case("fwd-nvt32-short-last-group", FWD, (2, 300, 21, 2, 3, 5), (MFMA, 32, 4, 0), features=["short_last_group"]),
    Case("fwd-nvt128-one-group-774-tiles", FWD, (2, 6, 22, 17, 30, 97), (MFMA, 128, 8, 0), features=["one_group_overhang"]),
    # ---------------------------------------------------------------- forward, M355_COMPUTE_F32X3
    Case("x3-nvt128", FWD, (2, 17, 5, 3, 5, 7), (X3, 128, 4, 0), F32X3),
    Case("x3-nvt64", FWD, (1, 130, 70, 2, 9, 20), (X3, 64, 4, 0), F32X3, features=["short_last_group"]),
    Case("x3-nvt32", FWD, (1, 320, 24, 2, 3, 5), (X3, 32, 4, 0), F32X3, features=["short_last_group"]),
    Case("x3-cin340-falls-back-to-fp32-mfma", FWD, (1, 340, 9, 3, 5, 7), (MFMA, 32, 4, 0), F32X3, features=["x3_fallback"]),
    Case("x3-cin520-direct", FWD, (1, 520, 8, 2, 2, 2), (DIRECT, 0, 0, 0), F32X3, features=["x3_cin_over_512"]),
    # ---------------------------------------------------------------- data gradient, fp32 MFMA: <NVT, MT>
    Case("dx-nvt256-mt2", BWD_DATA, (2, 3, 5) + BIG, (MFMA, 256, 2, 1), features=["split_1"]),
    Case("dx-nvt128-mt2", BWD_DATA, (1, 3, 5) + BIG, (MFMA, 128, 2, 1), features=["split_1"]),
    Case("dx-nvt256-mt4", BWD_DATA, (2, 70, 5) + BIG, (MFMA, 256, 4, 1), features=["split_1"]),
    Case("dx-nvt128-mt4", BWD_DATA, (1, 70, 5) + BIG, (MFMA, 128, 4, 1), features=["split_1"]),
    Case("dx-nvt64-mt2", BWD_DATA, (2, 5, 7, 3, 5, 6), (MFMA, 64, 2, 1), features=["split_1"]),
    Case("dx-nvt64-mt4", BWD_DATA, (2, 96, 20, 3, 5, 7), (MFMA, 64, 4, 1), features=["split_1"]),
    Case("dx-split4x16-n2", BWD_DATA, (2, 40, 64, 3, 5, 7), (MFMA, 64, 2, 4), features=["even_split", "reduce_n2"]),
    Case("dx-split-20+17", BWD_DATA, (1, 96, 37, 2, 3, 5), (MFMA, 64, 4, 2), features=["partial_final_step"]),
    Case("dx-split-20+17-n2", BWD_DATA, (2, 96, 37, 2, 3, 5), (MFMA, 64, 4, 2), features=["partial_final_step", "reduce_n2"]),
    Case("dx-ks6-split5", BWD_DATA, (1, 40, 100, 3, 5, 7), (MFMA, 64, 2, 5), features=["split_below_ks", "even_split"]),
    # ---------------------------------------------------------------- weight gradient, fp32 MFMA: <MT>
    Case("dw-mt4-51-splits-57-tiles", BWD_WEIGHT, (1, 130, 70, 9, 20, 20), (MFMA, 4, 51, 0),
         features=["second_trip", "ragged_channels", "dbias"]),
    Case("dw-mt4-51-splits-57-tiles-no-dbias", BWD_WEIGHT, (1, 130, 70, 9, 20, 20), (MFMA, 4, 51, 0), dbias=False,
         features=["second_trip", "ragged_channels", "no_dbias"]),
    Case("dw-mt4-51-splits-60-tiles-n2", BWD_WEIGHT, (2, 130, 70, 5, 19, 20), (MFMA, 4, 51, 0),
         features=["second_trip", "tile_straddles_samples", "ragged_channels", "dbias"]),
    Case("dw-mt2-512-splits-526-tiles-n2", BWD_WEIGHT, (2, 8, 8, 17, 30, 33), (MFMA, 2, 512, 0),
         features=["second_trip", "tile_straddles_samples", "ragged_channels", "dbias"]),
    Case("dw-mt2-512-splits-526-tiles-n2-no-dbias", BWD_WEIGHT, (2, 8, 8, 17, 30, 33), (MFMA, 2, 512, 0), dbias=False,
         features=["second_trip", "tile_straddles_samples", "ragged_channels", "no_dbias"]),
    # ---------------------------------------------------------------- direct kernels beyond the small grid below
    Case("direct-fwd-non-cubic", FWD, (2, 3, 5, 2, 3, 5), (DIRECT, 0, 0, 0), geom=(3, 2, 1, 1), features=["non_cubic"]),
    Case("direct-dx-non-cubic", BWD_DATA, (2, 3, 5, 2, 3, 5), (DIRECT, 0, 0, 0), geom=(3, 2, 1, 1), features=["non_cubic"]),
    Case("direct-dw-non-cubic", BWD_WEIGHT, (2, 3, 5, 2, 3, 5), (DIRECT, 0, 0, 0), geom=(3, 2, 1, 1), features=["non_cubic"]),
    Case("direct-fwd-k2s2-odd-ybs", FWD, (2, 5, 7, 3, 5, 6), (DIRECT, 0, 0, 0), odd_ybs=True, features=["k2s2_forced_direct"]),
    Case("direct-dx-k2s2-odd-ybs", BWD_DATA, (2, 5, 7, 3, 5, 6), (DIRECT, 0, 0, 0), odd_ybs=True,
         features=["k2s2_forced_direct"]),
    Case("direct-dw-k2s2-odd-ybs", BWD_WEIGHT, (2, 5, 7, 3, 5, 6), (DIRECT, 0, 0, 0), odd_ybs=True,
         features=["k2s2_forced_direct"]),
]

# ---- c8 entry points, each case in both 16-bit types
_H16_ON = {"M355_CONVT_H16": 1}
_C8 = [
    # forward, family 3: convt_k2s2_fwd_c8_kernel<NVT, HT>
    ("c8fwd-nvt64", FWD_C8, (2, 24, 13, 3, 5, 6), (C8, 64, 4, 0), {}, ["cout_pad_lanes"], {}),
    ("c8fwd-nvt64-short-last-group", FWD_C8, (2, 24, 45, 3, 5, 6), (C8, 64, 4, 0), {}, ["cout_pad_lanes", "short_last_group"], {}),
    ("c8fwd-nvt32", FWD_C8, (1, 320, 13, 2, 3, 5), (C8, 32, 4, 0), {}, ["cout_pad_lanes"], {}),
    # forward, family 4: convt_k2s2_fwd_h16_kernel<HT, KS, NG>
    ("h16fwd-ks4-ng1", FWD_C8, (1, 24, 40, 17, 31, 33), (H16, 4, 1, 10), _H16_ON, [], {}),
    ("h16fwd-ks4-ng2-260-tiles-256-wgs", FWD_C8, (2, 16, 8, 33, 33, 61), (H16, 4, 2, 2), _H16_ON, ["second_voxel_tile"], {}),
    ("h16fwd-ks8-ng2-260-tiles-256-wgs", FWD_C8, (2, 72, 13, 33, 33, 61), (H16, 8, 2, 4), _H16_ON,
     ["second_voxel_tile", "cout_pad_lanes"], {}),
    ("h16fwd-ks8-ng1-136-tiles-86-wgs", FWD_C8, (2, 120, 72, 17, 31, 33), (H16, 8, 1, 8), _H16_ON, ["second_voxel_tile"], {}),
    # data gradient, family 4: convt_k2s2_bwd_data_h16_kernel<HT, MTW>
    ("c8dx-mtw2-19-tiles-5-wgs", BWD_DATA_C8, (2, 72, 40, 6, 10, 40), (H16, 2, 5, 0), {}, ["ragged_share"], {}),
    ("c8dx-mtw3-becomes-2", BWD_DATA_C8, (2, 72, 24, 6, 10, 40), (H16, 2, 5, 0), {}, ["rule_3_to_2", "ragged_share"], {}),
    ("c8dx-mtw1-29-tiles-8-wgs", BWD_DATA_C8, (1, 130, 70, 9, 20, 20), (H16, 1, 8, 0), {}, ["ragged_share", "cin_pad_lanes"], {}),
    ("c8dx-mtw4-10-tiles-3-wgs", BWD_DATA_C8, (1, 130, 24, 4, 9, 33), (H16, 4, 3, 0), {}, ["ragged_share", "cin_pad_lanes"], {}),
    ("c8dx-nks64", BWD_DATA_C8, (1, 40, 125, 3, 9, 33), (H16, 1, 2, 0), {}, ["nks_64", "ragged_share"], {}),
    # weight gradient, family 3: convt_k2s2_bww_c8_kernel<HT, CT>
    ("c8dw-ct1-128-splits-180-tiles", BWD_WEIGHT_C8, (2, 24, 40, 9, 9, 40), (C8, 1, 128, 0), {},
     ["second_trip", "odd_h_ragged_w", "unscale"], {"unscale": 0.5}),
    ("c8dw-ct2-64-splits-120-tiles", BWD_WEIGHT_C8, (2, 72, 40, 6, 10, 40), (C8, 2, 64, 0), {}, ["second_trip"], {}),
    ("c8dw-ct4-42-splits-90-tiles", BWD_WEIGHT_C8, (1, 130, 70, 9, 20, 20), (C8, 4, 42, 0), {}, ["second_trip"], {}),
]
for _id, _which, _shape, _plan, _tuning, _features, _kw in _C8:
    for _compute in (BF16, F16):
        CASES.append(Case(f"{_id}-{HT[_compute]}", _which, _shape, _plan, _compute, tuning=_tuning, features=_features, **_kw))


# ---- direct kernels, the small grid: every valid (k, stride, pad, out_pad) of k 1..5, stride 1..3, pad 0..2 (at most k - 1:
# the equivalent convolution pads k - 1 - pad), out_pad 0 or stride - 1, except k2 s2 p0 (the MFMA kernels' own); channel
# counts and extents cycle through {1, 3, 5} and {3, 4, 5} so that every entry point meets each of them, N = 2
def _direct_grid():
    chans, extents, i = (1, 3, 5), ((3, 4, 5), (5, 3, 4), (4, 5, 3)), 0
    for k in (1, 2, 3, 4, 5):
        for s in (1, 2, 3):
            for p in range(0, min(2, k - 1) + 1):
                for op in sorted({0, s - 1}):
                    if (k, s, p, op) == K2S2:
                        continue
                    shape = (2, chans[i % 3], chans[(i // 3 + i) % 3]) + extents[i % 3]
                    i += 1
                    for which, name in ((FWD, "fwd"), (BWD_DATA, "dx"), (BWD_WEIGHT, "dw")):
                        yield Case(f"direct-{name}-k{k}s{s}p{p}o{op}", which, shape, (DIRECT, 0, 0, 0), geom=(k, s, p, op))


CASES += list(_direct_grid())
