"""tests/convt_cases.py is the checked inventory of csrc/convt.hip's launch switches: every entry reports exactly the plan it
names (m355_conv_transpose3d_plan, pure host code: num_cus() is 256 without a device), every feature a case is listed for
holds as an inequality over the tile counts of that plan, and REQUIRED -- every kernel instantiation the launchers can
select, every persistent loop's second trip and every split variant -- is reached by name.  The instantiations are also
read from the launchers' own macros in the source, so one added later fails here until it gets a case."""
import ctypes as C
import os
import re

import pytest

import convt_cases as T
from segmentation_pipeline_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "segmentation-pipeline_amd", "csrc", "convt.hip")

HTS = ("bf16", "f16")
# kernel family x template parameters (x both 16-bit types where the kernel is templated on HT)
INSTANTIATIONS = (
    [f"fwd_mfma<{nvt}>" for nvt in (128, 64, 32)] + [f"fwd_x3<{nvt}>" for nvt in (128, 64, 32)]
    + [f"bwd_data_mfma<{nvt},{mt}>" for nvt in (256, 128, 64) for mt in (2, 4)] + ["dx_reduce"]
    + [f"bwd_weight_mfma<{mt}>" for mt in (2, 4)]
    + [f"fwd_c8<{nvt},{ht}>" for nvt in (64, 32) for ht in HTS]
    + [f"fwd_h16<{ht},{ks},{ng}>" for ht in HTS for ks in (4, 8) for ng in (1, 2)]
    + [f"bwd_data_h16<{ht},{mtw}>" for ht in HTS for mtw in (1, 2, 4)]
    + [f"bww_c8<{ht},{ct}>" for ht in HTS for ct in (1, 2, 4)]
    + ["direct_fwd", "direct_bwd_data", "direct_bwd_weight"])
REQUIRED = INSTANTIATIONS + (
    # forward: several m-tile groups with a short last one, on every voxel-tile width; one group of more rows than there are
    [f"fwd_mfma<{nvt}>:short_last_group" for nvt in (128, 64, 32)] + ["fwd_mfma<128>:one_group_overhang"]
    + ["fwd_mfma<32>:x3_fallback", "direct_fwd:x3_cin_over_512"]
    # data gradient: each instantiation unsplit, and the split variants
    + [f"bwd_data_mfma<{nvt},{mt}>:split_1" for nvt in (256, 128, 64) for mt in (2, 4)]
    + ["bwd_data_mfma<64,2>:even_split", "bwd_data_mfma<64,4>:partial_final_step", "bwd_data_mfma<64,2>:split_below_ks",
       "bwd_data_mfma<64,2>:reduce_n2", "bwd_data_mfma<64,4>:reduce_n2"]
    # weight gradient: a second trip of the persistent loop with an uneven share, on both channel tiles
    + [f"bwd_weight_mfma<{mt}>:{f}" for mt in (2, 4)
       for f in ("second_trip", "tile_straddles_samples", "ragged_channels", "dbias", "no_dbias")]
    + [f"fwd_c8<{nvt},{ht}>:cout_pad_lanes" for nvt in (64, 32) for ht in HTS]
    + [f"fwd_h16<{ht},{ks},{ng}>:second_voxel_tile" for ht in HTS for ks, ng in ((4, 2), (8, 2), (8, 1))]
    + [f"bwd_data_h16<{ht},{mtw}>:ragged_share" for ht in HTS for mtw in (1, 2, 4)]
    + [f"bwd_data_h16<{ht},{f}" for ht in HTS for f in ("2>:rule_3_to_2", "1>:nks_64", "1>:cin_pad_lanes")]
    + [f"bww_c8<{ht},{ct}>:second_trip" for ht in HTS for ct in (1, 2, 4)]
    + [f"bww_c8<{ht},1>:{f}" for ht in HTS for f in ("odd_h_ragged_w", "unscale")]
    + [f"direct_{e}:{f}" for e in ("fwd", "bwd_data", "bwd_weight") for f in ("non_cubic", "k2s2_forced_direct")])


def plan(case):
    d = _lib.ConvDesc()
    d.N, d.Cin, d.Cout, d.D, d.H, d.W = case.shape
    d.k, d.stride, d.pad, d.out_pad = case.geom
    d.compute = case.compute if case.which == T.FWD else 0
    if case.odd_ybs:
        _, Cout, OD, OH, OW = case.out_shape()
        d.y_batch_stride = Cout * OD * OH * OW + 1
    out = (C.c_int32 * 4)()
    assert _lib.lib().m355_conv_transpose3d_plan(C.byref(d), case.which, None, out) == 0
    return tuple(out)


@pytest.mark.parametrize("case", T.CASES, ids=repr)
def test_case_reports_its_plan_and_its_features_hold(case, tuning):
    tuning(**case.tuning)
    assert plan(case) == case.plan
    n = T.counts(case)
    for f in case.features:
        assert eval(T.FEATURES[f], {}, dict(n)), f"{case.id}: {f} ({T.FEATURES[f]}) does not hold for {n}"
    if case.which == T.BWD_DATA and case.plan[0] == T.MFMA:
        assert T.ceil_div(n["Cout"], n["o_per_split"]) == n["split"], "counts() restates the router's split of K"
    if T.persistent_or_split(case) and case.which == T.BWD_WEIGHT_C8:
        tuning(M355_CONVT_WGS=8)
        assert plan(case)[2] == n["tiles"], "under M355_CONVT_WGS=8 every workgroup has one tile"


def test_case_ids_are_unique_and_shapes_stay_small():
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids))
    for c in T.CASES:
        N, Cin, Cout, D, H, W = c.shape
        if c.plan[0] == T.DIRECT:
            assert max(D, H, W) <= 5 or c.geom == T.K2S2, c
        # (the CPU oracle's time: voxels x channel pairs x taps)
        assert N * D * H * W * Cin * Cout * 8 <= 2.5e9, c


def test_table_reaches_every_instantiation_and_second_trip_by_name():
    reached = set().union(*(T.instantiations(c) for c in T.CASES))
    missing = [name for name in REQUIRED if name not in reached]
    assert not missing, f"no case in tests/convt_cases.py reaches: {missing}"


def test_direct_grid_is_complete():
    """the small grid of the direct kernels: every valid geometry, on all three entry points, over every channel count"""
    valid = {(k, s, p, op) for k in (1, 2, 3, 4, 5) for s in (1, 2, 3) for p in (0, 1, 2) for op in {0, s - 1}
             if p <= k - 1 and (k, s, p, op) != T.K2S2}
    grid = {c.geom for c in T.CASES if c.plan[0] == T.DIRECT and not c.features}
    assert grid == valid and len(grid) == 59
    for e in (T.FWD, T.BWD_DATA, T.BWD_WEIGHT):
        cases = [c for c in T.CASES if c.which == e and c.plan[0] == T.DIRECT and not c.features]
        assert {c.geom for c in cases} == grid
        assert {c.shape[1] for c in cases} == {c.shape[2] for c in cases} == {1, 3, 5}
        assert all(c.shape[0] == 2 and all(v > 0 for v in c.out_shape()) for c in cases)


def test_inventory_matches_the_launchers_in_the_source():
    """the template arguments the launch macros of convt.hip are invoked with == INSTANTIATIONS"""
    with open(SOURCE) as f:
        src = f.read()
    found = {f"fwd_mfma<{a}>" for a in re.findall(r"M355_CONVT_FWD\((\d+)\);", src)}
    found |= {f"bwd_data_mfma<{a},{b}>" for a, b in re.findall(r"M355_CONVT_BWD\((\d+), (\d+)\);", src)}
    found |= {f"bwd_weight_mfma<{a}>" for a in re.findall(r"hipLaunchKernelGGL\(convt_k2s2_bwd_weight_mfma_kernel<(\d+)>", src)}
    found |= {f"fwd_c8<{a},{ht}>" for a in re.findall(r"M355_CONVT_C8\((\d+), HT\);", src) for ht in HTS}
    found |= {f"fwd_h16<{ht},{a},{b}>" for a, b in re.findall(r"M355_CONVT_H16\(HT, (\d+), (\d+)\);", src) for ht in HTS}
    found |= {f"bwd_data_h16<{ht},{a}>" for a in re.findall(r"M355_CTBD\(HT, (\d+)\);", src) for ht in HTS}
    found |= {f"bww_c8<{ht},{a}>" for a in re.findall(r"M355_CTBW\(HT, (\d+)\);", src) for ht in HTS}
    found |= {{"fwd": "direct_fwd", "bwd_data": "direct_bwd_data", "bwd_weight": "direct_bwd_weight"}[a]
              for a in re.findall(r"hipLaunchKernelGGL\(convt_direct_(\w+?)_kernel", src)}
    if "convt_dx_reduce_kernel, dim3" in src:
        found.add("dx_reduce")
    x3 = {f"fwd_x3<{nvt}>" for nvt in (128, 64, 32)}     # (launch_convt_fwd_x3: conv3d_f32x3.hip, widths of convt_fwd_x3_nvt)
    assert found | x3 == set(INSTANTIATIONS), sorted(found.symmetric_difference(set(INSTANTIATIONS) - x3))
