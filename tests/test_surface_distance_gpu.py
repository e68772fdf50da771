"""Distance transform and surface distances on the device (csrc/distance.hip via ops.edt_sq / surface_mask /
surface_gather, post_processing.distance_transform_edt, evaluators.SurfaceDistanceEvaluator) against the
brute-force fp64 reference tests/distance_ref.py and scipy's answers in tests/golden/surface_distance.npz
(tools/gen_golden_surface_distance.py).  The code under test is never its own reference."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
from torch import nn

import distance_ref as R
from conftest import ROOT
from segmentation_pipeline_amd import _lib, ops
from segmentation_pipeline_amd.evaluators import (SURFACE_STAT_NAMES, LabelMap, SegmentationEvaluator,
                                                  SurfaceDistanceEvaluator, surface_distances)
from segmentation_pipeline_amd.post_processing import distance_transform_edt
from segmentation_pipeline_amd.prediction import add_evaluation_labels
from test_evaluation_cpu import _msseg2_chain

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 64
CANARY = -12345.0
SPACINGS = [(0.5, 1.0, 2.5), (1.2, 0.7, 3.0)]
# the issue's shapes (each axis in turn across a 64-lane boundary), then: several waves and blocks in the D sweep
# ((24, 20, 9): 480 rows at 113 per wave), rows of several 64-voxel chunks with two rows per wave ((2, 3, 400)), and each
# staged axis at the limit, where the line fills the 64 KiB of LDS ((512, 1, 2), (1, 512, 3)) -- the H / W kernels stage
# a line whole, so there is no longer line to test, only the limit.
SHAPES = [(1, 1, 1), (1, 1, 17), (5, 7, 9), (3, 2, 70), (2, 130, 3), (67, 3, 5), (24, 20, 9), (2, 3, 400), (512, 1, 2),
          (1, 512, 3), (2, 2, 512)]
PATTERNS = ["none", "all", "corner", "equidistant", "plane", "half", "sparse"]


def _sites(shape, pattern):
    rng = np.random.default_rng(sum(shape) * 7 + len(pattern))
    s = np.zeros(shape, dtype=np.uint8)
    if pattern == "all":
        s[:] = 1
    elif pattern == "corner":
        s[-1, -1, -1] = 1
    elif pattern == "equidistant":        # two sites at the ends of the longest axis: its middle voxels are ties
        axis = int(np.argmax(shape))
        first, last = [0, 0, 0], [0, 0, 0]
        last[axis] = shape[axis] - 1
        s[tuple(first)] = s[tuple(last)] = 1
    elif pattern == "plane":              # the middle plane across the longest axis, thinned
        axis = int(np.argmax(shape))
        index = [slice(None)] * 3
        index[axis] = shape[axis] // 2
        s[tuple(index)] = rng.random(s[tuple(index)].shape) < 0.7
    elif pattern == "half":
        s[:] = rng.random(shape) < 0.5
    elif pattern == "sparse":
        s[:] = rng.random(shape) < 0.01
    return s


@functools.lru_cache(maxsize=None)
def _ref_sq(shape, pattern, spacing):
    out = R.edt_sq(_sites(shape, pattern), spacing)
    out.setflags(write=False)
    return out


def _guarded(n, dtype, fill):
    big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return big, big[GUARD:GUARD + n]


def _edt_sq_guarded(sites, spacing):
    """ops.edt_sq into the middle of canary-filled buffers (output and workspace); asserts the canaries afterwards"""
    t = torch.from_numpy(sites).to(DEV)
    n = t.numel()
    big, mid = _guarded(n, torch.float32, CANARY)
    ws_bytes = int(_lib.lib().m355_edt_workspace((ctypes.c_int32 * 3)(*sites.shape)))
    ws_big = torch.full((ws_bytes + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    d2 = ops.edt_sq(t, spacing, out=mid.view(sites.shape), workspace=ws_big[256:256 + ws_bytes])
    torch.cuda.synchronize()
    assert (big[:GUARD] == CANARY).all() and (big[GUARD + n:] == CANARY).all(), "edt_sq wrote outside [0, nvox)"
    assert (ws_big[:256] == 0xA5).all() and (ws_big[256 + ws_bytes:] == 0xA5).all(), "edt_sq wrote outside its workspace"
    assert torch.equal(t.cpu(), torch.from_numpy(sites)), "edt_sq changed its input"
    return d2


# ------------------------------------------------------------------------------------------------ EDT
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edt_sq_unit_spacing_is_exact(shape):
    assert sum((n - 1) ** 2 for n in shape) < 2 ** 24
    for pattern in PATTERNS:
        sites = _sites(shape, pattern)
        want = _ref_sq(shape, pattern, (1.0, 1.0, 1.0))
        got = _edt_sq_guarded(sites, (1.0, 1.0, 1.0)).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == shape
        assert np.array_equal(got, want.astype(np.float32)), (pattern, np.abs(got - want.astype(np.float32)).max())
        if pattern == "none":
            assert np.isposinf(got).all()
        if pattern == "all":
            assert not got.any()
        # scipy's meaning: the nonzero voxels of (sites == 0) measure their distance to the sites
        dist = distance_transform_edt(torch.from_numpy(sites == 0).to(DEV))
        assert dist.is_cuda and dist.dtype == torch.float32
        assert np.array_equal(dist.cpu().numpy(), np.sqrt(got.astype(np.float64)).astype(np.float32)), pattern


@pytest.mark.parametrize("spacing", SPACINGS, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edt_general_spacing(shape, spacing):
    for pattern in PATTERNS:
        sites = _sites(shape, pattern)
        want = np.sqrt(_ref_sq(shape, pattern, spacing))
        d2 = _edt_sq_guarded(sites, spacing)
        got = ops.edt_sqrt(d2).cpu().numpy()
        assert np.array_equal(np.isinf(got), np.isinf(want)), pattern
        finite = np.isfinite(want)
        err = np.abs(got[finite] - want[finite]) / np.maximum(want[finite], 1e-300)
        print(shape, spacing, pattern, "max relative error", err.max() if err.size else 0.0)
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=0, err_msg=pattern)
        assert np.array_equal(got == 0, sites != 0)


def test_edt_sq_does_not_depend_on_reused_scratch():
    """handing in the output and the workspace of another call (stale contents) gives the same bits"""
    shape = (5, 7, 9)
    sites = torch.from_numpy(_sites(shape, "half")).to(DEV)
    fresh = ops.edt_sq(sites, (1.2, 0.7, 3.0))
    out = torch.full(shape, 7.0, device=DEV)
    ws = torch.full((4096,), 0xFF, dtype=torch.uint8, device=DEV)
    again = ops.edt_sq(sites, (1.2, 0.7, 3.0), out=out, workspace=ws)
    assert again is out and torch.equal(fresh, again)
    with pytest.raises(_lib.M355Error, match="workspace of 16 bytes"):
        ops.edt_sq(sites, workspace=ws[:16])
    with pytest.raises(_lib.M355Error, match="at most M355_EDT_MAX_DIM"):
        ops.edt_sq(torch.zeros((1, 1, _lib.EDT_MAX_DIM + 1), dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------------ distance_transform_edt
@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "surface_distance.npz")))


def _labels(fx):
    return dict(zip([str(n) for n in fx["label_names"]], [int(v) for v in fx["label_values"]]))


def test_distance_transform_edt_fixture(fx):
    """scipy's meaning: distance_transform_edt(~border, sampling) as scipy computed it"""
    checked = 0
    for c in range(int(fx["cases"])):
        spacing = tuple(fx[f"{c}.spacing"])
        for name in _labels(fx):
            for side in ("pred", "target"):
                key = f"{c}.{name}.edt_to_{side}"
                if key not in fx:
                    continue
                got = distance_transform_edt(~fx[f"{c}.{name}.border_{side}"], sampling=spacing)
                assert isinstance(got, np.ndarray) and got.dtype == np.float32
                if spacing == (1.0, 1.0, 1.0):
                    assert np.array_equal(got, fx[key].astype(np.float32))
                else:
                    np.testing.assert_allclose(got, fx[key], rtol=1e-6, atol=0)
                checked += 1
    assert checked >= 20


def test_distance_transform_edt_kinds_and_types():
    rng = np.random.default_rng(5)
    img = (rng.random((6, 9, 11)) < 0.8) * rng.integers(1, 5, (6, 9, 11))
    want = R.edt(img).astype(np.float32)
    for dtype in (np.bool_, np.uint8, np.int64, np.float32):
        a = img.astype(dtype)
        got = distance_transform_edt(a)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, want), dtype
        on_device = distance_transform_edt(torch.from_numpy(a).to(DEV))
        assert on_device.is_cuda and on_device.dtype == torch.float32 and np.array_equal(on_device.cpu().numpy(), want)
    on_cpu = distance_transform_edt(torch.from_numpy(img))
    assert not on_cpu.is_cuda and np.array_equal(on_cpu.numpy(), want)
    for sampling, sp in ((2, (2.0, 2.0, 2.0)), ((0.5, 1.0, 2.5), (0.5, 1.0, 2.5))):
        np.testing.assert_allclose(distance_transform_edt(img, sampling=sampling), R.edt(img, sp), rtol=1e-6, atol=0)
    full = distance_transform_edt(np.ones((3, 4, 5), dtype=np.uint8))
    assert full.dtype == np.float32 and np.isposinf(full).all()
    a = np.ones((3, 4, 5), dtype=np.float32)
    a[1, 2, 3] = -0.0                               # a negative zero is a zero voxel
    assert distance_transform_edt(a)[1, 2, 3] == 0 and np.isfinite(distance_transform_edt(a)).all()


# ------------------------------------------------------------------------------------------------ surface_mask
def _mask_cases():
    touching = np.zeros((7, 6, 9), dtype=np.int32)
    touching[0:4, 2:5, 5:9] = 1                                  # touches the W = 0 and D = 8 faces
    single = np.zeros((5, 5, 5), dtype=np.int32)
    single[2, 3, 1] = 1
    full = np.ones((5, 4, 70), dtype=np.int32)                   # the border is the faces of the volume
    nested = np.zeros((9, 10, 11), dtype=np.int32)
    nested[1:8, 1:9, 1:10] = 1
    nested[3:6, 3:7, 3:8] = 2                                    # value 2 embedded in value 1
    return [("touching", touching, 1), ("single", single, 1), ("full", full, 1), ("nested_inner", nested, 2),
            ("nested_outer", nested, 1), ("absent", nested, 3)]


@pytest.mark.parametrize("name,x,value", _mask_cases(), ids=[c[0] for c in _mask_cases()])
def test_surface_mask(name, x, value):
    want = R.border(x, value)
    n = x.size
    big, mid = _guarded(n, torch.uint8, 0x5A)
    border, count = ops.surface_mask(torch.from_numpy(x).to(DEV), value, border=mid.view(x.shape))
    assert border.dtype == torch.uint8 and count.dtype == torch.int32 and count.shape == (1,)
    assert np.array_equal(border.cpu().numpy(), want.astype(np.uint8))
    assert int(count.item()) == int(want.sum())
    assert (big[:GUARD] == 0x5A).all() and (big[GUARD + n:] == 0x5A).all()
    if name == "full":
        inner = want[1:-1, 1:-1, 1:-1]
        assert not inner.any() and int(want.sum()) == n - inner.size
    if name == "absent":
        assert int(count.item()) == 0 and not border.any()
    # the count accumulates: the caller zeroes it
    ops.surface_mask(torch.from_numpy(x).to(DEV), value, count=count)
    assert int(count.item()) == 2 * int(want.sum())


# ------------------------------------------------------------------------------------------------ surface_gather
def test_surface_gather_sorted_and_short_buffer():
    rng = np.random.default_rng(11)
    shape = (9, 10, 33)
    border = (rng.random(shape) < 0.3).astype(np.uint8)
    d2 = (rng.random(shape) * 1000).astype(np.float32)
    on_border = np.argwhere(border)
    d2[tuple(on_border[0])], d2[tuple(on_border[1])] = 0.0, np.inf
    k = int(border.sum())
    want = np.sort(np.sqrt(d2.astype(np.float64)).astype(np.float32)[border != 0])
    b, d = torch.from_numpy(border).to(DEV), torch.from_numpy(d2).to(DEV)
    big, out = _guarded(k, torch.float32, CANARY)
    cursor = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert ops.surface_gather(b, d, out, cursor) is out
    assert int(cursor.item()) == k
    assert np.array_equal(np.sort(out.cpu().numpy()), want)
    assert (big[:GUARD] == CANARY).all() and (big[GUARD + k:] == CANARY).all()
    # one slot short: the tail canary stays, the cursor reports the full count, what was written is a sub-multiset
    big, out = _guarded(k - 1, torch.float32, CANARY)
    cursor.zero_()
    ops.surface_gather(b, d, out, cursor)
    assert int(cursor.item()) == k
    assert (big[:GUARD] == CANARY).all() and (big[GUARD + k - 1:] == CANARY).all()
    got = np.sort(out.cpu().numpy())
    assert np.isin(got, want).all() and (got != CANARY).all()


# ------------------------------------------------------------------------------------------------ the evaluator
def _subject(name, pred, target, labels, spacing=None):
    attrs = {} if spacing is None else {"spacing": spacing}
    return {"name": name,
            "pred": LabelMap(torch.from_numpy(np.asarray(pred, dtype=np.int64))[None].to(DEV), labels, **attrs),
            "target": LabelMap(torch.from_numpy(np.asarray(target, dtype=np.int64))[None].to(DEV), labels, **attrs)}


def _row(df, subject, label):
    rows = df[(df["subject"] == subject) & (df["label"] == label)]
    assert len(rows) == 1
    return rows.iloc[0]


def _same_frames(a, b):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for c in a.columns:
        x, y = a[c].to_numpy(), b[c].to_numpy()
        if x.dtype.kind == "f":
            assert np.array_equal(np.float64(x).view(np.int64), np.float64(y).view(np.int64)), c
        else:
            assert list(x) == list(y), c


def test_evaluator_fixture(fx):
    """every case of the fixture in one call, each subject with its own 'spacing' key"""
    labels = _labels(fx)
    subjects = [_subject(f"case{c}", fx[f"{c}.pred"], fx[f"{c}.target"], labels, tuple(fx[f"{c}.spacing"]))
                for c in range(int(fx["cases"]))]
    ev = SurfaceDistanceEvaluator("pred", "target", percentile=int(fx["percentile"]), tolerance=float(fx["tolerance"]),
                                  stats_to_output=SURFACE_STAT_NAMES)
    df = ev(subjects)["subject_stats"]
    nans = 0
    for c in range(int(fx["cases"])):
        for name in labels:
            want, row = fx[f"{c}.{name}.stats"], _row(df, f"case{c}", name)
            for k, stat in enumerate(SURFACE_STAT_NAMES):
                print(c, name, stat, row[stat], want[k])
                if np.isnan(want[k]):
                    nans += 1
                    assert np.isnan(row[stat]), (c, name, stat)
                elif stat.endswith("_surface"):
                    assert row[stat] == want[k], (c, name, stat)
                else:
                    assert abs(row[stat] - want[k]) <= 2e-6 * abs(want[k]), (c, name, stat, row[stat], want[k])
    assert nans >= 6
    # the functional form gives the evaluator's row
    c = 2
    one = surface_distances(fx[f"{c}.pred"], fx[f"{c}.target"], labels, spacing=tuple(fx[f"{c}.spacing"]),
                            percentile=int(fx["percentile"]), tolerance=float(fx["tolerance"]))
    assert list(one) == list(labels)
    for name in labels:
        assert tuple(one[name]) == SURFACE_STAT_NAMES
        for stat in SURFACE_STAT_NAMES:
            assert np.float32(one[name][stat]) == np.float32(_row(df, f"case{c}", name)[stat]), (name, stat)


def test_evaluator_identical_maps(fx):
    labels = _labels(fx)
    s = _subject("same", fx["1.target"], fx["1.target"], labels)
    ev = SurfaceDistanceEvaluator("pred", "target", spacing=(1.2, 0.7, 3.0), stats_to_output=SURFACE_STAT_NAMES)
    df = ev([s])["subject_stats"]
    for name in labels:
        row = _row(df, "same", name)
        assert row["hd"] == 0 and row["hd95"] == 0 and row["assd"] == 0 and row["nsd"] == 1
        assert row["asd_pred_to_target"] == 0 and row["asd_target_to_pred"] == 0
        assert row["pred_surface"] == row["target_surface"] == fx[f"1.{name}.border_target"].sum()

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_evaluator_shifted_cube(axis):
    spacing = (0.5, 1.0, 2.5)
    target = np.zeros((12, 13, 14), dtype=np.int64)
    target[3:8, 4:9, 3:9] = 1
    pred = np.roll(target, 1, axis=axis)
    ev = SurfaceDistanceEvaluator("pred", "target", spacing=spacing, stats_to_output=('hd', 'hd95', 'assd'))
    row = _row(ev([_subject("cube", pred, target, {"cube": 1})])["subject_stats"], "cube", "cube")
    assert row["hd"] == spacing[axis]
    assert 0 < row["assd"] < row["hd95"] <= row["hd"]


def test_evaluator_many_subjects_layout_and_repeatability():
    labels = {"inner": 1, "outer": 2}
    rng = np.random.default_rng(3)
    subjects = []
    for i, shape in enumerate([(9, 8, 7), (5, 12, 70), (16, 6, 10)]):
        target = rng.integers(0, 3, shape) * (rng.random(shape) < 0.4)
        pred = np.where(rng.random(shape) < 0.9, target, rng.integers(0, 3, shape))
        subjects.append(_subject(f"s{i}", pred, target, labels, spacing=(1.0 + i, 0.7, 1.5)))
    stats = ('hd', 'hd95', 'assd', 'nsd', 'pred_surface')
    ev = SurfaceDistanceEvaluator("pred", "target", stats_to_output=stats)
    together = ev(subjects)
    for i, s in enumerate(subjects):
        alone = ev([s])["subject_stats"]
        part = together["subject_stats"].iloc[2 * i:2 * i + 2].reset_index(drop=True)
        _same_frames(part, alone)
    seg = SegmentationEvaluator("pred", "target", stats_to_output=('dice',))(subjects)
    df = together["subject_stats"]
    assert list(df.columns) == ["subject", "label", *stats]
    assert list(df["subject"]) == list(seg["subject_stats"]["subject"]) and list(df["label"]) == list(seg["subject_stats"]["label"])
    assert together["summary_stats"].dim_names == ["summary_stat", "label", "stat"]
    assert together["summary_stats"].dim_keys == [('mean', 'std', 'min', 'max'), ["inner", "outer"], stats]
    assert together["summary_stats"].dim_keys[:2] == seg["summary_stats"].dim_keys[:2]
    again = ev(subjects)
    _same_frames(again["subject_stats"], df)
    assert torch.equal(again["summary_stats"].data.view(torch.int32), together["summary_stats"].data.view(torch.int32))


def test_evaluator_reads_a_pending_score_label_map():
    g = torch.Generator().manual_seed(3)
    sh = (12, 11, 6)
    y_pred = torch.softmax(torch.randn(2, 2, *sh, generator=g), dim=1)
    y = nn.functional.one_hot(torch.randint(0, 2, (2,) + sh, generator=g), 2).permute(0, 4, 1, 2, 3).float()
    batch = {"y_pred": y_pred.to(DEV), "y": y.to(DEV), "name": ["a", "b"]}
    lazy = add_evaluation_labels(dict(batch), _msseg2_chain(), {"lesion": 1})
    written = add_evaluation_labels(dict(batch), _msseg2_chain(), {"lesion": 1}, write=True)
    assert all(s["y_pred_eval"].pending for s in lazy) and not any(s["y_pred_eval"].pending for s in written)
    ev = SurfaceDistanceEvaluator("y_pred_eval", "y_eval", stats_to_output=SURFACE_STAT_NAMES)
    got = ev(lazy)
    assert not any(s["y_pred_eval"].pending for s in lazy)
    _same_frames(got["subject_stats"], ev(written)["subject_stats"])
    lesion = (y_pred[0].argmax(0) == 1).numpy().astype(np.int64)
    want = R.stats(lesion, y[0].argmax(0).numpy(), 1)
    row = _row(got["subject_stats"], "a", "lesion")
    for stat in SURFACE_STAT_NAMES:
        assert abs(row[stat] - want[stat]) <= 2e-6 * abs(want[stat]), stat
