"""Region statistics, ImageRegionEvaluator and the dataset fingerprint: what can be checked without a GPU -- the
restatement of the GPU tests (tests/region_stats_ref.py) against the fixture made by the reference's own functions, the
host logic of the new Python on host tensors through a stand-in for ops.region_stats, the binding, and the argument
checks of the entry points (no launches)."""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import region_stats_ref as R
from conftest import ROOT
from segmentation_pipeline_amd import _lib, evaluators, ops
from segmentation_pipeline_amd.data_processing import dataset_fingerprint as F
from segmentation_pipeline_amd.evaluators import ImageRegionEvaluator, LabelMap, ScalarImage

P = ctypes.c_void_p
ENTRY_POINTS = ("m355_region_stats_workspace", "m355_region_stats_plan", "m355_region_stats")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("region_stats.npz")


def _json(fx, key):
    return json.loads(str(fx[key]))


def _subjects(fx, device=None):
    label_values = _json(fx, "label_values")
    out = []
    for i in range(int(fx["n"])):
        def t(k):
            x = fx.t(f"{i}.{k}")
            return x if device is None else x.to(device)
        out.append({"name": str(fx["names"][i]), "spacing": tuple(float(v) for v in fx["spacing"][i]),
                    "seg": LabelMap(t("seg"), label_values["seg"]), "lesion": LabelMap(t("lesion"), label_values["lesion"]),
                    "t1": ScalarImage(t("t1")), "dwi": ScalarImage(t("dwi"))})
    return out


def _plain(x):
    """tuples as lists, as a JSON round trip leaves them"""
    return json.loads(json.dumps(x))


# ---------------------------------------------------------------------------------------------- restatement vs the reference
def test_restatement_agrees_with_the_reference_fixture(fx):
    want = _json(fx, "subject_fingerprints")
    label_values = _json(fx, "label_values")
    for i, s in enumerate(_subjects(fx)):
        fp = want[s["name"]]
        for map_name in ("seg", "lesion"):
            names = list(label_values[map_name])
            masks = R.region_masks(s[map_name].data, list(label_values[map_name].values()))
            count, bounds, _ = R.region_stats_ref(s[map_name].data, [], list(label_values[map_name].values()))
            for row, name in list(enumerate(names)) + [(len(names), "all")]:
                views = R.bounds_views(masks[row])
                assert views == fp["label_bounds"][map_name][name], (i, map_name, name)
                assert bounds[row].tolist() == views["extents"] and count[row] == masks[row].sum()
        _, _, stats = R.region_stats_ref(s["seg"].data, [s["t1"].data, s["dwi"].data], [])
        for k, image in enumerate(("t1", "dwi")):
            got = dict(zip(R.STATS, stats[-1, k].tolist()))
            ref = fp["intensity_stats"][image]
            for stat in ("median", "min", "max"):
                assert got[stat] == ref[stat], (i, image, stat)
            for stat in ("mean", "std"):   # the reference sums in float32
                assert got[stat] == pytest.approx(ref[stat], rel=1e-5), (i, image, stat)
    assert R.bounds_views(fx["0.lesion"][0] != 0) == _json(fx, "mask_bounds")


def test_across_subject_summary_is_exact(fx):
    merged = {}
    for fp in _json(fx, "subject_fingerprints").values():
        F.merge_dict(fp, merged)
    assert merged["spacing"] == [list(v) for v in fx["spacing"].tolist()]
    assert _plain(F.summarize(merged)) == _json(fx, "summary_fingerprint")
    with pytest.raises(RuntimeError, match="Unexpected element"):
        F.summarize({"a": 3})
    host = F.get_summary_stats(torch.tensor([[1, 5], [3, 2], [9, 4]]), dim=0)
    assert host == {'mean': (pytest.approx(13 / 3), pytest.approx(11 / 3)), 'std': (pytest.approx(np.std([1, 3, 9], ddof=1)),
                    pytest.approx(np.std([5, 2, 4], ddof=1))), 'median': (3, 4), 'min': (1, 2), 'max': (9, 5)}
    assert F.get_summary_stats(torch.tensor([4.0, 1.0, 3.0, 2.0]))['median'] == 2.0   # the lower middle value


def test_restatement_semantics():
    lab = np.array([[[0, 1, 1, 2], [5, 5, 0, 2]]], dtype=np.int16)
    img = np.array([[[[1.0, 2.0, 4.0, -1.0], [np.inf, 3.0, 0.0, np.nan]]]], dtype=np.float32)
    count, bounds, stats = R.region_stats_ref(lab, [img], [1, 2, 9, 1])
    assert count.tolist() == [2, 2, 0, 2, 6, 8] and np.array_equal(stats[3], stats[0])
    assert bounds[0].tolist() == [0, 0, 0, 0, 1, 2] and bounds[2].tolist() == [1, -1, 2, -1, 4, -1]
    assert bounds[4].tolist() == [0, 0, 0, 1, 0, 3] and bounds[5].tolist() == [0, 0, 0, 1, 0, 3]
    assert stats[0, 0].tolist() == [3.0, pytest.approx(2.0 ** 0.5), 2.0, 2.0, 4.0]
    assert np.isnan(stats[1, 0]).all() and np.isnan(stats[2, 0]).all() and np.isnan(stats[5, 0]).all()
    one = R.stats5([7.0])
    assert one[0] == 7.0 and np.isnan(one[1]) and one[2:].tolist() == [7.0, 7.0, 7.0]
    assert R.stats5([-np.inf, 1.0, np.inf])[2:].tolist() == [1.0, -np.inf, np.inf]
    assert R.ulp_distance(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1
    assert R.ulp_distance(np.float32(np.nan), np.float32(np.nan)) == 0 and R.ulp_distance(np.float32(np.nan), 1.0) > 2
    assert R.ulp_distance(np.float32(-0.0), np.float32(0.0)) == 0


# ---------------------------------------------------------------------------------------------- host logic on a stand-in
def test_fingerprint_nesting_and_values_on_host_tensors(fx, monkeypatch, tmp_path):
    monkeypatch.setattr(ops, "region_stats", R.stub_region_stats)
    subjects = _subjects(fx)
    want, want_summary = _json(fx, "subject_fingerprints"), _json(fx, "summary_fingerprint")

    class Dataset:
        all_subjects = subjects
        root = str(tmp_path)

    per_subject, summary = F.get_dataset_fingerprint(Dataset(), save=True)
    assert list(per_subject) == [s["name"] for s in subjects]
    for s in subjects:
        got, ref = per_subject[s["name"]], want[s["name"]]
        assert list(got) == ['spacing', 'spatial_shape', 'label_bounds', 'intensity_stats']
        assert got['spacing'] == s["spacing"] and got['spatial_shape'] == tuple(s["seg"].data.shape[1:])
        assert _plain(got['label_bounds']) == ref['label_bounds']
        assert list(got['label_bounds']['seg']) == ['all', 'left', 'right', 'stem']
        assert list(got['intensity_stats']) == ['t1', 'dwi']
        for image, stats in got['intensity_stats'].items():
            assert list(stats) == list(R.STATS)
            for stat in ("median", "min", "max"):
                assert stats[stat] == ref['intensity_stats'][image][stat]
            for stat in ("mean", "std"):
                assert stats[stat] == pytest.approx(ref['intensity_stats'][image][stat], rel=1e-5)
    # the summary: integer fields exact, the rest through the same float32 torch functions on nearly the same numbers
    assert _plain(summary['label_bounds']) == want_summary['label_bounds']
    assert _plain(summary['spacing']) == want_summary['spacing']
    assert _plain(summary['spatial_shape']) == want_summary['spatial_shape']
    assert summary['intensity_stats']['t1']['max']['max'] == want_summary['intensity_stats']['t1']['max']['max']
    # save=True: the two files hold what was returned
    with open(tmp_path / "fingerprint" / "subject_fingerprints.json") as f:
        assert json.load(f) == _plain(per_subject)
    with open(tmp_path / "fingerprint" / "fingerprint.json") as f:
        assert json.load(f) == _plain(summary)

    # a plain sequence of subjects, image_names filtering, a transform on a copy
    only, _ = F.get_dataset_fingerprint(subjects[:2], image_names=["t1", "lesion", "missing"])
    assert list(only["subject_0"]['intensity_stats']) == ['t1'] and list(only["subject_0"]['label_bounds']) == ['lesion']

    def halve(subject):
        subject["t1"] = ScalarImage(subject["t1"].data * 0.5)
        return subject
    halved, _ = F.get_dataset_fingerprint(subjects[:1], transform=halve, image_names=["t1"])
    assert halved["subject_0"]['intensity_stats']['t1']['max'] == 0.5 * per_subject["subject_0"]['intensity_stats']['t1']['max']
    assert subjects[0]["t1"].data.max().item() == per_subject["subject_0"]['intensity_stats']['t1']['max']

    assert F.get_bounds(fx.t("0.lesion")[0] != 0) == _json(fx, "mask_bounds")
    assert _plain(F.get_label_bounds(subjects[1]["seg"])) == want["subject_1"]['label_bounds']['seg']


def test_empty_label_raises_value_error(fx, monkeypatch):
    monkeypatch.setattr(ops, "region_stats", R.stub_region_stats)
    s = _subjects(fx)[0]
    s["seg"] = LabelMap(s["seg"].data, {"left": 1, "absent": 42})
    with pytest.raises(ValueError, match="absent"):
        F.get_dataset_fingerprint([s])
    with pytest.raises(ValueError, match="no voxel"):
        F.get_bounds(torch.zeros(3, 4, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="no voxel"):
        F.get_label_bounds(LabelMap(torch.zeros(1, 3, 4, 5, dtype=torch.uint8), {"a": 1}))


def test_image_region_evaluator_on_host_tensors(fx, monkeypatch):
    monkeypatch.setattr(ops, "region_stats", R.stub_region_stats)
    subjects = _subjects(fx)
    sig = inspect.signature(ImageRegionEvaluator.__init__)
    assert list(sig.parameters)[1:] == ["label_map_name", "image_names", "stats_to_output", "summary_stats_to_output"]
    ev = ImageRegionEvaluator("seg", ["t1", "dwi"])
    assert ev.stats_to_output == ('mean', 'std', 'median', 'min', 'max', 'volume')
    assert ev.summary_stats_to_output == ('mean', 'std', 'min', 'max')
    assert isinstance(ev, evaluators.Evaluator) and "ImageRegionEvaluator" in evaluators.__all__
    out = ev(subjects)
    df, summary = out['subject_stats'], out['summary_stats']
    assert list(df.columns) == ['subject', 'label', 'image_name', 'mean', 'std', 'median', 'min', 'max', 'volume']
    assert len(df) == len(subjects) * 3 * 2
    assert summary.dim_names == ['summary_stat', 'label', 'image_name', 'stat']
    for s in subjects:
        count, _, stats = R.region_stats_ref(s["seg"].data, [s["t1"].data, s["dwi"].data], [1, 2, 7])
        for l, label in enumerate(("left", "right", "stem")):
            for k, image in enumerate(("t1", "dwi")):
                row = df[(df.subject == s["name"]) & (df.label == label) & (df.image_name == image)].iloc[0]
                assert [np.float32(row[c]) for c in R.STATS] == stats[l, k].tolist()
                assert row["volume"] == count[l]
    col = torch.tensor(df[(df.label == "stem") & (df.image_name == "dwi")]["median"].to_numpy(), dtype=torch.float32)
    assert summary["mean", "stem", "dwi", "median"].item() == col.mean().item()
    few = ImageRegionEvaluator("lesion", ["t1"], stats_to_output=("volume", "max"), summary_stats_to_output=("max",))(subjects)
    assert list(few['subject_stats'].columns) == ['subject', 'label', 'image_name', 'volume', 'max']
    with pytest.raises(_lib.M355Error, match="unknown image region stats .'dice'."):
        ImageRegionEvaluator("a", ["b"], stats_to_output=("mean", "dice"))


# ---------------------------------------------------------------------------------------------- binding and argument checks
def test_symbols_are_bound_and_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (m355_\w+)", out))
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and name in exported and getattr(_lib.lib(), name) is not None
    header = open(os.path.join(ROOT, "include", "m355seg.h")).read()
    assert "m355_region_image" in header and "#define M355_ABI_VERSION 3" in header
    assert _lib.lib().m355_version() == 3 == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.RegionImage) == 16
    assert {"get_bounds", "get_label_bounds", "get_summary_stats", "merge_dict", "summarize",
            "get_dataset_fingerprint"} <= set(F.__all__)
    assert list(inspect.signature(F.get_dataset_fingerprint).parameters) == ["dataset", "transform", "save", "image_names"]
    assert ops.REGION_STATS == R.STATS


def test_plan_and_workspace_queries():
    L = _lib.lib()
    cap, block, per_thread, group = ops.region_stats_plan()
    assert cap >= 256 and block % 64 == 0 and per_thread >= 1 and group >= 1
    assert L.m355_region_stats_plan(None) == -1 and b"region_stats_plan" in L.m355_last_error()
    sizes = [L.m355_region_stats_workspace(l, 1, 1) for l in (0, 1, 2, 8, 64)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert L.m355_region_stats_workspace(2, 1, 0) < L.m355_region_stats_workspace(2, 1, 1)
    assert L.m355_region_stats_workspace(-1, 1, 1) == 0 and L.m355_region_stats_workspace(65, 1, 1) == 0
    assert L.m355_region_stats_workspace(2, 0, 1) == 0
    result, ws = ops.region_stats_bytes(2, 1)
    assert result == 8 * 4 + 24 * 4 + 20 * 4 and ws == L.m355_region_stats_workspace(2, 1, 1)
    assert ops.region_stats_bytes(70, 0)[1] == 0


def _call(labels=P(64), dtype=_lib.EV_I16, size=(4, 4, 4), image=(P(64), _lib.EV_F32, 1), K=1, values=(1, 2), L=None,
          count=P(64), bounds=P(64), stats=P(64), ws=P(64), ws_bytes=1 << 24, size_null=False, images_null=False,
          values_null=False):
    lib = _lib.lib()
    images = (_lib.RegionImage * 1)()
    images[0].data, images[0].dtype, images[0].channels = (image[0].value if image[0] else None), image[1], image[2]
    vals = (ctypes.c_int32 * max(1, len(values)))(*values)
    rc = lib.m355_region_stats(labels, dtype, None if size_null else (ctypes.c_int32 * 3)(*size),
                               None if images_null else images, K, None if values_null else vals,
                               len(values) if L is None else L, 1, count, bounds, stats, ws, ws_bytes, None)
    return rc, lib.m355_last_error()


def test_argument_checks_reject_before_any_launch():
    for kw in (dict(labels=None), dict(size_null=True), dict(count=None), dict(bounds=None), dict(stats=None),
               dict(ws=None), dict(images_null=True), dict(values_null=True), dict(image=(None, _lib.EV_F32, 1))):
        rc, msg = _call(**kw)
        assert rc == -1 and b"region_stats: " in msg and b"null pointer" in msg, kw
    for size in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        rc, msg = _call(size=size)
        assert rc == -1 and b"region_stats: non-positive size" in msg, size
    rc, msg = _call(image=(P(64), _lib.EV_F32, 0))
    assert rc == -1 and b"non-positive channels" in msg
    rc, msg = _call(L=-1)
    assert rc == -1 and b"region_stats: negative" in msg
    rc, msg = _call(K=-1)
    assert rc == -1 and b"region_stats: negative" in msg
    rc, msg = _call(values=tuple(range(1, 66)))
    assert rc == -2 and b"65 label values" in msg
    rc, msg = _call(dtype=_lib.EV_BF16)
    assert rc == -2 and b"label element type" in msg
    for bad in (_lib.EV_I64, _lib.EV_I32, _lib.EV_BOOL, 17):
        rc, msg = _call(image=(P(64), bad, 1))
        assert rc == -2 and b"image 0: element type" in msg, bad
    rc, msg = _call(values=(2 ** 31 - 1,), dtype=_lib.EV_F32)
    assert rc == -2 and b"out of range" in msg
    rc, msg = _call(size=(2048, 2048, 512), image=(P(64), _lib.EV_F32, 2))
    assert rc == -2 and b"2^32 values" in msg
    need = _lib.lib().m355_region_stats_workspace(2, 1, 1)
    rc, msg = _call(ws_bytes=need - 1)
    assert rc == -4 and b"region_stats: workspace too small" in msg
    # an invalid argument is reported before an unsupported one
    rc, _ = _call(size=(0, 4, 4), dtype=_lib.EV_BF16)
    assert rc == -1


def test_wrapper_checks_need_no_gpu():
    lab = torch.zeros(1, 3, 4, 5, dtype=torch.int16)
    with pytest.raises(_lib.M355Error, match="expected a device tensor"):
        ops.region_stats(lab, [], [1])
    with pytest.raises(_lib.M355Error, match=r"a label volume \[W, H, D\]"):
        ops.region_stats(torch.zeros(2, 3, 4, 5, dtype=torch.int16), [], [1])
    with pytest.raises(_lib.M355Error, match="one list of images per label volume"):
        ops.region_stats([lab, lab], [[]], [1])
    with pytest.raises(_lib.M355Error, match="element type torch.float64"):
        ops.region_stats(torch.zeros(1, 3, 4, 5, dtype=torch.float64), [], [1])
    values, uniq, chunks = ops._rs_chunks([3, 1, 3] + list(range(100, 170)))
    assert uniq[:2] == [3, 1] and [len(c) for c in chunks] == [64, 8] and len(values) == 73
