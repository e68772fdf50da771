"""Contour images without a GPU: the make_grid geometry, ContourImageEvaluator.get_slice_property, the host-side checks
of ops.slice_mosaic and of the three C entry points (csrc/contour.hip), and tests/contour_ref.py against the reference's
recorded planes, slice ids and mosaics (tests/golden/contour.npz, tools/gen_golden_contour.py)."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

import contour_ref
from conftest import GOLDEN
from segmentation_pipeline_amd import _lib, ops
from segmentation_pipeline_amd.evaluators import (ContourImageEvaluator, FindInterestingSlice, LabelMap, ScalarImage,
                                                  _RankCall, _RankedPlanes)


@pytest.mark.parametrize("n,ncol", [(1, 1), (1, 4), (5, 2), (3, 7), (4, 2), (6, 1)])
def test_grid_geometry_matches_the_numpy_grid(n, ncol):
    h, w = 3, 5
    tiles = [np.full((h, w), k + 1, np.int32) for k in range(n)]
    grid = contour_ref.make_grid(tiles, ncol, -1)
    rows, cols, at = ops.grid_geometry(n, h, w, ncol)
    assert grid.shape == (rows, cols) and len(at) == n
    if n == 1:
        assert (rows, cols) == (h, w) and at == [(0, 0)]      # no padding at all
    else:
        xmaps = min(ncol, n)
        assert (rows, cols) == (-(-n // xmaps) * (h + 1) + 1, xmaps * (w + 1) + 1)
    covered = np.zeros_like(grid, dtype=bool)
    for k, (r, c) in enumerate(at):
        assert (grid[r:r + h, c:c + w] == k + 1).all()
        covered[r:r + h, c:c + w] = True
    assert (grid[~covered] == -1).all()      # everything else is padding, the missing tiles of a ragged row too
    with pytest.raises(ValueError):
        ops.grid_geometry(0, h, w, ncol)


def test_slice_shape_and_unknown_plane():
    assert ops.slice_shape((5, 7, 9), "Axial") == (5, 7)
    assert ops.slice_shape((5, 7, 9), "Coronal") == (9, 5)
    assert ops.slice_shape((5, 7, 9), "Saggital") == (9, 7)
    with pytest.raises(ValueError):
        ops.slice_shape((5, 7, 9), "interesting")
    x = np.arange(5 * 7 * 9).reshape(5, 7, 9)
    for plane in contour_ref.PLANES:
        assert contour_ref.slice_volume(x, plane, 1).shape == ops.slice_shape(x.shape, plane)


def test_get_slice_property_three_branches():
    ev = ContourImageEvaluator("Axial", "img", "y_pred", "y", 1, False, 2, interesting_slice=True)
    image = LabelMap(torch.zeros(1, 4, 6, 9))
    prop = {"Axial": torch.tensor([7, 2, 5]), "Coronal": torch.tensor([], dtype=torch.int64), "Saggital": torch.tensor([3])}
    assert int(ev.get_slice_property(image, prop, 1, "Axial")) == 2          # the entry at the rank
    assert int(ev.get_slice_property(image, prop, 3, "Axial")) == 5          # past the end: the last entry
    assert int(ev.get_slice_property(image, prop, 1, "Saggital")) == 3
    assert ev.get_slice_property(image, prop, 0, "Coronal") == 6 // 2        # nothing ranked: the middle of the axis
    assert ev.get_slice_property(image, {"Axial": torch.tensor([])}, 0, "Axial") == 9 // 2
    # without interesting_slice the slice id and the plane pass through
    assert ContourImageEvaluator("Coronal", "img", "y_pred", "y", 4, False, 2).get_slice_id({}, "Coronal") == (4, "Coronal")


def test_ranked_planes_is_a_mapping_that_survives_copies():
    # one holder of [2, 3, 4]: the tables as ops.slice_rank lays them out (padded with id -1 / count 0)
    ids = torch.tensor([1, -1, 2, 0, -1, -1, -1, -1, -1], dtype=torch.int32)
    ranked = torch.tensor([5, 0, 4, 1, 0, 0, 0, 0, 0], dtype=torch.int32)
    call = _RankCall(ids, ranked, torch.tensor([1, 2, 0], dtype=torch.int32), [(0, 2), (2, 3), (5, 4)])
    planes = _RankedPlanes(call, call.ids, 0)
    want = {"Saggital": [1], "Coronal": [2, 0], "Axial": []}
    assert list(planes) == list(want) and len(planes) == 3 and "Axial" in planes and "axial" not in planes
    for copy in (planes, dict(planes), {**planes}, dict(planes.items())):
        assert {k: v.tolist() for k, v in copy.items()} == want
    assert [v.tolist() for v in planes.values()] == list(want.values()) and planes.get("nowhere") is None
    with pytest.raises(KeyError):
        planes["nowhere"]
    assert call.pick(0).tolist() == [[1, 5], [2, 4], [2, 2]]      # an empty plane: the middle of the axis, for both
    assert call.pick(7).tolist() == [[1, 5], [0, 1], [2, 2]]      # past the end: the last entry


def test_find_interesting_slice_picks_the_label_maps_of_a_subject():
    is_label_map = FindInterestingSlice._is_label_map

    class Holder(dict):             # what a torchio image looks like from here
        @property
        def data(self):
            return self["data"]
    t = torch.zeros(1, 2, 2, 2)
    assert is_label_map(LabelMap(t)) and is_label_map(Holder(data=t)) and is_label_map(Holder(data=t, type="label"))
    assert not is_label_map(ScalarImage(t)) and not is_label_map(Holder(data=t, type="intensity"))
    assert not is_label_map("name") and not is_label_map(t) and not is_label_map({"data": t})


def test_mosaic_shape_and_dtype_mismatches_raise_before_any_launch():
    a, b = torch.zeros(5, 7, 9), torch.zeros(5, 7, 8)
    with pytest.raises(ValueError, match="among tiles"):
        ops.slice_mosaic([([(a, "Coronal", 0), (b, "Coronal", 0)], 2, 0, None)])
    ops_ok_axial = [(a, "Axial", 0), (b, "Axial", 0)]         # the axial slices of both are 5 x 7 ...
    with pytest.raises(ValueError, match="among tiles"):      # ... but not the imputed shape of a zeros tile
        ops.slice_mosaic([(ops_ok_axial + [(None, "Axial", 0)], 2, 0, (7, 5))])
    with pytest.raises(ValueError, match="element type"):
        ops.slice_mosaic([([(a, "Axial", 0), (a.long(), "Axial", 0)], 2, 0, None)])
    with pytest.raises(ValueError, match="plane"):
        ops.slice_mosaic([([(a, "interesting", 0)], 2, 0, None)])
    with pytest.raises(ValueError):
        ops.slice_mosaic([([(None, "Axial", 0)], 2, 0, None)])
    with pytest.raises(_lib.M355Error):      # shapes agree: the next check wants device tensors
        ops.slice_mosaic([(ops_ok_axial, 2, 0, None)])


def _err(L):
    return L.m355_last_error()


def test_slice_counts_argument_validation():
    L = _lib.lib()
    dev, p = ctypes.c_void_p(256), ctypes.c_void_p(512)

    def desc(size3=(4, 5, 6), dtype=_lib.EV_U8, channels=0, offset=0, data=1024):
        d = (_lib.SliceCountsDesc * 1)()
        d[0].data, d[0].counts_offset, d[0].dtype, d[0].channels = data, offset, dtype, channels
        d[0].size3[:] = size3
        return d
    assert L.m355_slice_counts(None, 1, dev, p, None) == -1 and b"slice_counts" in _err(L)
    assert L.m355_slice_counts(desc(), 0, dev, p, None) == -1 and b"subjects" in _err(L)
    assert L.m355_slice_counts(desc(data=None), 1, dev, p, None) == -1 and b"null volume" in _err(L)
    assert L.m355_slice_counts(desc(size3=(2048, 1024, 1024)), 1, dev, p, None) == -1 and b"2^31" in _err(L)
    assert L.m355_slice_counts(desc(size3=(1, 1, 2049)), 1, dev, p, None) == -1 and b"axis 2" in _err(L)
    assert L.m355_slice_counts(desc(size3=(0, 1, 1)), 1, dev, p, None) == -1
    assert L.m355_slice_counts(desc(dtype=_lib.EV_BF16), 1, dev, p, None) == -1 and b"element type" in _err(L)
    assert L.m355_slice_counts(desc(dtype=_lib.EV_I64, channels=2), 1, dev, p, None) == -1 and b"one-hot" in _err(L)
    assert L.m355_slice_counts(desc(dtype=_lib.EV_F32, channels=65), 1, dev, p, None) == -1 and b"channels" in _err(L)
    assert L.m355_slice_counts(desc(offset=8), 1, dev, p, None) == -1 and b"offset" in _err(L)


def test_slice_rank_argument_validation():
    L = _lib.lib()
    p = ctypes.c_void_p(512)

    def segs(offset=0, n=4):
        s = (_lib.SliceSeg * 1)()
        s[0].offset, s[0].len = offset, n
        return s
    assert L.m355_slice_rank(None, segs(), 1, p, p, p, p, None) == -1 and b"slice_rank" in _err(L)
    assert L.m355_slice_rank(p, segs(), 0, p, p, p, p, None) == -1 and b"segments" in _err(L)
    assert L.m355_slice_rank(p, segs(n=0), 1, p, p, p, p, None) == -1 and b"slices" in _err(L)
    assert L.m355_slice_rank(p, segs(n=2049), 1, p, p, p, p, None) == -1
    assert L.m355_slice_rank(p, segs(offset=-1), 1, p, p, p, p, None) == -1


def test_slice_mosaic_argument_validation():
    L = _lib.lib()
    dev = ctypes.c_void_p(256)

    def call(n=2, ncol=2, rows=None, cols=None, plane=_lib.PLANE_AXIAL, slice_id=0, dtype=_lib.EV_F32,
             tile_dtype=_lib.EV_F32, size3=(5, 7, 9), at=None, nm=1, first=0, hw=(5, 7)):
        r, c, pos = ops.grid_geometry(n, hw[0], hw[1], ncol)
        m = (_lib.SliceMosaicDesc * 1)()
        m[0].out, m[0].dtype, m[0].rows, m[0].cols = 4096, dtype, r if rows is None else rows, c if cols is None else cols
        m[0].tile_h, m[0].tile_w, m[0].ncol, m[0].ntiles, m[0].first_tile, m[0].pad = hw[0], hw[1], ncol, n, first, -1.0
        t = (_lib.SliceTileDesc * n)()
        for k in range(n):
            t[k].src, t[k].dtype, t[k].plane, t[k].slice = 8192, tile_dtype, plane, slice_id
            t[k].size3[:] = size3
            t[k].row0, t[k].col0 = pos[k] if at is None else at
        return L.m355_slice_mosaic(m, nm, t, n, dev, None)
    assert L.m355_slice_mosaic(None, 1, None, 1, dev, None) == -1 and b"slice_mosaic" in _err(L)
    assert call(nm=4) == -1 and b"mosaics" in _err(L)
    assert call(rows=3) == -1 and b"cells" in _err(L)
    assert call(slice_id=9) == -1 and b"slice 9 of 9" in _err(L)
    assert call(slice_id=-1) == -1
    assert call(plane=3) == -1 and b"plane" in _err(L)
    assert call(plane=_lib.PLANE_CORONAL) == -1 and b"9 x 5" in _err(L)      # a coronal slice is D x W
    assert call(tile_dtype=_lib.EV_I64) == -1 and b"element type" in _err(L)
    assert call(dtype=_lib.EV_I64, tile_dtype=_lib.EV_BF16) == -1
    assert call(at=(0, 0)) == -1 and b"make_grid" in _err(L)
    assert call(first=1) == -1 and b"tiles" in _err(L)
    assert call(size3=(5, 7, 4096)) == -1


# ------------------------------------------------------------------------------------------------ golden
@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "contour.npz")))


def golden_cases(fx):
    return json.loads(str(fx["cases"]))


def golden_subjects(fx, case, device=None):
    """the subjects of one recorded case as evaluators' holders, on `device` when given"""
    lv = dict(zip([str(n) for n in fx["label_names"]], [int(v) for v in fx["label_values"]]))

    def put(a):
        t = torch.from_numpy(a)[None]
        return t if device is None else t.to(device)
    out = []
    for pos, i in enumerate(case["subjects"]):
        s = {"name": f"s{pos}", "img": ScalarImage(put(fx[f"subject.{i}.img"])),
             "y": LabelMap(put(fx[f"subject.{i}.y"]), lv), "y_pred": LabelMap(put(fx[f"subject.{i}.y_pred"]), lv)}
        for name in case.get("drop", {}).get(str(pos), []):
            del s[name]
        out.append(s)
    return out


def golden_calls(fx, key, case, subjects):
    """[(subjects of the get_image call, recorded plane, slice ids, {name: mosaic})]"""
    groups = [[s] for s in subjects] if case.get("split_subjects") else [subjects]
    assert int(fx[f"{key}.calls"]) == len(groups)
    return [(g, str(fx[f"{key}.{n}.plane"]), fx[f"{key}.{n}.slice_ids"].tolist(),
             {name: fx[f"{key}.{n}.{name}"] for name in ("img", "y", "y_pred") if f"{key}.{n}.{name}" in fx})
            for n, g in enumerate(groups)]


def test_contour_ref_reproduces_the_reference(fx):
    cases = golden_cases(fx)
    assert len(cases) >= 8
    for key, case in cases.items():
        subjects = golden_subjects(fx, case)
        if "seed" in case:
            random.seed(case["seed"])
        for group, plane, slice_ids, want in golden_calls(fx, key, case, subjects):
            resolved, img, y, y_pred, _ = contour_ref.mosaics(group, case["plane"], "img", "y_pred", "y", case["slice_id"],
                                                              case["ncol"], case.get("interesting_slice", False))
            assert [p for _, p in resolved] == [plane] * len(group), key
            assert [int(k) for k, _ in resolved] == slice_ids, key
            for name, got in (("img", img), ("y", y), ("y_pred", y_pred)):
                assert (got is None) == (name not in want), (key, name)
                if got is not None:
                    assert got.dtype == want[name].dtype and got.shape == want[name].shape, (key, name)
                    np.testing.assert_array_equal(got, want[name], err_msg=f"{key} {name}")


def test_rank_orders_ties_by_ascending_slice_id():
    ids, counts = contour_ref.rank(torch.tensor([3, 0, 5, 3, 5, 1, 0, 3]))
    assert ids == [2, 4, 0, 3, 7, 5] and counts == [5, 5, 3, 3, 3, 1]
