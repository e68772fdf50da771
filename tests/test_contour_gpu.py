"""Contour images on the device (csrc/contour.hip via ops.slice_counts / slice_rank / slice_mosaic, evaluators.
find_interesting_slices, FindInterestingSlice, ContourImageEvaluator, TrainLoop's evaluation_images)
against tests/contour_ref.py and the reference's recorded results (tests/golden/contour.npz)."""
import contextlib
import random

import matplotlib
import numpy as np
import PIL.Image
import pytest
import torch
from torch import nn

import contour_ref
from segmentation_pipeline_amd import ops
from segmentation_pipeline_amd.evaluators import (ContourImageEvaluator, FindInterestingSlice, LabelMap, ScalarImage,
                                                  SegmentationEvaluator, find_interesting_slices)
from segmentation_pipeline_amd.prediction import StandardPredict
from segmentation_pipeline_amd.trainer import ScheduledEvaluation, TrainLoop
from test_contour_cpu import fx, golden_calls, golden_cases, golden_subjects  # noqa: F401
from test_evaluation_cpu import _msseg2_chain

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MAP_DTYPES = [torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.float32]
# smaller than one vector; rows that are no multiple of the vector; several rows per lane; a row longer than a tile's
# share of a wave; more than one tile of 4096 voxels, the block's tiles ending inside a row
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 33, 65), (5, 3, 257), (17, 16, 16)]


def _label_map(g, shape, dtype, density=0.3):
    fg = torch.rand(shape, generator=g) < density
    if dtype == torch.bool:
        return fg
    vals = torch.randint(1, 4, shape, generator=g) * fg
    if dtype == torch.float32:
        v = vals.float()
        v[torch.rand(shape, generator=g) < 0.05] = 0.5            # foreground: != 0
        v[torch.rand(shape, generator=g) < 0.03] = float("nan")   # foreground: a NaN is not 0
        return v
    if dtype != torch.uint8:
        vals = vals * (1 - 2 * (torch.rand(shape, generator=g) < 0.3).long())   # negative labels too
    return vals.to(dtype)


def _want_counts(maps, one_hot=None):
    one_hot = one_hot or [False] * len(maps)
    return torch.cat([c for m, oh in zip(maps, one_hot)
                      for c in contour_ref.slice_counts(contour_ref.foreground(m if oh else m[None], oh))])


@pytest.mark.parametrize("dtype", MAP_DTYPES)
def test_slice_counts_label_maps(dtype):
    g = torch.Generator().manual_seed(MAP_DTYPES.index(dtype))
    maps = [_label_map(g, s, dtype) for s in SHAPES]
    maps.append(torch.zeros((4, 9, 21), dtype=dtype))                        # all background
    maps.append(torch.ones((4, 9, 21)).to(dtype))                            # all foreground
    maps.append(_label_map(g, (3, 4, 5), dtype, density=1.0))                # D below the vector width, dense
    maps.append(_label_map(g, (3, 50, 449), dtype, density=0.1))             # two blocks: the first ends inside a row
    counts, layout = ops.slice_counts([m.to(DEV) for m in maps])
    assert counts.dtype == torch.int32
    assert [size3 for _, size3 in layout] == [tuple(m.shape) for m in maps]
    assert torch.equal(counts.cpu().long(), _want_counts(maps))


def test_slice_counts_unaligned_view():
    g = torch.Generator().manual_seed(3)
    base = _label_map(g, (7 * 9 * 11 + 3,), torch.uint8).to(DEV)
    m = base[3:].view(7, 9, 11)          # contiguous, 3 bytes off the 16-byte alignment: the scalar loads
    counts, _ = ops.slice_counts([m])
    assert torch.equal(counts.cpu().long(), _want_counts([m.cpu()]))


@pytest.mark.parametrize("sdtype", [torch.float32, torch.bfloat16, torch.float16])
def test_slice_counts_one_hot(sdtype):
    g = torch.Generator().manual_seed(11)
    maps = []
    for C, shape in [(1, (3, 5, 7)), (2, (2, 33, 65)), (3, (5, 3, 257)), (3, (4, 4, 8)), (2, (3, 5, 7))]:
        s = torch.randint(0, 3, (C,) + shape, generator=g).float()            # many ties: the first maximum wins
        s[0][torch.rand(shape, generator=g) < 0.05] = float("nan")            # a NaN in channel 0: background
        if C > 1:
            s[C - 1][torch.rand(shape, generator=g) < 0.05] = float("nan")    # ... in a later channel: foreground
        maps.append(s.to(sdtype))
    # a label map among them: both kinds in one launch
    maps.append(_label_map(g, (3, 5, 7), torch.int64))
    one_hot = [True] * 5 + [False]
    counts, _ = ops.slice_counts([m.to(DEV) for m in maps], one_hot)
    want = _want_counts(maps, one_hot)
    assert torch.equal(counts.cpu().long(), want)
    assert want[:3 + 5 + 7].sum() == 0                                       # one channel: argmax is 0 everywhere


def test_slice_rank_orders_by_count_then_slice_id():
    g = torch.Generator().manual_seed(5)
    lens = [1, 7, 64, 257, 300, 5]
    tables = [torch.randint(0, 6, (n,), generator=g) for n in lens]          # few distinct counts: long ties
    tables[5][:] = 0                                                          # nothing to rank
    tables[2] = torch.randperm(64, generator=g) + 1                          # all distinct
    counts = torch.cat(tables).to(torch.int32).to(DEV)
    segments, off = [], 0
    for n in lens:
        segments.append((off, n))
        off += n
    ids, ranked, nums = (t.cpu() for t in ops.slice_rank(counts, segments))
    for (off, n), table, num in zip(segments, tables, nums.tolist()):
        want_ids, want_counts = contour_ref.rank(table)
        assert num == len(want_ids)
        got_ids, got_counts = ids[off:off + num].tolist(), ranked[off:off + num].tolist()
        assert got_counts == want_counts                                      # the count sequences are equal
        for c in set(want_counts):
            run = [i for i, v in zip(got_ids, got_counts) if v == c]
            assert run == sorted(run) and set(run) == {i for i, v in zip(want_ids, want_counts) if v == c}
        assert got_ids == want_ids
        assert (ids[off + num:off + n] == -1).all() and (ranked[off + num:off + n] == 0).all()


# ------------------------------------------------------------------------------------------------ mosaics
VOL = (5, 7, 9)


def _volumes(dtype, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype.is_floating_point:
        return [torch.randn(VOL, generator=g).to(dtype) for _ in range(n)]
    if dtype == torch.bool:
        return [torch.rand(VOL, generator=g) < 0.5 for _ in range(n)]
    return [torch.randint(0, 100, VOL, generator=g).to(dtype) for _ in range(n)]


def _ref_mosaic(vols, plane, ks, ncol, pad, dtype):
    shape = contour_ref.slice_shape(VOL, plane)
    tiles = [np.zeros(shape, dtype) if v is None else contour_ref.slice_volume(contour_ref.to_numpy(v), plane, k)
             for v, k in zip(vols, ks)]
    return contour_ref.make_grid(tiles, ncol, pad)


@pytest.mark.parametrize("plane", contour_ref.PLANES)
@pytest.mark.parametrize("n,ncol", [(1, 1), (5, 2), (3, 7)])
def test_mosaic_planes_and_grids(plane, n, ncol):
    dim = VOL[contour_ref.PLANES.index(plane)]
    img = _volumes(torch.float32, n, 1)
    lab = _volumes(torch.int64, n, 2)
    ks = [0, dim - 1, 2, 0, dim - 1][:n]                                     # first and last slice
    if n > 1:
        img[1] = None                                                         # a subject without the image: zeros
    shape = contour_ref.slice_shape(VOL, plane)
    outs, buf = ops.slice_mosaic([
        ([(None if v is None else v.to(DEV), plane, k) for v, k in zip(img, ks)], ncol, -1, shape),
        ([(v.to(DEV), plane, k) for v, k in zip(lab, ks)], ncol, 0, shape)])
    want_img, want_lab = _ref_mosaic(img, plane, ks, ncol, -1, np.float32), _ref_mosaic(lab, plane, ks, ncol, 0, np.int64)
    assert outs[0].dtype == torch.float32 and outs[1].dtype == torch.int64
    np.testing.assert_array_equal(outs[0].cpu().numpy(), want_img)           # pad cells included, bit for bit
    np.testing.assert_array_equal(outs[1].cpu().numpy(), want_lab)
    if n == 1:
        assert tuple(outs[0].shape) == shape                                  # the bare tile


@pytest.mark.parametrize("dtype", MAP_DTYPES + [torch.bfloat16, torch.float16])
def test_mosaic_element_types(dtype):
    vols = _volumes(dtype, 3, 7)
    pad = -1 if dtype.is_floating_point else 1      # (a pad every element type holds)
    outs, _ = ops.slice_mosaic([([(v.to(DEV), "Coronal", 3) for v in vols], 2, 0, None),
                                ([(v.to(DEV), "Saggital", 4) for v in vols], 3, pad, None),
                                ([(v.to(DEV), "Axial", 8) for v in vols], 1, 0, None)])
    want_dtype = torch.float32 if dtype in (torch.bfloat16, torch.float16) else dtype
    for out, (plane, k, ncol, pad) in zip(outs, [("Coronal", 3, 2, 0), ("Saggital", 4, 3, pad), ("Axial", 8, 1, 0)]):
        assert out.dtype == want_dtype
        np.testing.assert_array_equal(out.cpu().numpy(), _ref_mosaic(vols, plane, [k] * 3, ncol, pad, None))


# ------------------------------------------------------------------------------------------------ interesting slices
def test_find_interesting_slices_stores_the_reference_keys():
    g = torch.Generator().manual_seed(9)
    a = LabelMap(_label_map(g, (1, 6, 7, 9), torch.int64).to(DEV), {"a": 1})
    b = LabelMap(torch.randn(3, 4, 5, 6, generator=g).to(DEV), {"a": 1}, one_hot=True)
    c = LabelMap(torch.zeros(1, 3, 3, 3, dtype=torch.uint8), {"a": 1})        # a host volume, empty
    find_interesting_slices([a, b])
    assert FindInterestingSlice()(c) is c
    for image in (a, b, c):
        want_ids, want_counts = contour_ref.interesting(image.data, bool(image.get("one_hot", False)))
        assert list(image["interesting_slice_ids"]) == ["Saggital", "Coronal", "Axial"]
        for plane in contour_ref.PLANES:
            ids, counts = image["interesting_slice_ids"][plane], image["interesting_slice_counts"][plane]
            assert ids.is_cuda and ids.shape[0] == len(want_ids[plane])
            assert ids.tolist() == want_ids[plane] and counts.tolist() == want_counts[plane]
    subject = {"name": "s", "y": LabelMap(a.data, {"a": 1}), "img": ScalarImage(torch.zeros(1, 6, 7, 9))}
    FindInterestingSlice()(subject)
    assert "interesting_slice_ids" in subject["y"] and "interesting_slice_ids" not in subject["img"]


# ------------------------------------------------------------------------------------------------ golden
def _evaluator(case, **kw):
    return ContourImageEvaluator(case["plane"], "img", "y_pred", "y", case["slice_id"], False, case["ncol"],
                                 interesting_slice=case.get("interesting_slice", False),
                                 split_subjects=case.get("split_subjects", False), **kw)


@contextlib.contextmanager
def _traffic(monkeypatch):
    """counts the launches of the three ops and every copy of a device tensor to the host while the block runs"""
    seen = {"slice_counts": 0, "slice_rank": 0, "slice_mosaic": 0, "to_host": 0}
    with monkeypatch.context() as m:
        for name in ("slice_counts", "slice_rank", "slice_mosaic"):
            def counted(*args, _fn=getattr(ops, name), _name=name, **kwargs):
                seen[_name] += 1
                return _fn(*args, **kwargs)
            m.setattr(ops, name, counted)
        for name in ("cpu", "item", "tolist", "numpy"):
            def copied(self, *args, _fn=getattr(torch.Tensor, name), **kwargs):
                seen["to_host"] += bool(self.is_cuda)
                return _fn(self, *args, **kwargs)
            m.setattr(torch.Tensor, name, copied)
        to = torch.Tensor.to

        def moved(self, *args, **kwargs):
            out = to(self, *args, **kwargs)
            seen["to_host"] += bool(self.is_cuda and not out.is_cuda)
            return out
        m.setattr(torch.Tensor, "to", moved)
        yield seen


@pytest.mark.parametrize("on_device", [True, False])
def test_contour_image_evaluator_golden(fx, monkeypatch, on_device):  # noqa: F811
    cases = golden_cases(fx)
    assert {"fixed_axial", "fixed_coronal", "interesting_split", "random_interesting", "target_only",
            "prediction_only", "past_the_end"} <= set(cases)
    for key, case in cases.items():
        subjects = golden_subjects(fx, case, DEV if on_device else None)
        ev = _evaluator(case)
        seen = []
        mosaics = ev._mosaics

        def spy(subjects, resolved, names, impute_shape):
            arrays = mosaics(subjects, resolved, names, impute_shape)
            seen.append((resolved, dict(zip([n for n, _ in names], arrays))))
            return arrays
        monkeypatch.setattr(ev, "_mosaics", spy)
        if "seed" in case:
            random.seed(case["seed"])
        with _traffic(monkeypatch) as traffic:
            result = ev(subjects)
        calls = golden_calls(fx, key, case, subjects)
        assert len(seen) == len(calls), key
        # per get_image call: all its subjects share one count and one rank launch (none without interesting_slice) and
        # one mosaic launch; the chosen ranks come back in one copy, the mosaics in another, and nothing else does
        ranked = 1 if case.get("interesting_slice") else 0
        assert traffic == {"slice_counts": ranked * len(calls), "slice_rank": ranked * len(calls),
                           "slice_mosaic": len(calls), "to_host": (ranked + 1) * len(calls)}, (key, traffic)
        if case.get("split_subjects"):
            assert list(result) == [s["name"] for s in subjects] and all(isinstance(v, PIL.Image.Image) for v in result.values())
        else:
            assert isinstance(result, PIL.Image.Image)
        for (resolved, got), (group, plane, slice_ids, want) in zip(seen, calls):
            assert [p for _, p in resolved] == [plane] * len(group), key
            assert [int(k) for k, _ in resolved] == slice_ids, key
            assert set(got) == set(want), key
            for name in want:
                assert got[name].numpy().dtype == want[name].dtype, (key, name)
                np.testing.assert_array_equal(got[name].numpy(), want[name], err_msg=f"{key} {name}")


# ------------------------------------------------------------------------------------------------ rendering
def _same_picture(a, b):
    return a.size == b.size and a.mode == b.mode and np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("key,legend", [("fixed_axial", True), ("interesting_split", False), ("target_only", False),
                                        ("prediction_only", True)])
def test_rendered_picture_equals_the_cpu_rendering(fx, key, legend):  # noqa: F811
    case = golden_cases(fx)[key]
    subjects = golden_subjects(fx, case, DEV)
    result = _evaluator(case, scale=0.2, line_width=1.0)
    result.legend = legend
    got = result(subjects)
    host = golden_subjects(fx, case)
    groups = [[s] for s in host] if case.get("split_subjects") else [host]
    pictures = list(got.values()) if case.get("split_subjects") else [got]
    for group, picture in zip(groups, pictures):
        _, img, y, y_pred, lv = contour_ref.mosaics(group, case["plane"], "img", "y_pred", "y", case["slice_id"],
                                                    case["ncol"], case.get("interesting_slice", False))
        want = contour_ref.render(img, y, y_pred, lv, scale=0.2, line_width=1.0, legend=legend)
        assert _same_picture(picture, want), key
    assert _same_picture(contour_ref.render(img, y, y_pred, lv, 0.2, 1.0, legend), want)   # a render repeats itself


# ------------------------------------------------------------------------------------------------ training loop
def _run_loop(evaluation_images):
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(2)
    sh = (8, 8, 8)
    lab = torch.randint(0, 3, (4,) + sh, generator=g)
    lab[:, :, :4] = 0
    x = torch.randn(4, 3, *sh, generator=g) + nn.functional.one_hot(lab, 3).permute(0, 4, 1, 2, 3).float() * 2
    y = nn.functional.one_hot((lab > 0).long(), 2).permute(0, 4, 1, 2, 3).float()
    model = nn.Sequential(nn.Conv3d(3, 2, 1), nn.Softmax(dim=1)).to(DEV)
    opt = torch.optim.SGD(model.parameters(), lr=0.5)

    def criterion(p, t):
        return {"loss": -(t * torch.log(p + 1e-6)).mean()}
    batches = [{"X": x[:2].to(DEV), "y": y[:2].to(DEV), "name": ["t0", "t1"]}] * 2
    val = {"cohort": [{"name": f"v{i}", "X": x[2 + i].to(DEV), "y": y[2 + i].to(DEV)} for i in range(2)]}
    training = [ScheduledEvaluation(SegmentationEvaluator("y_pred_eval", "y_eval"), "training_segmentation_eval")]
    validation = [ScheduledEvaluation(SegmentationEvaluator("y_pred_eval", "y_eval"), "segmentation_eval", cohorts=["cohort"])]
    if evaluation_images:
        training.append(ScheduledEvaluation(ContourImageEvaluator(
            "random", "img", "y_pred_eval", "y_eval", 0, legend=False, ncol=2, interesting_slice=True), "training_image"))
        validation.append(ScheduledEvaluation(ContourImageEvaluator(
            "interesting", "img", "y_pred_eval", "y_eval", 0, legend=True, ncol=1, interesting_slice=True,
            split_subjects=True), "validation_image", subjects=["v0", "v1"]))
    logs = []
    random.seed(4)
    TrainLoop().run(model, criterion, opt, StandardPredict(), iter(batches), DEV, 2, log_fn=logs.append,
                    training_evaluators=training, validation_evaluators=validation, validation_subjects=val,
                    label_transform=_msseg2_chain(), label_values={"lesion": 1}, evaluation_images=evaluation_images)
    return logs


def test_train_loop_logs_contour_images_and_the_same_scores():
    plain, with_images = _run_loop(None), _run_loop({"img": ("X", 0)})
    assert len(plain) == len(with_images) == 2
    for a, b in zip(plain, with_images):
        assert "training_image" not in a and "validation_image" not in a
        assert isinstance(b["training_image"], PIL.Image.Image)
        assert list(b["validation_image"]) == ["v0", "v1"]
        assert all(isinstance(v, PIL.Image.Image) for v in b["validation_image"].values())
        assert torch.equal(a["loss"], b["loss"])
        for name, pick in (("training_segmentation_eval", lambda r: r), ("segmentation_eval", lambda r: r["cohort"])):
            ta, tb = pick(a[name]), pick(b[name])
            assert ta["subject_stats"].equals(tb["subject_stats"])
            assert torch.equal(ta["summary_stats"].data, tb["summary_stats"].data)
