"""Host side of the device preprocessing (segmentation_pipeline_amd.preprocessing): the numpy restatement
against hand-worked cases, the spacing / padding arithmetic, the metadata bookkeeping and argument validation of the
new entry points.  No GPU: nothing here launches a kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

import preprocess_ref as R
from segmentation_pipeline_amd import _lib
from segmentation_pipeline_amd import augmentation as A
from segmentation_pipeline_amd import preprocessing as P
from segmentation_pipeline_amd._lib import M355Error


# ------------------------------------------------------------------------------------------------ restatement
def _mask(shape, lo, hi):
    m = np.zeros(shape, np.uint8)
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    return m


def test_crop_or_pad_bounds_hand_worked():
    # axis 0: box [4, 6) -> centre 5 on an index, target 4 even -> no shift: begin 3, end 7
    # axis 1: box [2, 5) -> centre 3.5, target 4 even -> -0.5: centre 3, begin 1, end 5
    # axis 2: box [0, 1) -> centre 0.5, target 5 odd -> no shift: begin -2 (pad 2), end 3
    pad, crop = R.crop_or_pad_bounds((10, 8, 6), (4, 4, 5), _mask((10, 8, 6), (4, 2, 0), (6, 5, 1)))
    assert pad == (0, 0, 0, 0, 2, 0) and crop == (3, 3, 1, 3, 0, 3)
    # axis 0: box [3, 4) -> centre 3.5, target 3 odd -> no shift: begin 2, end 5; axis 1 box [0, 8) centre 4 target 3
    # odd -> 3.5: begin 2; axis 2 box [5, 6) centre 5.5, target 8 even -> 5: begin 1, end 9 (pad 3)
    pad, crop = R.crop_or_pad_bounds((10, 8, 6), (3, 3, 8), _mask((10, 8, 6), (3, 0, 5), (4, 8, 6)))
    assert pad == (0, 0, 0, 0, 0, 3) and crop == (2, 5, 2, 3, 1, 0)


def test_crop_or_pad_empty_mask_is_centred():
    pad, crop = R.crop_or_pad_bounds((10, 7, 4), (7, 4, 9), np.zeros((10, 7, 4)))
    assert crop == (2, 1, 2, 1, 0, 0) and pad == (0, 0, 0, 0, 3, 2)    # ini = ceil(n / 2), fin = floor(n / 2)
    assert P._centred_offsets((10, 7, 4), (7, 4, 9)) == (2, 2, -3)
    assert P._centred_offsets((5, 5, 5), (5, 6, 4)) == (0, -1, 1)


def test_crop_to_mask_drops_the_last_slice():
    m = _mask((9, 8, 7), (2, 3, 1), (6, 4 + 2, 7))[None]
    c = R.crop_to_mask_bounds(m)
    assert c == (2, 9 - 5, 3, 8 - 5, 1, 7 - 6)
    x = np.arange(9 * 8 * 7).reshape(1, 9, 8, 7)
    y = R.crop(x, c)
    assert y.shape == (1, 3, 2, 5)     # [min, max): the last mask index of each axis is not kept
    assert y[0, 0, 0, 0] == x[0, 2, 3, 1] and y[0, -1, -1, -1] == x[0, 4, 4, 5]


def test_minimum_padding_is_the_minimum_over_the_axes_left():
    """np.pad 'minimum' pads axis by axis, so a voxel outside along the axes A holds the minimum over A of the input,
    the other coordinates fixed: what the device tables hold"""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 5, 4, 3))
    y = R.pad(x, (2, 1, 0, 2, 1, 1), "minimum")
    for c in range(2):
        for o in np.ndindex(*y.shape[1:]):
            i = [o[0] - 2, o[1], o[2] - 1]
            out = [a for a in range(3) if not 0 <= i[a] < x.shape[1 + a]]
            sl = tuple(slice(None) if a in out else i[a] for a in range(3))
            assert y[(c,) + o] == x[c][sl].min()


# ------------------------------------------------------------------------------------------------ spacing
def test_target_spacing_rounds_half_to_even():
    new = P.target_spacing((1.125, 0.8, 1.0), (1.0, 1.0, 1.0), (0.11, 0.11, 0.11))
    assert new == pytest.approx((0.9375, 0.8 * 4 / 3, 1.0), abs=1e-12)
    assert new == R.target_spacing((1.125, 0.8, 1.0), (1, 1, 1), (0.11,) * 3)
    assert P.target_spacing((0.8, 1.0, 1.5), (1, 1, 1), (0.11,) * 3) == pytest.approx((0.8 * 4 / 3, 1.0, 1.0))


def test_target_spacing_noop_inside_tolerance():
    assert P.target_spacing((1.05, 0.95, 1.1), (1, 1, 1), (0.11,) * 3) is None
    assert R.target_spacing((1.05, 0.95, 1.1), (1, 1, 1), (0.11,) * 3) is None
    assert P.target_spacing((1.05, 0.95, 1.2), (1, 1, 1), (0.11,) * 3) is not None


def test_resample_shape():
    assert P.resample_shape((60, 1, 40), (0.8, 2.0, 1.5), (0.8 * 4 / 3, 1.0, 1.0)) == (45, 1, 60)
    assert P.resample_shape((7, 9, 11), (1.0, 1.0, 1.0), (0.9375, 1.0, 2.0)) == (8, 9, 6)


def test_min_size_pad_split():
    assert P.min_size_padding((90, 96, 101), (96, 96, 96)) == (3, 3, 0, 0, 0, 0)
    assert P.min_size_padding((91, 40, 97), (96, 41, 96)) == (2, 3, 0, 1, 0, 0)
    assert P.min_size_padding((91, 40, 97), (96, 41, 96)) == R.min_size_padding((91, 40, 97), (96, 41, 96))
    with pytest.raises(KeyError):
        P.MinSizePad([96, 96, 96])


def test_six_bounds():
    assert P.six_bounds(2) == (2,) * 6
    assert P.six_bounds((1, 2, 3)) == (1, 1, 2, 2, 3, 3)
    with pytest.raises(ValueError):
        P.six_bounds((1, 2))


# ------------------------------------------------------------------------------------------------ metadata
def _state(subject, labels, label_values):
    return A._State(subject, labels, (1.0, 1.0, 1.0), None, label_values)


def test_label_values_follow_remap_and_rename():
    subject = {"img": torch.zeros(1, 4, 5, 6), "whole_roi": torch.zeros(1, 4, 5, 6, dtype=torch.int64)}
    lv = {"whole_roi": {"left_whole": 1, "right_whole": 2}}
    st = _state(subject, ("whole_roi",), lv)
    P.CustomRemapLabels([("right_whole", 2, 1)], masking_method="Right")._run(st)
    assert st.label_values["whole_roi"] == {"left_whole": 1, "right_whole": 1}
    assert lv["whole_roi"]["right_whole"] == 2          # the caller's dict is not changed
    assert "whole_roi" in st.deferred and st.data["whole_roi"] is not subject["whole_roi"]   # deferred, not launched
    P.RenameProperty("whole_roi", "y")._run(st)
    assert "y" in st.labels and "whole_roi" not in st.labels and "whole_roi" not in st.data
    assert st.label_values == {"y": {"left_whole": 1, "right_whole": 1}}
    assert "y" in st.deferred and st.deferred["y"]._name == "y"
    # a dict remapping leaves label_values alone; a map without label_values gets none
    st = _state(subject, ("whole_roi",), lv)
    P.CustomRemapLabels({1: 3})._run(st)
    assert st.label_values == lv
    st = _state(subject, ("whole_roi",), None)
    P.CustomRemapLabels([("right_whole", 2, 1)])._run(st)
    assert st.label_values == {} and st.meta()["label_maps"] == ["whole_roi"]


def test_one_hot_classes_from_label_values(monkeypatch):
    calls = []

    class Fake:
        def m355_pre_one_hot(self, x, dtype, size3, K, y, bad, stream):
            calls.append(K)
            return 0
    monkeypatch.setattr(P._lib, "lib", lambda: Fake())
    monkeypatch.setattr(P, "_stream", lambda: None)
    subject = {"y": torch.zeros(1, 3, 4, 5, dtype=torch.uint8)}
    st = _state(subject, ("y",), {"y": {"left_whole": 1, "right_whole": 1}})
    P.CustomOneHot()._run(st)
    assert calls == [2] and st.data["y"].shape == (2, 3, 4, 5) and st.data["y"].dtype == torch.uint8
    assert st.meta()["one_hot"] == ["y"]
    st = _state(subject, ("y",), None)
    with pytest.raises(M355Error, match="label_values"):
        P.CustomOneHot()._run(st)
    P.CustomOneHot(num_classes=4)._run(st)
    assert calls[-1] == 4 and st.data["y"].shape[0] == 4


def test_image_from_labels_resolves_names():
    t = P.ImageFromLabels("p", [("m", "brain", 1)])
    st = _state({"m": torch.zeros(1, 2, 2, 2, dtype=torch.uint8)}, ("m",), {"m": {"lesion": 1}})
    with pytest.raises(M355Error, match="brain"):
        t._run(st)
    with pytest.raises(ValueError):
        P.ImageFromLabels("p", [], mode="max")


def test_argument_validation_python():
    with pytest.raises(NotImplementedError):
        P.Pad(1, padding_mode="reflect")
    with pytest.raises(NotImplementedError):
        P.CropOrPad(4, padding_mode="edge")
    with pytest.raises(NotImplementedError):
        P.TargetResample(1, 0.11, pre_affine_name="t1")
    with pytest.raises(NotImplementedError):
        P.TargetResample(1, 0.11, scalars_only=True)
    with pytest.raises(ValueError):
        P.TargetResample("mode", 0.11)
    with pytest.raises(ValueError):
        P.CustomRemapLabels([("a", 1)])
    with pytest.raises(ValueError):
        P.CustomRemapLabels({"a": 1})
    with pytest.raises(M355Error):
        P.CustomRemapLabels({k: k + 1 for k in range(9)})
    with pytest.raises(M355Error):
        P.SetDataType(torch.float64)


# ------------------------------------------------------------------------------------------------ the C ABI
def _desc(**kw):
    d = _lib.PreGatherDesc()
    d.x, d.y, d.C = 16, 32, 1
    d.in_dtype = d.out_dtype = _lib.PRE_F32
    for f in ("src3", "in3", "out3"):
        getattr(d, f)[:] = (4, 4, 4)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[:] = v
        else:
            setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,msg", [
    (dict(y=16), b"x == y"),
    (dict(in_dtype=7), b"element type"),
    (dict(nremap=9), b"remap pairs"),
    (dict(pad_mode=1), b"pad mode"),
    (dict(base3=(1, 0, 0)), b"outside"),
    (dict(pad_mode=1, tables=64, in3=(3, 4, 4)), b"minimum"),
    (dict(mask_kind=2, nremap=1, mask_C=3), b"mask map"),
    (dict(mask_kind=1, nremap=1, mask_axis=3), b"half-space"),
    (dict(out3=(0, 4, 4)), b"non-positive"),
])
def test_gather_argument_validation(kw, msg):
    L = _lib.lib()
    d = _desc(**kw)
    assert L.m355_pre_gather(C.byref(d), None) == -1
    assert msg in L.m355_last_error()
    assert L.m355_pre_gather(None, None) == -1


def test_entry_point_argument_validation():
    L = _lib.lib()
    s3 = (C.c_int32 * 3)(4, 5, 6)
    p = C.c_void_p(64)
    assert L.m355_pre_bbox(p, 0, 2, s3, 2, 0, 0.0, p, None) == -1 and b"channel" in L.m355_last_error()
    assert L.m355_pre_bbox(p, 0, 1, s3, 0, 2, 0.0, p, None) == -1 and b"predicate" in L.m355_last_error()
    assert L.m355_pre_bbox(p, 9, 1, s3, 0, 0, 0.0, p, None) == -1
    assert L.m355_pre_crop_or_pad_offsets(None, s3, s3, p, None) == -1
    per = 5 * 6 + 4 * 6 + 4 * 5 + 4 + 5 + 6 + 1
    assert L.m355_pre_min_tables_bytes(3, s3) == 3 * per * 8
    assert L.m355_pre_min_tables_bytes(0, s3) == 0
    assert L.m355_pre_min_tables(p, 4, 1, s3, 0, 0.0, p, per * 8 - 1, None) == -4
    big = (C.c_int32 * 3)(2, 5000, 5000)
    assert L.m355_pre_min_tables(p, 4, 1, big, 0, 0.0, p, 1 << 40, None) == -1 and b"V1 + V2" in L.m355_last_error()
    assert L.m355_pre_one_hot(p, 0, s3, 0, C.c_void_p(128), p, None) == -1 and b"classes" in L.m355_last_error()
    assert L.m355_pre_one_hot(p, 0, s3, 2, p, C.c_void_p(8), None) == -1
    e = (_lib.PreLabelEntry * 9)()
    assert L.m355_pre_image_from_labels(e, 9, s3, 0, p, None) == -1 and b"entries" in L.m355_last_error()
    assert L.m355_pre_image_from_labels(e, 1, s3, 2, p, None) == -1 and b"mode" in L.m355_last_error()
    assert L.m355_pre_image_from_labels(e, 1, s3, 0, p, None) == -1 and b"null map" in L.m355_last_error()
