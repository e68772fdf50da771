"""Device preprocessing (segmentation_pipeline_amd.preprocessing, csrc/preprocess.hip) against the float64 numpy
restatement in tests/preprocess_ref.py, transform by transform and as the production chains of both configs."""
import numpy as np
import pytest
import torch

import augment_ref as AR
import preprocess_ref as R
from segmentation_pipeline_amd import augmentation as A
from segmentation_pipeline_amd import preprocessing as P
from segmentation_pipeline_amd._lib import M355Error
from test_augmentation_gpu import msseg2_chain, replay, dmri_chain, _boundary, _edge

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LABEL_DTYPES = [torch.uint8, torch.bool, torch.int32, torch.int64, torch.float32]
_CPU = torch.Tensor.cpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def _np_dtype(dtype):
    return torch.empty(0, dtype=dtype).numpy().dtype


def _labels(shape, dtype, seed, hi=5):
    x = np.random.default_rng(seed).integers(0, hi, shape)
    return x.astype(_np_dtype(dtype)) if dtype != torch.bool else (x > 2)


def _run(t, subject, labels=(), **kw):
    before = {k: v.clone() for k, v in subject.items()}
    out = t(subject, label_maps=labels, **kw)
    for k in subject:
        assert torch.allclose(subject[k], before[k], rtol=0, atol=0, equal_nan=True), f"{k} was modified"
    return out


# ------------------------------------------------------------------------------------------------ crop / pad
@pytest.mark.parametrize("dtype", LABEL_DTYPES)
@pytest.mark.parametrize("mode", [0, 3, "minimum"])
def test_crop_pad_and_centred_crop_or_pad_exact(dtype, mode):
    x = _labels((2, 9, 6, 5), dtype, 1, hi=7)
    if dtype == torch.float32:
        x = x * np.float32(1.37) - np.float32(4.0)
    lab = () if dtype == torch.float32 else ("x",)
    s = {"x": dev(x)}
    y = _run(P.Pad((2, 1, 0, 3, 1, 2), padding_mode=mode), s, lab)["x"]
    want = R.pad(x, (2, 1, 0, 3, 1, 2), mode)
    assert y.dtype == s["x"].dtype and np.array_equal(host(y), want)
    y = _run(P.Crop((1, 2, 0, 1, 2, 0)), s, lab)["x"]
    assert np.array_equal(host(y), R.crop(x, (1, 2, 0, 1, 2, 0)))
    # mixed crop and pad per axis: 9 -> 4 (crop), 6 -> 9 (pad), 5 -> 5
    t = P.CropOrPad((4, 9, 5), padding_mode=mode)
    y = _run(t, s, lab)["x"]
    pad, crop = R.crop_or_pad_bounds(x.shape[1:], (4, 9, 5))
    assert np.array_equal(host(y), R.crop_or_pad(x, pad, crop, mode))
    # a crop folded into a later pad: one pass
    y = _run(A.Compose([P.Crop((1, 2, 0, 1, 2, 0)), P.Pad(2, padding_mode=0)]), s, lab)["x"]
    assert np.array_equal(host(y), R.pad(R.crop(x, (1, 2, 0, 1, 2, 0)), (2,) * 6, 0))


FACES = [((0, 2, 2), (3, 4, 4)), ((5, 2, 2), (9, 4, 4)), ((2, 0, 1), (4, 2, 3)), ((2, 4, 1), (4, 6, 3)),
         ((2, 2, 0), (4, 4, 1)), ((2, 2, 3), (4, 4, 5)), ((0, 0, 0), (9, 6, 5)), ((4, 3, 2), (5, 4, 3))]


@pytest.mark.parametrize("box", FACES + [None])
@pytest.mark.parametrize("target", [(4, 9, 5), (7, 4, 8), (9, 6, 5)])
def test_mask_centred_crop_or_pad(box, target):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((1, 9, 6, 5)).astype(np.float32)
    m = np.zeros((1, 9, 6, 5), np.uint8)
    if box is not None:
        m[0, box[0][0]:box[1][0], box[0][1]:box[1][1], box[0][2]:box[1][2]] = 1
    s = {"x": dev(x), "m": dev(m)}
    t = P.CropOrPad(target, padding_mode="minimum", mask_name="m")
    out = _run(t, s, ("m",))
    pad, crop = R.crop_or_pad_bounds(x.shape[1:], target, m[0])
    want_off = [crop[2 * a] - pad[2 * a] for a in range(3)]
    assert host(t.last_history["offsets"]).tolist() == want_off
    assert np.array_equal(host(out["x"]), R.crop_or_pad(x, pad, crop, "minimum"))
    assert np.array_equal(host(out["m"]), R.crop_or_pad(m, pad, crop, "minimum"))


def test_crop_to_mask_and_min_size_pad():
    m = np.zeros((1, 12, 10, 9), np.int32)
    m[0, 3:8, 0:10, 2:4] = 2
    m[0, 5, 5, 5] = 1
    x = np.random.default_rng(3).standard_normal((1, 12, 10, 9)).astype(np.float32)
    s = {"x": dev(x), "m": dev(m)}
    t = A.Compose([P.CropToMask("m", label_id=2), P.MinSizePad(6)])
    out = _run(t, s, ("m",))
    c = R.crop_to_mask_bounds(m, 2)
    q = R.min_size_padding(R.crop(x, c).shape[1:], (6, 6, 6))
    assert np.array_equal(host(out["x"]), R.pad(R.crop(x, c), q, 0))
    assert np.array_equal(host(out["m"]), R.pad(R.crop(m, c), q, 0))
    with pytest.raises(M355Error, match="no voxel"):
        P.CropToMask("m", label_id=7)(s, label_maps=("m",))


# ------------------------------------------------------------------------------------------------ fused per-voxel
@pytest.mark.parametrize("dtype", LABEL_DTYPES)
@pytest.mark.parametrize("method", [None, "Right", "left", "Anterior", "Posterior", "Superior", "Inferior", "roi"])
def test_remap_is_simultaneous_and_masked(dtype, method):
    shape = (1, 7, 5, 3)        # odd sizes: 'Right' is [:, W // 2:]
    x = _labels(shape, dtype, 4)
    roi = (np.random.default_rng(5).random(shape) > 0.5).astype(np.uint8)
    mapping = {1: 2, 2: 3, 3: 1} if dtype != torch.bool else {1: 0}
    s = {"x": dev(x), "roi": dev(roi)}
    out = _run(P.CustomRemapLabels(mapping, masking_method=method), s, ("x", "roi"))
    mask = None if method is None else (roi != 0) if method == "roi" else R.anatomical_mask(method.title(), shape)
    assert np.array_equal(host(out["x"]), R.remap(x, mapping, mask))


def test_nan_crop_or_pad_remap_cast_fuse_into_one_pass():
    rng = np.random.default_rng(6)
    img = rng.standard_normal((2, 11, 9, 7)).astype(np.float32)
    img[0, 3, 4, 5] = img[1, 0, 0, 0] = img[1, 10, 8, 6] = np.nan
    lab = rng.integers(0, 4, (1, 11, 9, 7)).astype(np.int64)
    roi = np.zeros((1, 11, 9, 7), np.uint8)
    roi[0, 2:9, 1:6, 3:7] = 1
    s = {"img": dev(img), "lab": dev(lab), "roi": dev(roi)}
    chain = A.Compose([P.ReplaceNan(-5), P.CropOrPad((8, 12, 6), padding_mode="minimum", mask_name="roi"),
                       P.CustomRemapLabels({2: 1, 1: 2}, masking_method="Right", include=["lab"]),
                       P.SetDataType(torch.int32, intensity_only=False, include=["lab"]),
                       P.SetDataType(torch.float32, intensity_only=False, include=["roi"])])
    calls = []
    import segmentation_pipeline_amd._lib as L
    lib = L.lib()

    class Count:
        def __getattr__(self, k):
            f = getattr(lib, k)
            return (lambda *a: (calls.append(k), f(*a))[1]) if k.startswith("m355_pre_gather") else f
    P._lib.lib, orig = (lambda: Count()), P._lib.lib
    try:
        out = _run(chain, s, ("lab", "roi"))
    finally:
        P._lib.lib = orig
    assert len(calls) == 3          # one pass per tensor
    pad, crop = R.crop_or_pad_bounds(img.shape[1:], (8, 12, 6), roi[0])
    want = R.crop_or_pad(R.replace_nan(img, -5), pad, crop, "minimum")
    assert np.array_equal(host(out["img"]), want)
    wl = R.crop_or_pad(lab, pad, crop, "minimum")
    wl = R.remap(wl, {2: 1, 1: 2}, R.anatomical_mask("Right", wl.shape)).astype(np.int32)
    assert out["lab"].dtype == torch.int32 and np.array_equal(host(out["lab"]), wl)
    assert out["roi"].dtype == torch.float32
    assert np.array_equal(host(out["roi"]), R.crop_or_pad(roi, pad, crop, "minimum").astype(np.float32))


@pytest.mark.parametrize("dtype", LABEL_DTYPES)
def test_one_hot_and_out_of_range_report(dtype):
    x = _labels((1, 7, 6, 5), dtype, 7, hi=3)
    t = P.CustomOneHot(include=["y"])
    out = _run(t, {"y": dev(x)}, ("y",), label_values={"y": {"a": 1, "b": 2}})
    assert out["y"].dtype == dev(x).dtype and np.array_equal(host(out["y"]), R.one_hot(x, 3))
    assert int(t.last_history["y"]["out_of_range"].item()) == 0 and t.last_meta["one_hot"] == ["y"]
    if dtype == torch.bool:
        return
    bad = x.copy()
    bad[0, 0, 0, 0], bad[0, 6, 5, 4] = 5, 3
    if dtype != torch.uint8:
        bad[0, 1, 1, 1] = -1
    t = P.CustomOneHot(3)
    out = _run(t, {"y": dev(bad)}, ("y",))
    n = 2 if dtype == torch.uint8 else 3
    assert int(t.last_history["y"]["out_of_range"].item()) == n
    y = host(out["y"])
    assert (y[:, 0, 0, 0] == 0).all() and (y[:, 6, 5, 4] == 0).all()


def test_image_from_labels_rename_and_concatenate():
    rng = np.random.default_rng(8)
    brain = (rng.random((1, 9, 8, 7)) > 0.3).astype(np.uint8)
    les = rng.integers(0, 2, (1, 9, 8, 7)).astype(np.float32)
    a, b = (rng.standard_normal((1, 9, 8, 7)).astype(np.float32) for _ in range(2))
    s = {"a": dev(a), "b": dev(b), "brain_mask": dev(brain), "ground_truth": dev(les)}
    lv = {"brain_mask": {"brain": 1}, "ground_truth": {"lesion": 1}}
    chain = A.Compose([P.ConcatenateImages(["a", "b"], [1, 1], "X"), P.RenameProperty("ground_truth", "y"),
                       P.CustomOneHot(include="y"),
                       P.ImageFromLabels("p", [("brain_mask", "brain", 1), ("y", "lesion", 100), ("nope", 1, 3)]),
                       P.ImageFromLabels("q", [("brain_mask", 1, 2.5), ("y", 1, 0.25)], mode="additive")])
    out = _run(chain, s, ("brain_mask", "ground_truth"), label_values=lv)
    assert set(out) == {"a", "b", "brain_mask", "y", "X", "p", "q"}
    assert np.array_equal(host(out["X"]), np.concatenate([a, b]))
    oh = R.one_hot(les, 2)
    assert np.array_equal(host(out["y"]), oh)
    assert chain.last_meta["label_maps"] == ["brain_mask", "y"] and chain.last_meta["one_hot"] == ["y"]
    assert chain.last_meta["label_values"] == {"brain_mask": {"brain": 1}, "y": {"lesion": 1}}
    want = R.image_from_labels([(brain, 1, 1, False), (oh, 1, 100, True)], brain.shape[1:])
    assert out["p"].dtype == torch.float32 and np.array_equal(host(out["p"]), want)
    want = R.image_from_labels([(brain, 1, 2.5, False), (oh, 1, 0.25, True)], brain.shape[1:], "additive")
    assert np.array_equal(host(out["q"]), want)


# ------------------------------------------------------------------------------------------------ resampling
@pytest.mark.parametrize("spacing", [(0.8, 1.0, 1.5), (1.125, 1.0, 0.95)])
def test_target_resample(spacing):
    rng = np.random.default_rng(9)
    shape = (23, 17, 12)
    img = (rng.standard_normal((1,) + shape)).astype(np.float32)
    lab = rng.integers(0, 4, (1,) + shape).astype(np.int32)
    t = P.TargetResample(1, 0.11)
    out = _run(t, {"img": dev(img), "lab": dev(lab)}, ("lab",), spacing=spacing)
    new = R.target_spacing(spacing, (1, 1, 1), (0.11,) * 3)
    assert t.last_meta["spacing"] == pytest.approx(new)
    want, q = R.resample(img, spacing, new, "linear")
    assert out["img"].shape[1:] == want.shape[1:]
    assert np.abs(host(out["img"]) - want).max() <= 1e-4
    wl, _ = R.resample(lab, spacing, new, "nearest")
    ok = ~_boundary(q, shape)        # a coordinate within 1e-4 of a rounding tie may round either way in fp32
    assert ok.mean() > 0.4 and np.array_equal(host(out["lab"])[:, ok], wl[:, ok])
    same = _run(P.TargetResample(1, 0.11), {"img": dev(img)}, spacing=(1.05, 0.95, 1.0))
    assert np.array_equal(host(same["img"]), img)


# ------------------------------------------------------------------------------------------------ production chains
def dmri_common_1():
    return A.Compose([
        P.ReplaceNan(),
        P.CropOrPad((96, 88, 24), padding_mode="minimum", mask_name="whole_roi_union"),
        P.CustomRemapLabels(remapping=[("right_whole", 2, 1)], masking_method="Right", include=["whole_roi"]),
        P.CustomRemapLabels(remapping=[("right_head", 4, 1), ("right_body", 5, 2), ("right_tail", 6, 3)],
                            masking_method="Right", include=["hbt_roi"])])


def dmri_common_2():
    return A.Compose([
        A.RescaleIntensity((-1., 1.), (0.5, 99.5)),
        P.ConcatenateImages(image_names=["mean_dwi", "md", "fa"], image_channels=[1, 1, 1], new_image_name="X"),
        P.RenameProperty(old_name="whole_roi", new_name="y"),
        P.CustomOneHot(include=["y"])])


def msseg2_common_1(patch=48):
    return A.Compose([P.SetDataType(torch.float), P.EnforceConsistentAffine(source_image_name="flair_time01"),
                      P.TargetResample(target_spacing=1, tolerance=0.11), P.CropToMask("brain_mask"),
                      P.MinSizePad(patch)])


def msseg2_common_2():
    return A.Compose([
        A.RescaleIntensity((-1, 1.), (0.05, 99.5)),
        P.ConcatenateImages(image_names=["flair_time01", "flair_time02"], image_channels=[1, 1], new_image_name="X"),
        P.RenameProperty(old_name="ground_truth", new_name="y"),
        P.CustomOneHot(include="y")])


def chain_of(kind, training):
    if kind == "dmri":
        parts = [dmri_common_1()] + ([dmri_chain()] if training else []) + [dmri_common_2()]
    else:
        parts = [msseg2_common_1()] + ([msseg2_chain()] if training else []) + [msseg2_common_2()]
        if training:
            parts.append(P.ImageFromLabels(new_image_name="patch_probability",
                                           label_weights=[("brain_mask", "brain", 1), ("y", "lesion", 100)]))
    return A.Compose(parts)


def subject(kind):
    rng = np.random.default_rng(11 if kind == "dmri" else 12)
    if kind == "dmri":
        shape = (101, 93, 19)          # crops axes 0 and 1 to (96, 88), pads axis 2 to 24
        base = np.stack([np.cumsum(rng.standard_normal(shape), axis=a) for a in range(3)])
        imgs = {n: (base[i:i + 1] / 20 + 2.0 + i).astype(np.float32) for i, n in enumerate(["mean_dwi", "md", "fa"])}
        imgs["md"][0, 50, 40, 10] = np.nan
        roi = np.zeros((1,) + shape, np.int64)
        roi[0, 30:60, 20:44, 4:16] = 1
        roi[0, 30:60, 44:70, 4:16] = 2
        union = (roi > 0).astype(np.uint8)
        labs = {"whole_roi": roi, "whole_roi_union": union}
        return imgs, labs, (1.0, 1.0, 1.0), {"whole_roi": {"left_whole": 1, "right_whole": 2}}
    shape = (72, 60, 40)               # spacing (0.8, 1, 1.5): resampled to (54, 60, 60) at (16 / 15, 1, 1) mm
    base = np.stack([np.cumsum(rng.standard_normal(shape), axis=a) for a in range(2)])
    imgs = {"flair_time01": (base[0:1] / 20 + 1.0).astype(np.float32),
            "flair_time02": (base[1:2] * 3).astype(np.int32)}
    brain = np.zeros((1,) + shape, np.uint8)
    brain[0, 8:60, 5:55, 6:36] = 1     # edges away from the nearest-neighbour ties of both resampled axes
    les = np.zeros((1,) + shape, np.uint8)
    les[0, 20:32, 20:30, 12:20] = 1
    return imgs, {"brain_mask": brain, "ground_truth": les}, (0.8, 1.0, 1.5), \
        {"brain_mask": {"brain": 1}, "ground_truth": {"lesion": 1}}


def reference(kind, hist, imgs, labs, spacing, aug=None):
    """the chain in float64 numpy, replaying the training augmentations from `hist`; returns (outputs, near)"""
    d = {k: v.astype(np.float64) for k, v in imgs.items()}
    d.update({k: v.copy() for k, v in labs.items()})
    near = {}
    if kind == "dmri":
        for k in imgs:
            d[k] = R.replace_nan(d[k])
        pad, crop = R.crop_or_pad_bounds(d["mean_dwi"].shape[1:], (96, 88, 24), labs["whole_roi_union"][0])
        for k in d:
            d[k] = R.crop_or_pad(d[k], pad, crop, "minimum")
        d["whole_roi"] = R.remap(d["whole_roi"], {2: 1}, R.anatomical_mask("Right", d["whole_roi"].shape))
        outm, pct, names, rename, K = (-1., 1.), (0.5, 99.5), ["mean_dwi", "md", "fa"], "whole_roi", 2
    else:
        d = {k: (v.astype(np.float64) if k in imgs else v) for k, v in d.items()}
        new = R.target_spacing(spacing, (1, 1, 1), (0.11,) * 3)
        shape = imgs["flair_time01"].shape[1:]
        for k in d:
            x = d[k]
            d[k], q = R.resample(x, spacing, new, "nearest" if k in labs else "linear")
            if k in labs:   # a tie of nearest rounding matters only where the two neighbours differ
                near[k] = _boundary(q, shape) & np.any(AR.sample(x, q - 1e-3, "nearest") != AR.sample(x, q + 1e-3,
                                                                                                     "nearest"), 0)
            else:
                near[k] = _edge(q, shape)
        spacing = new
        c = R.crop_to_mask_bounds(d["brain_mask"])
        for k in d:
            d[k] = R.crop(d[k], c)
            near[k] = R.crop(near[k][None], c)[0]
        p = R.min_size_padding(d["brain_mask"].shape[1:], (48, 48, 48))
        for k in d:
            d[k] = R.pad(d[k], p, 0)
            near[k] = R.pad(near[k][None], p, 0)[0]
        outm, pct, names, rename, K = (-1., 1.), (0.05, 99.5), ["flair_time01", "flair_time02"], "ground_truth", 2
    for k in d:
        near.setdefault(k, np.zeros(d[k].shape[1:], bool))
    if aug is not None:
        d = replay(aug, hist, d, set(labs), spacing, near)
    for k in names:
        d[k] = AR.rescale(d[k], outm, pct)
    d["X"] = np.concatenate([d[k] for k in names])
    near["X"] = np.logical_or.reduce([near[k] for k in names])
    d["y"], near["y"] = d.pop(rename), near.pop(rename)
    d["y"] = R.one_hot(d["y"], K)
    if kind == "msseg2" and aug is not None:
        d["patch_probability"] = R.image_from_labels([(d["brain_mask"], 1, 1, False), (d["y"], 1, 100, True)],
                                                     d["y"].shape[1:])
        near["patch_probability"] = near["y"] | near["brain_mask"]
    return d, near


@pytest.mark.parametrize("kind", ["dmri", "msseg2"])
@pytest.mark.parametrize("training", [False, True])
def test_production_chains_in_reference_order(kind, training):
    imgs, labs, sp, lv = subject(kind)
    chain = chain_of(kind, training)
    s = {k: dev(v) for k, v in {**imgs, **labs}.items()}
    seeds = (1, 3, 8) if training else (0,)
    for seed in seeds:
        out = _run(chain, s, tuple(labs), spacing=sp, label_values=lv, generator=torch.Generator().manual_seed(seed))
        aug = chain.transforms[1] if training else None
        hist = chain.last_history[1][1] if training else None
        ref, near = reference(kind, hist, imgs, labs, sp, aug)
        assert set(out) == set(ref), (set(out), set(ref))
        tol = 2e-4 if training else 1e-5
        for k, v in ref.items():
            y = host(out[k])
            assert y.shape == v.shape, (k, y.shape, v.shape)
            ok = ~near[k]
            assert ok.mean() > 0.9, k
            if k in labs or k in ("y",):
                assert np.array_equal(y[:, ok], v[:, ok]), (seed, k)
            else:
                err = np.abs(y.astype(np.float64) - v)[:, ok]
                assert err.max(initial=0) <= tol * max(1.0, np.abs(v).max()), (seed, k, err.max())
        assert chain.last_meta["one_hot"] == ["y"]
        if kind == "msseg2":
            assert chain.last_meta["spacing"] == pytest.approx(R.target_spacing(sp, (1, 1, 1), (0.11,) * 3))


def _no_sync(monkeypatch, fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            torch.zeros(1, device=DEV).item()
        except RuntimeError:
            honoured = True
        if not honoured:
            def guard(orig):
                def f(self, *a, **k):
                    if self.is_cuda:
                        raise RuntimeError("host synchronisation")
                    return orig(self, *a, **k)
                return f

            def boom(*a, **k):
                raise RuntimeError("host synchronisation")
            monkeypatch.setattr(torch.cuda, "synchronize", boom)
            for name in ("item", "cpu", "tolist", "numpy", "nonzero"):
                monkeypatch.setattr(torch.Tensor, name, guard(getattr(torch.Tensor, name)))
            monkeypatch.setattr(torch.cuda.Stream, "synchronize", boom)
            monkeypatch.setattr(torch.cuda.Event, "synchronize", boom)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            outs = fn()
    finally:
        torch.cuda.set_sync_debug_mode(0)
        monkeypatch.undo()
    torch.cuda.current_stream().wait_stream(side)
    return outs


@pytest.mark.parametrize("kind", ["dmri", "msseg2"])
def test_chains_synchronise_only_in_crop_to_mask(kind, monkeypatch):
    imgs, labs, sp, lv = subject(kind)
    s = {k: dev(v) for k, v in {**imgs, **labs}.items()}
    chains = [chain_of(kind, False), chain_of(kind, True)]
    run = lambda: [c(s, label_maps=tuple(labs), spacing=sp, label_values=lv, generator=torch.Generator().manual_seed(3))
                   for c in chains]
    refs = run()
    reads = []
    if kind == "msseg2":   # the one allowed read: CropToMask's six bounds, outside the guard
        orig = P.CropToMask._apply

        def allowed(self, state):
            mode = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode(0)
            with monkeypatch.context() as m:
                m.setattr(torch.Tensor, "cpu", _CPU)
                try:
                    reads.append(1)
                    return orig(self, state)
                finally:
                    torch.cuda.set_sync_debug_mode(mode)
        monkeypatch.setattr(P.CropToMask, "_apply", allowed)
    outs = _no_sync(monkeypatch, run)
    assert len(reads) == (2 if kind == "msseg2" else 0)
    for a, b in zip(outs, refs):
        for k in a:
            assert torch.equal(a[k], b[k]), k
