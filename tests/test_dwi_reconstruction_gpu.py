"""Device mean-DWI reconstruction (augmentation.MeanDWI / ReconstructMeanDWI / ReconstructMeanDWIClassic,
csrc/dwi.hip) against np.mean, alone, in preprocessing chains and in the dmri_hippo augmentation modes."""
import numpy as np
import pytest
import torch

import augment_ref as AR
import preprocess_ref as R
from segmentation_pipeline_amd import augmentation as A
from segmentation_pipeline_amd import preprocessing as P
from segmentation_pipeline_amd._lib import M355Error
from test_preprocessing_gpu import _no_sync, dmri_common_1, dmri_common_2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def dwi(N, shape, seed, nan=False):
    """float32 values over six decades, so that the summation order shows in the last bits"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N,) + tuple(shape)) * 10.0 ** rng.uniform(-3, 3, (N,) + tuple(shape))
    x = x.astype(np.float32)
    if nan:
        x[rng.random(x.shape) < 1e-3] = np.nan
    return x


def grad_table(N, seed, n_b0=4, n_high=4):
    """unit bvecs; the first n_b0 rows b = 0, the last n_high rows b = 1000, the rest b = 500"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((N, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    b = np.full((N, 1), 500.0)
    b[:n_b0] = 0.0
    b[N - n_high:] = 1000.0
    v[:n_b0] = 0.0
    return np.concatenate([v, b], axis=1)


def same(a, b):
    """bit-identical (NaN included)"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def np_mean(x, channels):
    return np.mean(x[np.asarray(channels)], axis=0, keepdims=True)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("N,shape,channels", [
    (5, (7, 5, 3), [2]),                                  # k = 1, voxel count not a multiple of 4
    (100, (7, 5, 3), list(range(0, 100, 3))[:64] * 1),    # k = 34, N = 100
    (100, (7, 5, 3), [7] * 10 + [99, 0, 7, 63] * 13 + [5, 5]),   # k = 64 with duplicates
    (64, (96, 88, 24), [3, 17, 3, 40, 63, 8, 3]),         # dmri_hippo size, k = 7
    (100, (96, 88, 24), [(i * 37) % 100 for i in range(64)]),    # k = 64, N = 100
    (3, (1, 1, 1), [1, 1, 2]),
    (9, (4, 4, 4), list(range(9))),
])
def test_mean_dwi_is_bit_exact_against_np_mean(N, shape, channels):
    x = dwi(N, shape, seed=len(channels) + N)
    xd = dev(x)
    before = xd.clone()
    t = A.MeanDWI(channels)
    out = t({"full_dwi": xd})
    y = host(out["mean_dwi"])
    want = np_mean(x, channels)
    assert y.dtype == np.float32 and y.shape == (1,) + tuple(shape)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    if len(channels) <= 14:   # the Classic variant's torch.mean (CPU) at its sizes; beyond, torch sums in a cascade
        assert np.array_equal(y, torch.mean(torch.from_numpy(x)[channels], 0, keepdim=True).numpy())
    assert torch.equal(xd, before) and set(out) == {"full_dwi", "mean_dwi"} and out["full_dwi"] is xd
    assert t.last_history == {"channels": channels}


def test_mean_dwi_of_an_unaligned_tensor():
    N, shape = 6, (8, 4, 2)
    x = dwi(N, shape, seed=3)
    S = int(np.prod(shape))
    big = torch.zeros(N * S + 1, device=DEV)
    big[1:] = dev(x.reshape(-1))
    xd = big[1:].view((N,) + shape)      # 4 bytes past a 16-byte boundary: the scalar path
    y = host(A.MeanDWI([5, 0, 5, 2])({"full_dwi": xd})["mean_dwi"])
    assert np.array_equal(y, np_mean(x, [5, 0, 5, 2]))


def test_mean_dwi_rejects_bad_channels_and_types():
    x = dev(dwi(4, (3, 3, 3), 0))
    with pytest.raises(M355Error, match="channel 4"):
        A.MeanDWI([0, 4])({"full_dwi": x})
    with pytest.raises(M355Error, match="float32"):
        A.MeanDWI([0])({"full_dwi": x.to(torch.int32)})


# ------------------------------------------------------------------------------------------------ the transforms
def _random(kind):
    if kind == "reconstruct":
        return A.ReconstructMeanDWI(num_dwis=(1, 7), num_directions=(1, 3), directionality=(4, 10))
    return A.ReconstructMeanDWIClassic(subset_size=15)


@pytest.mark.parametrize("kind", ["reconstruct", "classic"])
def test_random_transforms_replay_bit_exact_and_leave_inputs_alone(kind):
    N, shape = 64, (13, 11, 7)
    x = dwi(N, shape, 5)
    g = grad_table(N, 5)
    old = dwi(1, shape, 6)
    s = {"full_dwi": dev(x), "mean_dwi": dev(old), "md": dev(dwi(1, shape, 7))}
    before = {k: v.clone() for k, v in s.items()}
    t = _random(kind)
    seen = set()
    for seed in range(6):
        out = t(s, generator=torch.Generator().manual_seed(seed), attributes={"full_dwi": {"grad": g}})
        h = t.last_history
        ch = h["channels"]
        assert all(4 <= c < N - 4 for c in ch)          # b = 0 and b = 1000 rows never
        y = host(out["mean_dwi"])
        assert np.array_equal(y.view(np.uint32), np_mean(x, ch).view(np.uint32)), seed
        replay = A.MeanDWI(ch)({"full_dwi": s["full_dwi"]})["mean_dwi"]
        assert torch.equal(replay, out["mean_dwi"])
        assert out["md"] is s["md"] and out["full_dwi"] is s["full_dwi"]
        assert list(out) == ["full_dwi", "mean_dwi", "md"]   # replaced in place in the subject's order
        seen.add(tuple(ch))
        again = t(s, generator=torch.Generator().manual_seed(seed), attributes={"full_dwi": {"grad": g}})
        assert torch.equal(again["mean_dwi"], out["mean_dwi"])
        assert t.last_meta["attributes"]["full_dwi"]["grad"] is g
    assert len(seen) > 3
    for k in s:
        assert same(s[k], before[k]), k


def test_mean_dwi_is_created_when_absent():
    N, shape = 16, (9, 6, 5)
    x = dwi(N, shape, 8)
    g = grad_table(N, 8, n_b0=2, n_high=0)
    t = A.ReconstructMeanDWI(num_dwis=4, num_directions=1)
    out = t({"full_dwi": dev(x)}, generator=torch.Generator().manual_seed(2), attributes={"full_dwi": {"grad": g}})
    assert list(out) == ["full_dwi", "mean_dwi"]
    assert out["mean_dwi"].dtype == torch.float32 and tuple(out["mean_dwi"].shape) == (1,) + shape
    assert t.last_history["num_directions"] == 4 and len(t.last_history["channels"]) == 4
    assert np.array_equal(host(out["mean_dwi"]), np_mean(x, t.last_history["channels"]))
    assert t.last_meta["attributes"]["mean_dwi"]["grad"] is g       # the reference deep-copies full_dwi's image
    # without attributes, last_meta keeps its former keys
    plain = A.MeanDWI([0])
    plain({"full_dwi": dev(x)})
    assert "attributes" not in plain.last_meta


def test_missing_full_dwi_is_a_no_op():
    m = dev(dwi(1, (5, 4, 3), 9))
    for t in (_random("reconstruct"), _random("classic"), A.MeanDWI([0, 1])):
        out = t({"mean_dwi": m}, generator=torch.Generator().manual_seed(0))
        assert list(out) == ["mean_dwi"] and out["mean_dwi"] is m


def test_gate_and_host_errors():
    N, shape = 8, (4, 4, 4)
    s = {"full_dwi": dev(dwi(N, shape, 1)), "mean_dwi": dev(dwi(1, shape, 2))}
    g = grad_table(N, 1, n_b0=1, n_high=1)
    t = A.ReconstructMeanDWI(num_dwis=(1, 3), num_directions=(1, 2), p=0.0)
    out = t(s, generator=torch.Generator().manual_seed(0), attributes={"full_dwi": {"grad": g}})
    assert out["mean_dwi"] is s["mean_dwi"] and t.last_history is None
    for x in (_random("reconstruct"), _random("classic")):
        with pytest.raises(M355Error, match="gradient table"):
            x(s, generator=torch.Generator().manual_seed(0))
        with pytest.raises(M355Error, match="rows"):
            x(s, attributes={"full_dwi": {"grad": g[:-1]}})
        with pytest.raises(M355Error, match="host"):
            x(s, attributes={"full_dwi": {"grad": torch.from_numpy(g).to(DEV)}})
        nob = g.copy()
        nob[:, 3] = 0
        with pytest.raises(M355Error, match="no gradient"):
            x(s, attributes={"full_dwi": {"grad": torch.from_numpy(nob)}})


# ------------------------------------------------------------------------------------------------ chain semantics
def test_pending_work_of_full_dwi_runs_first_and_that_of_the_old_mean_is_dropped():
    N, shape = 12, (11, 9, 7)
    full = dwi(N, shape, 4, nan=True)
    full = np.where(np.isnan(full), full, np.abs(full) + 1.0).astype(np.float32)
    old = dwi(1, shape, 5, nan=True)
    roi = np.zeros((1,) + shape, np.uint8)
    roi[0, 2:9, 1:6, 3:7] = 1
    g = grad_table(N, 4, n_b0=2, n_high=2)
    s = {"mean_dwi": dev(old), "full_dwi": dev(full), "roi": dev(roi)}
    before = {k: v.clone() for k, v in s.items()}
    t = A.Compose([P.ReplaceNan(), P.CropOrPad((8, 12, 6), padding_mode="minimum", mask_name="roi"),
                   A.ReconstructMeanDWI(num_dwis=(3, 9), num_directions=(1, 3), directionality=(4, 10))])
    for seed in range(3):
        out = t(s, label_maps=("roi",), generator=torch.Generator().manual_seed(seed),
                attributes={"full_dwi": {"grad": g}})
        ch = t.last_history[2][1]["channels"]
        pad, crop = R.crop_or_pad_bounds(shape, (8, 12, 6), roi[0])
        fc = R.crop_or_pad(R.replace_nan(full), pad, crop, "minimum")
        assert np.array_equal(host(out["full_dwi"]), fc)
        assert np.array_equal(host(out["mean_dwi"]).view(np.uint32), np_mean(fc, ch).view(np.uint32)), seed
    # a pending rescale of full_dwi is applied before the gather; one of the old mean_dwi is dropped
    t2 = A.Compose([A.RescaleIntensity((0, 1), include=["full_dwi", "mean_dwi"]), A.RandomBlur((1, 2), include=["mean_dwi"]),
                    A.MeanDWI([3, 1, 3])])
    clean = {"full_dwi": dev(np.abs(dwi(N, shape, 6))), "mean_dwi": dev(dwi(1, shape, 7))}
    out = t2(clean, generator=torch.Generator().manual_seed(0))
    assert np.array_equal(host(out["mean_dwi"]), np_mean(host(out["full_dwi"]), [3, 1, 3]))
    assert float(out["full_dwi"].max()) == 1.0
    for k in s:
        assert same(s[k], before[k]), k


# ------------------------------------------------------------------------------------------------ dmri_hippo modes
def standard_augmentations():
    noise, blur = A.RandomNoise(std=0.035, p=0.3), A.RandomBlur((0, 1), p=0.2)
    return A.Compose([
        A.RandomFlip(axes=(0, 1, 2)),
        A.RandomElasticDeformation(p=0.5, num_control_points=(7, 7, 4), locked_borders=1,
                                   image_interpolation="bspline", exclude="full_dwi"),
        A.RandomBiasField(p=0.5), A.RescaleIntensity((0, 1), (0.01, 99.9)), A.RandomGamma(p=0.8),
        A.RescaleIntensity((-1, 1)), A.OneOf([A.Compose([blur, noise]), A.Compose([noise, blur])])],
        exclude="full_dwi")


def dwi_augmentation():
    return A.ReconstructMeanDWI(num_dwis=(1, 7), num_directions=(1, 3), directionality=(4, 10))


def mode_chain(mode):
    """research/dmri_hippo/configs/augmentation.py: the training transform with its second element replaced"""
    middle = {"no_augmentation": [], "standard": [standard_augmentations()], "dwi_reconstruction": [dwi_augmentation()],
              "combined": [A.Compose([dwi_augmentation(), standard_augmentations()])]}[mode]
    return A.Compose([dmri_common_1()] + middle + [dmri_common_2()])


N_GRAD = 64


def dmri_subject(n=N_GRAD):
    rng = np.random.default_rng(21)
    shape = (101, 93, 19)          # crops axes 0 and 1 to (96, 88), pads axis 2 to 24
    base = np.stack([np.cumsum(rng.standard_normal(shape), axis=a) for a in range(3)])
    imgs = {n: (base[i:i + 1] / 20 + 2.0 + i).astype(np.float32) for i, n in enumerate(["mean_dwi", "md", "fa"])}
    full = (np.abs(base[rng.integers(0, 3, n)] / 20 + rng.uniform(0.5, 2.0, (n, 1, 1, 1))) * 100)
    full = full.astype(np.float32)
    full[3, 50, 40, 10] = np.nan
    imgs["full_dwi"] = full
    imgs["mean_dwi"][0, 10, 10, 5] = np.nan
    roi = np.zeros((1,) + shape, np.int64)
    roi[0, 30:60, 20:44, 4:16] = 1
    roi[0, 30:60, 44:70, 4:16] = 2
    labs = {"whole_roi": roi, "whole_roi_union": (roi > 0).astype(np.uint8)}
    return imgs, labs, {"whole_roi": {"left_whole": 1, "right_whole": 2}}, grad_table(n, 21)


def _call(chain, s, labs, lv, g, seed):
    return chain(s, label_maps=tuple(labs), spacing=(1.0, 1.0, 1.0), label_values=lv,
                 generator=torch.Generator().manual_seed(seed), attributes={"full_dwi": {"grad": g}})


def test_dmri_hippo_modes_end_to_end():
    imgs, labs, lv, g = dmri_subject()
    s = {k: dev(v) for k, v in {**imgs, **labs}.items()}
    before = {k: v.clone() for k, v in s.items()}
    pad, crop = R.crop_or_pad_bounds(imgs["mean_dwi"].shape[1:], (96, 88, 24), labs["whole_roi_union"][0])
    fc = R.crop_or_pad(R.replace_nan(imgs["full_dwi"]), pad, crop, "minimum")
    full_want = AR.rescale(fc.astype(np.float64), (-1., 1.), (0.5, 99.5))
    plain = _call(mode_chain("no_augmentation"), s, labs, lv, g, 0)
    assert tuple(plain["full_dwi"].shape) == (N_GRAD, 96, 88, 24)
    assert np.abs(host(plain["full_dwi"]) - full_want).max() <= 1e-5
    dwi_chain, comb = mode_chain("dwi_reconstruction"), mode_chain("combined")
    for seed in (0, 1, 2, 5):
        out = _call(dwi_chain, s, labs, lv, g, seed)
        ch = dwi_chain.last_history[1][1]["channels"]
        assert 1 <= len(ch) <= 7
        mean = np_mean(fc, ch).astype(np.float64)
        want = AR.rescale(mean, (-1., 1.), (0.5, 99.5))
        assert tuple(out["X"].shape) == (3, 96, 88, 24)
        assert np.abs(host(out["X"][0:1]) - want).max() <= 1e-5, seed
        assert torch.equal(out["full_dwi"], plain["full_dwi"])
        out = _call(comb, s, labs, lv, g, seed)
        hist = comb.last_history[1][1]
        assert hist[0][0] == "ReconstructMeanDWI" and 1 <= len(hist[0][1]["channels"]) <= 7
        # the standard augmentations exclude full_dwi: only the common stages touched it
        assert torch.equal(out["full_dwi"], plain["full_dwi"]), seed
        assert tuple(out["X"].shape) == (3, 96, 88, 24) and torch.isfinite(out["X"]).all()
    for k in s:
        assert same(s[k], before[k]), k


def test_dmri_hippo_modes_never_synchronise(monkeypatch):
    imgs, labs, lv, g = dmri_subject()
    s = {k: dev(v) for k, v in {**imgs, **labs}.items()}
    chains = [mode_chain(m) for m in ("dwi_reconstruction", "combined")] + [
        A.Compose([dmri_common_1(), A.ReconstructMeanDWIClassic(), dmri_common_2()])]
    gt = torch.from_numpy(g)     # a host tensor works as well as an array
    run = lambda: [_call(c, s, labs, lv, gt, seed) for c in chains for seed in range(2)]
    refs = run()
    outs = _no_sync(monkeypatch, run)
    for a, b in zip(outs, refs):
        for k in a:
            assert torch.equal(a[k], b[k]), k
