"""Device augmentation (segmentation_pipeline_amd.augmentation, csrc/augment.hip) replayed from `last_history` against
the float64 restatement in tests/augment_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import augment_ref as R
from segmentation_pipeline_amd import _lib
from segmentation_pipeline_amd import augmentation as A
from segmentation_pipeline_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ndi = pytest.importorskip("scipy.ndimage")


def smooth(shape, seed, offset=0.0, sigma=2.0):
    rng = np.random.default_rng(seed)
    x = np.stack([ndi.gaussian_filter(rng.standard_normal(shape[1:]), sigma) for _ in range(shape[0])])
    x = x / (np.abs(x).max() + 1e-12) + offset
    return x.astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ exact paths
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8, torch.int32, torch.int64])
def test_flip_and_permute_are_exact(dtype):
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.integers(0, 200, (2, 7, 5, 3))).to(dtype).to(DEV)
    if dtype == torch.float32:
        x = x * 1.37 - 11.0
    before = x.clone()
    labels = () if dtype == torch.float32 else ("x",)
    for perm in [(0, 1, 2), (2, 0, 1), (1, 2, 0), (0, 2, 1)]:
        for flip in [(), (0,), (1, 2), (0, 1, 2)]:
            y = A.PermuteDimensions(perm)({"x": x}, label_maps=labels)["x"]
            y = A.Flip(flip)({"x": y}, label_maps=labels)["x"]
            want = x.permute(0, *[p + 1 for p in perm]).flip([a + 1 for a in flip]) if flip else x.permute(
                0, *[p + 1 for p in perm])
            assert y.dtype == dtype and y.shape == want.shape
            assert torch.equal(y, want)
    assert torch.equal(x, before)   # inputs are never modified


@pytest.mark.parametrize("interp", ["nearest", "linear", "bspline"])
def test_identity_and_integer_translation(interp):
    x = smooth((2, 13, 9, 6), 1, offset=3.0)
    M = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    y = host(A.Affine(M, interp)({"x": dev(x)})["x"])
    if interp == "bspline":
        np.testing.assert_allclose(y, x, rtol=1e-5, atol=0)
    else:
        assert np.array_equal(y, x)
    M[:, 3] = (2, -1, 1)      # integer translation: the input sampled at integer points, pad elsewhere
    y = host(A.Affine(M, interp, default_pad_value=-7.0)({"x": dev(x)})["x"])
    q = R.coordinates(M, x.shape[1:])
    want = R.sample(x.astype(np.float64), q, "nearest", pad=-7.0)
    want = np.where(R.inside(q, x.shape[1:])[None], want, -7.0)
    np.testing.assert_allclose(y, want, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ random fields
SHAPES = [(37, 29, 11), (96, 88, 24), (1, 1, 40)]


def _boundary(q, in_shape, tol=1e-4):
    """voxels whose reference coordinate lies within tol of a rounding or inside/outside boundary"""
    near = np.zeros(q.shape[1:], bool)
    for a in range(3):
        f = q[a] + 0.5
        near |= np.abs(f - np.round(f)) < tol
    return near


def _edge(q, in_shape, tol=1e-4):
    """voxels whose reference coordinate lies within tol of the inside / outside boundary (-0.5 or V - 0.5)"""
    near = np.zeros(q.shape[1:], bool)
    for a in range(3):
        near |= (np.abs(q[a] + 0.5) < tol) | (np.abs(q[a] - (in_shape[a] - 0.5)) < tol)
    return near


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["affine", "elastic"])
def test_random_fields_match_reference(shape, kind):
    x = smooth((2,) + shape, 2, offset=0.5)
    onehot = np.eye(3, dtype=np.float32)[np.digitize(x[0], [0.3, 0.7])].transpose(3, 0, 1, 2).copy()
    g = torch.Generator().manual_seed(5)
    sp = (1.0, 1.2, 2.0)
    if kind == "affine":
        t = A.RandomAffine(scales=0.2, degrees=45, default_pad_value="otsu")
    else:
        t = A.RandomElasticDeformation(num_control_points=(7, 7, 4), max_displacement=(6, 6, 4), locked_borders=1)
    for interp in ("linear", "bspline"):
        t.image_interpolation = interp
        g = torch.Generator().manual_seed(5)
        out = t({"x": dev(x), "seg": dev(onehot)}, label_maps=("seg",), spacing=sp, generator=g)
        h = t.last_history
        if kind == "affine":
            M, grid, pad = h["matrix"], None, R.otsu_pad(x)
        else:
            M = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
            grid, pad = h["control_grid"] / np.asarray(sp), x.reshape(2, -1).min(1)
        q = R.coordinates(M, shape, grid)
        src = R.prefilter(x) if interp == "bspline" else x.astype(np.float64)
        want = R.sample(src, q, interp, pad=pad)
        y = host(out["x"])
        ok = ~_boundary(q, shape)   # inside / outside decided at the boundary by fp32 vs fp64 coordinates
        err = np.abs(y - want)[:, ok].max(initial=0)
        assert err <= 1e-4 * (x.max() - x.min()), (interp, err)
        # nearest labels: exact away from rounding boundaries, and one-hot stays one-hot
        seg = host(out["seg"])
        want_seg = R.sample(onehot, q, "nearest")
        want_seg = np.where(R.inside(q, shape)[None], want_seg, 0)
        assert np.array_equal(seg[:, ok], want_seg[:, ok])
        s = seg.sum(0)
        assert np.all(np.isin(seg, (0.0, 1.0))) and np.all((s == 1) | (s == 0))
        assert np.all(s[~R.inside(q, shape) & ok] == 0)
        # outside points hold the pad value
        outside = ~R.inside(q, shape) & ok
        for c in range(2):
            np.testing.assert_allclose(y[c][outside], pad[c], rtol=1e-6, atol=1e-6)


def test_ramp_reproduces_the_sampled_coordinate():
    shape = (37, 29, 11)
    x = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float32) for n in shape], indexing="ij"))
    g = torch.Generator().manual_seed(3)
    t = A.RandomElasticDeformation(num_control_points=(7, 7, 4), max_displacement=3, locked_borders=2)
    y = host(t({"x": dev(x)}, generator=g)["x"])
    q = R.coordinates(np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1), shape, t.last_history["control_grid"])
    ins = R.inside(q, shape) & np.all([(q[a] >= 0) & (q[a] <= shape[a] - 1) for a in range(3)], axis=0)
    assert ins.mean() > 0.5
    assert np.abs(y - q)[:, ins].max() <= 1e-4


# ------------------------------------------------------------------------------------------------ order statistics
def _order_stats(x, ks, fracs):
    L = _lib.lib()
    t = dev(x.reshape(1, 1, 1, -1))
    out = torch.empty(len(ks), dtype=torch.float64, device=DEV)
    ws = torch.empty(int(L.m355_aug_workspace()), dtype=torch.uint8, device=DEV)
    _lib.check(L.m355_aug_order_stats(_p(t), 1, (C.c_int32 * 3)(1, 1, x.size), None, 0, len(ks),
                                      (C.c_int64 * 2)(*ks), (C.c_double * 2)(*fracs), _p(out), _p(ws), ws.numel(),
                                      _stream()), "order_stats")
    return host(out)


@pytest.mark.parametrize("n", [1, 2, 255, 1000, 70001])
def test_order_statistics_exact(n):
    rng = np.random.default_rng(n)
    x = np.round(rng.standard_normal(n) * 4).astype(np.float32) / 4   # duplicates
    x[: n // 7] *= -1
    if n > 4:
        x[1], x[2], x[3] = 0.0, -0.0, -1e-30
    s = np.sort(x)
    for k in sorted({0, n // 3, n // 2, n - 1, max(0, n - 2)}):
        got = _order_stats(x, [k, 0], [0.0, 0.0])
        assert got[0] == s[k] and got[1] == s[0], (k, got, s[k])
    for q in (0.01, 0.05, 50.0, 99.5, 99.9):
        k0, t0 = A._percentile_rank(n, q)
        k1, t1 = A._percentile_rank(n, 100 - q)
        got = _order_stats(x, [k0, k1], [t0, t1])
        want = np.percentile(x.astype(np.float64), [q, 100 - q])
        for gv, wv in zip(got, want):
            assert abs(gv - wv) <= np.spacing(abs(wv)), (q, gv, wv)


# ------------------------------------------------------------------------------------------------ intensity and blur
def test_intensity_chain_and_blur():
    x = smooth((2, 23, 6, 3), 4, offset=1.5)
    g = torch.Generator().manual_seed(11)
    chain = A.Compose([A.RandomBiasField(), A.RescaleIntensity((0, 1), (0.01, 99.9)), A.RandomGamma(),
                       A.RescaleIntensity((-1, 1)), A.Blur((0.0, 2.5, 2.0)), A.RescaleIntensity((-1, 1), (1, 99))])
    y = host(chain({"x": dev(x)}, spacing=(1.0, 1.0, 0.8), generator=g)["x"])
    h = dict((n, v) for n, v in chain.last_history)
    r = x.astype(np.float64) * R.bias_field(x.shape[1:], h["RandomBiasField"]["coefficients"]["x"])[None]
    r = R.rescale(r, (0, 1), (0.01, 99.9))
    r = R.gamma(r, h["RandomGamma"]["gammas"]["x"])
    r = R.rescale(r, (-1, 1))
    r = R.gaussian_blur(r, (0.0, 2.5, 2.5))
    r = R.rescale(r, (-1, 1), (1, 99))
    assert np.abs(y - r).max() <= 1e-5


def test_noise_stream_and_blur_order():
    x = np.zeros((1, 100, 100, 100), np.float32)
    n1 = A.Noise(0.25, 1.0, 1234)
    y = host(n1({"x": dev(x)})["x"])
    want = R.noise(x.astype(np.float64), 0.25, 1.0, 1234)
    assert np.abs(y - want).max() <= 1e-6 * 10      # std 1: |z| <= 7
    assert abs(y.mean() - 0.25) < 5 / np.sqrt(y.size)
    assert abs(y.std() - 1.0) < 5 / np.sqrt(2 * y.size)
    assert np.array_equal(host(A.Noise(0.25, 1.0, 1234)({"x": dev(x)})["x"]), y)
    assert not np.array_equal(host(A.Noise(0.25, 1.0, 1235)({"x": dev(x)})["x"]), y)
    small = A.Noise(0.0, 0.1, 99)({"x": dev(x[:, :20, :20, :20])})["x"]
    assert np.abs(host(small) - R.noise(np.zeros((1, 20, 20, 20)), 0.0, 0.1, 99)).max() <= 1e-6
    img = dev(smooth((1, 20, 16, 12), 5))
    bn = A.Compose([A.Blur((1.0, 1.0, 1.0)), A.Noise(0, 0.1, 7)])({"x": img})["x"]
    nb = A.Compose([A.Noise(0, 0.1, 7), A.Blur((1.0, 1.0, 1.0))])({"x": img})["x"]
    r_bn = R.noise(R.gaussian_blur(host(img).astype(np.float64), (1, 1, 1)), 0, 0.1, 7)
    r_nb = R.gaussian_blur(R.noise(host(img).astype(np.float64), 0, 0.1, 7), (1, 1, 1))
    assert np.abs(host(bn) - r_bn).max() <= 1e-5 and np.abs(host(nb) - r_nb).max() <= 1e-5
    assert np.abs(host(bn) - host(nb)).max() > 1e-2


# ------------------------------------------------------------------------------------------------ end to end
def dmri_chain():
    noise, blur = A.RandomNoise(std=0.035, p=0.3), A.RandomBlur((0, 1), p=0.2)
    return A.Compose([
        A.RandomFlip(axes=(0, 1, 2)),
        A.RandomElasticDeformation(p=0.5, num_control_points=(7, 7, 4), locked_borders=1, image_interpolation="bspline"),
        A.RandomBiasField(p=0.5), A.RescaleIntensity((0, 1), (0.01, 99.9)), A.RandomGamma(p=0.8),
        A.RescaleIntensity((-1, 1)), A.OneOf([A.Compose([blur, noise]), A.Compose([noise, blur])])])


def msseg2_chain():
    return A.Compose([
        A.RandomPermuteDimensions(), A.RandomFlip(axes=(0, 1, 2)),
        A.OneOf({A.RandomElasticDeformation(): 0.2,
                 A.RandomAffine(scales=0.2, degrees=45, default_pad_value="otsu"): 0.8}, p=0.75),
        A.RandomBiasField(p=0.5), A.RescaleIntensity((0, 1), (0.01, 99.9)), A.RandomGamma(p=0.8),
        A.RescaleIntensity((-1, 1)), A.RandomBlur((0, 1), p=0.2), A.RandomNoise(std=0.1, p=0.35)])


def replay(t, hist, data, labels, spacing, near):
    """apply one history entry of `t` to the float64 arrays in `data` (labels: nearest, pad 0).  near[k]: voxels whose
    result may legitimately differ in fp32 -- a reference coordinate within 1e-4 of a rounding or inside / outside
    boundary (_boundary), carried through later flips / permutations and widened by the blur radius"""
    if hist is None:
        return data
    if isinstance(t, A.OneOf):
        return replay(t.transforms[hist["chosen"]], hist["history"][1], data, labels, spacing, near)
    if isinstance(t, A.Compose):
        for c, (_, h) in zip(t.transforms, hist):
            data = replay(c, h, data, labels, spacing, near)
        return data
    out = {}
    for k, x in data.items():
        nk = near.setdefault(k, np.zeros(x.shape[1:], bool))
        lab = k in labels
        if isinstance(t, (A.RandomFlip, A.Flip)):
            out[k] = np.flip(x, [a + 1 for a in range(3) if hist["flip"][a]]).copy()
            near[k] = np.flip(nk, [a for a in range(3) if hist["flip"][a]]).copy()
        elif isinstance(t, A.RandomPermuteDimensions):
            out[k] = x.transpose(0, *[p + 1 for p in hist["permutation"]]).copy()
            near[k] = nk.transpose(*hist["permutation"]).copy()
        elif isinstance(t, (A.RandomElasticDeformation, A.RandomAffine)):
            shape = x.shape[1:]
            if isinstance(t, A.RandomAffine):
                q = R.coordinates(hist["matrix"], shape)
                pad = R.otsu_pad(x) if t.pad == "otsu" else x.reshape(x.shape[0], -1).min(1)
            else:
                q = R.coordinates(np.concatenate([np.eye(3), np.zeros((3, 1))], 1), shape,
                                  hist["control_grid"] / np.asarray(spacing))
                pad = x.reshape(x.shape[0], -1).min(1)
            mode = "nearest" if lab else t.image_interpolation
            src = R.prefilter(x) if mode == "bspline" else x
            y = R.sample(src, q, mode, pad=0.0 if lab else pad)
            if lab:
                y = np.where(R.inside(q, shape)[None], y, 0)
            out[k] = y
            # images interpolate continuously: only the inside / outside decision can flip; labels round as well
            near[k] = nk | (_boundary(q, shape) if lab else _edge(q, shape))
        elif lab:
            out[k] = x
        elif isinstance(t, A.RandomBiasField):
            out[k] = x * R.bias_field(x.shape[1:], hist["coefficients"][k])[None]
        elif isinstance(t, A.RescaleIntensity):
            out[k] = R.rescale(x, hist["out_min_max"], hist["percentiles"])
        elif isinstance(t, A.RandomGamma):
            out[k] = R.gamma(x, hist["gammas"][k])
        elif isinstance(t, A.RandomBlur):
            sv = np.asarray(hist["sigmas"][k]) / np.asarray(spacing)
            out[k] = R.gaussian_blur(x, sv)
            m = nk
            for a in range(3):
                if sv[a] > 0:
                    m = ndi.maximum_filter1d(m, 2 * int(4.0 * sv[a] + 0.5) + 1, axis=a, mode="reflect")
            near[k] = m
        elif isinstance(t, A.RandomNoise):
            out[k] = R.noise(x, hist["mean"], hist["std"], hist["seed"])
        else:
            raise AssertionError(type(t))
    return out


def _subject(kind):
    if kind == "dmri":
        shape = (96, 88, 24)
        imgs = {f"img{i}": smooth((1,) + shape, 10 + i, offset=2.0) for i in range(3)}
        lab = np.eye(3, dtype=np.float32)[np.digitize(imgs["img0"][0], [1.8, 2.2])].transpose(3, 0, 1, 2).copy()
        return imgs, {"seg": lab}, (1.0, 1.0, 1.0)
    shape = (160, 192, 160)
    imgs = {f"img{i}": smooth((1,) + shape, 20 + i, offset=1.0, sigma=3.0) for i in range(2)}
    lab = (imgs["img0"] > 1.4).astype(np.uint8)
    return imgs, {"seg": lab}, (1.0, 1.0, 1.0)


# seeds chosen so that every branch runs: dmri 1 / 8 / 10 / 11 / 99 / 104 elastic (with blur, Blur o Noise and
# Noise o Blur), 3 / 4 / 5 intensity only; msseg2 3 / 11 affine (with blur / bias + noise), 9 elastic, 4 no spatial OneOf
@pytest.mark.parametrize("kind,seeds", [("dmri", (1, 3, 4, 5, 8, 10, 11, 99, 104)), ("msseg2", (3, 4, 9, 11))])
def test_production_chains_match_reference(kind, seeds):
    imgs, labs, sp = _subject(kind)
    chain = dmri_chain() if kind == "dmri" else msseg2_chain()
    subject = {k: dev(v) for k, v in {**imgs, **labs}.items()}
    before = {k: v.clone() for k, v in subject.items()}
    for seed in seeds:
        out = chain(subject, label_maps=tuple(labs), spacing=sp, generator=torch.Generator().manual_seed(seed))
        near = {}
        ref = replay(chain, chain.last_history, {k: v.astype(np.float64) if k in imgs else v
                                                 for k, v in {**imgs, **labs}.items()}, set(labs), sp, near)
        for k in imgs:
            ok = ~near[k]
            assert ok.mean() > 0.99
            err = np.abs(host(out[k]) - ref[k])[:, ok]
            assert err.max(initial=0) <= 1e-4, (seed, k, err.max())
        for k in labs:
            y = host(out[k])
            assert y.dtype == labs[k].dtype and np.array_equal(y[:, ~near[k]], ref[k][:, ~near[k]]), (seed, k)
    for k in subject:
        assert torch.equal(subject[k], before[k])


@pytest.mark.parametrize("kind", ["dmri", "msseg2"])
def test_chains_never_synchronise_and_run_on_a_side_stream(kind, monkeypatch):
    imgs, labs, sp = _subject(kind)
    subject = {k: dev(v) for k, v in {**imgs, **labs}.items()}
    chain = dmri_chain() if kind == "dmri" else msseg2_chain()
    ref_outs = [chain(subject, label_maps=tuple(labs), spacing=sp, generator=torch.Generator().manual_seed(s))
                for s in range(3)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            torch.zeros(1, device=DEV).item()
        except RuntimeError:
            honoured = True
        if not honoured:   # this torch build ignores the mode: make every host synchronisation raise instead
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
            outs = [chain(subject, label_maps=tuple(labs), spacing=sp, generator=torch.Generator().manual_seed(s))
                    for s in range(3)]
    finally:
        torch.cuda.set_sync_debug_mode(0)
        monkeypatch.undo()
    torch.cuda.current_stream().wait_stream(side)
    for a, b in zip(outs, ref_outs):
        for k in a:
            assert torch.equal(a[k], b[k]), k
