"""Augmentation without a GPU: the float64 restatement (augment_ref) against scipy / numpy, the host parameter draws of
segmentation_pipeline_amd.augmentation, and argument validation of the m355_aug_* entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

import augment_ref as R
from segmentation_pipeline_amd import _lib
from segmentation_pipeline_amd import augmentation as A

ndi = pytest.importorskip("scipy.ndimage")


def _inside_coords(shape, n, rng):
    return np.stack([rng.uniform(0, s - 1, n) for s in shape])


def test_ref_linear_matches_scipy_map_coordinates():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 9, 7, 5))
    q = _inside_coords(x.shape[1:], 300, rng).reshape(3, 300, 1, 1)
    got = R.sample(x, q, "linear")[0].ravel()
    want = ndi.map_coordinates(x[0], q.reshape(3, -1), order=1, mode="nearest")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_ref_bspline_matches_scipy_on_mirror_prefiltered_coefficients():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((1, 9, 7, 6))
    q = _inside_coords(x.shape[1:], 300, rng).reshape(3, 300, 1, 1)
    got = R.sample(R.prefilter(x), q, "bspline")[0].ravel()
    want = ndi.map_coordinates(x[0], q.reshape(3, -1), order=3, mode="mirror")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-10)


@pytest.mark.parametrize("sig", [(0.7, 1.3, 2.5), (0.0, 1.0, 0.4)])
def test_ref_blur_matches_scipy_gaussian_filter(sig):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 11, 6, 3))   # radius 10 > 3 voxels: repeated reflection
    got = R.gaussian_blur(x, sig)
    want = np.stack([ndi.gaussian_filter(c, sig, mode="reflect", truncate=4.0) for c in x])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_ref_percentile_and_rank_split():
    rng = np.random.default_rng(3)
    for n in (1, 2, 17, 1000):
        v = np.sort(rng.standard_normal(n))
        for q in (0, 0.01, 50, 99.9, 100):
            k, t = A._percentile_rank(n, q)
            a, b = v[k], v[min(k + 1, n - 1)]
            lerp = b - (b - a) * (1 - t) if t >= 0.5 else a + (b - a) * t
            assert lerp == np.percentile(v, q)


def test_ref_philox_known_answer():
    # Random123 known-answer vector for philox4x32-10: counter 0, key 0
    w = R.philox4x32(np.array([0]), np.array([0]), 0)
    assert [int(a[0]) for a in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


class _FakeState(A._State):
    def __init__(self, shape=(1, 4, 4, 4), names=("img",), labels=(), seed=0):
        g = torch.Generator().manual_seed(seed)
        super().__init__({n: torch.zeros(shape) for n in names}, labels, (1.0, 1.0, 1.0), g)


def _draws(t, n, seed=0, names=("img",), labels=()):
    """run only the host side of a random transform: its deterministic counterpart is stubbed out"""
    out = []
    st = _FakeState(names=names, labels=labels, seed=seed)
    for _ in range(n):
        t._run(st)
        out.append(t.last_history)
    return out


@pytest.fixture
def no_device(monkeypatch):
    """stub every device call: the transforms record what they would apply"""
    calls = []
    monkeypatch.setattr(A, "_resample", lambda state, name, *a, **k: calls.append(("resample", name, a, k)))
    monkeypatch.setattr(A._State, "flush", lambda self, name: self.pending.pop(name, None))
    return calls


def test_flip_frequency(no_device):
    t = A.RandomFlip(axes=(0, 1, 2))
    hist = _draws(t, 4000)
    f = np.array([h["flip"] for h in hist], dtype=np.float64).mean(0)
    assert np.all(np.abs(f - 0.5) < 5 * 0.5 / np.sqrt(4000))
    t = A.RandomFlip(axes=(1,))
    assert all(not h["flip"][0] and not h["flip"][2] for h in _draws(t, 200))


def test_gamma_log_uniform_range(no_device):
    t = A.RandomGamma(log_gamma=0.3)
    g = np.array([h["gammas"]["img"][0] for h in _draws(t, 3000)])
    lg = np.log(g)
    assert lg.min() >= -0.3 and lg.max() <= 0.3 and lg.min() < -0.28 and lg.max() > 0.28
    assert abs(lg.mean()) < 5 * 0.3 / np.sqrt(3 * 3000)


def test_oneof_weights_and_p(no_device):
    a, b = A.RandomFlip(axes=(0,), flip_probability=1.0), A.RandomFlip(axes=(1,), flip_probability=1.0)
    t = A.OneOf({a: 0.2, b: 0.8}, p=0.75)
    hist = _draws(t, 4000)
    applied = [h for h in hist if h is not None]
    assert abs(len(applied) / 4000 - 0.75) < 5 * np.sqrt(0.75 * 0.25 / 4000)
    share = np.mean([h["chosen"] == 1 for h in applied])
    assert abs(share - 0.8) < 5 * np.sqrt(0.16 / len(applied))


def test_elastic_locked_borders_are_zero(no_device):
    for lb in (1, 2):
        t = A.RandomElasticDeformation(num_control_points=(7, 7, 5), max_displacement=(7.5, 5, 2), locked_borders=lb)
        g = _draws(t, 1)[0]["control_grid"]
        assert g.shape == (7, 7, 5, 3)
        for b in range(lb):
            for sl in (np.s_[b], np.s_[-1 - b], np.s_[:, b], np.s_[:, -1 - b], np.s_[:, :, b], np.s_[:, :, -1 - b]):
                assert np.all(g[sl] == 0)
        inner = g[lb:-lb, lb:-lb, lb:-lb]
        assert np.all(np.abs(inner) <= np.array([7.5, 5, 2])) and np.any(inner != 0)


def test_include_exclude_and_label_routing(no_device):
    st = _FakeState(names=("a", "b", "seg"), labels=("seg",))
    A.RandomFlip(axes=(0,), flip_probability=1.0, exclude=["b"])._run(st)
    assert [c[1] for c in no_device] == ["a", "seg"]
    A.RandomGamma(include=["a", "seg"])._run(st)
    assert list(st.pending) == ["a"]             # labels skip intensity transforms
    no_device.clear()
    A.Compose([A.RandomFlip(axes=(0,), flip_probability=1.0), A.RandomGamma()], exclude="a")._run(st)
    assert [c[1] for c in no_device] == ["b", "seg"] and set(st.pending) == {"a", "b"}


def test_identity_flip_and_permutation_touch_nothing(no_device):
    st = _FakeState(names=("a", "seg"), labels=("seg",))
    A.RandomFlip(axes=(0, 1, 2), flip_probability=0.0)._run(st)
    A.PermuteDimensions((0, 1, 2))._run(st)
    assert no_device == [] and not st.owned


def test_per_image_draws(no_device):
    st = _FakeState(names=("a", "b"))
    t = A.RandomBiasField()
    t._run(st)
    c = t.last_history["coefficients"]
    assert set(c) == {"a", "b"} and len(c["a"]) == 20 and c["a"] != c["b"]
    t = A.RandomBlur((0, 1))
    t._run(st)
    s = t.last_history["sigmas"]
    assert set(s) == {"a", "b"} and s["a"] != s["b"] and all(0 <= v <= 1 for v in s["a"] + s["b"])


def test_zero_blur_then_intensity_never_writes_the_callers_tensor(monkeypatch):
    """sigma = 0 on every axis is the identity: the tensor stays the caller's, so the fused pass after it must write a
    new tensor (it once wrote the input in place)"""
    calls = []
    monkeypatch.setattr(A, "_run_program", lambda x, y, stages, state: calls.append((x, y, [s[0] for s in stages])))
    monkeypatch.setattr(A, "_run_blur", lambda *a: pytest.fail("a zero blur must not launch"))
    x = torch.zeros(1, 4, 4, 4)
    st = A._State({"img": x}, (), (1.0, 1.0, 1.0), torch.Generator().manual_seed(0))
    A.Compose([A.Blur((0.0, 0.0, 0.0)), A.RandomNoise(std=0.1, p=1.0), A.RescaleIntensity((-1, 1))])._run(st)
    st.flush_all()
    assert len(calls) == 1 and calls[0][2] == ["noise", "rescale"]
    assert calls[0][0] is x and calls[0][1] is not x and st.data["img"] is not x


def test_blur_takes_the_following_stages_up_to_a_rescale_as_its_epilogue(monkeypatch):
    blurs, progs = [], []
    monkeypatch.setattr(A, "_run_blur", lambda x, sig, ep, state: blurs.append((sig, [s[0] for s in ep])) or x.clone())
    monkeypatch.setattr(A, "_run_program", lambda x, y, stages, state: progs.append([s[0] for s in stages]))
    x = torch.zeros(1, 4, 4, 4)
    st = A._State({"img": x}, (), (1.0, 2.0, 1.0), torch.Generator().manual_seed(0))
    A.Compose([A.RandomGamma(), A.Blur((1.0, 1.0, 0.0)), A.Noise(0, 0.1, 5), A.BiasField([0.1] * 20),
               A.RescaleIntensity((-1, 1)), A.Noise(0, 0.1, 6)])._run(st)
    st.flush_all()
    assert progs == [["gamma"], ["rescale", "noise"]]
    assert blurs == [((1.0, 0.5, 0.0), ["noise", "bias"])]


def test_same_seed_same_history(no_device):
    def chain():
        return A.Compose([A.RandomPermuteDimensions(), A.RandomFlip(axes=(0, 1, 2)),
                          A.OneOf({A.RandomElasticDeformation(): 0.2, A.RandomAffine(scales=0.2, degrees=45): 0.8}),
                          A.RandomBiasField(p=0.5), A.RandomGamma(p=0.8), A.RandomNoise(std=0.1, p=0.35)])
    h = [_draws(chain(), 3, seed=7) for _ in range(2)]
    assert repr(h[0]) == repr(h[1])
    assert repr(_draws(chain(), 3, seed=8)) != repr(h[0])


# ------------------------------------------------------------------------------------------------ C ABI validation
def _i3(*v):
    return (C.c_int32 * 3)(*v)


def test_aug_entry_points_reject_bad_arguments():
    L = _lib.lib()
    P = C.c_void_p(256)
    eye = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    ws = int(L.m355_aug_workspace())
    assert ws > 0
    ks, fr = (C.c_int64 * 2)(0, 64), (C.c_double * 2)(0.0, 0.0)
    cases = [
        (lambda: L.m355_aug_resample(None, P, 1, _i3(4, 4, 4), _i3(4, 4, 4), 4, 1, eye, None, None, None, None, 0.0, None),
         b"null"),
        (lambda: L.m355_aug_resample(P, C.c_void_p(512), 1, _i3(4, 0, 4), _i3(4, 4, 4), 4, 1, eye, None, None, None, None, 0.0,
                             None), b"non-positive"),
        (lambda: L.m355_aug_resample(P, C.c_void_p(512), 1, _i3(4, 4, 4), _i3(4, 4, 4), 4, 3, eye, None, None, None, None, 0.0,
                             None), b"interpolation"),
        (lambda: L.m355_aug_resample(P, C.c_void_p(512), 1, _i3(4, 4, 4), _i3(4, 4, 4), 8, 1, eye, None, None, None, None, 0.0,
                             None), b"nearest"),
        (lambda: L.m355_aug_resample(P, C.c_void_p(512), 1, _i3(4, 4, 4), _i3(4, 4, 4), 2, 0, eye, None, None, None, None, 0.0,
                             None), b"element size"),
        (lambda: L.m355_aug_resample(P, C.c_void_p(512), 1, _i3(4, 4, 4), _i3(4, 4, 4), 4, 1, eye, None, P, _i3(3, 7, 7), None,
                             0.0, None), b">= 4"),
        (lambda: L.m355_aug_prefilter(None, 1, _i3(4, 4, 4), None), b"aug_prefilter"),
        (lambda: L.m355_aug_intensity(P, P, 1, _i3(4, 4, 4), (_lib.AugStage * 1)(_lib.AugStage(op=9)), 1, None), b"unknown op"),
        (lambda: L.m355_aug_intensity(P, P, 1, _i3(4, 4, 4), None, 9, None), b"stages"),
        (lambda: L.m355_aug_intensity(P, P, 1, _i3(4, 4, 4), (_lib.AugStage * 1)(_lib.AugStage(op=_lib.AUG_RESCALE)), 1, None),
         b"statistics"),
        (lambda: L.m355_aug_blur(P, P, 1, _i3(4, 4, 4), 0, 1.0, None, 0, None), b"x == y"),
        (lambda: L.m355_aug_blur(P, C.c_void_p(512), 1, _i3(4, 4, 4), 3, 1.0, None, 0, None), b"axis"),
        (lambda: L.m355_aug_blur(P, C.c_void_p(512), 1, _i3(4, 4, 4), 0, 0.0, None, 0, None), b"sigma"),
        (lambda: L.m355_aug_otsu_pad(P, 0, _i3(4, 4, 4), P, None), b"channels"),
        (lambda: L.m355_aug_channel_minmax(P, 2, _i3(4, 4, 4), 2, P, P, 16, None), b"which"),
        (lambda: L.m355_aug_channel_minmax(None, 2, _i3(4, 4, 4), 0, P, P, 16, None), b"null"),
    ]
    cases.append((lambda: L.m355_aug_order_stats(P, 1, _i3(4, 4, 4), None, 0, 2, ks, fr, P, P, ws, None), b"rank"))
    cases.append((lambda: L.m355_aug_order_stats(P, 1, _i3(4, 4, 4), None, 0, 3, ks, fr, P, P, ws, None), b"queries"))
    cases.append((lambda: L.m355_aug_order_stats(None, 1, _i3(4, 4, 4), None, 0, 1, ks, fr, P, P, ws, None), b"null"))
    for call, msg in cases:
        rc = call()
        assert rc == -1, msg
        assert msg in L.m355_last_error(), (msg, L.m355_last_error())
    assert L.m355_aug_order_stats(P, 1, _i3(4, 4, 4), None, 0, 1, ks, fr, P, P, ws - 1, None) == -4
    assert L.m355_aug_channel_minmax(P, 2, _i3(4, 4, 4), 0, P, P, 15, None) == -4
