"""Host-side parameter draws of ReconstructMeanDWI / ReconstructMeanDWIClassic (augmentation.py): the laws
are restated here independently of the implementation and checked with chi-square tests at fixed seeds."""
import math

import numpy as np
import pytest
import torch

from segmentation_pipeline_amd import augmentation as A
from segmentation_pipeline_amd._lib import M355Error


def chi2_ok(counts, probs, z=3.719):
    """Pearson's chi-square below its upper 1e-4 quantile (Wilson-Hilferty), cells with expectation >= 5 only"""
    counts, probs = np.asarray(counts, dtype=np.float64), np.asarray(probs, dtype=np.float64)
    n = counts.sum()
    exp = n * probs / probs.sum()
    keep = exp >= 5
    assert counts[~keep].sum() <= max(5.0, 1e-3 * n)   # what is left out is rare
    stat = float(np.sum((counts[keep] - exp[keep]) ** 2 / exp[keep]))
    k = int(keep.sum()) - 1
    crit = k * (1 - 2 / (9 * k) + z * math.sqrt(2 / (9 * k))) ** 3
    return stat < crit, (stat, crit)


def grad_table(n=64, seed=0, bval=500.0):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.concatenate([v, np.full((n, 1), bval)], axis=1)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def test_num_dwis_follows_the_squared_uniform_law():
    lo, hi = 1, 7
    t = A.ReconstructMeanDWI(num_dwis=(lo, hi), num_directions=(1, 3), directionality=(4, 10))
    g = grad_table(8)
    G = gen(11)
    draws = [t.draw(g, G)["num_dwis"] for _ in range(20000)]
    counts = np.bincount(draws, minlength=hi + 1)[lo:]
    assert min(draws) == lo and max(draws) == hi
    # int(u^2 (hi - lo + 1) + lo) = j  <=>  (j - lo) / w <= u^2 < (j - lo + 1) / w, w = hi - lo + 1
    w = hi - lo + 1
    probs = [math.sqrt((j - lo + 1) / w) - math.sqrt((j - lo) / w) for j in range(lo, hi + 1)]
    ok, info = chi2_ok(counts, probs)
    assert ok, info


def test_num_directions_is_uniform_on_the_inclusive_range():
    t = A.ReconstructMeanDWI(num_dwis=(1, 7), num_directions=(1, 3), directionality=(4, 10))
    g = grad_table(8)
    G = gen(12)
    hs = [t.draw(g, G) for _ in range(20000)]
    m = [h["num_directions"] for h in hs]
    assert set(m) == {1, 2, 3}
    ok, info = chi2_ok(np.bincount(m)[1:], [1, 1, 1])
    assert ok, info
    for h in hs[:200]:
        assert h["directions"].shape == (3, h["num_directions"])
        assert np.allclose(np.linalg.norm(h["directions"], axis=0), 1.0)
        assert 4.0 <= h["directionality"] < 10.0


def test_int_num_directions_quirk_returns_num_dwis():
    g = grad_table(16)
    h = A.ReconstructMeanDWI(num_dwis=5, num_directions=1).draw(g, gen(0))
    assert h["num_dwis"] == 5 and h["num_directions"] == 5 and h["directions"].shape == (3, 5)
    h = A.ReconstructMeanDWI().draw(g, gen(0))   # the defaults: 15 images, so 15 directions
    assert h["num_dwis"] == 15 and h["num_directions"] == 15 and len(h["channels"]) == 15
    with pytest.raises(M355Error, match="num_directions"):
        A.ReconstructMeanDWI(num_dwis=(1, 7), num_directions=2)


def test_pick_frequencies_match_the_direction_law():
    g = grad_table(32, seed=3)
    g[5, :3] = 0.0            # an eligible gradient along no direction: never picked (unless directionality is 0)
    n = 20000
    t = A.ReconstructMeanDWI(num_dwis=(n, n), num_directions=(2, 2), directionality=(3.0, 3.0))
    h = t.draw(g, gen(5))
    d = h["directions"]
    # restated: p_i proportional to max over the directions of |b_i . d_j| ** directionality
    p = np.array([max(abs(float(np.dot(g[i, :3], d[:, j]))) ** 3.0 for j in range(d.shape[1])) for i in range(32)])
    counts = np.bincount(h["channels"], minlength=32)
    assert counts.sum() == n and counts[5] == 0
    ok, info = chi2_ok(counts, p)
    assert ok, info


def test_gradients_outside_the_bval_range_are_never_picked():
    g = grad_table(40, seed=4)
    g[:6, 3] = 0.0            # b = 0
    g[6:9, 3] = 1e-5          # the open lower bound
    g[9:12, 3] = 501.0        # the open upper bound
    g[12:16, 3] = 1000.0      # the second shell
    g[:16, :3] = [0.0, 0.0, 1.0]   # and they would be the likeliest picks
    excluded = set(range(16))
    t = A.ReconstructMeanDWI(num_dwis=(1, 7), num_directions=(1, 3), directionality=(4, 10))
    c = A.ReconstructMeanDWIClassic(subset_size=15)
    G = gen(7)
    seen = set()
    for _ in range(2000):
        seen |= set(t.draw(g, G)["channels"])
        h = c.draw(g, G)
        seen |= set(h["channels"]) | set(h["subset"]) | {h["reference"]}
    assert not seen & excluded
    assert seen == set(range(16, 40))


def test_classic_picks_among_the_nearest_and_never_more_than_subset_size_minus_one():
    g = grad_table(48, seed=8)
    g[:3, 3] = 0.0
    S = 6
    t = A.ReconstructMeanDWIClassic(subset_size=S)
    G = gen(9)
    elig = np.arange(3, 48)
    nsel = []
    refs = set()
    for _ in range(4000):
        h = t.draw(g, G)
        r = h["reference"]
        refs.add(r)
        dist = np.sum((g[elig, :3] - g[r, :3]) ** 2, axis=1)
        nearest = set(elig[np.argsort(dist, kind="stable")[:S]].tolist())
        assert set(h["subset"]) == nearest and r in nearest
        assert set(h["channels"]) <= nearest
        assert len(set(h["channels"])) == len(h["channels"]) == h["num_selections"] <= S - 1
        nsel.append(h["num_selections"])
    assert refs == set(elig.tolist())
    ok, info = chi2_ok(np.bincount(nsel)[1:], [1] * (S - 1))   # randint(1, S): 1 .. S - 1, uniform
    assert ok, info


def test_classic_with_fewer_eligible_gradients_than_the_subset():
    g = grad_table(5, seed=2)
    h = A.ReconstructMeanDWIClassic(subset_size=15).draw(g, gen(3))
    assert sorted(h["subset"]) == list(range(5)) and len(h["channels"]) == min(h["num_selections"], 5)


def test_the_same_seed_gives_the_same_history():
    g = grad_table(64, seed=1)
    for t in (A.ReconstructMeanDWI(num_dwis=(1, 7), num_directions=(1, 3), directionality=(4, 10)),
              A.ReconstructMeanDWIClassic()):
        a, b = t.draw(g, gen(21)), t.draw(g, gen(21))
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        assert any(not np.array_equal(np.asarray(t.draw(g, gen(s))["channels"]), np.asarray(a["channels"]))
                   for s in range(22, 26))


def test_documented_errors():
    g = grad_table(10)
    t = A.ReconstructMeanDWI(num_dwis=(1, 7), num_directions=(1, 3))
    c = A.ReconstructMeanDWIClassic()
    none = g.copy()
    none[:, 3] = 0.0
    for x in (t, c):
        with pytest.raises(M355Error, match="no gradient"):
            x.draw(none, gen(0))
        with pytest.raises(M355Error, match="rows"):
            x.draw(g, gen(0), num_channels=11)
        with pytest.raises(M355Error, match=r"\[N, 4\]"):
            x.draw(g[:, :3], gen(0))
    zero = g.copy()
    zero[:, :3] = 0.0
    with pytest.raises(M355Error, match="probability zero"):
        t.draw(zero, gen(0))
    for s in (1, 0, -3):
        with pytest.raises(M355Error, match="subset_size"):
            A.ReconstructMeanDWIClassic(subset_size=s)
    with pytest.raises(M355Error, match="num_directions"):
        A.ReconstructMeanDWI(num_dwis=(1, 7), num_directions=1)
    with pytest.raises(M355Error, match="num_dwis"):
        A.ReconstructMeanDWI(num_dwis=(0, 3), num_directions=(1, 3))
    with pytest.raises(M355Error, match="channels"):
        A.MeanDWI([])
    with pytest.raises(M355Error, match="channels"):
        A.MeanDWI([0, -1])
