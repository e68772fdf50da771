"""Connected components and post-processing on the device against the reference's results
(tests/golden/postprocessing.npz, tools/gen_golden_postprocessing.py), hand-built edge cases and, where scipy is
installed, an in-test scipy restatement on random maps."""
import numpy as np
import pytest
import torch

from segmentation_pipeline_amd import evaluators as E
from segmentation_pipeline_amd import post_processing as PP

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _label(img, conn):
    out, n = PP.label(img, connectivity=conn, return_num=True)
    assert out.dtype == np.int64 and out.shape == img.shape
    return out, n


# ------------------------------------------------------------------------------------------------ label
@pytest.mark.parametrize("case", ["hippo", "lesion"])
@pytest.mark.parametrize("conn", [1, 2, 3])
def test_label_golden(golden, case, conn):
    g = golden("postprocessing.npz")
    img = g[f"{case}/img"]
    out, n = _label(img, conn)
    assert n == int(g[f"{case}/n{conn}"])
    np.testing.assert_array_equal(out, g[f"{case}/label{conn}"].astype(np.int64))
    # device input stays on the device, same result
    t = torch.from_numpy(img).to(DEV)
    td, tn = PP.label(t, connectivity=conn, return_num=True)
    assert td.is_cuda and tn == n
    np.testing.assert_array_equal(td.cpu().numpy(), out)


def test_label_default_connectivity_is_full(golden):
    g = golden("postprocessing.npz")
    np.testing.assert_array_equal(PP.label(g["hippo/img"]), g["hippo/label3"].astype(np.int64))


@pytest.mark.parametrize("conn", [1, 2, 3])
def test_label_trivial_volumes(conn):
    z = np.zeros((9, 10, 70), np.int32)
    out, n = _label(z, conn)
    assert n == 0 and not out.any()
    full = np.full((9, 10, 70), 3, np.uint8)
    out, n = _label(full, conn)
    assert n == 1 and (out == 1).all()
    one = np.zeros((17, 33, 65), bool)
    one[16, 32, 64] = True
    out, n = _label(one, conn)
    assert n == 1 and out[16, 32, 64] == 1 and out.sum() == 1


def test_label_diagonal_contacts():
    img = np.zeros((4, 4, 4), np.int32)
    img[0, 0, 0] = img[1, 1, 1] = 1      # corner contact: 26-connected only
    img[0, 2, 2] = img[0, 3, 3] = 2      # edge contact: 18- and 26-connected
    img[3, 0, 0] = img[3, 0, 1] = 5      # face contact: always connected
    img[3, 3, 3] = 7
    img[2, 3, 3] = 6                     # face contact but another value: never connected
    expect = {1: 7, 2: 6, 3: 5}
    for conn, n_expect in expect.items():
        out, n = _label(img, conn)
        assert n == n_expect, (conn, n)
    out, _ = _label(img, 3)
    assert out[0, 0, 0] == out[1, 1, 1] == 1 and out[0, 2, 2] == out[0, 3, 3] == 2
    assert out[2, 3, 3] != out[3, 3, 3]


def test_label_d1_and_raster_numbering():
    img = np.zeros((1, 5, 130), np.int32)
    img[0, 4, 0] = 1          # first in raster order of its component: numbered after the one below
    img[0, 0, 129] = 1
    img[0, 1, 5:120] = 2      # crosses the 64-wide tile boundary
    out, n = _label(img, 1)
    assert n == 3
    assert out[0, 0, 129] == 1 and out[0, 1, 5] == 2 and (out[0, 1, 5:120] == 2).all() and out[0, 4, 0] == 3


@pytest.mark.parametrize("conn", [1, 3])
def test_label_serpentine_across_many_tiles(conn):
    # one 6-connected path that snakes through every row of every plane: long merge chains across tiles
    D, H, W = 20, 34, 150
    img = np.zeros((D, H, W), np.uint8)
    for z in range(0, D, 2):
        img[z, 0::2, :] = 1                       # every even row
        img[z, 1::4, W - 1] = 1                   # joined alternately at the right ...
        img[z, 3::4, 0] = 1                       # ... and at the left end
        img[z + 1, 0, 0] = 1                      # and the plane to the next one
    out, n = _label(img, conn)
    assert n == 1
    np.testing.assert_array_equal(out, img.astype(np.int64))


def test_label_spiral():
    # a square spiral in every plane, planes joined at the centre: one component; the gaps are background
    sp = pytest.importorskip("scipy.ndimage")
    D, N = 6, 101
    img = np.zeros((D, N, N), np.int16)
    for z in range(D):
        lo, hi = 0, N - 1
        while lo + 2 <= hi:
            img[z, lo, lo:hi + 1] = 4                  # top, right, bottom, left of the ring ...
            img[z, lo:hi + 1, hi] = 4
            img[z, hi, lo:hi + 1] = 4
            img[z, lo + 2:hi + 1, lo] = 4              # ... open at its top-left corner
            img[z, lo + 2, lo:lo + 3] = 4              # into the next ring inwards
            lo, hi = lo + 2, hi - 2
    img[:, N // 2, N // 2] = 4
    out, n = _label(img, 1)
    ref, rn = sp.label(img != 0, structure=sp.generate_binary_structure(3, 1))
    assert n == rn
    np.testing.assert_array_equal(out, ref)


# ---------------------------------------------------------------------------- post-processing vs golden
CASES = [
    ("hippo/holes64", "hippo/img", "remove_holes", (64,), {}),
    ("hippo/chain_keep", "hippo/holes64/out", "keep_components", None, {}),
    ("hippo/keep3", "hippo/img", "keep_components", (3,), {}),
    ("hippo/small3", "hippo/img", "remove_small_components", (3,), {}),
    ("hippo/keep1_md2", "hippo/img", "keep_components", (1,), {"max_dilations": 2}),
    ("hippo/holes2000_md2", "hippo/img", "remove_holes", (2000,), {"max_dilations": 2}),
    ("hippo/keep_many", "hippo/holes64/out", "keep_components", (100000,), {}),
    ("lesion/holes64", "lesion/img", "remove_holes", (64,), {}),
    ("lesion/small3", "lesion/holes64/out", "remove_small_components", (3,), {}),
    ("lesion/small40", "lesion/img", "remove_small_components", (40,), {}),
    ("lesion/keep5", "lesion/img", "keep_components", (5,), {}),
]


@pytest.mark.parametrize("tag,src,fn,args,kw", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("kind", ["numpy", "device"])
def test_post_processing_golden(golden, tag, src, fn, args, kw, kind):
    g = golden("postprocessing.npz")
    img = g[src].copy()
    if args is None:   # the dmri_hippo chain: keep as many components as the largest class value
        args = (int(img.max()),)
    before = img.copy()
    x = img if kind == "numpy" else torch.from_numpy(img).to(DEV)
    res = getattr(PP, fn)(x, *args, **kw)
    out = res[0]
    if kind == "numpy":
        assert isinstance(out, np.ndarray) and out.dtype == img.dtype
        np.testing.assert_array_equal(img, before)
    else:
        assert out.is_cuda and out.dtype == torch.uint8
        np.testing.assert_array_equal(x.cpu().numpy(), before)
        out = out.cpu().numpy()
    np.testing.assert_array_equal(out, g[f"{tag}/out"])
    assert [int(c) for c in res[1:]] == g[f"{tag}/counts"].tolist()


@pytest.mark.parametrize("dtype", [np.bool_, np.int8, np.int16, np.int32, np.int64])
def test_dtypes_round_trip(golden, dtype):
    g = golden("postprocessing.npz")
    img = g["lesion/img"].astype(dtype)
    out, cnt = PP.remove_holes(img, 64)
    assert out.dtype == img.dtype and cnt == int(g["lesion/holes64/counts"][0])
    np.testing.assert_array_equal(out.astype(np.uint8), g["lesion/holes64/out"])
    out, cnt = PP.remove_small_components(img, 40)
    assert out.dtype == img.dtype
    np.testing.assert_array_equal(out.astype(np.uint8), g["lesion/small40/out"])


@pytest.mark.parametrize("kind", ["numpy", "device"])
def test_keep_components_with_the_maps_own_max(golden, kind):
    # the reference's callers pass label_data.max(): a uint8 scalar (numpy) or a 0-d uint8 tensor (device); the counts
    # must be Python ints computed as in the reference, not in uint8 (726 - 1 - 3 overflows it)
    g = golden("postprocessing.npz")
    img = g["hippo/holes64/out"]
    assert img.dtype == np.uint8
    x = img if kind == "numpy" else torch.from_numpy(img).to(DEV)
    out, comps, elems = PP.keep_components(x, x.max())
    assert type(comps) is int and type(elems) is int
    assert [comps, elems] == g["hippo/chain_keep/counts"].tolist()
    np.testing.assert_array_equal(out if kind == "numpy" else out.cpu().numpy(), g["hippo/chain_keep/out"])
    # more components asked for than exist: a negative count, not a wrapped uint8
    small = np.zeros((4, 4, 4), np.uint8)
    small[0, 0, 0] = 1
    small[3, 3, 3] = 2
    xs = small if kind == "numpy" else torch.from_numpy(small).to(DEV)
    three = np.uint8(3) if kind == "numpy" else torch.tensor(3, dtype=torch.uint8, device=DEV)
    _, comps, elems = PP.keep_components(xs, three)
    assert (comps, elems) == (-1, 0)


@pytest.mark.parametrize("shape", [(600_000, 1, 1), (1, 600_000, 1), (2, 530_000, 2)])
def test_label_long_thin_volumes(shape):
    # more than 65536 tiles along z or y (8-voxel tile edges there)
    img = np.zeros(shape, np.uint8)
    flat = img.reshape(-1)
    flat[::3] = 1
    out, n = _label(img, 1)
    if shape[2] == 1:   # every third voxel along one line: isolated voxels, numbered in order
        assert n == flat[::3].size
        np.testing.assert_array_equal(out.reshape(-1)[::3], np.arange(1, n + 1))
        assert not out.reshape(-1)[1::3].any() and not out.reshape(-1)[2::3].any()
    else:
        sp = pytest.importorskip("scipy.ndimage")
        ref, rn = sp.label(img, structure=sp.generate_binary_structure(3, 1))
        assert n == rn
        np.testing.assert_array_equal(out, ref)


def test_cpu_tensor_comes_back_on_the_cpu(golden):
    g = golden("postprocessing.npz")
    t = torch.from_numpy(g["hippo/img"])
    out, removed, elems = PP.keep_components(t, 3)
    assert not out.is_cuda
    np.testing.assert_array_equal(out.numpy(), g["hippo/keep3/out"])


# ---------------------------------------------------------------------------- lesion-wise detection
@pytest.mark.parametrize("tag", ["pair0", "pair1", "pair2_empty_pred"])
def test_instance_stats_golden(golden, tag):
    g = golden("postprocessing.npz")
    names = [str(s) for s in g["stat_names"]]
    assert tuple(names) == E.STAT_NAMES
    for kind in ("numpy", "device"):
        p, t = g[f"{tag}/pred"], g[f"{tag}/target"]
        if kind == "device":
            p, t = torch.from_numpy(p).to(DEV)[None], torch.from_numpy(t).to(DEV)[None]
        stats = E.instance_segmentation_stats(p, t)
        got = np.array([float(stats[k]) for k in names])
        np.testing.assert_array_equal(got, g[f"{tag}/stats"])


def test_overlap_histogram_golden(golden):
    g = golden("postprocessing.npz")
    for tag in ("pair0", "pair1"):
        tl = PP.label(g[f"{tag}/target"] > 0, connectivity=2)
        pl = PP.label(torch.from_numpy(g[f"{tag}/pred"] > 0).to(DEV), connectivity=2)
        h = E.overlap_histogram(torch.from_numpy(tl).to(DEV), pl)
        assert h.is_cuda and h.dtype == torch.int64
        np.testing.assert_array_equal(h.cpu().numpy().astype(np.float32), g[f"{tag}/hist"])
        hn = E.overlap_histogram(tl, pl.cpu().numpy())
        assert isinstance(hn, np.ndarray)
        np.testing.assert_array_equal(hn, h.cpu().numpy())


def test_overlap_table_cap(monkeypatch, golden):
    g = golden("postprocessing.npz")
    monkeypatch.setattr(E, "MAX_OVERLAP_ENTRIES", 16)
    with pytest.raises(Exception, match="MAX_OVERLAP_ENTRIES"):
        E.instance_segmentation_stats(g["pair0/pred"], g["pair0/target"])


# ---------------------------------------------------------------------------- random maps vs scipy
def _sp_label(img, conn):
    import scipy.ndimage as ndi
    st = ndi.generate_binary_structure(3, conn)
    out = np.zeros(img.shape, np.int64)
    n = 0
    for v in np.unique(img):
        if v == 0:
            continue
        lab, k = ndi.label(img == v, structure=st)
        out[lab > 0] = lab[lab > 0] + n
        n += k
    if n:
        ids, first = np.unique(out.ravel(), return_index=True)
        keep = ids != 0
        remap = np.zeros(n + 1, np.int64)
        remap[ids[keep][np.argsort(first[keep], kind="stable")]] = np.arange(1, keep.sum() + 1)
        out = remap[out]
    return out, n


def _sp_remove_holes(img, hole_size, max_dilations=100):
    import scipy.ndimage as ndi
    img = img.copy()
    total = 0
    cross = ndi.generate_binary_structure(3, 1)
    for it in range(max_dilations):
        lab, _ = ndi.label(~(img > 0), structure=cross)
        small = np.bincount(lab.ravel()) < hole_size
        small[0] = False
        holes = small[lab]
        if it == 0:
            total = int(holes.sum())
        if not holes.any():
            break
        img[holes] = ndi.grey_dilation(img, footprint=cross)[holes]
    return img, total


def _sp_keep_components(img, num, max_dilations=100):
    import scipy.ndimage as ndi
    cross = ndi.generate_binary_structure(3, 1)
    img = img.copy()
    comps = elems = 0
    for it in range(max_dilations):
        lab, _ = _sp_label(img, 3)
        ids, cnt = np.unique(lab, return_counts=True)
        rank = np.empty(ids.max() + 1, np.int64)
        rank[ids[np.argsort(cnt, kind="stable")[::-1]]] = np.arange(ids.size)
        keep = rank[lab] <= num
        if it == 0:
            elems, comps = int((~keep).sum()), ids.size - 1 - num
        if keep.all():
            break
        cls, ccnt = np.unique(img, return_counts=True)
        order = np.argsort(ccnt, kind="stable")
        crank = np.zeros(int(cls.max()) + 1, np.int64)
        crank[cls[order]] = np.arange(cls.size)
        key = crank[img] * keep
        dil = ndi.grey_dilation(key, footprint=cross)
        change = (dil != key) & ~keep
        img[change] = cls[order][dil[change]]
    return img, comps, elems


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_maps_against_scipy(seed):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(seed)
    shape = [(17, 33, 65), (9, 70, 130), (40, 12, 5)][seed]
    f = ndi.gaussian_filter(rng.standard_normal(shape), 1.2)
    img = np.digitize(f, np.quantile(f, [0.3, 0.6, 0.85])).astype(np.int32)
    img[rng.random(shape) < 0.02] = 0
    for conn in (1, 2, 3):
        out, n = _label(img, conn)
        ref, rn = _sp_label(img, conn)
        assert n == rn
        np.testing.assert_array_equal(out, ref)
    got, cnt = PP.remove_holes(img, 20)
    ref, rcnt = _sp_remove_holes(img, 20)
    assert cnt == rcnt
    np.testing.assert_array_equal(got, ref)
    got, cnt = PP.remove_small_components(img, 5)
    rh, rcnt = _sp_remove_holes((img == 0), 5)
    ref = img.copy()
    ref[rh] = 0
    assert cnt == rcnt
    np.testing.assert_array_equal(got, ref)
    for num in (2, 7):
        got, c, e = PP.keep_components(img, num)
        ref, rc, re = _sp_keep_components(img, num)
        assert (c, e) == (rc, re)
        np.testing.assert_array_equal(got, ref)
