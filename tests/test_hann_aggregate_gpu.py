"""overlap_mode='hann' on the device: m355_patch_aggregate_grid_weighted against the sequential scatter reference
(tests/aggregate_ref.py), bit for bit -- every product, sum and quotient of both is one rounded fp32 operation in the same
order, so a difference means the kernel contracts or reorders -- its ties to the average kernel, the host-side refusals
of ops.patch_aggregate_grid, and PatchPredict(overlap_mode='hann') end to end."""
import itertools

import pytest
import torch

import aggregate_ref as AR

pytestmark = pytest.mark.gpu

GRIDS = [
    ((20, 17, 23), (8, 6, 10), (2, 2, 4), (0, 0, 0)),    # ragged last step on every axis
    ((12, 12, 12), (8, 8, 8), (4, 4, 4), (2, 2, 2)),     # padded and cropped
    ((9, 30, 11), (9, 7, 5), (0, 3, 1), (0, 1, 0)),      # a single-tile axis, odd overlaps, a border on one axis
    ((7, 7, 7), (1, 2, 7), (0, 1, 0), (0, 0, 0)),        # windows of length 1 and 2; 42 tiles
]


def rnd(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _grid(vshape, ps, ov, border):
    pshape = tuple(v + 2 * b for v, b in zip(vshape, border))
    axes = AR.grid_axes(pshape, ps, ov)
    return axes, list(itertools.product(*axes))


@pytest.mark.parametrize("vshape,ps,ov,border", GRIDS, ids=["ragged", "padded", "single_tile_axis", "short_windows"])
def test_weighted_kernel_equals_the_sequential_reference(vshape, ps, ov, border):
    from segmentation_pipeline_amd import ops
    from segmentation_pipeline_amd.prediction import grid_axes, hann_window_axes
    axes, locs = _grid(vshape, ps, ov, border)
    assert axes == grid_axes(tuple(v + 2 * b for v, b in zip(vshape, border)), ps, ov)
    tiles = rnd(len(locs), 3, *ps, seed=4)
    window = hann_window_axes(ps)
    assert all(torch.equal(a, b) for a, b in zip(window, AR.hann_axes(ps)))
    got = ops.patch_aggregate_grid(tiles.cuda(), axes, vshape, border, window=window)
    ref = AR.aggregate_windowed(tiles, axes, vshape, border)
    assert got.shape == ref.shape == (3,) + vshape and torch.isfinite(ref).all()
    diff = (got.cpu() - ref).abs().max().item()
    print(f"hann aggregate {vshape} patch {ps}: {len(locs)} tiles, max |kernel - reference| = {diff:.3e}")
    assert torch.equal(got.cpu(), ref)


def test_weighted_kernel_properties():
    """on the ragged grid: constant tiles come back within 4 ulp (a voxel under one tile is (t * w) / w, not t), the
    blend is not the average, and an all-ones window gives the average kernel's bits (the sum of ones is the count);
    seven channels cross the kernel's register group of four"""
    from segmentation_pipeline_amd import ops
    from segmentation_pipeline_amd.prediction import hann_window_axes
    vshape, ps, ov, border = GRIDS[0]
    axes, locs = _grid(vshape, ps, ov, border)
    window = hann_window_axes(ps)
    consts = torch.tensor([0.7, -1.3, 3.0, 1e-3, 5.0, -0.11, 129.7])
    tiles = consts.view(1, 7, 1, 1, 1).expand(len(locs), 7, *ps).contiguous().cuda()
    got = ops.patch_aggregate_grid(tiles, axes, vshape, border, window=window).cpu()
    want = consts.view(7, 1, 1, 1).expand_as(got)
    ulp = (torch.nextafter(consts.abs(), torch.tensor(float("inf"))) - consts.abs()).view(7, 1, 1, 1)
    worst = ((got - want).abs() / ulp).max().item()
    print(f"constant tiles: worst error {worst:.2f} ulp")
    assert worst <= 4.0

    tiles = rnd(len(locs), 7, *ps, seed=5).cuda()
    hann = ops.patch_aggregate_grid(tiles, axes, vshape, border, window=window)
    avg = ops.patch_aggregate_grid(tiles, axes, vshape, border)
    assert torch.equal(hann[:3].cpu(), AR.aggregate_windowed(tiles[:, :3].contiguous(), axes, vshape, border))
    assert torch.equal(hann[3:].cpu(), AR.aggregate_windowed(tiles[:, 3:].contiguous(), axes, vshape, border))
    assert not torch.equal(hann, avg) and (hann - avg).abs().max().item() > 1e-3
    ones = ops.patch_aggregate_grid(tiles, axes, vshape, border, window=[torch.ones(p) for p in ps])
    assert torch.equal(ones, avg)
    # and on the padded, cropped grid
    vshape, ps, ov, border = GRIDS[1]
    axes, locs = _grid(vshape, ps, ov, border)
    tiles = rnd(len(locs), 2, *ps, seed=6).cuda()
    assert torch.equal(ops.patch_aggregate_grid(tiles, axes, vshape, border, window=[torch.ones(p) for p in ps]),
                       ops.patch_aggregate_grid(tiles, axes, vshape, border))


def test_misuse_is_refused_on_the_host(monkeypatch):
    """a window of the wrong length and a tile count that does not match the grid raise before the library is touched:
    every native entry point is replaced by one that fails the test"""
    from segmentation_pipeline_amd import _lib, ops
    from segmentation_pipeline_amd.prediction import hann_window_axes
    vshape, ps, ov, border = GRIDS[1]
    axes, locs = _grid(vshape, ps, ov, border)
    tiles = rnd(len(locs), 2, *ps, seed=7).cuda()
    torch.cuda.synchronize()

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")

    monkeypatch.setattr(_lib, "lib", lambda: NoLaunch())
    with pytest.raises(_lib.M355Error, match="window lengths"):
        ops.patch_aggregate_grid(tiles, axes, vshape, border, window=hann_window_axes((8, 8, 7)))
    with pytest.raises(_lib.M355Error, match="three 1-D float32"):
        ops.patch_aggregate_grid(tiles, axes, vshape, border, window=hann_window_axes(8)[:2])
    with pytest.raises(_lib.M355Error, match="three 1-D float32"):
        ops.patch_aggregate_grid(tiles, axes, vshape, border, window=[w.double() for w in hann_window_axes(8)])
    with pytest.raises(_lib.M355Error, match="tiles for a"):
        ops.patch_aggregate_grid(tiles[:-1], axes, vshape, border, window=hann_window_axes(8))
    with pytest.raises(AssertionError, match="was reached"):     # the stand-in does catch a call that goes through
        ops.patch_aggregate_grid(tiles, axes, vshape, border, window=hann_window_axes(8))


@pytest.fixture(scope="module")
def unet_and_volume():
    from segmentation_pipeline_amd.models import ModularUNet
    torch.manual_seed(0)
    model = ModularUNet(2, 3, [8, 16], 2).cuda().eval()
    return model, rnd(2, 20, 12, 16, seed=11).cuda()


@pytest.fixture(scope="module")
def hann_reference(unet_and_volume):
    """padding_mode -> the reference blend of the model's own tile outputs (same tile batching: batches of 4)"""
    from segmentation_pipeline_amd import ops
    model, vol = unet_and_volume
    cache = {}

    def get(padding_mode):
        if padding_mode not in cache:
            ps, ov, vshape = (8, 8, 8), (4, 4, 4), tuple(vol.shape[1:])
            border = (2, 2, 2) if padding_mode is not None else (0, 0, 0)
            axes, locs = _grid(vshape, ps, ov, border)
            outs = []
            with torch.no_grad():
                for s in range(0, len(locs), 4):
                    loc = torch.tensor(locs[s:s + 4], dtype=torch.int32, device="cuda")
                    tin = ops.patch_gather(vol, loc, ps) if padding_mode is None else \
                        ops.patch_gather_padded(vol, loc, ps, border, padding_mode)
                    outs.append(model(tin))
            cache[padding_mode] = AR.aggregate_windowed(torch.cat(outs).cpu(), axes, vshape, border)
        return cache[padding_mode]
    return get


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("padding_mode", [None, "edge"])
def test_patch_predict_hann_end_to_end(unet_and_volume, hann_reference, padding_mode, graph):
    from segmentation_pipeline_amd.prediction import PatchPredict
    model, vol = unet_and_volume
    ref = hann_reference(padding_mode)
    timings = {}
    pp = PatchPredict(patch_size=8, patch_overlap=4, overlap_mode="hann", patch_batch_size=4, padding_mode=padding_mode,
                      graph=graph, timings=timings)
    got = pp.predict_volume(model, vol)
    assert got.shape == ref.shape == (3, 20, 12, 16)
    diff = (got.cpu() - ref).abs().max().item()
    print(f"hann end to end (padding {padding_mode}, graph {graph}): max |predicted - reference| = {diff:.3e}")
    assert torch.equal(got.cpu(), ref)
    assert "aggregate" in timings and "accumulate" not in timings
    assert (got.sum(0) - 1).abs().max().item() < 1e-5            # a blend of softmax outputs is a distribution
    avg = PatchPredict(patch_size=8, patch_overlap=4, patch_batch_size=4, padding_mode=padding_mode).predict_volume(model, vol)
    assert not torch.equal(avg, got)
    batch = pp.predict(model, torch.device("cuda"), {"X": vol[None]})
    assert torch.equal(batch["y_pred"][0].cpu(), ref)
