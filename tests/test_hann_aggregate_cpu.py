"""overlap_mode='hann' without a GPU: the window, the constructor, PatchPredict's plumbing through a CPU ops double
(the window it hands to patch_aggregate_grid, the tile order, the padded tiling and the crop, two gloo ranks) and the
host-side argument checks of the new entry point.  The kernel's arithmetic is tested on the device (test_hann_aggregate_gpu.py)."""
import ctypes
import itertools

import pytest
import torch

import aggregate_ref as AR
from segmentation_pipeline_amd import _lib
from segmentation_pipeline_amd import distributed as D
from segmentation_pipeline_amd.prediction import PatchPredict, grid_axes, hann_window_axes
from test_distributed_cpu import CpuPatchOps, TileModel, _volume, spawn


class CpuGridOps(CpuPatchOps):
    """CpuPatchOps plus the one-pass aggregation with the signature of ops.patch_aggregate_grid; records its calls."""
    calls = []

    @staticmethod
    def patch_aggregate_grid(tiles, axes, volume_shape, border=(0, 0, 0), window=None):
        CpuGridOps.calls.append(window)
        ps = tuple(tiles.shape[2:])
        w0, w1, w2 = window if window is not None else [torch.ones(p) for p in ps]
        assert (w0.numel(), w1.numel(), w2.numel()) == ps
        win = (w0[:, None, None] * w1[None, :, None]) * w2[None, None, :]
        pshape = tuple(v + 2 * b for v, b in zip(volume_shape, border))
        acc, den = torch.zeros((tiles.shape[1],) + pshape), torch.zeros(pshape)
        for t, (i, j, k) in zip(tiles, itertools.product(*axes)):
            acc[:, i:i + ps[0], j:j + ps[1], k:k + ps[2]] += t * win
            den[i:i + ps[0], j:j + ps[1], k:k + ps[2]] += win
        sl = (slice(None),) + tuple(slice(b, b + v) for b, v in zip(border, volume_shape))
        return (acc / den)[sl].contiguous()


def test_hann_window_axes_values():
    for p in (1, 2, 8):
        w = hann_window_axes(p)
        assert len(w) == 3
        for a in w:
            assert a.dtype == torch.float32 and a.device.type == "cpu" and a.shape == (p,)
            assert torch.equal(a, torch.hann_window(p + 2, periodic=False)[1:-1])
            assert (a > 0).all() and (a <= 1).all()
            torch.testing.assert_close(a, a.flip(0), rtol=0, atol=1e-7)     # symmetric
    assert torch.equal(hann_window_axes(1)[0], torch.tensor([1.0]))
    torch.testing.assert_close(hann_window_axes(2)[1], torch.tensor([0.75, 0.75]), rtol=0, atol=1e-7)   # (0.5 - 0.5 cos(2 pi / 3))
    # 0.5 - 0.5 cos(2 pi n / 9), n = 1..8
    n = torch.arange(1, 9, dtype=torch.float64)
    torch.testing.assert_close(hann_window_axes(8)[2].double(), 0.5 - 0.5 * torch.cos(2 * torch.pi * n / 9), rtol=0, atol=1e-7)
    a, b, c = hann_window_axes((3, 1, 5))
    assert (a.numel(), b.numel(), c.numel()) == (3, 1, 5)


def test_overlap_modes_accepted_and_refused():
    assert PatchPredict(patch_size=8, overlap_mode="hann").overlap_mode == "hann"
    assert PatchPredict(patch_size=8, overlap_mode="average").overlap_mode == "average"
    for mode in ("crop", "nonsense"):
        with pytest.raises(NotImplementedError):
            PatchPredict(patch_size=8, overlap_mode=mode)


def test_hann_needs_the_one_pass_backend():
    """the accumulate / finalize fallback serves 'average' only: a backend without patch_aggregate_grid refuses 'hann'"""
    assert not hasattr(CpuPatchOps, "patch_aggregate_grid")
    PatchPredict(patch_size=6, overlap_mode="average", ops_backend=CpuPatchOps)
    with pytest.raises(NotImplementedError, match="patch_aggregate_grid"):
        PatchPredict(patch_size=6, overlap_mode="hann", ops_backend=CpuPatchOps)


@pytest.mark.parametrize("padding_mode", [None, "edge"])
def test_predict_volume_hann_equals_the_reference(padding_mode):
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)   # torch-CPU softmax bits depend on the thread split
    try:
        vol = torch.randn((2, 14, 12, 13), generator=torch.Generator().manual_seed(7))
        ps, ov = (6, 5, 4), (2, 3, 2)
        model = TileModel()
        CpuGridOps.calls.clear()
        pp = PatchPredict(patch_batch_size=2, patch_size=ps, patch_overlap=ov, padding_mode=padding_mode,
                          overlap_mode="hann", ops_backend=CpuGridOps)
        got = pp.predict_volume(model, vol)
        pp.predict_volume(model, vol)
        assert len(CpuGridOps.calls) == 2 and CpuGridOps.calls[0] is CpuGridOps.calls[1], "the window is cached"
        assert all(torch.equal(a, b) for a, b in zip(CpuGridOps.calls[0], AR.hann_axes(ps)))

        vshape = tuple(vol.shape[1:])
        border = tuple(o // 2 for o in ov) if padding_mode else (0, 0, 0)
        pshape = tuple(v + 2 * b for v, b in zip(vshape, border))
        axes = AR.grid_axes(pshape, ps, ov)
        assert axes == grid_axes(pshape, ps, ov)
        locs = list(itertools.product(*axes))
        tiles_in = AR.gather_padded(vol, locs, ps, border, padding_mode)
        with torch.no_grad():
            tiles = torch.cat([model(tiles_in[s:s + 2]) for s in range(0, len(locs), 2)])
        ref = AR.aggregate_windowed(tiles, axes, vshape, border)
        assert got.shape == ref.shape == (3,) + vshape
        assert torch.equal(got, ref)
        # and 'average' through the same double passes no window and gives another volume
        CpuGridOps.calls.clear()
        avg = PatchPredict(patch_batch_size=2, patch_size=ps, patch_overlap=ov, padding_mode=padding_mode,
                           ops_backend=CpuGridOps).predict_volume(model, vol)
        assert CpuGridOps.calls == [None]
        assert not torch.equal(avg, got)
    finally:
        torch.set_num_threads(nthreads)


def _predict_hann_rank0(rank=0, world=1):
    torch.set_num_threads(1)
    pp = PatchPredict(patch_batch_size=2, patch_size=6, patch_overlap=2, overlap_mode="hann", ops_backend=CpuGridOps,
                      result_on="rank0")
    with D.unit_sharding():
        return pp.predict_volume(TileModel(), _volume())


def test_sharded_hann_window_is_bit_identical_to_unsharded():
    """tile sharding and the rank-0 gather run before the blend: two gloo ranks give one process's bits on rank 0"""
    nthreads = torch.get_num_threads()
    single = _predict_hann_rank0()
    torch.set_num_threads(nthreads)
    r0, r1 = spawn(_predict_hann_rank0)
    assert r1 is None and torch.equal(r0, single)


def test_weighted_entry_point_validates_on_the_host():
    """null pointers, non-positive sizes and negative borders are refused before any launch (no GPU needed)"""
    L = _lib.lib()
    p = ctypes.c_void_p(64)
    good = [2, 2, 2, p, p, 3, 8, 8, 8, 4, 4, 4, 0, 0, 0, None]

    def call(tiles=p, starts=p, **kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.m355_patch_aggregate_grid_weighted(tiles, starts, *a)

    for rc in (call(tiles=None), call(starts=None), call(a3=None), call(a4=None)):
        assert rc == -1 and b"patch_aggregate_grid_weighted: null pointer" in L.m355_last_error()
    for idx in (0, 1, 2, 5, 6, 7, 8, 9, 10, 11):
        assert call(**{f"a{idx}": 0}) == -1 and b"patch_aggregate_grid_weighted: bad shape" in L.m355_last_error()
    for idx in (12, 13, 14):
        assert call(**{f"a{idx}": -1}) == -1 and b"patch_aggregate_grid_weighted: bad shape" in L.m355_last_error()
