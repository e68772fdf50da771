"""Reference for the windowed overlap blend of a sliding window (torchio GridAggregator('hann')), in plain torch and
in torchio's sequential scatter form: per tile, in GridSampler order, `out[...] += patch * win3; mask[...] += win3`
on the (virtually padded) volume, then `out / mask`, then the crop of the border.  Every step is one rounded fp32
operation, which is what the one-pass kernel is held to bit for bit."""
import itertools

import numpy as np
import torch


def hann_axes(patch_size):
    """per axis torch.hann_window(p + 2, periodic=False)[1:-1]: p strictly positive fp32 values"""
    return [torch.hann_window(p + 2, periodic=False, dtype=torch.float32)[1:-1] for p in patch_size]


def grid_axes(pshape, patch_size, overlap):
    """GridSampler's per-axis start lists: steps of patch - overlap, the last tile shifted back to end at the border"""
    axes = []
    for size, p, o in zip(pshape, patch_size, overlap):
        starts = list(range(0, size - p + 1, p - o))
        if starts[-1] != size - p:
            starts.append(size - p)
        axes.append(starts)
    return axes


def aggregate_windowed(tiles, axes, vshape, border=(0, 0, 0), window=None):
    """tiles [P, C, *patch] (CPU fp32) in itertools.product order over `axes` (padded coordinates) -> [C, *vshape];
    window: three 1-D fp32 tensors (default: the Hann window of the patch size)"""
    tiles = tiles.detach().cpu()
    ps = tuple(tiles.shape[2:])
    w0, w1, w2 = hann_axes(ps) if window is None else [w.detach().cpu() for w in window]
    win3 = (w0[:, None, None] * w1[None, :, None]) * w2[None, None, :]
    pshape = tuple(v + 2 * b for v, b in zip(vshape, border))
    out = torch.zeros((tiles.shape[1],) + pshape, dtype=torch.float32)
    mask = torch.zeros(pshape, dtype=torch.float32)
    locs = list(itertools.product(*axes))
    assert len(locs) == tiles.shape[0]
    for patch, (i, j, k) in zip(tiles, locs):
        out[:, i:i + ps[0], j:j + ps[1], k:k + ps[2]] += patch * win3
        mask[i:i + ps[0], j:j + ps[1], k:k + ps[2]] += win3
    out = out / mask
    return out[:, border[0]:border[0] + vshape[0], border[1]:border[1] + vshape[1],
               border[2]:border[2] + vshape[2]].contiguous()


def gather_padded(volume, locs, ps, border, mode):
    """the tiles of `volume` [C, *vshape] (CPU) at `locs` (padded coordinates); mode: None or a numpy.pad mode"""
    v = volume.detach().cpu()
    if mode is not None:
        v = torch.from_numpy(np.pad(v.numpy(), ((0, 0),) + tuple((b, b) for b in border), mode=mode))
    return torch.stack([v[:, i:i + ps[0], j:j + ps[1], k:k + ps[2]] for i, j, k in locs])
