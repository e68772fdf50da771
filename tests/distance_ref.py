"""Brute-force restatement, in numpy fp64 and without scipy, of what csrc/distance.hip and SurfaceDistanceEvaluator
compute: the squared Euclidean distance to the nearest site as a minimum over ALL sites, the six-neighbour border of a
label and the surface-distance statistics (the medpy conventions).  Small volumes only: the minimum is
O(voxels x sites), chunked over voxels so a case needs tens of MB."""
import numpy as np

STAT_NAMES = ('hd', 'hd95', 'assd', 'asd_pred_to_target', 'asd_target_to_pred', 'nsd', 'pred_surface', 'target_surface')
_CHUNK_ENTRIES = 1 << 21   # voxel x site pairs per chunk (three fp64 temporaries of that size)


def edt_sq(sites, spacing=(1.0, 1.0, 1.0)):
    """fp64 [W, H, D]: min over the voxels s with sites[s] != 0 of sum_a (spacing_a (v_a - s_a))^2; +inf without a site.
    With unit spacing every value is an integer."""
    sites = np.asarray(sites)
    sp = np.asarray(spacing, dtype=np.float64)
    out = np.full(sites.shape, np.inf)
    s = np.argwhere(sites != 0).astype(np.float64)               # [n_sites, 3], index coordinates
    if s.shape[0] == 0:
        return out
    v = np.argwhere(np.ones(sites.shape, dtype=bool)).astype(np.float64)
    flat = out.reshape(-1)
    step = max(1, _CHUNK_ENTRIES // s.shape[0])
    for at in range(0, v.shape[0], step):
        d = (v[at:at + step, None, :] - s[None, :, :]) * sp      # the index difference is exact; one rounding per term
        flat[at:at + step] = (d * d).sum(axis=2).min(axis=1)
    return out


def edt(img, sampling=None):
    """scipy.ndimage.distance_transform_edt's meaning in fp64: distance of every nonzero voxel to the nearest zero voxel"""
    img = np.asarray(img)
    sp = (1.0, 1.0, 1.0) if sampling is None else (sampling,) * 3 if np.isscalar(sampling) else tuple(sampling)
    return np.sqrt(edt_sq(img == 0, sp))


def border(x, value):
    """bool [W, H, D]: x == value and on a face of the volume or with a six-neighbour != value"""
    m = np.asarray(x) == value
    padded = np.pad(m, 1, constant_values=False)
    inside = padded[1:-1, 1:-1, 1:-1].copy()
    for axis in range(3):
        for shift in (-1, 1):
            inside &= np.roll(padded, shift, axis=axis)[1:-1, 1:-1, 1:-1]
    return m & ~inside


def stats(pred, target, value, spacing=(1.0, 1.0, 1.0), percentile=95, tolerance=1.0):
    """{stat: float} of STAT_NAMES for one label value; nan distance stats when either border is empty"""
    bp, bt = border(pred, value), border(target, value)
    out = {k: float("nan") for k in STAT_NAMES}
    out['pred_surface'], out['target_surface'] = float(bp.sum()), float(bt.sum())
    if not bp.any() or not bt.any():
        return out
    a = np.sqrt(edt_sq(bt, spacing))[bp]
    b = np.sqrt(edt_sq(bp, spacing))[bt]
    both = np.concatenate([a, b])
    out['hd'] = float(both.max())
    out['hd95'] = float(np.percentile(both, percentile))
    out['asd_pred_to_target'], out['asd_target_to_pred'] = float(a.mean()), float(b.mean())
    out['assd'] = (out['asd_pred_to_target'] + out['asd_target_to_pred']) / 2
    out['nsd'] = float(((a <= tolerance).sum() + (b <= tolerance).sum()) / both.size)
    return out
