"""Plain numpy / torch-CPU restatement of ops.region_stats (csrc/region_stats.hip) and of the reference's
bounding-box views: fp64 two-pass mean and unbiased std rounded to float32 once, np.sort for the rank (n - 1) // 2
median, np.where bounds.  Also a stand-in for ops.region_stats on host tensors, so the host logic of
ImageRegionEvaluator and of the dataset fingerprint runs without a GPU."""
import numpy as np
import torch

STATS = ('mean', 'std', 'median', 'min', 'max')


def as_numpy(t):
    """a tensor's values as numpy; 16-bit floats widened to float32 (exact)"""
    if torch.is_tensor(t):
        t = t.detach().cpu()
        if t.dtype in (torch.bfloat16, torch.float16):
            t = t.float()
        return t.numpy()
    return np.asarray(t)


def region_masks(labels, values):
    """[L + 2] boolean masks of a label volume [W, H, D]: `data == value` with the value cast to the map's type (a
    value given twice gives the same mask twice); then data != 0 and every voxel"""
    lab = as_numpy(labels)
    lab = lab.reshape(lab.shape[-3:])
    masks = []
    for v in values:
        with np.errstate(over="ignore"):
            cast = np.asarray(int(v), dtype=np.int64).astype(lab.dtype)
        masks.append(lab == cast)
    masks.append(lab != 0)
    masks.append(np.ones(lab.shape, dtype=bool))
    return masks


def stats5(x):
    """float32 (mean, std, median, min, max) of the float32 values x as region_stats defines them"""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = x.size
    nan = np.float32(np.nan)
    if n == 0 or np.isnan(x).any():
        return np.full(5, nan, dtype=np.float32)
    with np.errstate(all="ignore"):
        x64 = x.astype(np.float64)
        mean = x64.sum() / n
        std = np.sqrt(((x64 - mean) ** 2).sum() / (n - 1)) if n > 1 else np.nan
    return np.array([np.float32(mean), np.float32(std), np.sort(x)[(n - 1) // 2], x.min(), x.max()], dtype=np.float32)


def region_stats_ref(labels, images, values, median=True):
    """-> count int64 [R], bounds int32 [R, 6], stats float32 [R, K, 5]; images: [C, W, H, D] (or [W, H, D]) each"""
    masks = region_masks(labels, values)
    shape = masks[0].shape
    R, K = len(masks), len(images)
    count = np.zeros(R, dtype=np.int64)
    bounds = np.zeros((R, 6), dtype=np.int32)
    stats = np.zeros((R, K, 5), dtype=np.float32)
    ims = []
    for im in images:
        im = as_numpy(im).astype(np.float32)
        ims.append(im.reshape((-1,) + shape))
    for r, m in enumerate(masks):
        count[r] = m.sum()
        where = np.where(m)
        for a in range(3):
            bounds[r, 2 * a] = where[a].min() if count[r] else shape[a]
            bounds[r, 2 * a + 1] = where[a].max() if count[r] else -1
        for k, im in enumerate(ims):
            stats[r, k] = stats5(im[:, m])
            if not median:
                stats[r, k, 2] = np.nan
    return count, bounds, stats


def bounds_views(mask):
    """the reference's get_bounds on a boolean volume, restated: extents, crop, size, center"""
    out = {"extents": [], "crop": [], "size": [], "center": []}
    for axis, w in enumerate(np.where(as_numpy(mask))):
        lo, hi = int(w.min()), int(w.max())
        out["extents"] += [lo, hi]
        out["crop"] += [lo, mask.shape[axis] - hi]
        out["size"].append(hi - lo)
        out["center"].append((hi + lo) / 2)
    return out


def ordered(a):
    """float32 -> int64 keys whose differences count representable values between two floats (-0 and +0 coincide)"""
    i = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def ulp_distance(a, b):
    """elementwise distance in float32 ulps; 0 where both are NaN or the same infinity, a large number where only one
    of the two is NaN or infinite"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    d = np.abs(ordered(a) - ordered(b))
    special = ~(np.isfinite(a) & np.isfinite(b))
    same = (np.isnan(a) & np.isnan(b)) | (a == b)
    return np.where(special, np.where(same, 0, 1 << 40), d)


def same_values(a, b):
    """a == b elementwise with NaN equal to NaN (the sign of a zero is not compared)"""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------- ops.region_stats stand-in
def stub_region_stats(labels, images, values, median=True, result=None, workspace=None):
    """ops.region_stats's three calling forms on host tensors, computed by region_stats_ref"""
    from segmentation_pipeline_amd.ops import RegionStats

    def one(lab, ims, vals):
        c, b, s = region_stats_ref(lab, list(ims), [int(v) for v in vals], median)
        return RegionStats(torch.from_numpy(c), torch.from_numpy(b), torch.from_numpy(s))

    if torch.is_tensor(labels):
        return one(labels, images, values)
    values = list(values)
    if values and isinstance(values[0], (list, tuple)):
        return [one(lab, ims, vals) for lab, ims, vals in zip(labels, images, values)]
    per = [one(lab, ims, values) for lab, ims in zip(labels, images)]
    return RegionStats(*(torch.stack(f) for f in zip(*per)))
