"""Writes the surface-distance fixture: small prediction / target label maps with two labels, and scipy's fp64 answers
for them -- the six-neighbour borders (mask ^ binary_erosion), scipy.ndimage.distance_transform_edt of the inverted
borders and the statistics of evaluators.SurfaceDistanceEvaluator (the medpy conventions: DESIGN §4.20) computed from
those with numpy.  Nothing of this project's code runs here; tests/distance_ref.py and the device code are checked
against the file.

    python tools/gen_golden_surface_distance.py   # writes tests/golden/surface_distance.npz + MANIFEST_surface_distance.txt
"""
import os

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")
SEED = 20261019
LABELS = {"inner": 1, "outer": 2}
STAT_NAMES = ('hd', 'hd95', 'assd', 'asd_pred_to_target', 'asd_target_to_pred', 'nsd', 'pred_surface', 'target_surface')
PERCENTILE, TOLERANCE = 95, 1.0
# (shape, spacing, label missing from the prediction or None)
CASES = [((5, 7, 9), (1.0, 1.0, 1.0), None),
         ((12, 10, 9), (0.5, 1.0, 2.5), None),
         ((9, 33, 17), (1.2, 0.7, 3.0), None),
         ((3, 2, 70), (1.0, 1.0, 1.0), 2),
         ((67, 3, 5), (0.5, 1.0, 2.5), None),
         ((2, 130, 3), (1.2, 0.7, 3.0), 1)]


def blob(shape, rng, jitter):
    """an ellipsoid of label 2 around a smaller one of label 1, centre and radii drawn per call"""
    grid = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), axis=-1).astype(np.float64)
    size = np.asarray(shape, dtype=np.float64)
    centre = (size - 1) / 2 + rng.uniform(-jitter, jitter, 3) * size
    radius = size * rng.uniform(0.28, 0.42, 3) + 0.5
    r2 = (((grid - centre) / radius) ** 2).sum(axis=-1)
    out = np.zeros(shape, dtype=np.int16)
    out[r2 <= 1.0] = 2
    out[r2 <= 0.3] = 1
    return out


def border(mask):
    return mask ^ ndimage.binary_erosion(mask, ndimage.generate_binary_structure(3, 1), border_value=0)


def stats(bp, bt, to_t, to_p):
    out = np.full(len(STAT_NAMES), np.nan)
    out[6], out[7] = bp.sum(), bt.sum()
    if bp.any() and bt.any():
        a, b = to_t[bp], to_p[bt]
        both = np.concatenate([a, b])
        out[0], out[1] = both.max(), np.percentile(both, PERCENTILE)
        out[3], out[4] = a.mean(), b.mean()
        out[2] = (out[3] + out[4]) / 2
        out[5] = ((a <= TOLERANCE).sum() + (b <= TOLERANCE).sum()) / both.size
    return out


def main():
    rng = np.random.default_rng(SEED)
    out = {"seed": np.asarray(SEED), "label_names": np.asarray(list(LABELS)), "label_values": np.asarray(list(LABELS.values())),
           "stat_names": np.asarray(STAT_NAMES), "percentile": np.asarray(PERCENTILE), "tolerance": np.asarray(TOLERANCE),
           "cases": np.asarray(len(CASES))}
    for c, (shape, spacing, missing) in enumerate(CASES):
        target, pred = blob(shape, rng, 0.05), blob(shape, rng, 0.12)
        if missing is not None:
            pred[pred == missing] = 0
        out[f"{c}.target"], out[f"{c}.pred"], out[f"{c}.spacing"] = target, pred, np.asarray(spacing, dtype=np.float64)
        for name, v in LABELS.items():
            bp, bt = border(pred == v), border(target == v)
            out[f"{c}.{name}.border_pred"], out[f"{c}.{name}.border_target"] = bp, bt
            # distance_transform_edt of a volume without a zero is undefined: stored only where the border exists
            to_t = ndimage.distance_transform_edt(~bt, sampling=spacing) if bt.any() else None
            to_p = ndimage.distance_transform_edt(~bp, sampling=spacing) if bp.any() else None
            if to_t is not None:
                out[f"{c}.{name}.edt_to_target"] = to_t
            if to_p is not None:
                out[f"{c}.{name}.edt_to_pred"] = to_p
            out[f"{c}.{name}.stats"] = stats(bp, bt, to_t, to_p)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "surface_distance.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(OUT, "MANIFEST_surface_distance.txt"), "w") as f:
        f.write("surface_distance.npz: written by tools/gen_golden_surface_distance.py with scipy.ndimage (binary_erosion, "
                "distance_transform_edt) and numpy; none of this project's code runs there.\n")
        for k in sorted(out):
            f.write(f"{k} {out[k].dtype} {tuple(out[k].shape)}\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
