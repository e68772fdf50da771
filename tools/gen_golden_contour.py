"""Generate tests/golden/contour.npz from the REAL reference contour evaluator.

Runs the reference's evaluators/contour_image_evaluator.py, transforms/find_interesting_slice.py and
utils/utils.py (slice_volume) unchanged.  Stubbed, in the manner of tools/gen_golden_evaluation.py: torchio
(tio.Transform, tio.LabelMap), the Evaluator base class, the package's typing module, matplotlib.cm.get_cmap (gone from
current matplotlib; the pictures are not stored) and torchvision.utils.make_grid, restated here:

    N tiles of h x w, nrow = ncol, padding 1:  xmaps = min(ncol, N), ymaps = ceil(N / xmaps); the grid is
    (ymaps * (h + 1) + 1) x (xmaps * (w + 1) + 1) filled with pad_value, tile k at rows (k // xmaps) * (h + 1) + 1 ...,
    columns (k % xmaps) * (w + 1) + 1 ...; a single tile comes back bare.

Only data is stored: the input volumes, the label values, each case's arguments (as JSON), and per get_image call the
resolved plane, the slice id of every subject and the three mosaics, captured by wrapping slice_and_make_grid and
get_slice_id.  No rendered pixels (they depend on the matplotlib and font build).

The reference ranks equal counts in whatever order an unstable argsort leaves them, so the inputs are drawn until no
result hangs on that order, and this is asserted per case: the count at every requested rank is unique within its
plane; where slice_id runs past the end the smallest count is unique; for 'interesting' the three planes' counts at
that rank are distinct.

    python tools/gen_golden_contour.py   # writes tests/golden/contour.npz + MANIFEST_contour.txt
"""
import importlib.util
import json
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden_evaluation import REF  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden")
PKG = "_refcontour"
PLANES = ("Saggital", "Coronal", "Axial")
LABEL_VALUES = {"left": 1, "right": 2}
SHAPE = (7, 8, 10)

# name -> ContourImageEvaluator arguments, the subjects (indices into the stored ones), names dropped from a subject,
# and the random seed set before the call
CASES = {
    "fixed_axial": dict(plane="Axial", slice_id=9, ncol=2, subjects=[0, 1, 2]),
    "fixed_coronal": dict(plane="Coronal", slice_id=2, ncol=5, subjects=[0, 1, 2]),
    "interesting_split": dict(plane="interesting", slice_id=0, ncol=1, interesting_slice=True, split_subjects=True,
                              subjects=[0, 1, 2]),
    "random_interesting": dict(plane="random", slice_id=1, ncol=2, interesting_slice=True, subjects=[0, 1, 2, 0, 1], seed=5),
    "random_interesting_b": dict(plane="random", slice_id=1, ncol=2, interesting_slice=True, subjects=[2, 1], seed=1),
    "target_only": dict(plane="Saggital", slice_id=3, ncol=2, subjects=[0, 1], drop={"0": ["y_pred"], "1": ["y_pred"]}),
    "prediction_only": dict(plane="interesting", slice_id=1, ncol=3, interesting_slice=True, subjects=[1, 2],
                            drop={"0": ["y"], "1": ["y"]}),
    "past_the_end": dict(plane="Axial", slice_id=50, ncol=2, interesting_slice=True, subjects=[0, 3, 2]),
}


def make_grid(tensor, nrow=8, padding=2, pad_value=0.0):
    t = torch.stack(list(tensor), dim=0)          # [N, 1, h, w]
    if t.shape[0] == 1:
        return t[0]
    n, _, h, w = t.shape
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    grid = t.new_full((1, ymaps * (h + padding) + padding, xmaps * (w + padding) + padding), pad_value)
    for k in range(n):
        r, c = (k // xmaps) * (h + padding) + padding, (k % xmaps) * (w + padding) + padding
        grid[:, r:r + h, c:c + w] = t[k]
    return grid


class LabelMap(dict):
    @property
    def data(self):
        return self["data"]


class Transform:
    def __init__(self, include=None, exclude=None, **kwargs):
        self.include, self.exclude = include, exclude

    def __call__(self, data):
        images = [data] if isinstance(data, LabelMap) else [v for v in data.values() if isinstance(v, LabelMap)]
        holder = types.SimpleNamespace(get_images=lambda **kw: images)
        self.apply_transform(holder)
        return data


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _reference():
    os.environ.setdefault("MPLBACKEND", "Agg")
    import matplotlib
    import matplotlib.cm
    if not hasattr(matplotlib.cm, "get_cmap"):
        matplotlib.cm.get_cmap = lambda name: matplotlib.colormaps[name]
    tio = types.ModuleType("torchio")
    tio.Transform, tio.LabelMap, tio.Subject = Transform, LabelMap, dict
    tv = types.ModuleType("torchvision")
    tvu = types.ModuleType("torchvision.utils")
    tvu.make_grid = make_grid
    tv.utils = tvu
    sys.modules.update({"torchio": tio, "torchvision": tv, "torchvision.utils": tvu})
    for name in (PKG, PKG + ".evaluators", PKG + ".transforms", PKG + ".utils"):
        sys.modules[name] = types.ModuleType(name)
        sys.modules[name].__path__ = []
    typing_mod = types.ModuleType(PKG + ".typing")
    typing_mod.PathLike = str
    base = types.ModuleType(PKG + ".evaluators.evaluator")
    base.Evaluator = type("Evaluator", (), {})
    sys.modules.update({PKG + ".typing": typing_mod, PKG + ".evaluators.evaluator": base})
    utils = _load(PKG + ".utils.utils", os.path.join(REF, "utils", "utils.py"))
    sys.modules[PKG + ".utils"].slice_volume = utils.slice_volume
    fis = _load(PKG + ".transforms.find_interesting_slice", os.path.join(REF, "transforms", "find_interesting_slice.py"))
    sys.modules[PKG + ".transforms"].FindInterestingSlice = fis.FindInterestingSlice
    return _load(PKG + ".evaluators.contour_image_evaluator",
                 os.path.join(REF, "evaluators", "contour_image_evaluator.py")).ContourImageEvaluator


def _volumes(rng):
    """four subjects: image, target and prediction label maps; subject 3 has an empty target"""
    out = []
    for i in range(4):
        img = rng.normal(size=SHAPE).astype(np.float32)
        # foreground with a different density in every slice of every axis: few equal counts
        profile = [rng.uniform(0.2, 1.0, size=n) for n in SHAPE]
        density = profile[0][:, None, None] * profile[1][None, :, None] * profile[2][None, None, :]
        y = np.where(rng.random(SHAPE) < density, rng.choice([1, 2], size=SHAPE), 0).astype(np.int64)
        y_pred = np.where(rng.random(SHAPE) < 0.2, rng.choice([0, 1, 2], size=SHAPE), y).astype(np.int64)
        if i == 3:
            y[:] = 0
        out.append({"img": img, "y": y, "y_pred": y_pred})
    return out


def _subjects(volumes, case):
    subjects = []
    for pos, i in enumerate(case["subjects"]):
        v = volumes[i]
        s = {"name": f"s{pos}", "img": LabelMap(data=torch.from_numpy(v["img"])[None]),
             "y": LabelMap(data=torch.from_numpy(v["y"])[None], label_values=dict(LABEL_VALUES)),
             "y_pred": LabelMap(data=torch.from_numpy(v["y_pred"])[None], label_values=dict(LABEL_VALUES))}
        for name in case.get("drop", {}).get(str(pos), []):
            del s[name]
        subjects.append(s)
    return subjects


def _tie_free(case, subjects):
    """the conditions of the module docstring for one case"""
    if not case.get("interesting_slice"):
        return True
    k = case["slice_id"]
    for pos, s in enumerate(subjects):
        holder = s["y"] if "y" in s else s["y_pred"]
        mask = holder.data[0] != 0
        at_rank = []
        for axis in range(3):
            counts = mask.sum(dim=[a for a in range(3) if a != axis])
            ranked = sorted((int(c) for c in counts if c > 0), reverse=True)
            if not ranked:
                at_rank.append(None)
                continue
            c = ranked[min(k, len(ranked) - 1)]
            if ranked.count(c) != 1:
                return False
            at_rank.append(c)
        first = pos == 0 or case.get("split_subjects")
        if case["plane"] == "interesting" and first and len(set(at_rank)) != 3:
            return False
    return True


def _run(Evaluator, case, subjects, out, key):
    ev = Evaluator(case["plane"], "img", "y_pred", "y", case["slice_id"], False, case["ncol"],
                   interesting_slice=case.get("interesting_slice", False), split_subjects=case.get("split_subjects", False))
    calls = []
    grid, pick = ev.slice_and_make_grid, ev.get_slice_id

    def slice_and_make_grid(subjects, plane, image_name, impute_shape, pad_value=0):
        ids = [pick(s, plane) for s in subjects]
        mosaic = grid(subjects, plane, image_name, impute_shape, pad_value=pad_value)
        if image_name == "img":
            calls.append({"plane": ids[0][1], "slice_ids": [int(i) for i, _ in ids]})
        calls[-1][image_name] = mosaic.numpy()
        return mosaic
    ev.slice_and_make_grid = slice_and_make_grid
    if "seed" in case:
        random.seed(case["seed"])
    ev(subjects)
    out[f"{key}.calls"] = np.array(len(calls))
    for n, call in enumerate(calls):
        out[f"{key}.{n}.plane"] = np.array(call["plane"])
        out[f"{key}.{n}.slice_ids"] = np.array(call["slice_ids"], dtype=np.int64)
        for name in ("img", "y", "y_pred"):
            if name in call:
                out[f"{key}.{n}.{name}"] = call[name]


def main():
    Evaluator = _reference()
    for seed in range(20261018, 20261018 + 2000):
        volumes = _volumes(np.random.default_rng(seed))
        if all(_tie_free(case, _subjects(volumes, case)) for case in CASES.values()):
            break
    else:
        raise SystemExit("no tie-free inputs found")
    out = {"seed": np.array(seed), "cases": np.array(json.dumps(CASES)),
           "label_names": np.array(list(LABEL_VALUES)), "label_values": np.array(list(LABEL_VALUES.values()))}
    for i, v in enumerate(volumes):
        for name, a in v.items():
            out[f"subject.{i}.{name}"] = a
    for key, case in CASES.items():
        subjects = _subjects(volumes, case)
        assert _tie_free(case, subjects), key
        _run(Evaluator, case, subjects, out, key)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "contour.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(OUT, "MANIFEST_contour.txt"), "w") as f:
        f.write("contour.npz: written by tools/gen_golden_contour.py from the reference's ContourImageEvaluator, "
                "FindInterestingSlice and slice_volume, run unchanged (inputs, arguments, planes, slice ids, mosaics).\n")
        for k in sorted(out):
            f.write(f"{k} {out[k].dtype} {tuple(out[k].shape)}\n")
    print(path, os.path.getsize(path), "bytes; seed", seed)


if __name__ == "__main__":
    main()
