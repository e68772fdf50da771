"""Generate tests/golden/region_stats.npz from the REAL reference fingerprint functions.

Runs the reference's data_processing/dataset_fingerprint.py unchanged: get_bounds, get_label_bounds, get_summary_stats,
merge_dict and summarize, on seeded synthetic subjects.  Its imports are stubbed the way tools/gen_golden_evaluation.py
does it: torchio (annotations and the two image classes), the SubjectFolder module and the package's utils (the JSON
encoder, formatting only).  Only inputs and results are stored: the label maps and images, names, label values,
spacings, and the per-subject and summary fingerprints as JSON text.

    python tools/gen_golden_region_stats.py   # writes tests/golden/region_stats.npz + MANIFEST_region_stats.txt
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/segmentation_pipeline"
OUT = os.path.join(HERE, "..", "tests", "golden")
PKG = "_reffp"

LABEL_VALUES = {"seg": {"left": 1, "right": 2, "stem": 7}, "lesion": {"lesion": 1}}
SHAPES = [(13, 17, 11), (20, 15, 18), (9, 22, 14), (16, 16, 16)]
SPACINGS = [(1.0, 1.0, 1.0), (0.9, 0.9, 1.2), (1.0, 1.0, 2.5), (0.8, 0.8, 0.8)]
SEG_DTYPES = [np.int16, np.uint8, np.float32, np.int64]


class Image(dict):
    @property
    def data(self):
        return self["data"]


class ScalarImage(Image):
    pass


class LabelMap(Image):
    pass


def _reference():
    tio = types.ModuleType("torchio")
    tio.ScalarImage, tio.LabelMap, tio.Transform = ScalarImage, LabelMap, object
    sys.modules["torchio"] = tio
    pkg = types.ModuleType(PKG)
    pkg.__path__ = []
    utils = types.ModuleType(PKG + ".utils")
    utils.CompactJSONEncoder = json.JSONEncoder
    dp = types.ModuleType(PKG + ".data_processing")
    dp.__path__ = []
    folder = types.ModuleType(PKG + ".data_processing.subject_folder")
    folder.SubjectFolder = object
    sys.modules.update({PKG: pkg, PKG + ".utils": utils, PKG + ".data_processing": dp,
                        PKG + ".data_processing.subject_folder": folder})
    full = PKG + ".data_processing.dataset_fingerprint"
    spec = importlib.util.spec_from_file_location(full, os.path.join(REF, "data_processing", "dataset_fingerprint.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[full] = mod
    spec.loader.exec_module(mod)
    return mod


def _blob(shape, centre, radius):
    g = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1)
    return (((g - np.asarray(centre)) / np.asarray(radius)) ** 2).sum(-1) <= 1.0


def _subject(rng, i):
    shape = np.asarray(SHAPES[i])
    seg = np.zeros(SHAPES[i], dtype=np.int64)
    seg[_blob(shape, shape * (0.35, 0.5, 0.5), shape * 0.22)] = 1
    seg[_blob(shape, shape * (0.68, 0.5, 0.45), shape * 0.2)] = 2
    seg[_blob(shape, shape * (0.5, 0.25, 0.6), shape * 0.12)] = 7
    seg[tuple(shape // 2)] = 5   # a value outside label_values: counted by 'all' only
    lesion = (_blob(shape, shape * (0.4, 0.6, 0.3), shape * 0.1) | _blob(shape, shape * (0.7, 0.3, 0.7), shape * 0.08))
    t1 = (rng.normal(300.0 + 40.0 * i, 25.0, SHAPES[i]) + 80.0 * (seg > 0)).astype(np.float32)[None]
    t1[0][rng.random(SHAPES[i]) < 0.2] = 0.0   # a background of exact ties
    dwi = rng.gamma(2.0, 1.5e-3, (3,) + SHAPES[i]).astype(np.float32)
    return {"name": f"subject_{i}", "spacing": SPACINGS[i], "spatial_shape": SHAPES[i],
            "seg": LabelMap(data=torch.from_numpy(seg.astype(SEG_DTYPES[i]))[None], label_values=LABEL_VALUES["seg"]),
            "lesion": LabelMap(data=torch.from_numpy(lesion.astype(np.uint8))[None], label_values=LABEL_VALUES["lesion"]),
            "t1": ScalarImage(data=torch.from_numpy(t1)), "dwi": ScalarImage(data=torch.from_numpy(dwi))}


def main():
    ref = _reference()
    rng = np.random.default_rng(20261020)
    subjects = [_subject(rng, i) for i in range(len(SHAPES))]
    fingerprints = {}
    for s in subjects:
        fingerprints[s["name"]] = {
            "spacing": s["spacing"], "spatial_shape": s["spatial_shape"],
            "label_bounds": {k: ref.get_label_bounds(v) for k, v in s.items() if isinstance(v, LabelMap)},
            "intensity_stats": {k: ref.get_summary_stats(v.data) for k, v in s.items() if isinstance(v, ScalarImage)}}
    merged = {}
    for fp in fingerprints.values():
        ref.merge_dict(fp, merged)
    summary = ref.summarize(merged)
    # get_bounds on a bare mask, as the reference's callers use it
    mask_bounds = ref.get_bounds(subjects[0]["lesion"].data[0] != 0)

    out = {"n": np.array(len(subjects)), "names": np.array([s["name"] for s in subjects]),
           "spacing": np.asarray(SPACINGS, dtype=np.float64), "label_values": np.array(json.dumps(LABEL_VALUES)),
           "subject_fingerprints": np.array(json.dumps(fingerprints)), "summary_fingerprint": np.array(json.dumps(summary)),
           "mask_bounds": np.array(json.dumps(mask_bounds))}
    for i, s in enumerate(subjects):
        for k in ("seg", "lesion", "t1", "dwi"):
            out[f"{i}.{k}"] = s[k].data.numpy()
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "region_stats.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(OUT, "MANIFEST_region_stats.txt"), "w") as f:
        f.write("region_stats.npz: written by tools/gen_golden_region_stats.py from the reference's\n"
                "data_processing/dataset_fingerprint.py (get_bounds, get_label_bounds, get_summary_stats, merge_dict,\n"
                "summarize) on seeded synthetic subjects.  Data only:\n")
        for k in sorted(out):
            a = np.asarray(out[k])
            f.write(f"  {k}: {a.dtype} {list(a.shape)}\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
