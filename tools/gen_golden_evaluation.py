"""Generate tests/golden/evaluation.npz from the REAL reference evaluators.

Runs the reference's evaluators/segmentation_evaluator.py, label_map_evaluator.py, instance_segmentation_evaluator.py
and labeled_tensor.py unchanged.  Their imports are stubbed the way tools/gen_golden_postprocessing.py does it: torchio
(type annotations only), the Evaluator base class, the package's utils (as_list / is_sequence / auto_str, restated
here) and skimage.morphology.label (the scipy restatement of gen_golden_postprocessing.py).  Only inputs and results
are stored: label maps, names, label values, the subject tables as DataFrame columns / values and the summary tables.

    python tools/gen_golden_evaluation.py   # writes tests/golden/evaluation.npz + MANIFEST_evaluation.txt
"""
import importlib.util
import os
import sys
import types
from collections.abc import Sequence

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/segmentation_pipeline"
OUT = os.path.join(HERE, "..", "tests", "golden")
PKG = "_refeval"

CURVE_PARAMS = {"left_whole": np.array([-1.96312119e-01, 9.46668029e+00, 2.33635173e+03]),
                "right_whole": np.array([-2.68467331e-01, 1.67925603e+01, 2.07224236e+03])}
SUMMARY = ('mean', 'median', 'mode', 'std', 'min', 'max')
SEG_STATS = ('target_volume', 'prediction_volume', 'TP', 'FP', 'TN', 'FN', 'dice', 'jaccard', 'precision', 'recall')


def _stubs():
    sys.path.insert(0, HERE)
    from gen_golden_postprocessing import sk_label
    tio = types.ModuleType("torchio")
    tio.Subject, tio.SubjectsDataset, tio.LabelMap = dict, list, dict
    sk = types.ModuleType("skimage")
    morph = types.ModuleType("skimage.morphology")
    morph.label = sk_label
    sk.morphology = morph
    sys.modules.update({"torchio": tio, "skimage": sk, "skimage.morphology": morph})

    def is_sequence(x):
        return isinstance(x, Sequence) and not isinstance(x, str)

    def as_list(x):
        return [] if x is None else (list(x) if is_sequence(x) else [x])

    pkg = types.ModuleType(PKG)
    pkg.__path__ = []
    utils = types.ModuleType(PKG + ".utils")
    utils.as_list, utils.is_sequence, utils.auto_str = as_list, is_sequence, lambda o: type(o).__name__
    ev = types.ModuleType(PKG + ".evaluators")
    ev.__path__ = []
    base = types.ModuleType(PKG + ".evaluators.evaluator")

    class Evaluator:
        pass
    base.Evaluator = Evaluator
    sys.modules.update({PKG: pkg, PKG + ".utils": utils, PKG + ".evaluators": ev, PKG + ".evaluators.evaluator": base})
    mods = {}
    for name in ("labeled_tensor", "segmentation_evaluator", "label_map_evaluator", "instance_segmentation_evaluator"):
        full = f"{PKG}.evaluators.{name}"
        spec = importlib.util.spec_from_file_location(full, os.path.join(REF, "evaluators", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[full] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


class Map(dict):
    @property
    def data(self):
        return self["data"]


def _map(a, label_values):
    return Map(data=torch.from_numpy(np.ascontiguousarray(a))[None], label_values=dict(label_values))


def _store(out, key, res, subjects, maps):
    df = res["subject_stats"]
    out[f"{key}.df_columns"] = np.array([str(c) for c in df.columns])
    for c in df.columns:
        v = df[c].to_numpy()
        out[f"{key}.df.{c}"] = v.astype(str) if v.dtype == object else v
    ss = res["summary_stats"]
    out[f"{key}.summary"] = ss.data.numpy()
    for i, keys in enumerate(ss.dim_keys):
        out[f"{key}.summary_keys{i}"] = np.array([str(k) for k in keys])
    out[f"{key}.names"] = np.array([s["name"] for s in subjects])
    out[f"{key}.n"] = np.array(len(subjects))
    for i, s in enumerate(subjects):
        for m in maps:
            out[f"{key}.{i}.{m}"] = s[m].data[0].numpy()
        if "age" in s:
            out[f"{key}.{i}.age"] = np.array(s["age"])


def main():
    mods = _stubs()
    rng = np.random.default_rng(20261016)
    out = {}
    lv = {"a": 1, "b": 3, "neg": -2, "only_target": 7, "only_pred": 9, "absent": 11}
    shapes = [(5, 6, 7), (8, 4, 3), (3, 3, 3), (9, 7, 5), (4, 10, 6), (6, 6, 2)]
    dtypes = [np.int64, np.int32, np.uint8, np.int16, np.float32, np.int64]
    subjects = []
    for i, (sh, dt) in enumerate(zip(shapes, dtypes)):
        vals = np.array([0, 1, 3, -2, 5] if dt != np.uint8 else [0, 1, 3, 5])
        t = rng.choice(vals, size=sh)
        p = np.where(rng.random(sh) < 0.3, rng.choice(vals, size=sh), t)
        if i == 1:
            t[0, 0, :] = 7          # a label only the target has
        if i == 3:
            p[0, :, 0] = 9          # a label only the prediction has
        if i == 2:
            p[:] = 0                # nothing predicted: precision 0 / 0
        subjects.append({"name": f"s{i}", "pred": _map(p.astype(dt), lv), "target": _map(t.astype(dt), lv)})
    out["seg.label_names"] = np.array(list(lv))
    out["seg.label_values"] = np.array(list(lv.values()))
    seg = mods["segmentation_evaluator"].SegmentationEvaluator("pred", "target", stats_to_output=SEG_STATS,
                                                              summary_stats_to_output=SUMMARY)
    _store(out, "seg", seg(subjects), subjects, ("pred", "target"))
    _store(out, "seg_default", mods["segmentation_evaluator"].SegmentationEvaluator("pred", "target")(subjects),
           subjects, ("pred", "target"))
    _store(out, "seg_single", seg(subjects[:1]), subjects[:1], ("pred", "target"))
    dup = [dict(s) for s in subjects[:3]]
    dup[2]["name"] = "s0"           # a name given twice: the reference's key map keeps its last position
    _store(out, "seg_dup", seg(dup), dup, ("pred", "target"))

    hv = {"left_whole": 1, "right_whole": 2}
    hip = []
    for i in range(5):
        sh = (12, 10, 6)
        m = rng.choice([0, 1, 2], size=sh, p=[0.5, 0.3, 0.2]).astype(np.int64)
        hip.append({"name": f"h{i}", "y_pred_eval": _map(m, hv), "age": float(rng.integers(4, 80))})
    lme = mods["label_map_evaluator"].LabelMapEvaluator(
        "y_pred_eval", curve_params=CURVE_PARAMS, curve_attribute="age",
        stats_to_output=('volume', 'error', 'absolute_error', 'squared_error', 'percent_diff'),
        summary_stats_to_output=SUMMARY)
    _store(out, "lme", lme(hip), hip, ("y_pred_eval",))
    _store(out, "lme_volume", mods["label_map_evaluator"].LabelMapEvaluator("y_pred_eval")(hip), hip, ("y_pred_eval",))

    les = []
    for i in range(3):
        sh = (10, 12, 9)
        t = (rng.random(sh) < 0.06).astype(np.uint8)
        p = t.copy()
        p[rng.random(sh) < 0.04] ^= 1
        les.append({"name": f"l{i}", "pred": _map(p, {"lesion": 1}), "target": _map(t, {"lesion": 1})})
    ise = mods["instance_segmentation_evaluator"].InstanceSegmentationEvaluator("pred", "target")
    _store(out, "ise", ise(les), les, ("pred", "target"))

    lt = mods["labeled_tensor"].LabeledTensor(["a", "b", "c"], [["x", "y"], ["p", "q", "r"], ["u", "v"]])
    lt.data[:] = torch.from_numpy(rng.normal(size=(2, 3, 2)).astype(np.float32))
    lt.data[0, 1, 0] = float("nan")
    lt.data[:, 2, 1] = float("inf")
    out["lt.data"] = lt.data.numpy().copy()
    out["lt.summary"] = lt.compute_summary_stats(list(SUMMARY)).data.numpy()
    out["lt.getitem_x_q"] = lt["x", "q"].numpy()
    out["lt.getitem_list"] = lt[["y", "x"], :, "v"].numpy()

    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "evaluation.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(OUT, "MANIFEST_evaluation.txt"), "w") as f:
        f.write("evaluation.npz: written by tools/gen_golden_evaluation.py from the reference's evaluators "
                "(segmentation, label map, instance segmentation, labeled tensor), run unchanged.\n")
        for k in sorted(out):
            f.write(f"{k} {out[k].dtype} {tuple(out[k].shape)}\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
