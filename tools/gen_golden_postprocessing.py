"""Generate tests/golden/postprocessing.npz from the REAL reference post-processing and lesion evaluator.

The reference's segmentation_pipeline/post_processing.py and evaluators/instance_segmentation_evaluator.py import
skimage.morphology, torchio and pandas.  None of them is needed for the arithmetic: skimage.morphology is stubbed with
scipy.ndimage restatements of the three functions used (skimage 0.18 semantics: `label` multi-class with background 0,
`remove_small_holes` with connectivity 1 and a strict `<`, `dilation` with the cross footprint), the evaluator's base
class and LabeledTensor are stubbed with a recorder.  The reference files themselves run unchanged; only their
results are stored.

Ties: the reference orders sizes with numpy's default argsort, whose order of equal sizes is unspecified.  Every
post-processing case runs twice, with ties in stable order and in reversed order; a case is kept only when both runs
agree, so ties decide nothing in the fixture.

    python tools/gen_golden_postprocessing.py   # writes tests/golden/postprocessing.npz + MANIFEST_postprocessing.txt
"""
import importlib.util
import os
import sys
import types

import numpy as np
import scipy
import scipy.ndimage as ndi
import torch

REF = "/root/reference/segmentation_pipeline"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


# ---------------------------------------------------------------- skimage.morphology stand-ins (scipy)
def sk_label(img, connectivity=None, return_num=False, background=0):
    img = np.asarray(img)
    conn = img.ndim if connectivity is None else connectivity
    st = ndi.generate_binary_structure(img.ndim, conn)
    out = np.zeros(img.shape, dtype=np.int64)
    n = 0
    for v in np.unique(img):
        if v == background:
            continue
        lab, k = ndi.label(img == v, structure=st)
        out[lab > 0] = lab[lab > 0] + n
        n += k
    if n:   # renumber in raster order of each component's first voxel
        flat = out.ravel()
        ids, first = np.unique(flat, return_index=True)
        keep = ids != 0
        order = np.argsort(first[keep], kind="stable")
        remap = np.zeros(n + 1, dtype=np.int64)
        remap[ids[keep][order]] = np.arange(1, order.size + 1)
        out = remap[out]
    return (out, n) if return_num else out


def sk_remove_small_holes(ar, area_threshold=64, connectivity=1):
    inverted = ~np.asarray(ar, dtype=bool)
    if area_threshold == 0:
        return ~inverted
    ccs, _ = ndi.label(inverted, structure=ndi.generate_binary_structure(inverted.ndim, connectivity))
    too_small = np.bincount(ccs.ravel()) < area_threshold
    inverted[too_small[ccs]] = False
    return ~inverted


def sk_dilation(image, selem=None):
    image = np.asarray(image)
    fp = ndi.generate_binary_structure(image.ndim, 1) if selem is None else selem
    if image.dtype == bool:
        return ndi.grey_dilation(image.astype(np.uint8), footprint=fp).astype(bool)
    return ndi.grey_dilation(image, footprint=fp)


class _TieNumpy(types.ModuleType):
    """numpy with argsort's tie order fixed: stable, or reversed (equal keys in descending index order)."""

    def __init__(self, reverse):
        super().__init__("numpy")
        self.reverse = reverse

    def __getattr__(self, name):
        return getattr(np, name)

    def argsort(self, a, *args, **kwargs):
        a = np.asarray(a)
        if self.reverse:
            return np.lexsort((-np.arange(a.size), a))
        return np.argsort(a, kind="stable")


def load_reference():
    sk = types.ModuleType("skimage")
    skm = types.ModuleType("skimage.morphology")
    skm.label, skm.remove_small_holes, skm.dilation = sk_label, sk_remove_small_holes, sk_dilation
    sk.morphology = skm
    sys.modules["skimage"], sys.modules["skimage.morphology"] = sk, skm

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    pp = {rev: load(f"ref_post_processing_{int(rev)}", os.path.join(REF, "post_processing.py")) for rev in (False, True)}
    for rev, mod in pp.items():
        mod.np = _TieNumpy(rev)

    # evaluator package shell: the base class and LabeledTensor (torchio / pandas) are stand-ins
    pkg = types.ModuleType("ref_eval")
    pkg.__path__ = []
    ev = types.ModuleType("ref_eval.evaluator")
    ev.Evaluator = type("Evaluator", (), {})
    lt = types.ModuleType("ref_eval.labeled_tensor")

    class Recorder:
        last = None

        def __init__(self, dim_names, dim_keys):
            self.values = {}
            Recorder.last = self

        def __setitem__(self, key, value):
            self.values[key[1]] = value

        def compute_summary_stats(self, names):
            return None

        def to_dataframe(self):
            return None

    lt.LabeledTensor = Recorder
    sys.modules.update({"ref_eval": pkg, "ref_eval.evaluator": ev, "ref_eval.labeled_tensor": lt})
    ise = load("ref_eval.instance_segmentation_evaluator", os.path.join(REF, "evaluators", "instance_segmentation_evaluator.py"))
    return pp, ise, Recorder


# ---------------------------------------------------------------- synthetic maps
def smooth_classes(rng, shape, classes, sigma, speckle):
    f = ndi.gaussian_filter(rng.standard_normal(shape), sigma)
    edges = np.quantile(f, np.linspace(0, 1, classes + 1)[1:-1])
    img = np.digitize(f, edges).astype(np.uint8)
    m = rng.random(shape) < speckle   # single-voxel holes and islands
    img[m] = rng.integers(0, classes, int(m.sum()))
    return img


def lesions(rng, shape, count, rmax):
    img = np.zeros(shape, dtype=np.uint8)
    zz, yy, xx = np.indices(shape, sparse=True)
    centres = []
    for _ in range(count):
        c = rng.integers(0, shape)
        r = rng.uniform(0.6, rmax, 3)
        img[((zz - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((xx - c[2]) / r[2]) ** 2 <= 1] = 1
        centres.append((c, r))
    holes = rng.random(shape) < 0.002
    img[holes & (img == 1)] = 0
    return img, centres


def main():
    pp, ise, Recorder = load_reference()
    rng = np.random.default_rng(20261015)
    out, manifest = {}, []

    def run(fn_name, *args, **kw):
        res = [getattr(pp[rev], fn_name)(*args, **kw) for rev in (False, True)]
        a, b = res
        same = np.array_equal(a[0], b[0]) and all(int(x) == int(y) for x, y in zip(a[1:], b[1:]))
        return a if same else None

    def add_case(tag, fn_name, img, *args, **kw):
        r = run(fn_name, img, *args, **kw)
        if r is None:
            manifest.append(f"{tag}: {fn_name} dropped (tie order changes the result)")
            return False
        out[f"{tag}/out"] = r[0].astype(np.uint8)
        out[f"{tag}/counts"] = np.array([int(x) for x in r[1:]], dtype=np.int64)
        manifest.append(f"{tag}: {fn_name}{tuple(a for a in args)} {kw or ''} -> counts {out[f'{tag}/counts'].tolist()}, "
                        f"{int((r[0] != img).sum())} voxels changed")
        return True

    def add_labels(tag, img):
        for c in (1, 2, 3):
            lab, n = sk_label(img, connectivity=c, return_num=True)
            assert n < 32767
            out[f"{tag}/label{c}"] = lab.astype(np.int16)
            out[f"{tag}/n{c}"] = np.array(n, dtype=np.int64)
            manifest.append(f"{tag}: label connectivity {c}: {n} components")

    # 1. hippo-like 4-class crop (D, H, W) = (96, 88, 24): the dmri_hippo chain and its parts
    hippo = smooth_classes(rng, (96, 88, 24), 4, 3.0, 0.01)
    out["hippo/img"] = hippo
    add_labels("hippo", hippo)
    add_case("hippo/holes64", "remove_holes", hippo, 64)
    filled = out["hippo/holes64/out"]
    add_case("hippo/chain_keep", "keep_components", filled, int(filled.max()))
    add_case("hippo/keep3", "keep_components", hippo, 3)
    add_case("hippo/small3", "remove_small_components", hippo, 3)
    # partial results: max_dilations = 2
    add_case("hippo/keep1_md2", "keep_components", hippo, 1, max_dilations=2)
    add_case("hippo/holes2000_md2", "remove_holes", hippo, 2000, max_dilations=2)
    # num beyond the number of components: nothing removed, a negative component count
    add_case("hippo/keep_many", "keep_components", filled, 100000)

    # 2. binary lesion-like 128^3: the msseg2 chain
    les, centres = lesions(rng, (128, 128, 128), 90, 7.0)
    out["lesion/img"] = les
    add_labels("lesion", les)
    add_case("lesion/holes64", "remove_holes", les, 64)
    add_case("lesion/small3", "remove_small_components", out["lesion/holes64/out"], 3)
    add_case("lesion/small40", "remove_small_components", les, 40)
    add_case("lesion/keep5", "keep_components", les, 5)

    # 3. pred / target pairs for the lesion-wise detection statistics
    names = ise.InstanceSegmentationEvaluator(prediction_label_map_name="pred", target_label_map_name="target").stats_to_output
    out["stat_names"] = np.array(names)
    pairs = []
    tgt, _ = lesions(rng, (64, 72, 80), 30, 5.0)
    pred = np.roll(tgt, 1, axis=2).copy()
    pred[:, :20] = 0                               # missed lesions
    extra, _ = lesions(rng, (64, 72, 80), 8, 3.0)  # false positives
    pred |= extra
    pairs.append(("pair0", pred, tgt))
    t1, _ = lesions(rng, (48, 48, 48), 12, 4.0)
    p1 = ndi.binary_dilation(t1).astype(np.uint8)  # over-segmentation: merges
    pairs.append(("pair1", p1, t1))
    pairs.append(("pair2_empty_pred", np.zeros_like(t1), t1))
    for tag, p, t in pairs:
        hists = []

        def recording_test(h, **kw):
            r = ise.msseg_detection_test(h, **kw)
            hists.append((h.clone(), r.clone()))
            return r

        evaluator = ise.InstanceSegmentationEvaluator("pred", "target", detection_test=recording_test)
        evaluator([{"name": tag, "pred": types.SimpleNamespace(data=torch.from_numpy(p[None].astype(np.int64))),
                    "target": types.SimpleNamespace(data=torch.from_numpy(t[None].astype(np.int64)))}])
        stats = Recorder.last.values
        out[f"{tag}/pred"], out[f"{tag}/target"] = p.astype(np.uint8), t.astype(np.uint8)
        out[f"{tag}/hist"] = hists[0][0].numpy().astype(np.float32)
        out[f"{tag}/det_target"] = hists[0][1].numpy().astype(bool) if hists[0][1].numel() else np.zeros(0, bool)
        out[f"{tag}/det_pred"] = hists[1][1].numpy().astype(bool) if hists[1][1].numel() else np.zeros(0, bool)
        out[f"{tag}/stats"] = np.array([float(stats[k]) for k in names], dtype=np.float64)
        manifest.append(f"{tag}: N={stats['target_components']} M={stats['predicted_components']} "
                        f"f1={float(stats['detection_f1']):.4f} dice={float(stats['dice']):.4f}")

    path = os.path.join(OUT, "postprocessing.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 2 << 20, size
    with open(os.path.join(OUT, "MANIFEST_postprocessing.txt"), "w") as f:
        f.write("Generated by tools/gen_golden_postprocessing.py from the reference's post_processing.py and\n"
                "evaluators/instance_segmentation_evaluator.py (skimage.morphology stubbed with scipy.ndimage)\n")
        f.write(f"numpy {np.__version__}  scipy {scipy.__version__}  torch {torch.__version__}\n")
        f.write(f"postprocessing.npz {size} bytes\n")
        f.write("\n".join(manifest) + "\n")
    print("\n".join(manifest))
    print(path, size, "bytes")


if __name__ == "__main__":
    main()
