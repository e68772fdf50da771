"""Times the device post-processing (segmentation_pipeline_amd.post_processing) against a scipy.ndimage restatement of
the reference's CPU process, on smooth-noise 4-class label maps: the dmri_hippo crop (96 x 88 x 24), 160^3 and a
cfg4-sized 256^3 volume.

    python tools/postproc_bench.py --gpu [--reps 5]     # device milliseconds per call + labelling passes per call
    python tools/postproc_bench.py --cpu                # the scipy restatement's seconds per call (no GPU needed)

GPU times are wall-clock per call including the host loop and its small read-backs (medians over --reps calls after
one warm-up call).  "passes" counts the labelling launches of one call, i.e. the fill loop's iterations.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("hippo 96x88x24", (96, 88, 24), 3.0), ("160^3", (160, 160, 160), 4.0), ("256^3 cfg4", (256, 256, 256), 5.0)]


def make_map(shape, sigma, seed=0):
    import scipy.ndimage as ndi
    rng = np.random.default_rng(seed)
    f = ndi.gaussian_filter(rng.standard_normal(shape).astype(np.float32), sigma)
    img = np.digitize(f, np.quantile(f, [0.4, 0.6, 0.8])).astype(np.int32)
    img[rng.random(shape) < 0.002] = 0     # speckle: small holes and small islands
    return img


def calls(img):
    num = int(img.max())
    return [("label(conn=3)", "label", (img,), {"connectivity": 3}),
            ("remove_holes(64)", "remove_holes", (img, 64), {}),
            ("keep_components(max)", "keep_components", (img, num), {}),
            ("remove_small_components(3)", "remove_small_components", (img, 3), {})]


# ---- scipy restatement of the reference's CPU process (skimage.morphology on scipy.ndimage) ----
def _sp_label(img, conn):
    import scipy.ndimage as ndi
    st = ndi.generate_binary_structure(3, conn)
    out = np.zeros(img.shape, np.int64)
    n = 0
    for v in np.unique(img):
        if v == 0:
            continue
        lab, k = ndi.label(img == v, structure=st)
        out[lab > 0] = lab[lab > 0] + n
        n += k
    return out, n


def _sp_sort_by_size(img, descending=False):
    ids, cnt = np.unique(img, return_counts=True)
    order = np.argsort(cnt, kind="stable")
    if descending:
        order = order[::-1]
    lut = np.zeros(int(ids.max()) + 1, np.int64)
    lut[ids[order]] = np.arange(ids.size)
    return lut[img], ids[order]


def sp_remove_holes(img, hole_size, max_dilations=100):
    import scipy.ndimage as ndi
    cross = ndi.generate_binary_structure(3, 1)
    img = img.copy()
    for _ in range(max_dilations):
        lab, _ = ndi.label(~(img > 0), structure=cross)
        small = np.bincount(lab.ravel()) < hole_size
        small[0] = False
        holes = small[lab]
        if not holes.any():
            break
        img[holes] = ndi.grey_dilation(img, footprint=cross)[holes]
    return img


def sp_keep_components(img, num, max_dilations=100):
    import scipy.ndimage as ndi
    cross = ndi.generate_binary_structure(3, 1)
    img = img.copy()
    for _ in range(max_dilations):
        comp, _ = _sp_label(img, 3)
        ranked, _ = _sp_sort_by_size(comp, descending=True)
        keep = ranked <= num
        if keep.all():
            break
        sorted_img, classes = _sp_sort_by_size(img)
        key = sorted_img * keep
        dil = ndi.grey_dilation(key, footprint=cross)
        change = (dil != key) & ~keep
        sorted_img[change] = dil[change]
        img = classes[sorted_img].astype(img.dtype)
    return img


def sp_call(fn, args, kw):
    if fn == "label":
        return _sp_label(args[0], kw["connectivity"])
    if fn == "remove_holes":
        return sp_remove_holes(*args, **kw)
    if fn == "keep_components":
        return sp_keep_components(*args, **kw)
    inv = sp_remove_holes(args[0] == 0, args[1])
    out = args[0].copy()
    out[inv] = 0
    return out


def run_gpu(reps):
    import torch
    from segmentation_pipeline_amd import post_processing as PP
    passes = [0]
    ccl = PP._ccl

    def counting(*a, **k):
        passes[0] += 1
        return ccl(*a, **k)

    PP._ccl = counting
    print(f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
    print(f"{'case':16s} {'call':28s} {'GPU ms (numpy in/out)':>22s} {'GPU ms (device)':>16s} {'passes':>7s}")
    for name, shape, sigma in CASES:
        img = make_map(shape, sigma)
        dimg = torch.from_numpy(img).cuda()
        for label, fn, args, kw in calls(img):
            f = getattr(PP, fn)
            res = []
            for kind, a0 in (("numpy", img), ("device", dimg)):
                f(a0, *args[1:], **kw)
                torch.cuda.synchronize()
                ts = []
                for _ in range(reps):
                    passes[0] = 0
                    t0 = time.perf_counter()
                    f(a0, *args[1:], **kw)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                res.append(float(np.median(ts)))
            print(f"{name:16s} {label:28s} {res[0]:22.3f} {res[1]:16.3f} {passes[0]:7d}", flush=True)


def run_cpu(reps, skip_slow):
    print(f"{'case':16s} {'call':28s} {'CPU s (scipy restatement)':>26s}")
    for name, shape, sigma in CASES:
        img = make_map(shape, sigma)
        for label, fn, args, kw in calls(img):
            if skip_slow and fn == "keep_components" and img.size > 100 ** 3:
                print(f"{name:16s} {label:28s} {'skipped':>26s}")
                continue
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                sp_call(fn, args, kw)
                ts.append(time.perf_counter() - t0)
            print(f"{name:16s} {label:28s} {float(np.median(ts)):26.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-slow", action="store_true", help="--cpu: skip keep_components above 100^3 voxels")
    a = ap.parse_args()
    if a.gpu:
        run_gpu(a.reps)
    if a.cpu:
        run_cpu(max(1, a.reps if not a.gpu else 1), a.skip_slow)


if __name__ == "__main__":
    main()
