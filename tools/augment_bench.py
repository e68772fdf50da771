"""Times the device augmentation chains of the reference's production configs (segmentation_pipeline_amd.augmentation)
against a scipy / numpy restatement of the same per-voxel work on the CPU.

    python tools/augment_bench.py --gpu [--reps 30]     # device ms per subject (median after warm-up)
    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d T -- python tools/augment_bench.py --gpu --case 0 --reps 5
    python tools/augment_bench.py --count T --reps 5    # launches and parameter copies per subject, from that trace
    python tools/augment_bench.py --cpu [--threads 16]  # the scipy restatement's seconds per subject

Workloads: dmri_hippo (3 single-channel images + a 3-class one-hot label at 96 x 88 x 24, elastic with cubic B-spline)
and msseg2 (2 images + a uint8 label at 160 x 192 x 160).  Every transform is forced on (p = 1) and the spatial OneOf of
msseg2 is timed for each branch, so the numbers are the per-subject worst case of each chain.  Kernel rates and launch counts come
from separate traced runs.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def chains(A):
    dmri = A.Compose([
        A.RandomFlip(axes=(0, 1, 2)),
        A.RandomElasticDeformation(num_control_points=(7, 7, 4), locked_borders=1, image_interpolation="bspline"),
        A.RandomBiasField(), A.RescaleIntensity((0, 1), (0.01, 99.9)), A.RandomGamma(), A.RescaleIntensity((-1, 1)),
        A.Compose([A.RandomBlur((0, 1)), A.RandomNoise(std=0.035)])])

    def ms(spatial):
        return A.Compose([A.RandomPermuteDimensions(), A.RandomFlip(axes=(0, 1, 2)), spatial,
                          A.RandomBiasField(), A.RescaleIntensity((0, 1), (0.01, 99.9)), A.RandomGamma(),
                          A.RescaleIntensity((-1, 1)), A.RandomBlur((0, 1)), A.RandomNoise(std=0.1)])
    return [("dmri_hippo 3 img + onehot 96x88x24", (96, 88, 24), 3, dmri),
            ("msseg2 affine 2 img + label 160x192x160", (160, 192, 160), 2,
             ms(A.RandomAffine(scales=0.2, degrees=45, default_pad_value="otsu"))),
            ("msseg2 elastic 2 img + label 160x192x160", (160, 192, 160), 2, ms(A.RandomElasticDeformation()))]


def subject(shape, nimg, seed=0):
    rng = np.random.default_rng(seed)
    imgs = {f"img{i}": (rng.random((1,) + shape, dtype=np.float32) + 1.0) for i in range(nimg)}
    if shape[2] == 24:
        lab = np.eye(3, dtype=np.float32)[rng.integers(0, 3, shape)].transpose(3, 0, 1, 2).copy()
    else:
        lab = (rng.random((1,) + shape) > 0.9).astype(np.uint8)
    return imgs, lab


def gpu(reps, warmup, case=None):
    """device ms per subject.  Every call uses the same seed, so every call issues the same launches: a trace of one
    case (--case) divided by warmup + reps calls gives launches per subject exactly (--count)."""
    import torch
    from segmentation_pipeline_amd import augmentation as A
    assert torch.cuda.is_available(), "--gpu needs a GPU"
    print(f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
    print(f"{'case':44s} {'ms/subject (median)':>20s} {'min':>8s}")
    for i, (label, shape, nimg, chain) in enumerate(chains(A)):
        if case is not None and i != case:
            continue
        imgs, lab = subject(shape, nimg)
        sub = {k: torch.from_numpy(v).cuda() for k, v in imgs.items()}
        sub["seg"] = torch.from_numpy(lab).cuda()
        torch.cuda.synchronize()
        for _ in range(warmup):
            chain(sub, label_maps=("seg",), generator=torch.Generator().manual_seed(0))
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            chain(sub, label_maps=("seg",), generator=torch.Generator().manual_seed(0))
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        print(f"{label:44s} {np.median(times):20.3f} {np.min(times):8.3f}")


def count(trace_dir, calls):
    """launches per subject from a rocprofv3 --kernel-trace --output-format csv run of one case: the augmentation kernels,
    the memsets (fillBuffer) and the copy kernels (copyBuffer: the pinned parameter uploads and the B-spline coefficient
    copy).  The subject's own upload before the timed calls goes through the memory-copy path, not a copy kernel."""
    import csv
    import glob
    kern = [r for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
            for r in csv.DictReader(open(f))]
    aug = sum(1 for r in kern if "m355::aug_" in r["Kernel_Name"])
    fill = sum(1 for r in kern if "fillBuffer" in r["Kernel_Name"])
    copy = sum(1 for r in kern if "copyBuffer" in r["Kernel_Name"])
    other = len(kern) - aug - fill - copy
    print(f"per subject: {(aug + fill + copy) / calls:.1f} launches = {aug / calls:.1f} augment kernels + "
          f"{fill / calls:.1f} memsets + {copy / calls:.1f} copy kernels; other kernels in the trace: {other}")


def cpu(threads):
    import scipy.ndimage as ndi
    from concurrent.futures import ThreadPoolExecutor
    import augment_ref as R
    print(f"# scipy restatement, {threads} threads (one image per thread; scipy releases the GIL)")
    for label, shape, nimg, _ in [(c[0], c[1], c[2], None) for c in chains(_Stub())]:
        imgs, lab = subject(shape, nimg)
        interp = 3 if "dmri" in label else 1
        rng = np.random.default_rng(1)
        coords = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float32) for n in shape], indexing="ij"))
        coords += rng.uniform(-2, 2, (3, 1, 1, 1)).astype(np.float32)

        def one(x):
            x = x[0].astype(np.float64)
            x = ndi.map_coordinates(x, coords, order=interp, mode="mirror" if interp == 3 else "nearest")
            x = x * R.bias_field(shape, rng.uniform(-0.5, 0.5, 20))
            lo, hi = np.percentile(x, (0.01, 99.9))
            x = (np.clip(x, lo, hi) - lo) / (hi - lo)
            x = x ** 1.1
            x = 2 * (x - x.min()) / (x.max() - x.min()) - 1
            x = ndi.gaussian_filter(x, 0.5)
            return x + rng.normal(0, 0.05, x.shape)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, list(imgs.values())))
            list(ex.map(lambda c: ndi.map_coordinates(c, coords, order=0), list(lab.reshape((-1,) + shape))))
        print(f"{label:44s} {time.perf_counter() - t0:10.3f} s/subject")


class _Stub:
    def __getattr__(self, k):
        return lambda *a, **kw: None


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", type=int, default=None, help="run only this case (index into chains())")
    ap.add_argument("--count", default=None, help="trace directory of one --case run: launches per subject")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    if a.count:
        count(a.count, a.reps + a.warmup)
    if a.gpu:
        gpu(a.reps, a.warmup, a.case)
    if a.cpu:
        cpu(a.threads)
