"""Times the dmri_hippo augmentation modes (research/dmri_hippo/configs/augmentation.py) on the device, one subject per
call, with ReconstructMeanDWI on the device (augmentation.py, csrc/dwi.hip).

    python tools/dwi_bench.py [--reps 30] [--warmup 3]    # ms per subject per mode and N, the gather kernel alone
    rocprofv3 --kernel-trace --output-format csv -d T -- python tools/dwi_bench.py --mode combined --grads 64 --reps 5
    python tools/dwi_bench.py --count T --reps 5          # launches per subject (seeds 0 .. 4 and 3 warm-ups), from it

The subject and chains are those of tests/test_dwi_reconstruction_gpu.py: mean_dwi, md, fa, whole_roi and
whole_roi_union at 101 x 93 x 19 plus an N-channel full_dwi, cropped / padded to 96 x 88 x 24, then
common_transforms_1 -> the mode's augmentation -> common_transforms_2.  The ', no full_dwi' rows leave full_dwi out of
the subject (the chains of tools/preprocess_bench.py); the other rows carry it, and common_transforms_2 rescales it over
all N channels as the reference does.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODES = ["no_augmentation", "standard", "dwi_reconstruction", "combined"]
GRADS = [32, 64, 100]


def _time(call, reps, warmup):
    """(device ms median, mean, host ms per call median) with events around each call; call i uses seed i, the same
    seeds in every row, so the random branches (elastic, bias, gamma, blur / noise) average out alike"""
    import torch
    for i in range(warmup):
        call(1000 + i)
    torch.cuda.synchronize()
    dev, hst = [], []
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        call(i)
        e1.record()
        t1 = time.perf_counter()
        e1.synchronize()
        dev.append(e0.elapsed_time(e1))
        hst.append((t1 - t0) * 1e3)
    return np.median(dev), np.mean(dev), np.median(hst)


def gpu(reps, warmup, modes, grads):
    import torch
    import test_dwi_reconstruction_gpu as T
    assert torch.cuda.is_available(), "needs a GPU"
    print(f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
    print(f"{'mode':30s} {'N':>4s} {'ms/subject (median)':>20s} {'mean':>8s} {'host ms/call':>13s}")
    for n in grads:
        imgs, labs, lv, g = T.dmri_subject(n)
        sub = {k: torch.from_numpy(v).cuda() for k, v in {**imgs, **labs}.items()}
        rows = [(m, sub) for m in modes]
        if n == grads[0]:
            rows[:0] = [(m + ", no full_dwi", {k: v for k, v in sub.items() if k != "full_dwi"})
                        for m in ("no_augmentation", "standard") if m in modes]
        for mode, s in rows:
            chain = T.mode_chain(mode.split(",")[0])
            med, mn, host = _time(lambda seed: T._call(chain, s, labs, lv, g, seed), reps, warmup)
            print(f"{mode:30s} {n if 'full_dwi' in s else 0:4d} {med:20.3f} {mn:8.3f} {host:13.3f}")


def kernel(reps, grads):
    """the gather alone: k = 7 picks at 96 x 88 x 24 (the mode's largest draw), events around `reps` launches"""
    import torch
    from segmentation_pipeline_amd import augmentation as A
    shape = (96, 88, 24)
    print(f"# m355_dwi_mean alone at {shape}, events around {reps} launches after 3 warm-ups")
    print(f"{'N':>4s} {'k':>3s} {'us/launch':>10s} {'GB/s':>8s}   {'MeanDWI call, host us':>22s}")
    from segmentation_pipeline_amd import _lib
    from segmentation_pipeline_amd.augmentation import _i3
    from segmentation_pipeline_amd.ops import _p, _stream
    L = _lib.lib()
    S = int(np.prod(shape))
    for n in grads:
        x = torch.rand((n,) + shape, device="cuda")
        y = torch.empty((1,) + shape, device="cuda")
        for k in (1, 7):
            idx = torch.tensor([(j * 7) % n for j in range(k)], dtype=torch.int32, device="cuda")

            def fn():
                return L.m355_dwi_mean(_p(x), n, _i3(shape), _p(idx), k, _p(y), _stream())
            for _ in range(3):
                assert fn() == 0
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / reps
            t = A.MeanDWI(idx.tolist())
            sub = {"full_dwi": x}
            t(sub)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                t(sub)
            host = (time.perf_counter() - t0) * 1e6 / reps
            torch.cuda.synchronize()
            print(f"{n:4d} {k:3d} {us:10.1f} {4 * S * (k + 1) / us / 1e3:8.0f}   {host:22.1f}")


def count(trace_dir, calls):
    import csv
    import glob
    kern = [r for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
            for r in csv.DictReader(open(f))]
    names = {}
    for r in kern:
        k = r["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "").strip()
        names[k] = names.get(k, 0) + 1
    print(f"per subject: {len(kern) / calls:.1f} launches")
    for k, v in sorted(names.items(), key=lambda kv: -kv[1]):
        print(f"  {v / calls:6.1f}  {k}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", default=None, choices=MODES, help="time only this mode")
    ap.add_argument("--grads", type=int, default=None, help="time only this N")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--count", default=None, help="trace directory of one --mode / --grads run: launches per subject")
    a = ap.parse_args()
    if a.count:
        count(a.count, a.reps + a.warmup)
    else:
        gpu(a.reps, a.warmup, [a.mode] if a.mode else MODES, [a.grads] if a.grads else GRADS)
        if not a.no_kernel and a.mode is None:
            kernel(a.reps, [a.grads] if a.grads else GRADS)
