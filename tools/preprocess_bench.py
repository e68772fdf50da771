"""Times the device preprocessing chains of the reference's production configs (segmentation_pipeline_amd.preprocessing,
DESIGN §4.11) and their numpy restatement, and the streaming rate of each preprocessing kernel.

    python tools/preprocess_bench.py --gpu [--reps 30]     # device ms per subject of both configs' chains, kernel GB/s
    rocprofv3 --kernel-trace --output-format csv -d T -- python tools/preprocess_bench.py --gpu --case 0 --reps 5 --no-rates
    python tools/preprocess_bench.py --count T --reps 5    # launches per subject, from that trace
    python tools/preprocess_bench.py --cpu                 # the numpy restatement's seconds per subject

Subjects and chains are those of tests/test_preprocessing_gpu.py: dmri_hippo (3 images + 2 label maps at 101 x 93 x 19,
cropped / padded to 96 x 88 x 24) and msseg2 (2 images + 2 label maps at 72 x 60 x 40, spacing (0.8, 1, 1.5) mm).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [("dmri_hippo default", "dmri", False), ("dmri_hippo training", "dmri", True),
         ("msseg2 default", "msseg2", False), ("msseg2 training", "msseg2", True)]


def gpu(reps, warmup, case=None):
    """device ms per subject (events around each call after warm-up; median and min).  Every call uses the same seed, so
    every call issues the same launches and a trace of one --case divided by warmup + reps gives launches per subject."""
    import torch
    import test_preprocessing_gpu as T
    assert torch.cuda.is_available(), "--gpu needs a GPU"
    print(f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
    print(f"{'chain':24s} {'ms/subject (median)':>20s} {'min':>8s}")
    for i, (label, kind, training) in enumerate(CASES):
        if case is not None and i != case:
            continue
        imgs, labs, sp, lv = T.subject(kind)
        sub = {k: torch.from_numpy(v).cuda() for k, v in {**imgs, **labs}.items()}
        chain = T.chain_of(kind, training)

        def call():
            return chain(sub, label_maps=tuple(labs), spacing=sp, label_values=lv,
                         generator=torch.Generator().manual_seed(0))
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        print(f"{label:24s} {np.median(times):20.3f} {np.min(times):8.3f}")


def rates(reps):
    """achieved GB/s of each streaming kernel on one large volume (bytes the kernel must move / event time per launch)"""
    import ctypes as C
    import torch
    from segmentation_pipeline_amd import _lib
    from segmentation_pipeline_amd.augmentation import _i3
    from segmentation_pipeline_amd.ops import _p, _stream
    L = _lib.lib()
    shape = (256, 256, 256)
    S = int(np.prod(shape))
    x = torch.rand((1,) + shape, device="cuda")
    lab = (torch.rand((1,) + shape, device="cuda") * 3).to(torch.uint8)
    out3 = (240, 272, 256)
    y = torch.empty((1,) + out3, device="cuda")
    oh = torch.empty((3,) + shape, dtype=torch.uint8, device="cuda")
    ifl = torch.empty((1,) + shape, device="cuda")
    bad = torch.empty(1, dtype=torch.int32, device="cuda")
    bb = torch.empty(8, dtype=torch.int32, device="cuda")
    nt = int(L.m355_pre_min_tables_bytes(1, _i3(shape)))
    tables = torch.empty(nt, dtype=torch.uint8, device="cuda")
    d = _lib.PreGatherDesc()
    d.x, d.y, d.in_dtype, d.out_dtype, d.C = x.data_ptr(), y.data_ptr(), _lib.PRE_F32, _lib.PRE_F32, 1
    d.src3[:], d.in3[:], d.out3[:], d.off3[:] = shape, shape, out3, (8, -8, 0)
    e = (_lib.PreLabelEntry * 2)()
    for j, w in enumerate((1.0, 100.0)):
        e[j].map, e[j].dtype, e[j].C, e[j].one_hot, e[j].weight, e[j].id = lab.data_ptr(), _lib.PRE_U8, 1, 0, w, j + 1
    kernels = [
        ("pre_gather f32 crop/pad", lambda: L.m355_pre_gather(C.byref(d), _stream()), 4 * S + 4 * int(np.prod(out3))),
        ("pre_min_tables f32", lambda: L.m355_pre_min_tables(_p(x), _lib.PRE_F32, 1, _i3(shape), 0, 0.0, _p(tables), nt,
                                                             _stream()), 4 * S),
        ("pre_bbox u8", lambda: L.m355_pre_bbox(_p(lab), _lib.PRE_U8, 1, _i3(shape), 0, 0, 0.0, _p(bb), _stream()), S),
        ("pre_one_hot u8 K=3", lambda: L.m355_pre_one_hot(_p(lab), _lib.PRE_U8, _i3(shape), 3, _p(oh), _p(bad),
                                                          _stream()), S + 3 * S),
        ("pre_image_from_labels 2", lambda: L.m355_pre_image_from_labels(e, 2, _i3(shape), 1, _p(ifl), _stream()),
         2 * S + 4 * S),
    ]
    print(f"# streaming kernels on {shape} (one channel); yardstick: 5.5-6.2 TB/s of plain streaming kernels (DESIGN §7)")
    print(f"{'kernel':28s} {'us/launch':>10s} {'GB/s':>8s}")
    for name, fn, nbytes in kernels:
        for _ in range(3):
            assert fn() == 0, name
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        print(f"{name:28s} {us:10.1f} {nbytes / us / 1e3:8.0f}")


def count(trace_dir, calls):
    import csv
    import glob
    kern = [r for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
            for r in csv.DictReader(open(f))]
    pre = sum(1 for r in kern if "m355::pre_" in r["Kernel_Name"])
    aug = sum(1 for r in kern if "m355::aug_" in r["Kernel_Name"])
    fill = sum(1 for r in kern if "fillBuffer" in r["Kernel_Name"])
    copy = sum(1 for r in kern if "copyBuffer" in r["Kernel_Name"])
    other = len(kern) - pre - aug - fill - copy
    print(f"per subject: {(pre + aug + fill + copy) / calls:.1f} launches = {pre / calls:.1f} preprocessing + "
          f"{aug / calls:.1f} augmentation kernels + {fill / calls:.1f} memsets + {copy / calls:.1f} copy kernels; "
          f"other kernels in the trace: {other}")


def cpu(reps):
    """the float64 numpy restatement of each 'default' chain (tests/preprocess_ref.py), seconds per subject"""
    import test_preprocessing_gpu as T
    print("# numpy restatement (float64, one thread)")
    for label, kind, training in CASES:
        if training:
            continue
        imgs, labs, sp, _ = T.subject(kind)
        t0 = time.perf_counter()
        for _ in range(reps):
            T.reference(kind, None, imgs, labs, sp)
        print(f"{label:24s} {(time.perf_counter() - t0) / reps:10.3f} s/subject")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--no-rates", action="store_true")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", type=int, default=None, help="run only this case (index into CASES)")
    ap.add_argument("--count", default=None, help="trace directory of one --case run: launches per subject")
    a = ap.parse_args()
    if a.count:
        count(a.count, a.reps + a.warmup)
    if a.gpu:
        gpu(a.reps, a.warmup, a.case)
        if not a.no_rates:
            rates(a.reps)
    if a.cpu:
        cpu(max(1, a.reps // 10))
