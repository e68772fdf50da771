"""Times the contour-image path (csrc/contour.hip, evaluators.ContourImageEvaluator) at the sizes of the
two production configs:

  counts     ops.slice_counts (one fused pass: every voxel read once for the three axes) against the three
             `(m != 0).sum(dim=...)` torch reductions on the device, and as a multiple of the time HBM needs to read
             the label maps once (the copy rate of MI355X_MICROARCH.md §HBM)
  get_image  one ContourImageEvaluator.get_image call with the volumes on the device against copying the image, target
             and prediction volumes to the host and building the same picture there (tests/contour_ref.py)

    python tools/contour_bench.py [--reps 50] [--out profiles/contour_bench.txt]

Workloads: dmri_hippo validation, 8 x [1, 96, 88, 24] int64 label maps and fp32 images, fixed axial slice, ncol 5;
msseg2 validation, 1 x [1, 192, 224, 176], 'interesting' plane with interesting_slice.  Device times of the count:
CUDA events around each call after warm-up, median of the repeats.  get_image returns a picture on the host, so it is
timed with the wall clock around the call (which ends in the drawing), median of the repeats; the drawing alone is
timed too, since both sides share it.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_RATE = 6.29e12    # float4 copy, MI355X_MICROARCH.md §HBM
WORKLOADS = [("dmri_hippo 8 x [96, 88, 24]", 8, (96, 88, 24), 0.03, dict(plane="Axial", slice_id=10, ncol=5)),
             ("msseg2 1 x [192, 224, 176]", 1, (192, 224, 176), 0.002,
              dict(plane="interesting", slice_id=0, ncol=1, interesting_slice=True))]


def _time_events(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(np.min(times))


def _time_wall(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import matplotlib
    matplotlib.use("Agg")
    import torch
    import contour_ref
    from segmentation_pipeline_amd import ops
    from segmentation_pipeline_amd.evaluators import ContourImageEvaluator, LabelMap, ScalarImage
    lines = [f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}  matplotlib {matplotlib.__version__}",
             f"# counts: median of {a.reps} after {a.warmup} warm-up calls, CUDA events around each call",
             f"# get_image: median of {max(5, a.reps // 5)} wall-clock times, synchronised before each call",
             f"{'workload':30s} {'counts ms':>9s} {'min':>7s} {'x HBM read':>13s} {'3 torch sums ms':>15s} "
             f"{'get_image ms':>12s} {'host path ms':>12s} {'drawing ms':>10s}"]
    print("\n".join(lines), flush=True)
    for name, n, shape, density, args in WORKLOADS:
        g = torch.Generator(device="cuda").manual_seed(0)
        lv = {"left": 1, "right": 2}
        subjects = []
        for i in range(n):
            y = (torch.rand((1,) + shape, generator=g, device="cuda") < density).long() * 2
            y_pred = torch.where(torch.rand((1,) + shape, generator=g, device="cuda") < 0.001, 1, y)
            subjects.append({"name": f"s{i}", "img": ScalarImage(torch.randn((1,) + shape, generator=g, device="cuda")),
                             "y_eval": LabelMap(y, lv), "y_pred_eval": LabelMap(y_pred, lv)})
        maps = [s["y_eval"].data[0] for s in subjects]
        nbytes = sum(m.numel() * m.element_size() for m in maps)

        def fused():
            return ops.slice_counts(maps)[0]

        def torch_sums():
            return [(m != 0).sum(dim=d) for m in maps for d in ((1, 2), (0, 2), (0, 1))]
        assert torch.equal(fused().long(), torch.cat(torch_sums())), "fused counts differ from the torch reductions"
        med, mn = _time_events(fused, a.reps, a.warmup)
        tmed, _ = _time_events(torch_sums, a.reps, a.warmup)

        ev = ContourImageEvaluator(args["plane"], "img", "y_pred_eval", "y_eval", args["slice_id"], True, args["ncol"],
                                   interesting_slice=args.get("interesting_slice", False))

        def device_path():
            for s in subjects:      # (the ranks are found anew in every call, as after a new prediction)
                s["y_eval"].pop("interesting_slice_ids", None)
                s["y_eval"].pop("interesting_slice_counts", None)
            return ev.get_image(subjects)

        def host_mosaics():
            host = [{"name": s["name"], "img": ScalarImage(s["img"].data.cpu()),
                     "y_eval": LabelMap(s["y_eval"].data.cpu(), lv),
                     "y_pred_eval": LabelMap(s["y_pred_eval"].data.cpu(), lv)} for s in subjects]
            return contour_ref.mosaics(host, args["plane"], "img", "y_pred_eval", "y_eval", args["slice_id"],
                                       args["ncol"], args.get("interesting_slice", False))

        def host_path():
            _, img, y, y_pred, labels = host_mosaics()
            return contour_ref.render(img, y, y_pred, labels, legend=True)
        _, img, y, y_pred, labels = host_mosaics()
        reps = max(5, a.reps // 5)
        gmed, _ = _time_wall(device_path, reps, 2)
        hmed, _ = _time_wall(host_path, reps, 2)
        dmed, _ = _time_wall(lambda: contour_ref.render(img, y, y_pred, labels, legend=True), reps, 2)
        ratio = (med * 1e-3) / (nbytes / COPY_RATE)
        line = (f"{name:30s} {med:9.4f} {mn:7.4f} {ratio:12.1f}x {tmed:15.4f} {gmed:12.2f} {hmed:12.2f} {dmed:10.2f}")
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
