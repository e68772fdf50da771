"""Times the distance transform and the surface-distance evaluator (csrc/distance.hip, evaluators.SurfaceDistanceEvaluator;
DESIGN §4.20) at 128^3 and 256 x 256 x 192:

  edt_sq     ops.edt_sq alone (three launches) on two kinds of sites -- the border of an ellipsoid, which is what the
             evaluator feeds it, and random sites at p = 0.01 --, device time between events, and its three kernels one
             by one from the torch profiler's device timeline (where the profiler is usable), each next to the bytes the
             pass must move (D sweep: 1 B read + 2 B written per voxel; H pass: 2 B + 4 B; W pass: 4 B + 4 B) as a
             fraction of the HBM copy rate
  evaluator  one SurfaceDistanceEvaluator call, one subject with two labels on the device (wall clock: the call ends
             in a copy to the host), against the same statistics on the host with scipy.ndimage (copy of both label
             maps included), where scipy is installed

    python tools/surface_distance_bench.py [--reps 20] [--out profiles/surface_distance_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12    # float4 copy, MI355X_MICROARCH.md §HBM
SHAPES = [(128, 128, 128), (256, 256, 192)]
PASS_BYTES = {"edt_d_kernel": 3, "edt_line_kernel<true>": 6, "edt_line_kernel<false>": 8}   # per voxel
LABELS = {"inner": 1, "outer": 2}


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


def _kernel_times(fn, reps):
    """{kernel name prefix: mean device ms per call} from the profiler's device timeline, or {} when it is not usable"""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            total = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)
            for key in PASS_BYTES:
                if key in e.key and total:
                    out[key] = out.get(key, 0.0) + total / 1e3 / reps
        return out
    except Exception as err:   # noqa: BLE001 -- the profiler is an extra here; the event times stand without it
        print(f"# profiler not usable: {err!r}", flush=True)
        return {}


def _blobs(shape, shift):
    import torch
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, device="cuda", dtype=torch.float32) for n in shape], indexing="ij"), -1)
    size = torch.tensor(shape, device="cuda", dtype=torch.float32)
    r2 = (((grid - (size - 1) / 2 - shift) / (size * 0.33)) ** 2).sum(-1)
    out = torch.zeros(shape, dtype=torch.int64, device="cuda")
    out[r2 <= 1.0] = 2
    out[r2 <= 0.3] = 1
    return out


def _host_stats(pred, target, spacing):
    from scipy import ndimage
    p, t = pred.cpu().numpy(), target.cpu().numpy()
    structure = ndimage.generate_binary_structure(3, 1)
    out = {}
    for name, v in LABELS.items():
        bp = (p == v) ^ ndimage.binary_erosion(p == v, structure, border_value=0)
        bt = (t == v) ^ ndimage.binary_erosion(t == v, structure, border_value=0)
        a = ndimage.distance_transform_edt(~bt, sampling=spacing)[bp]
        b = ndimage.distance_transform_edt(~bp, sampling=spacing)[bt]
        both = np.concatenate([a, b])
        out[name] = (both.max(), np.percentile(both, 95), (a.mean() + b.mean()) / 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from segmentation_pipeline_amd import ops
    from segmentation_pipeline_amd.evaluators import LabelMap, SurfaceDistanceEvaluator
    try:
        import scipy
        scipy_version = scipy.__version__
    except ImportError:
        scipy_version = None
    lines = [f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}  scipy {scipy_version}",
             f"# command: python tools/surface_distance_bench.py --reps {a.reps} --warmup {a.warmup}",
             f"# edt_sq: median (min) of {a.reps} calls after {a.warmup} warm-up calls, CUDA events around each call; kernels: "
             f"mean over {a.reps} calls from the profiler's device timeline; 'of HBM' = bytes the pass must move / time / "
             f"{COPY_RATE / 1e12:.2f} TB/s",
             "# evaluator: median wall clock of the call (one subject, two labels, maps on the device, table on the host); "
             "scipy: the same statistics on the host, one run"]
    print("\n".join(lines), flush=True)
    spacing = (1.0, 1.0, 1.2)
    for shape in SHAPES:
        S = int(np.prod(shape))
        target, pred = _blobs(shape, 0.0), _blobs(shape, 3.0)
        x = target.to(torch.int32)
        border, count = ops.surface_mask(x, 2)
        sparse = (torch.rand(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)) < 0.01).to(torch.uint8)
        mmed, _ = _time_events(lambda: ops.surface_mask(x, 2, border=border, count=count), a.reps, a.warmup)
        line = (f"{'x'.join(map(str, shape)):12s} surface_mask {mmed:8.4f} ms  {5 * S / (mmed * 1e-3) / COPY_RATE:6.1%} of HBM "
                f"(4 B + 1 B per voxel)")
        print(line, flush=True)
        lines.append(line)
        for kind, sites in (("border sites", border), ("random p=0.01", sparse)):
            d2 = torch.empty(shape, dtype=torch.float32, device="cuda")
            ws = torch.empty(2 * S + 256, dtype=torch.uint8, device="cuda")

            def run():
                return ops.edt_sq(sites, spacing, out=d2, workspace=ws)
            med, mn = _time_events(run, a.reps, a.warmup)
            line = (f"{'x'.join(map(str, shape)):12s} edt_sq {kind:14s} {med:8.4f} ms (min {mn:.4f})  "
                    f"{17 * S / (med * 1e-3) / COPY_RATE:6.1%} of HBM (17 B per voxel)")
            print(line, flush=True)
            lines.append(line)
            for key, ms in sorted(_kernel_times(run, a.reps).items()):
                line = f"{'':12s}   {key:24s} {ms:8.4f} ms  {PASS_BYTES[key] * S / (ms * 1e-3) / COPY_RATE:6.1%} of HBM"
                print(line, flush=True)
                lines.append(line)
            if scipy_version is not None and kind == "border sites":
                from scipy import ndimage
                host = (sites == 0).cpu().numpy()
                t0 = time.perf_counter()
                ref = ndimage.distance_transform_edt(host, sampling=spacing)
                ms = (time.perf_counter() - t0) * 1e3
                err = np.abs(np.sqrt(run().double().cpu().numpy()) - ref).max()
                line = f"{'':12s}   scipy distance_transform_edt on the host {ms:10.1f} ms  (max |difference| {err:.2e})"
                print(line, flush=True)
                lines.append(line)
        subject = {"name": "s0", "pred": LabelMap(pred[None], LABELS), "target": LabelMap(target[None], LABELS)}
        ev = SurfaceDistanceEvaluator("pred", "target", spacing=spacing)
        res = ev([subject])
        emed, emin = _time_wall(lambda: ev([subject]), max(5, a.reps // 2), 2)
        line = f"{'x'.join(map(str, shape)):12s} evaluator 1 subject x 2 labels {emed:10.2f} ms (min {emin:.2f})"
        if scipy_version is not None:
            t0 = time.perf_counter()
            host = _host_stats(pred, target, spacing)
            line += f"   scipy on the host {(time.perf_counter() - t0) * 1e3:10.1f} ms"
            df = res["subject_stats"]
            for name in LABELS:
                got = df[df["label"] == name].iloc[0]
                assert np.allclose([got["hd"], got["hd95"], got["assd"]], host[name], rtol=2e-6), (name, got, host[name])
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
