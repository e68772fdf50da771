"""Times ops.region_stats (csrc/region_stats.hip) at 256 x 256 x 192 with one float32 image and an int16
label map, for L = 2 and L = 8 label values, with and without the median:

  call      device time of one call between events (median and minimum of --reps calls after --warmup), the bytes its
            passes must read -- the label map for the count pass, label map + image for the sum pass and for every
            region group of every deviation / select pass -- and the resulting rate next to the streaming rate of plain
            kernels on this part (5.5 - 6.2 TB/s)
  kernels   the same per kernel from the torch profiler's device timeline, where the profiler is usable
  host      what the feature competes with: `.cpu()` of the same image and label tensors alone (wall clock), and the
            statistics on the host after that copy with torch on 16 threads

The one condition (exit status 1 when it does not hold): a full call with the median takes less time than the copy of
its inputs to the host.

    python tools/region_stats_bench.py [--reps 20] [--out profiles/region_stats_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_RATE = (5.5e12, 6.2e12)    # plain streaming kernels on this part, DESIGN §4.7 and §4.18
SHAPE = (256, 256, 192)
KERNELS = ("rs_count_kernel", "rs_sum_kernel", "rs_scan_kernel<true, true>", "rs_scan_kernel<false, true>",
           "rs_scan_kernel<true, false>", "rs_pick_kernel", "rs_mean_kernel", "rs_finalize_kernel", "rs_init_kernel")


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
    """{kernel: (mean device ms per launch, launches per call)} from the profiler's device timeline, {} when unusable"""
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
            for key in KERNELS:
                if key in e.key and total:
                    t, c = out.get(key, (0.0, 0))
                    out[key] = (t + total / 1e3, c + e.count)
        return {k: (t / c, c / reps) for k, (t, c) in out.items()}
    except Exception as err:   # noqa: BLE001 -- the profiler is an extra here; the event times stand without it
        print(f"# profiler not usable: {err!r}", flush=True)
        return {}


def _labels(L):
    """L nested shells around the centre, values 1 .. L, background 0"""
    import torch
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, device="cuda", dtype=torch.float32) for n in SHAPE], indexing="ij"), -1)
    size = torch.tensor(SHAPE, device="cuda", dtype=torch.float32)
    r2 = (((grid - (size - 1) / 2) / (size * 0.45)) ** 2).sum(-1)
    out = torch.zeros(SHAPE, dtype=torch.int16, device="cuda")
    for v in range(L, 0, -1):
        out[r2 <= v / L] = v
    return out


def _pass_bytes(L, median, group):
    """bytes each kernel must read per launch, and per call"""
    S = SHAPE[0] * SHAPE[1] * SHAPE[2]
    groups = -(-(L + 2) // group)
    per = {"rs_count_kernel": 2 * S, "rs_sum_kernel": 6 * S, "rs_scan_kernel<true, true>": 6 * S * groups,
           "rs_scan_kernel<false, true>": 6 * S * groups, "rs_scan_kernel<true, false>": 6 * S}
    total = per["rs_count_kernel"] + per["rs_sum_kernel"] + (3 * 6 * S * groups if median else 6 * S)
    return per, total, groups


def _host_stats(lab, img, values):
    import torch
    x = img[0]
    out = []
    for m in [lab == v for v in values] + [lab != 0, torch.ones_like(lab, dtype=torch.bool)]:
        sel = x[m]
        out.append((sel.double().mean().item(), sel.double().std().item(), sel.median().item(), sel.min().item(),
                    sel.max().item()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from segmentation_pipeline_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("region_stats_bench needs the GPU: nothing is timed without one")
    torch.set_num_threads(16)
    group = ops.region_stats_plan()[3]
    lines = [f"ops.region_stats at {SHAPE[0]} x {SHAPE[1]} x {SHAPE[2]}, one float32 image, int16 labels "
             f"({torch.cuda.get_device_name(0)}; median / min of {args.reps} calls after {args.warmup})",
             f"rates are bytes the passes must read over time; plain streaming kernels on this part reach "
             f"{STREAM_RATE[0] / 1e12:.1f} - {STREAM_RATE[1] / 1e12:.1f} TB/s (DESIGN §4.7, §4.18)", ""]
    g = torch.Generator(device="cuda").manual_seed(0)
    img = torch.randn((1,) + SHAPE, generator=g, device="cuda") * 50 + 300
    full_call = {}
    for L in (2, 8):
        lab = _labels(L)
        values = list(range(1, L + 1))
        for median in (True, False):
            per, total, groups = _pass_bytes(L, median, group)
            fn = lambda: ops.region_stats(lab, [img], values, median=median)   # noqa: E731
            med, low = _time_events(fn, args.reps, args.warmup)
            full_call[(L, median)] = med
            lines.append(f"L = {L}, median = {median}: {med:.3f} ms (min {low:.3f}), {total / 1e6:.0f} MB to read in "
                         f"{2 + (3 * groups if median else 1)} passes" + (f" ({groups} region group(s) per select pass)" if median else "") + " -> "
                         f"{total / med / 1e6:.0f} GB/s = {100 * total / med * 1e3 / STREAM_RATE[0]:.0f} % of {STREAM_RATE[0] / 1e12:.1f} TB/s")
            for name, (ms, launches) in sorted(_kernel_times(fn, 5).items(), key=lambda kv: KERNELS.index(kv[0])):
                rate = f", {per[name] / 1e6:.0f} MB -> {per[name] / ms / 1e6:.0f} GB/s" if name in per else ""
                lines.append(f"    {name:<30s} {ms * 1e3:9.1f} us x {launches:g}{rate}")
        lines.append("")
    lab = _labels(2)
    copy_med, copy_low = _time_wall(lambda: (img.cpu(), lab.cpu()), args.reps, args.warmup)
    himg, hlab = img.cpu(), lab.cpu()
    host_med, host_low = _time_wall(lambda: _host_stats(hlab, himg, [1, 2]), 3, 1)
    lines += [f".cpu() of the image ({img.numel() * 4 / 1e6:.0f} MB) and the label map ({lab.numel() * 2 / 1e6:.0f} MB) alone: "
              f"{copy_med:.3f} ms (min {copy_low:.3f})",
              f"the statistics of L = 2 on the host after that copy (torch, 16 threads): {host_med:.1f} ms (min {host_low:.1f})",
              ""]
    ok = all(full_call[(L, True)] < copy_med for L in (2, 8))
    lines.append(f"condition: a full call with the median ({full_call[(2, True)]:.3f} ms at L = 2, {full_call[(8, True)]:.3f} ms "
                 f"at L = 8) takes less time than the copy of its inputs to the host ({copy_med:.3f} ms): "
                 f"{'holds' if ok else 'DOES NOT HOLD'}")
    lines += ["",
              "what bounds each pass: none of them comes near the HBM rate; what each pays per voxel, beyond the bytes:",
              "rs_count_kernel reads 2 bytes per voxel and pays two integer divisions and six min / max per voxel;",
              "rs_sum_kernel and the deviation pass stream 6 bytes per voxel through 4- and 2-byte loads with an fp64 add",
              "per value and, per region met in a wave step, a masked fp64 butterfly, so they slow down as more waves",
              "straddle region borders (L = 8 against L = 2); the select passes are bound by LDS atomics (up to three",
              "histogram updates per value, serialised where many lanes hit one bin) at two blocks per CU, and read the",
              "volume once per group of seven regions."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
