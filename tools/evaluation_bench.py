"""Times the fused evaluation pass (ops.eval_scores: argmax over the channels, channel -> label table, TP / FP / FN
counts; csrc/evaluate.hip) on two workloads, against the same evaluation composed from torch ops on the
device and against a CPU restatement of the reference's per-label boolean passes (segmentation_evaluator.py:62-94).

    python tools/evaluation_bench.py [--reps 50] [--out profiles/evaluation_bench.txt]
    rocprofv3 --kernel-trace --stats -d T -o run -- python tools/evaluation_bench.py --reps 20 --no-cpu

Workloads: 8 x [4, 96, 88, 24] fp32 scores with fp32 one-hot targets (dmri_hippo hbt_roi validation, right-half
remap table) and 1 x [2, 192, 224, 176] (msseg2 scale).  Bytes counted are those the pass must read: scores and
targets once.  Device times: CUDA events around each call after warm-up, median of the repeats.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12    # float4 copy, MI355X_MICROARCH.md §HBM
WORKLOADS = [("dmri_hippo hbt_roi 8 x [4, 96, 88, 24]", 8, 4, (96, 88, 24), ([0, 1, 2, 3], [0, 4, 5, 6]), (0, 1),
              [1, 2, 3, 4, 5, 6]),
             ("msseg2 1 x [2, 192, 224, 176]", 1, 2, (192, 224, 176), ([0, 1], [0, 1]), None, [1])]


def _inputs(n, C, sp):
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    scores = [torch.rand((C,) + sp, generator=g, device="cuda") for _ in range(n)]
    targets = [torch.nn.functional.one_hot(torch.randint(0, C, sp, generator=g, device="cuda"), C)
               .permute(3, 0, 1, 2).float().contiguous() for _ in range(n)]
    return scores, targets


def _torch_eval(scores, targets, table, half, labels):
    """the same counts from torch ops on the device (argmax, gather through the table, per-label comparisons)"""
    import torch
    out = []
    for s, t in zip(scores, targets):
        am, ta = torch.argmax(s, 0), torch.argmax(t, 0)
        tab = torch.tensor(table, device=s.device)
        inside = torch.zeros(am.shape, dtype=torch.long, device=s.device)
        if half is not None:
            axis, upper = half
            idx = torch.arange(am.shape[axis], device=s.device).view([-1 if a == axis else 1 for a in range(3)])
            inside = ((idx >= am.shape[axis] // 2) == bool(upper)).long().expand(am.shape)
        p, q = tab[inside, am], tab[inside, ta]
        rows = []
        for v in labels:
            mp, mt = p == v, q == v
            rows.append(torch.stack([(mp & mt).sum(), (mp & ~mt).sum(), (~mp & mt).sum()]))
        out.append(torch.stack(rows))
    return torch.stack(out)


def _cpu_reference_style(pred_maps, target_maps, labels):
    """the reference's loop on the host: per subject and label four boolean passes, one .item() per statistic"""
    out = []
    for p, t in zip(pred_maps, target_maps):
        for v in labels:
            pl, tl = p == v, t == v
            TP = (tl & pl).sum(dim=(1, 2, 3)).float()
            FP = (~tl & pl).sum(dim=(1, 2, 3)).float()
            TN = (~tl & ~pl).sum(dim=(1, 2, 3)).float()
            FN = (tl & ~pl).sum(dim=(1, 2, 3)).float()
            stats = [TP + FN, TP + FP, TP, FP, TN, FN, 2 * TP / (2 * TP + FP + FN), TP / (TP + FP), TP / (TP + FN)]
            out.append([x.item() for x in stats])
    return out


def _time(fn, reps, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from segmentation_pipeline_amd import ops
    lines = [f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"# median of {a.reps} after {a.warmup} warm-up calls; CUDA events around each call",
             f"{'workload':40s} {'fused ms':>9s} {'min':>7s} {'TB/s':>6s} {'% copy':>7s} {'torch ms':>9s} {'cpu ms':>9s}"]
    print("\n".join(lines), flush=True)
    for name, n, C, sp, table, half, labels in WORKLOADS:
        scores, targets = _inputs(n, C, sp)
        nbytes = sum(s.numel() * 4 + t.numel() * 4 for s, t in zip(scores, targets))

        def fused():
            return ops.eval_scores(scores, table, labels, targets=targets, half=half)[0]
        counts = fused()
        ref = _torch_eval(scores, targets, table, half, labels)
        assert torch.equal(counts, ref), "fused counts differ from the torch composition"
        med, mn = _time(fused, a.reps, a.warmup)
        tmed, _ = _time(lambda: _torch_eval(scores, targets, table, half, labels), max(5, a.reps // 5), 2)
        cpu_ms = float("nan")
        if not a.no_cpu:
            _, maps, tmaps = ops.eval_scores(scores, table, labels, targets=targets, half=half, write_pred=True,
                                             write_target=True)
            pm, tm = [m.cpu() for m in maps], [m.cpu() for m in tmaps]
            t0 = time.perf_counter()
            _cpu_reference_style(pm, tm, labels)
            cpu_ms = (time.perf_counter() - t0) * 1e3
        rate = nbytes / (med * 1e-3)
        line = (f"{name:40s} {med:9.4f} {mn:7.4f} {rate / 1e12:6.2f} {100 * rate / COPY_RATE:6.1f}% {tmed:9.3f} "
                f"{cpu_ms:9.1f}")
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
