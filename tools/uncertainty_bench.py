"""Times the calibration pass (ops.eval_calibration; csrc/calibration.hip) and the entropy pass (ops.predictive_entropy;
csrc/uncertainty.hip) on two workloads, each next to a plain streaming read of the same tensors measured
in the same run (torch's .sum() over them) and next to the same statistics composed from torch ops on the device; and
EnsembleFlips on the cfg2 network with and without uncertainty=True.

    python tools/uncertainty_bench.py [--reps 30] [--out profiles/uncertainty_bench.txt]

Workloads: 1 x [4, 128, 128, 128] and 1 x [2, 256, 256, 192] fp32 softmax probabilities; calibration targets are int64
index maps; 15 bins.  The calibration pass is timed on random softmax probabilities and on confident ones (most top
labels in the last bin, where the LDS atomics of a wave meet on three addresses).
Device times: CUDA events around each call after warm-up, median of the repeats.
"""
import argparse
import os
import sys
from functools import partial

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = [("1 x [4, 128, 128, 128]", 4, (128, 128, 128)), ("1 x [2, 256, 256, 192]", 2, (256, 256, 192))]
BINS = 15


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
    return float(np.median(times))


def _torch_calibration(p, idx, bins):
    """top-label counts, hits and confidence sums, Brier and NLL from torch ops on the device (no classwise tables)"""
    import torch
    q, arg = p.max(dim=0)
    b = torch.bucketize(q, torch.linspace(0, 1, bins + 1, device=p.device)[1:-1], right=True).flatten()
    hit = (arg == idx).flatten()
    count = torch.bincount(b, minlength=bins)
    hits = torch.bincount(b, weights=hit.double(), minlength=bins)
    conf = torch.bincount(b, weights=q.flatten().double(), minlength=bins)
    y = torch.nn.functional.one_hot(idx, p.shape[0]).movedim(-1, 0)
    brier = ((p.double() - y) ** 2).sum()
    nll = -torch.log((p.gather(0, idx[None]).double() + 1e-8) / (1 + 1e-8)).sum()
    return count, hits, conf, brier, nll


def _torch_entropy(p):
    return -(p * p.log()).sum(1, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-ensemble", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from torch import nn
    from segmentation_pipeline_amd import ops
    from segmentation_pipeline_amd.models import EnsembleFlips, ModularUNet
    lines = [f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"# median ms of {a.reps} calls after {a.warmup} warm-up calls; CUDA events around each call",
             "# read: torch .sum() over the same tensors in the same run (a plain streaming read of the bytes the pass reads)"]
    print("\n".join(lines), flush=True)

    def emit(line):
        print(line, flush=True)
        lines.append(line)
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, C, sp in WORKLOADS:
        for what, scale in (("random softmax(2.5 randn)", 2.5), ("confident softmax(12 randn)", 12.0)):
            p = torch.softmax(scale * torch.randn((C,) + sp, generator=g, device="cuda"), dim=0)
            idx = torch.multinomial(p.reshape(C, -1).T.contiguous(), 1, generator=g)[:, 0].reshape(sp)
            mb = (p.numel() * 4 + idx.numel() * 8) / 2 ** 20
            read = _time(lambda: (p.sum(), idx.sum()), a.reps, a.warmup)
            cal = _time(lambda: ops.eval_calibration([p], [idx], BINS), a.reps, a.warmup)
            tt = _time(lambda: _torch_calibration(p, idx, BINS), max(5, a.reps // 3), 2)
            last = int(ops.eval_calibration([p], [idx], BINS).top[0, -1, 0]) / idx.numel()
            emit(f"calibration {name} {what} ({mb:.0f} MiB, {100 * last:.0f}% of top labels in the last bin): "
                 f"pass {cal:.3f}  read {read:.3f}  torch (top-label table only) {tt:.3f}")
        for dtype in (torch.float32, torch.bfloat16):
            q = p[None].to(dtype)
            read = _time(lambda: q.sum(), a.reps, a.warmup)
            ent = _time(lambda: ops.predictive_entropy(q), a.reps, a.warmup)
            entc = _time(lambda: ops.predictive_entropy(q, confidence=True), a.reps, a.warmup)
            tt = _time(lambda: _torch_entropy(q), a.reps, a.warmup)
            emit(f"entropy {name} {str(dtype).split('.')[1]} ({q.numel() * q.element_size() / 2 ** 20:.0f} MiB read): "
                 f"pass {ent:.3f}  with confidence {entc:.3f}  read {read:.3f}  torch -(p * p.log()).sum(1) {tt:.3f}")
        qb = torch.sigmoid(2.5 * torch.randn((1, C) + sp, generator=g, device="cuda"))
        emit(f"entropy {name} binary float32: pass {_time(lambda: ops.predictive_entropy(qb, 'binary'), a.reps, a.warmup):.3f}  "
             f"read {_time(lambda: qb.sum(), a.reps, a.warmup):.3f}  "
             f"torch {_time(lambda: -(qb * qb.log() + (1 - qb) * (1 - qb).log()), a.reps, a.warmup):.3f}")
    if not a.no_ensemble:
        torch.manual_seed(0)
        model = ModularUNet(4, 3, [32, 64, 128, 256, 320], 5, block_params={'normalization_class': partial(nn.GroupNorm, 8)},
                            upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2}).cuda().eval()
        x = torch.randn((1, 4, 128, 128, 128), generator=g, device="cuda")
        with torch.no_grad():
            reps = max(3, a.reps // 10)
            plain = _time(lambda: EnsembleFlips(model)(x), reps, 1)
            uq = _time(lambda: EnsembleFlips(model, uncertainty=True)(x), reps, 1)
        emit(f"EnsembleFlips cfg2 network, 1 x 4 x 128^3, 8 members: mean only {plain:.2f}  with uncertainty=True {uq:.2f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
