"""Measures deep supervision: the target pyramid kernel, and what the auxiliary heads cost a training step.

  kernel   m355_target_pyramid on 1 x 4 x 128^3 with levels = 3, area and nearest mode, beside three successive
           F.avg_pool3d(., 2) on the device (what one would write without the kernel), interleaved.  Bytes the
           algorithm moves, from the shapes: area reads the target once and writes the three levels; nearest reads the
           rows with even z and y (a quarter of the target) and writes the three levels; the pooling chain reads the target,
           writes level 1, reads it, writes level 2, reads it, writes level 3.  The share of the 6.29 TB/s float4 copy rate of
           the chip is quoted beside each -- the 33.5 MB target fits the 256 MiB Infinity Cache between calls, so a figure
           above 100 % is the cache's rate, not HBM's.
  step     cfg2 (1 x 4 x 128^3, filters [32, 64, 128, 256, 320], GroupNorm(8), ConvTranspose3d) in fp32 and bf16:
           DeepSupervisionUNet(aux_levels=3) + DeepSupervisionLoss(HybridLogisticDiceLoss()) against ModularUNet +
           HybridLogisticDiceLoss(), eager SGD steps in one process.  After warm-up the two alternate over windows of at
           least a second each, the yardstick first and last; a window's figure is its wall time per step (the host waits for
           the device at both ends).

    python tools/deep_supervision_bench.py [--window 1.0] [--warmup 5] [--out profiles/deep_supervision_bench.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (1, 4, 128, 128, 128)
LEVELS = 3
COPY_RATE = 6.29e12     # bytes / s, float4 copy
FILTERS, DEPTH, CLASSES = [32, 64, 128, 256, 320], 5, 3


def _time_interleaved(fns, batches, calls, warmup):
    import torch
    times = [[] for _ in fns]
    for r in range(warmup + batches):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[k].append(e0.elapsed_time(e1) / calls)
    return [(min(t), statistics.median(t)) for t in times]


def kernel_part(a, lines):
    import torch
    import torch.nn.functional as F
    from segmentation_pipeline_amd import _lib
    L = _lib.lib()
    N, Cc, D, H, W = SHAPE
    g = torch.Generator(device="cuda").manual_seed(0)
    lab = torch.randint(0, Cc, (N, D, H, W), generator=g, device="cuda")
    y = F.one_hot(lab, Cc).permute(0, 4, 1, 2, 3).float().contiguous()
    n_out = int(L.m355_target_pyramid_elems(N, Cc, D, H, W, LEVELS))
    out = torch.empty(n_out, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def pyramid(mode):
        def fn():
            rc = L.m355_target_pyramid(C.c_void_p(y.data_ptr()), N, Cc, D, H, W, LEVELS, mode, C.c_void_p(out.data_ptr()), st)
            assert rc == 0, L.m355_last_error()
        return fn

    def pool_chain():
        t = y
        for _ in range(LEVELS):
            t = F.avg_pool3d(t, 2)
        return t

    n_in = y.numel()
    level = [n_in >> (3 * j) for j in range(1, LEVELS + 1)]
    nbytes = {"area": 4 * (n_in + n_out), "nearest": 4 * (n_in // 4 + n_out),
              "avg_pool3d x 3": 4 * (n_in + 2 * level[0] + 2 * level[1] + level[2])}
    cols = [("avg_pool3d x 3", pool_chain), ("area", pyramid(0)), ("nearest", pyramid(1)), ("avg_pool3d x 3 again", pool_chain)]
    res = _time_interleaved([fn for _, fn in cols], a.batches, a.calls, 3)
    lines.append(f"# kernel: target {'x'.join(map(str, SHAPE))} fp32 one-hot, levels {LEVELS}; minimum (median) over {a.batches} "
                 f"batches of {a.calls} calls, per call, the columns interleaved, CUDA events around each batch")
    for (name, _), (best, med) in zip(cols, res):
        nb = nbytes[name.replace(" again", "")]
        rate = nb / (best * 1e-3)
        lines.append(f"kernel  {name:22s} {1e3 * best:7.1f} us ({1e3 * med:7.1f})  {nb / 1e6:6.1f} MB  {rate / 1e9:6.0f} GB/s  "
                     f"{rate / COPY_RATE:6.1%} of the 6.29 TB/s copy rate")
        print(lines[-1], flush=True)


def step_part(a, lines, precision):
    import torch
    from torch import nn
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd.criterions import DeepSupervisionLoss, HybridLogisticDiceLoss
    from segmentation_pipeline_amd.models import DeepSupervisionUNet, ModularUNet
    kw = dict(block_params={'normalization_class': partial(nn.GroupNorm, 8)}, upsample_class=nn.ConvTranspose3d,
              upsample_params={'kernel_size': 2, 'stride': 2})
    g = torch.Generator().manual_seed(1)
    x = torch.randn(SHAPE, generator=g).cuda()
    lab = torch.randint(0, CLASSES, (SHAPE[0],) + SHAPE[2:], generator=g)
    y = torch.nn.functional.one_hot(lab, CLASSES).permute(0, 4, 1, 2, 3).float().contiguous().cuda()

    def stepper(model, crit):
        model = model.cuda().train()
        opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)

        def step():
            opt.zero_grad(set_to_none=True)
            ld = crit(model(x), y)
            ld["loss"].backward()
            opt.step()
        return step

    torch.manual_seed(0)
    base = stepper(ModularUNet(SHAPE[1], CLASSES, FILTERS, DEPTH, **kw), HybridLogisticDiceLoss())
    torch.manual_seed(0)
    ds = stepper(DeepSupervisionUNet(SHAPE[1], CLASSES, FILTERS, DEPTH, aux_levels=3, **kw),
                 DeepSupervisionLoss(HybridLogisticDiceLoss()))

    def window(step):
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        while True:
            step()
            n += 1
            if n % 4 == 0:
                torch.cuda.synchronize()
                if time.perf_counter() - t0 >= a.window:
                    break
        return 1e3 * (time.perf_counter() - t0) / n, n

    with sp.precision(precision):
        for _ in range(a.warmup):
            base()
            ds()
        order = [("ModularUNet", base), ("DeepSupervisionUNet", ds), ("ModularUNet", base), ("DeepSupervisionUNet", ds),
                 ("ModularUNet", base)]
        got = [(name,) + window(fn) for name, fn in order]
    yard = [ms for name, ms, _ in got if name == "ModularUNet"]
    new = [ms for name, ms, _ in got if name != "ModularUNet"]
    lines.append(f"step {precision}: windows in order  " + "  ".join(f"{name} {ms:.2f} ms/step ({n} steps)" for name, ms, n in got))
    lines.append(f"step {precision}: ModularUNet + HybridLogisticDiceLoss {min(yard):.2f} ms (windows {min(yard):.2f} .. {max(yard):.2f}),  "
                 f"DeepSupervisionUNet(aux_levels=3) + DeepSupervisionLoss {min(new):.2f} ms (windows {min(new):.2f} .. {max(new):.2f}),  "
                 f"ratio of the minima {min(new) / min(yard):.3f}")
    print("\n".join(lines[-2:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--window", type=float, default=1.0, help="least seconds per timed window of the training-step part")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "deep_supervision_bench.py measures on the GPU"
    lines = [f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}"]
    print(lines[0], flush=True)
    kernel_part(a, lines)
    lines.append(f"# step: cfg2 ({'x'.join(map(str, SHAPE))}, filters {FILTERS}, GroupNorm(8), ConvTranspose3d), eager SGD steps; "
                 f"{a.warmup} warm-up steps each, then windows of >= {a.window:g} s alternated, the yardstick first and last; "
                 "wall time per step")
    for precision in ("fp32", "bf16"):
        step_part(a, lines, precision)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
