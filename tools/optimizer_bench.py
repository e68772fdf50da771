"""Measures the fused optimizer step on the parameter set of the cfg2 model (18.08 M parameters).

  step     the optimizer step alone, four rows: SGD + momentum, SGD + Nesterov + clip, Adam, AdamW + clip + EMA.  The native
           step (optim.FusedSGD / FusedAdam) beside the torch composition it stands in for: the fused=True optimizer,
           clip_grad_norm_(foreach=True) in front of it where the row clips, torch._foreach_lerp_ behind it where the row
           keeps an EMA.  After warm-up the two sides alternate over windows of at least half a second, the composition
           first and last; a window's figure is its wall time per step, the host waiting for the device at both ends.
           Launches per step: the native side's follow from the plan (norm launches + prepare + update launches); the
           composition's are counted from one profiled step (torch.profiler, in a run of its own after the timing).
           Bytes: tensor-sized transfers the algorithm needs (read p, g, state; write p, state; + one read of g for the
           norm; + read and write of the EMA) x 4 B x parameters, over the time.  A tensor class is 72 MB: rows whose
           classes together stay below the 256 MiB Infinity Cache can run at the cache's rate, so the figure is quoted
           beside the 6.29 TB/s float4 copy rate of HBM with the working set next to it.
  train    cfg2 (1 x 4 x 128^3, filters [32, 64, 128, 256, 320], GroupNorm(8), ConvTranspose3d) bf16 trainer.train_step with
           torch.optim.SGD and with FusedSGD at the same hyper-parameters (momentum 0.99, Nesterov), alternating windows.

    python tools/optimizer_bench.py [--window 0.5] [--out profiles/optimizer_bench.txt]
"""
import argparse
import os
import sys
import time
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (1, 4, 128, 128, 128)
FILTERS, DEPTH, CLASSES = [32, 64, 128, 256, 320], 5, 3
COPY_RATE = 6.29e12
CACHE = 256 * 2 ** 20


def cfg2():
    from torch import nn
    from segmentation_pipeline_amd.models import ModularUNet
    return ModularUNet(SHAPE[1], CLASSES, FILTERS, DEPTH, block_params={'normalization_class': partial(nn.GroupNorm, 8)},
                       upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2})


def window(step, seconds):
    import torch
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        step()
        n += 1
        if n % 8 == 0:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= seconds:
                break
    return 1e3 * (time.perf_counter() - t0) / n, n


def alternate(sides, seconds, rounds=3):
    """sides: [(name, fn)] -> {name: [ms per window]}; the first side also closes the sequence"""
    got = {name: [] for name, _ in sides}
    for _ in range(rounds):
        for name, fn in sides:
            got[name].append(window(fn, seconds)[0])
    got[sides[0][0]].append(window(sides[0][1], seconds)[0])
    return got


def count_kernels(step):
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return str(n) if n else "not measured"
    except Exception as e:   # (a profiler that does not start is not a measurement)
        return f"not measured ({type(e).__name__})"


def step_part(a, lines):
    import torch
    from segmentation_pipeline_amd import _lib, optim
    torch.manual_seed(0)
    shapes = [p.shape for p in cfg2().parameters()]
    n = sum(s.numel() for s in shapes)
    T = len(shapes)
    cap = int(_lib.lib().m355_optim_capacity())
    tables = -(-T // cap)
    lines.append(f"# step: {T} tensors, {n / 1e6:.2f} M parameters, {4 * n / 1e6:.1f} MB a tensor class; table capacity {cap} -> "
                 f"{tables} launches a pass; windows of >= {a.window:g} s, torch / native alternating, torch first and last")
    g = torch.Generator(device="cuda").manual_seed(1)

    def params():
        ps = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=g) * 0.1) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-3
        return ps

    rows = [
        ("SGD + momentum", 5, 3, None, None,
         lambda ps, **k: torch.optim.SGD(ps, lr=1e-6, momentum=0.9, fused=True),
         lambda ps, **k: optim.FusedSGD(ps, lr=1e-6, momentum=0.9, **k)),
        ("SGD + Nesterov + clip", 6, 3, 12.0, None,
         lambda ps, **k: torch.optim.SGD(ps, lr=1e-6, momentum=0.99, nesterov=True, fused=True),
         lambda ps, **k: optim.FusedSGD(ps, lr=1e-6, momentum=0.99, nesterov=True, **k)),
        ("Adam", 7, 4, None, None,
         lambda ps, **k: torch.optim.Adam(ps, lr=1e-6, fused=True),
         lambda ps, **k: optim.FusedAdam(ps, lr=1e-6, **k)),
        ("AdamW + clip + EMA", 10, 5, 12.0, 0.999,
         lambda ps, **k: torch.optim.AdamW(ps, lr=1e-6, weight_decay=0.01, fused=True),
         lambda ps, **k: optim.FusedAdam(ps, lr=1e-6, weight_decay=0.01, decoupled_weight_decay=True, **k)),
    ]
    for name, transfers, classes, clip, ema, mk_torch, mk_native in rows:
        pt, pn = params(), params()
        ot = mk_torch(pt)
        on = mk_native(pn, max_grad_norm=clip, ema_decay=ema)
        shadows = [p.detach().clone() for p in pt] if ema is not None else None

        def torch_step():
            if clip is not None:
                torch.nn.utils.clip_grad_norm_(pt, clip, foreach=True)
            ot.step()
            if shadows is not None:
                torch._foreach_lerp_(shadows, [p.detach() for p in pt], 1.0 - ema)

        for _ in range(a.warmup):
            torch_step()
            on.step()
        got = alternate([("torch", torch_step), ("native", on.step)], a.window)
        launches_native = (tables if clip is not None else 0) + 1 + tables
        launches_torch = count_kernels(torch_step)
        nbytes = transfers * 4 * n
        ws = classes * 4 * n
        for side, launches in (("torch", launches_torch), ("native", launches_native)):
            t = got[side]
            rate = nbytes / (min(t) * 1e-3)
            lines.append(f"step  {name:22s} {side:6s} {1e3 * min(t):7.1f} us/step (windows {1e3 * min(t):.1f} .. {1e3 * max(t):.1f})  "
                         f"launches {launches}  {transfers} transfers = {nbytes / 1e6:.0f} MB -> {rate / 1e9:5.0f} GB/s = "
                         f"{rate / COPY_RATE:5.1%} of the 6.29 TB/s HBM copy rate; working set {ws / 1e6:.0f} MB "
                         f"({'inside' if ws < CACHE else 'beyond'} the 256 MiB Infinity Cache)")
            print(lines[-1], flush=True)
        lines.append(f"step  {name:22s} native / torch, ratio of the minima {min(got['native']) / min(got['torch']):.3f}")
        print(lines[-1], flush=True)
        del pt, pn, ot, on, shadows
        torch.cuda.empty_cache()


def train_part(a, lines):
    import torch
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd import optim
    from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss
    from segmentation_pipeline_amd.prediction import StandardPredict
    from segmentation_pipeline_amd.trainer import train_step
    g = torch.Generator().manual_seed(1)
    x = torch.randn(SHAPE, generator=g).cuda()
    lab = torch.randint(0, CLASSES, (SHAPE[0],) + SHAPE[2:], generator=g)
    y = torch.nn.functional.one_hot(lab, CLASSES).permute(0, 4, 1, 2, 3).float().contiguous().cuda()
    crit, pred, dev = HybridLogisticDiceLoss(), StandardPredict(image_names=["X", "y"]), torch.device("cuda")
    hp = dict(lr=1e-3, momentum=0.99, nesterov=True)

    def stepper(make):
        torch.manual_seed(0)
        model = cfg2().cuda()
        opt = make(model.parameters())
        return lambda: train_step(model, crit, opt, pred, {"X": x, "y": y}, dev)

    sides = [("torch.optim.SGD", stepper(lambda ps: torch.optim.SGD(ps, **hp))),
             ("torch.optim.SGD(fused=True)", stepper(lambda ps: torch.optim.SGD(ps, fused=True, **hp))),
             ("FusedSGD", stepper(lambda ps: optim.FusedSGD(ps, **hp))),
             ("FusedSGD + clip + EMA + PolyLR", stepper(lambda ps: optim.FusedSGD(ps, max_grad_norm=12, ema_decay=0.999,
                                                                                   schedule=optim.PolyLR(100000), **hp)))]
    with sp.precision("bf16"):
        for _ in range(a.warmup):
            for _, fn in sides:
                fn()
        got = alternate(sides, max(a.window, 1.0), rounds=2)
    lines.append(f"# train: cfg2 bf16 trainer.train_step, SGD momentum 0.99 Nesterov; windows of >= {max(a.window, 1.0):g} s "
                 "alternating, the first side also last; wall time per step")
    for name, t in got.items():
        lines.append(f"train {name:32s} {min(t):7.2f} ms/step (windows {min(t):.2f} .. {max(t):.2f})")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "optimizer_bench.py measures on the GPU"
    lines = [f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}"]
    print(lines[0], flush=True)
    step_part(a, lines)
    if not a.skip_train:
        train_part(a, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
