"""Times the batched signed distance transform and the boundary loss (csrc/distance.hip, csrc/boundary_loss.hip; DESIGN
§4.27).

  transform   ops.signed_distance on three seeded synthetic targets, the background channel switched off (the criterion's
              default):
                sparse   1 x 4 x 128^3, a few blobs of radius 2-4 per foreground channel (msseg2-like lesions)
                large    1 x 4 x 128^3, one large ellipsoid per foreground channel
                hippo    2 x 8 x 96 x 88 x 24, nested thin shells (dmri_hippo-like subfields)
              The yardstick is the code that existed before the batched transform: per selected plane two ops.edt_sq calls
              on the two uint8 masks, two ops.edt_sqrt and the torch elementwise combine (no host read: the uniform-plane
              rule is a torch.where on the infinities).  The two variants alternate in one process; a sample is `calls`
              back-to-back calls between two device events; the figure is the median over the samples, per call.
              Bytes per voxel of a selected plane: sweep 4 read + 2 written, first line pass 2 + 4, last line pass 4 + 4 =
              20; the yardstick moves 2 x (1 + 2, 2 + 4, 4 + 4, 4 + 4) = 50 and the masks and the combine on top.
              Per-pass times come from torch's profiler (device durations of the three kernels) when it is available.
  loss        ops.boundary_loss forward and backward on the sparse target's phi and a random softmax: 8 B / element read
              in the forward, 4 read + 4 written in the backward.
  step        cfg2 (1 x 4 x 128^3 input, 3 classes), eager SGD, BoundaryLoss(HybridLogisticDiceLoss()) against
              HybridLogisticDiceLoss() alone: windows of at least `--window` seconds, alternated; ms / step is the median
              over the windows.  The target has small blobs in class 1 and a large ellipsoid in class 2.

    python tools/boundary_loss_bench.py [--samples 15] [--calls 3] [--warmup 3] [--window 1.0] [--rounds 3]
                                        [--no-step] [--out profiles/boundary_loss_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12   # B/s, the device-to-device copy rate all profiles here are quoted against


def _grid(shape, device):
    import torch
    return torch.meshgrid(*[torch.arange(float(n), device=device) for n in shape], indexing="ij")


def _ellipsoid(grid, centre, radii):
    return sum(((g - c) / r) ** 2 for g, c, r in zip(grid, centre, radii)) <= 1.0


def sparse_target(shape, classes, seed, device, blobs=5):
    """[1, classes, *shape] one-hot: `blobs` balls of radius 2-4 per foreground channel, channel 0 the rest"""
    import torch
    g = torch.Generator().manual_seed(seed)
    grid = _grid(shape, device)
    lab = torch.zeros(shape, dtype=torch.long, device=device)
    for c in range(1, classes):
        for _ in range(blobs):
            centre = [float(torch.randint(6, n - 6, (1,), generator=g)) for n in shape]
            r = 2.0 + 2.0 * float(torch.rand(1, generator=g))
            lab[_ellipsoid(grid, centre, (r, r, r))] = c
    return torch.nn.functional.one_hot(lab, classes).permute(3, 0, 1, 2)[None].float().contiguous()


def large_target(shape, classes, seed, device):
    """one ellipsoid with radii of 15-30 % of the axes per foreground channel"""
    import torch
    g = torch.Generator().manual_seed(seed)
    grid = _grid(shape, device)
    lab = torch.zeros(shape, dtype=torch.long, device=device)
    for c in range(1, classes):
        centre = [n * (0.3 + 0.4 * float(torch.rand(1, generator=g))) for n in shape]
        radii = [n * (0.15 + 0.15 * float(torch.rand(1, generator=g))) for n in shape]
        lab[_ellipsoid(grid, centre, radii)] = c
    return torch.nn.functional.one_hot(lab, classes).permute(3, 0, 1, 2)[None].float().contiguous()


def hippo_target(n, classes, shape, seed, device):
    """[n, classes, *shape]: nested ellipsoidal shells about two voxels thick around a seeded centre, one label each"""
    import torch
    g = torch.Generator().manual_seed(seed)
    grid = _grid(shape, device)
    out = []
    for _ in range(n):
        centre = [s * (0.4 + 0.2 * float(torch.rand(1, generator=g))) for s in shape]
        rho = torch.sqrt(sum(((gr - c) / (0.45 * s)) ** 2 for gr, c, s in zip(grid, centre, shape)))
        lab = torch.zeros(shape, dtype=torch.long, device=device)
        for c in range(1, classes):
            lab[(rho <= 1.0 - 0.09 * (c - 1)) & (rho > 1.0 - 0.09 * c)] = c
        out.append(torch.nn.functional.one_hot(lab, classes).permute(3, 0, 1, 2))
    return torch.stack(out).float().contiguous()


def yardstick_signed_distance(target, planes):
    """phi through two ops.edt_sq per selected plane, as the code before the batched transform had to do it"""
    import torch
    from segmentation_pipeline_amd import ops
    out = torch.zeros_like(target)
    C = target.shape[1]
    for i, on in enumerate(planes):
        if not on:
            continue
        t = target[i // C, i % C]
        m = t > 0.5
        to_in = ops.edt_sqrt(ops.edt_sq(m.to(torch.uint8)))
        to_out = ops.edt_sqrt(ops.edt_sq((~m).to(torch.uint8)))
        phi = torch.where(m, 1.0 - to_out, to_in)
        out[i // C, i % C] = torch.where(torch.isinf(phi), torch.zeros_like(phi), phi)
    return out


def _median_interleaved(fns, samples, calls, warmup):
    import torch
    got = [[] for _ in fns]
    for r in range(warmup + samples):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                got[k].append(e0.elapsed_time(e1) / calls)
    return [statistics.median(g) for g in got]


def _pass_times(fn, names, calls=5):
    """{kernel name fragment: mean device microseconds per launch} from torch's profiler, or None"""
    try:
        import torch
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for n in names:
                if n in ev.key:
                    total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                    out[n] = out.get(n, 0.0) + total / calls
        return out if len(out) == len(names) else None
    except Exception as e:   # the profiler is an extra: the figures above do not depend on it
        print(f"# per-pass times not measured: {type(e).__name__}: {e}", flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from segmentation_pipeline_amd import ops
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd.criterions import BoundaryLoss, HybridLogisticDiceLoss
    assert torch.cuda.is_available(), "boundary_loss_bench.py measures on the GPU"
    dev = torch.device("cuda")
    lines = [f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"# transform / loss: median over {a.samples} samples of {a.calls} calls after {a.warmup} warm-up samples, per call; the",
             "# variants of a row alternate, device events around each sample.  ratio = batched / yardstick (below 1: faster).",
             f"# share = 20 B x selected voxels / time / {COPY_RATE / 1e12:.2f} TB/s (targets of 8-32 MB stay in the Infinity Cache between",
             "# calls: not an HBM rate).  loss fwd is timed through ops.boundary_loss, loss bwd through the entry point itself."]
    print("\n".join(lines), flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    targets = [("sparse 1x4x128^3", sparse_target((128, 128, 128), 4, 1, dev)),
               ("large 1x4x128^3", large_target((128, 128, 128), 4, 2, dev)),
               ("hippo 2x8x96x88x24", hippo_target(2, 8, (96, 88, 24), 3, dev))]
    for name, t in targets:
        N, C = t.shape[:2]
        planes = [c != 0 for c in range(C)] * N
        phi = ops.signed_distance(t, planes=planes)
        same = torch.equal(phi, yardstick_signed_distance(t, planes))
        inside = [int((t[i // C, i % C] > 0.5).sum()) for i, on in enumerate(planes) if on]
        new, old = _median_interleaved([lambda: ops.signed_distance(t, planes=planes), lambda: yardstick_signed_distance(t, planes)],
                                       a.samples, a.calls, a.warmup)
        voxels = sum(planes) * t[0, 0].numel()
        emit(f"transform {name:20s} {sum(planes)} planes, inside voxels per plane {min(inside)}..{max(inside)}: batched {1e3 * new:8.1f} us  "
             f"yardstick {1e3 * old:8.1f} us  ratio {new / old:.3f}  share {20 * voxels / (new * 1e-3) / COPY_RATE:.1%}  "
             f"same bits as the yardstick: {same}")
        per = None
        for names in (["sd_sweep_kernel", "sd_line_kernel<true, false>", "sd_line_kernel<false, true>"],
                      ["sd_sweep_kernel", "sd_line_kernelILb1ELb0", "sd_line_kernelILb0ELb1"]):     # demangled or not
            per = per or _pass_times(lambda: ops.signed_distance(t, planes=planes), names)
            if per is not None:
                us, u1, u2 = (per[n] for n in names)
                break
        if per is not None:
            emit(f"          per pass (profiler): sweep {us:7.1f} us = {6 * voxels / (us * 1e-6) / COPY_RATE:.1%} of the copy rate at 6 B/voxel, "
                 f"first line pass {u1:7.1f} us = {6 * voxels / (u1 * 1e-6) / COPY_RATE:.1%} at 6, "
                 f"last line pass {u2:7.1f} us = {8 * voxels / (u2 * 1e-6) / COPY_RATE:.1%} at 8 (plus 4 B/voxel of zeros in the planes that are off)")
        else:
            emit("          per pass: not measured (no kernel durations from the profiler in this environment)")

    # the loss kernels on the sparse target
    t = targets[0][1]
    phi = ops.signed_distance(t, planes=[c != 0 for c in range(4)])
    p = torch.softmax(2 * torch.randn(t.shape, device=dev, generator=torch.Generator(device="cuda").manual_seed(4)), dim=1).requires_grad_()
    w = torch.tensor([0.0, 1.0, 1.0, 1.0], device=dev)
    import ctypes as C
    from segmentation_pipeline_amd import _lib
    L, dp, dloss = _lib.lib(), torch.empty_like(phi), torch.ones((), device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw_bwd():   # the entry point itself: through autograd the call is bound by its host time
        rc = L.m355_boundary_loss_bwd(C.c_void_p(phi.data_ptr()), C.c_void_p(dloss.data_ptr()), C.c_void_p(w.data_ptr()), 1, 4,
                                      phi[0, 0].numel(), C.c_void_p(dp.data_ptr()), stream)
        assert rc == 0, L.m355_last_error()
    (fwd,) = _median_interleaved([lambda: ops.boundary_loss(p.detach(), phi, w)], a.samples, a.calls, a.warmup)
    (bwd,) = _median_interleaved([raw_bwd], a.samples, a.calls, a.warmup)
    (g,) = torch.autograd.grad(ops.boundary_loss(p, phi, w), p)
    assert torch.equal(g, dp)
    n3 = 3 * t[0, 0].numel()
    emit(f"loss fwd  1x4x128^3, 3 weighted channels: {1e3 * fwd:7.1f} us  {8 * n3 / (fwd * 1e-3) / 1e9:6.0f} GB/s of p and phi read")
    emit(f"loss bwd  1x4x128^3 (zeros for channel 0):  {1e3 * bwd:7.1f} us  {(8 * n3 + 4 * n3 // 3) / (bwd * 1e-3) / 1e9:6.0f} GB/s of phi read and dp written")

    if not a.no_step:
        import bench
        cfg = bench.WORKLOADS["cfg2"]
        x = torch.randn((1, cfg[0]) + cfg[4], device=dev, generator=torch.Generator(device="cuda").manual_seed(5))
        lab = (sparse_target(cfg[4], 2, 6, dev)[0, 1] > 0.5).long()
        lab[(large_target(cfg[4], 2, 7, dev)[0, 1] > 0.5) & (lab == 0)] = 2
        y = torch.nn.functional.one_hot(lab, cfg[1]).permute(3, 0, 1, 2)[None].float().contiguous()
        for precision in ("fp32", "bf16"):
            model = bench.build_model(cfg).to(dev).train()
            opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)
            crits = [("HybridLogisticDiceLoss", HybridLogisticDiceLoss()), ("BoundaryLoss(HybridLogisticDiceLoss)", BoundaryLoss(HybridLogisticDiceLoss()))]

            def step(crit):
                opt.zero_grad(set_to_none=True)
                crit(model(x), y)["loss"].backward()
                opt.step()
            ms = [[] for _ in crits]
            with sp.precision(precision):
                for _, crit in crits:
                    for _ in range(3):
                        step(crit)
                torch.cuda.synchronize()
                for _ in range(a.rounds):
                    for k, (_, crit) in enumerate(crits):
                        n, t0 = 0, time.perf_counter()
                        while True:
                            step(crit)
                            n += 1
                            if n % 5 == 0:
                                torch.cuda.synchronize()
                                if time.perf_counter() - t0 >= a.window:
                                    break
                        ms[k].append(1e3 * (time.perf_counter() - t0) / n)
            base, with_b = statistics.median(ms[0]), statistics.median(ms[1])
            emit(f"step cfg2 {precision}: {crits[0][0]} {base:7.2f} ms/step   {crits[1][0]} {with_b:7.2f} ms/step   overhead "
                 f"{100 * (with_b - base) / base:+.2f} %   ({a.rounds} windows of >= {a.window:g} s each, alternated; windows "
                 f"{' '.join(f'{v:.2f}' for v in ms[0])} | {' '.join(f'{v:.2f}' for v in ms[1])})")
            del model, opt
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
