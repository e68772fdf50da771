"""Times the blob (lesion-wise) Dice loss (csrc/blob_loss.hip).

  passes     1 x 4 x 128^3, a seeded synthetic lesion target: about 100 balls of radius 2-8 voxels in channel 1, channels 2
             and 3 empty, channel 0 the rest; the prediction a random softmax.  With the criterion's default weights the
             planes 1..3 are on (3 x 128^3 stacked voxels), with weights (0, 1, 0, 0) only the lesion channel is.  Timed
             separately, each through its entry point (through autograd a call is bound by its host time):
               label     m355_blob_label: threshold, the six labelling passes, the per-plane ranges
               reduce    m355_blob_dice_fwd: zeroing, the segmented reduction, finalize, the scalar
               backward  m355_blob_dice_bwd
             Next to each time stands its floor: the bytes the pass MUST move (label: 4 B read of the target + 4 B written
             of the labels per on voxel; reduce: 4 B of p + 4 B of labels; backward: 4 B of labels, 4 B of p in the square
             form, 4 B of dp written for every voxel of all planes) over the device-to-device copy rate the profiles here
             are quoted against.  The labelling's own passes move about 44 B per voxel (x 4+4, par 4+4, 4, 4, 4+4 and the
             finds, 4 for the ranges): that figure is printed too.  A sample is `calls` back-to-back calls between two
             device events; the figure is the median over the samples with their minimum and maximum.
  torch      the same term the usual way, on the device: one masked full-volume Dice per component in a Python loop over
             precomputed labels (the labelling itself, cc3d on the host in the published implementation, is not counted).
  step       cfg2 (1 x 4 x 128^3 input, 3 classes), eager SGD, BlobLoss(HybridLogisticDiceLoss()) against
             HybridLogisticDiceLoss() alone -- which is the parent commit's step: no file on its path changed -- in fp32
             and bf16: windows of at least `--window` seconds, alternated; ms / step is the median over the windows, all
             windows are listed.

    python tools/blob_loss_bench.py [--samples 15] [--calls 3] [--warmup 3] [--window 1.0] [--rounds 3] [--no-step]
                                    [--out profiles/blob_loss_bench.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12   # B/s, the device-to-device copy rate all profiles here are quoted against


def lesion_target(shape, classes, seed, device, balls=100, channel=1):
    """[1, classes, *shape] one-hot: `balls` balls of radius 2-8 in `channel` (they may touch: the count is "about"),
    channel 0 the rest"""
    import torch
    g = torch.Generator().manual_seed(seed)
    grid = torch.meshgrid(*[torch.arange(float(n), device=device) for n in shape], indexing="ij")
    lab = torch.zeros(shape, dtype=torch.long, device=device)
    for _ in range(balls):
        centre = [float(torch.randint(8, n - 8, (1,), generator=g)) for n in shape]
        r = 2.0 + 6.0 * float(torch.rand(1, generator=g))
        lab[sum((gr - c) ** 2 for gr, c in zip(grid, centre)) <= r * r] = channel
    return torch.nn.functional.one_hot(lab, classes).permute(3, 0, 1, 2)[None].float().contiguous()


def _samples(fn, samples, calls, warmup):
    import torch
    got = []
    for r in range(warmup + samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        if r >= warmup:
            got.append(1e3 * e0.elapsed_time(e1) / calls)      # microseconds per call
    return statistics.median(got), min(got), max(got)


def torch_blob_dice(p, y, labels, ranges, weights, square, eps=1e-8):
    """the usual implementation on precomputed labels: a masked Dice per component, averaged per plane, then over the
    planes with a component by their weights"""
    import torch
    num, wsum = 0.0, 0.0
    slot = 0
    for c, w in enumerate(weights):
        if not w > 0:
            continue
        lab, (first, last) = labels[slot], ranges[slot]
        slot += 1
        if last < first:
            continue
        plane = 0.0
        for k in range(first, last + 1):
            mask = ((lab == 0) | (lab == k)).float()
            pm, tm = p[0, c] * mask, y[0, c] * mask
            total = (tm * tm).sum() + (pm * pm).sum() if square else tm.sum() + pm.sum()
            plane = plane + (1 - 2 * (pm * tm).sum() / (total + eps))
        num = num + w * plane / (last - first + 1)
        wsum += w
    return num / wsum


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
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd import _lib, ops
    from segmentation_pipeline_amd.criterions import BlobLoss, HybridLogisticDiceLoss
    assert torch.cuda.is_available(), "blob_loss_bench.py measures on the GPU"
    dev = torch.device("cuda")
    lines = [f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"# passes: median [min .. max] over {a.samples} samples of {a.calls} calls after {a.warmup} warm-up samples, per call, device events",
             f"# around each sample.  floor = the bytes the pass must move / {COPY_RATE / 1e12:.2f} TB/s; the tensors of a call (8 MB per plane) stay",
             "# in the Infinity Cache between calls, so the rates below are not HBM rates."]
    print("\n".join(lines), flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    shape = (128, 128, 128)
    S = shape[0] * shape[1] * shape[2]
    y = lesion_target(shape, 4, 1, dev)
    p = torch.softmax(2 * torch.randn(y.shape, device=dev, generator=torch.Generator(device="cuda").manual_seed(4)), dim=1)
    dp, dloss = torch.empty_like(p), torch.ones((), device=dev)
    for weights in ((0.0, 1.0, 1.0, 1.0), (0.0, 1.0, 0.0, 0.0)):
        flags = [w > 0 for w in weights]
        on = (C.c_uint8 * 4)(*flags)
        n_on = sum(flags)
        cw = torch.tensor(weights, device=dev)
        labels, ranges, count = ops.blob_labels(y, flags, 3)
        K = int(count)
        sizes = torch.bincount(labels.flatten().long())[1:]
        emit(f"target 1x4x128^3, weights {weights}: {n_on} planes on, {K} components of {int(sizes.min())}..{int(sizes.max())} voxels "
             f"(median {int(sizes.median())}), capacity {L.m355_blob_capacity(4, on, *shape, 3)}")
        ws_l = torch.empty(L.m355_blob_label_workspace(4, on, *shape), dtype=torch.uint8, device=dev)
        ws_d = torch.empty(L.m355_blob_dice_workspace(4, on, *shape, 3), dtype=torch.uint8, device=dev)
        tables = torch.empty(L.m355_blob_dice_tables(4, on, *shape, 3), dtype=torch.uint8, device=dev)
        loss, total = torch.empty((), device=dev), torch.empty((), dtype=torch.int32, device=dev)

        def label():
            rc = L.m355_blob_label(P(y), 4, on, *shape, 3, P(labels), P(ranges), P(count), P(ws_l), ws_l.numel(), stream)
            assert rc == 0, L.m355_last_error()
        med, lo, hi = _samples(label, a.samples, a.calls, a.warmup)
        floor = 8 * n_on * S / COPY_RATE * 1e6
        emit(f"  label            {med:8.1f} us [{lo:.1f} .. {hi:.1f}]   floor {floor:6.1f} us (8 B/voxel; x {med / floor:.1f})   "
             f"its passes' own ~44 B/voxel: {44 * n_on * S / COPY_RATE * 1e6:6.1f} us (x {med * COPY_RATE / (44 * n_on * S) / 1e6:.1f})")
        for square in (True, False):
            def fwd():
                rc = L.m355_blob_dice_fwd(P(p), P(labels), P(ranges), P(count), P(cw), 1, 4, on, *shape, 3, int(square), P(loss),
                                          P(total), P(tables), tables.numel(), P(ws_d), ws_d.numel(), stream)
                assert rc == 0, L.m355_last_error()

            def bwd():
                rc = L.m355_blob_dice_bwd(P(p), P(labels), P(tables), P(dloss), 1, 4, on, *shape, 3, int(square), P(dp), stream)
                assert rc == 0, L.m355_last_error()
            med, lo, hi = _samples(fwd, a.samples, a.calls, a.warmup)
            floor = 8 * n_on * S / COPY_RATE * 1e6
            emit(f"  reduce  square={int(square)} {med:8.1f} us [{lo:.1f} .. {hi:.1f}]   floor {floor:6.1f} us (8 B per on voxel; x {med / floor:.1f})   "
                 f"loss {loss.item():.7f}")
            med, lo, hi = _samples(bwd, a.samples, a.calls, a.warmup)
            floor = ((8 if square else 4) * n_on * S + 4 * 4 * S) / COPY_RATE * 1e6
            emit(f"  backward square={int(square)} {med:8.1f} us [{lo:.1f} .. {hi:.1f}]   floor {floor:6.1f} us ({8 if square else 4} B read per on voxel, 4 B "
                 f"written per voxel of all planes; x {med / floor:.1f})")
            host_ranges = ranges.tolist()
            t0 = time.perf_counter()
            ref = torch_blob_dice(p, y, labels, host_ranges, weights, square)
            torch.cuda.synchronize()
            first = time.perf_counter() - t0
            t0 = time.perf_counter()
            ref = torch_blob_dice(p, y, labels, host_ranges, weights, square)
            torch.cuda.synchronize()
            second = time.perf_counter() - t0
            emit(f"  torch loop, forward only, square={int(square)}: {1e3 * second:8.1f} ms (first call {1e3 * first:.1f} ms) for {K} components; "
                 f"value {float(ref):.7f} vs {loss.item():.7f}")

    if not a.no_step:
        import bench
        cfg = bench.WORKLOADS["cfg2"]
        x = torch.randn((1, cfg[0]) + cfg[4], device=dev, generator=torch.Generator(device="cuda").manual_seed(5))
        lab = (lesion_target(cfg[4], 2, 6, dev)[0, 1] > 0.5).long()
        lab[(lesion_target(cfg[4], 2, 7, dev, balls=3)[0, 1] > 0.5) & (lab == 0)] = 2
        ys = torch.nn.functional.one_hot(lab, cfg[1]).permute(3, 0, 1, 2)[None].float().contiguous()
        for precision in ("fp32", "bf16"):
            model = bench.build_model(cfg).to(dev).train()
            opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)
            crits = [("HybridLogisticDiceLoss", HybridLogisticDiceLoss()), ("BlobLoss(HybridLogisticDiceLoss)", BlobLoss(HybridLogisticDiceLoss()))]

            def step(crit):
                opt.zero_grad(set_to_none=True)
                ld = crit(model(x), ys)
                ld["loss"].backward()
                opt.step()
                return ld
            ms = [[] for _ in crits]
            with sp.precision(precision):
                for _, crit in crits:
                    for _ in range(3):
                        ld = step(crit)
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
                 f"{100 * (with_b - base) / base:+.2f} %   ({int(ld['blob_count'])} components; {a.rounds} windows of >= {a.window:g} s each, "
                 f"alternated; windows {' '.join(f'{v:.2f}' for v in ms[0])} | {' '.join(f'{v:.2f}' for v in ms[1])})")
            del model, opt
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
