"""Times the top-k cross-entropy + Dice loss (csrc/topk_loss.hip) next to the criteria it stands beside, at
cfg2's target shape 1 x 4 x 128^3, and the cfg2 training step with it.

  prob fwd / bwd     m355_topk_loss_fwd / _bwd at top_k 0.1 and 1.0     vs  m355_hybrid_loss_fwd / _bwd
  logits fwd / bwd   the same on the logits                             vs  m355_focal_tversky_fwd / _bwd (gamma 0, from_logits)
  torch              log_softmax, the weighted cross-entropy, torch.topk and its mean in torch on the device, forward and
                     forward + backward: what a user would otherwise pay for the log term alone
  step               trainer-style step of the cfg2 network (forward, criterion, backward) in fp32 and bf16 with
                     HybridTopKDiceLoss (prob and logits heads) next to the same step with HybridLogisticDiceLoss

    python tools/topk_loss_bench.py [--batches 12] [--calls 5] [--warmup 3] [--steps 5] [--no-step] [--out profiles/topk_loss_bench.txt]

The yardsticks are the kernels of hybrid_loss.hip and focal_tversky_loss.hip, which this criterion leaves untouched: the
same code the previous revision built, timed in the same process on the same tensors.  The columns of a row run
interleaved, the yardstick first AND last (the distance between its two columns is the spread of one kernel against itself
in this process order).  A timed batch is `calls` back-to-back calls between two CUDA events; the figure is the minimum over
the batches, per call.  Bytes: the forward reads x and t once (8 B / element), writes e once and reads it twice more
(12 B / voxel); the backward adds one read of e to the yardstick's 12 B / element.  67 MB of operands: the 256 MiB Infinity
Cache holds them between calls, so the GB/s are not HBM rates.  The forward is five launches (a memset of the histograms,
the first pass, two select passes, the finalize block) against the yardstick's two; `--only-fwd` runs nothing but the
logits forward at top_k 0.1, for a `rocprofv3 --kernel-trace --stats` run that splits its time by kernel.
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (1, 4, 128, 128, 128)


def _time_interleaved(fns, batches, calls, warmup):
    import torch
    best = [float("inf")] * len(fns)
    for r in range(warmup + batches):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                best[k] = min(best[k], e0.elapsed_time(e1) / calls)
    return best


def _step_times(a, lines):
    """the cfg2 training step (bench.py's network and patch) per criterion and head, fp32 and bf16"""
    import torch
    from torch import nn

    import bench
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss, HybridTopKDiceLoss
    from segmentation_pipeline_amd.models import ModularUNet
    from functools import partial
    cin, cout, filters, depth, patch = bench.WORKLOADS["cfg2"]
    x, _, y = bench.synth((1, cin) + tuple(patch), cout, 0, "cuda")

    def model(head, params):
        torch.manual_seed(0)
        return ModularUNet(cin, cout, filters, depth, block_params={'normalization_class': partial(nn.GroupNorm, 8)},
                           upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2},
                           hypothesis_class=head, hypothesis_params=params).cuda().train()
    variants = [("HybridLogisticDiceLoss, softmax head", nn.Softmax, {"dim": 1}, HybridLogisticDiceLoss()),
                ("HybridTopKDiceLoss(0.1), softmax head", nn.Softmax, {"dim": 1}, HybridTopKDiceLoss(0.1)),
                ("HybridTopKDiceLoss(0.1, from_logits), identity head", nn.Identity, {}, HybridTopKDiceLoss(0.1, from_logits=True)),
                ("HybridLogisticDiceLoss, softmax head, again", nn.Softmax, {"dim": 1}, HybridLogisticDiceLoss())]
    for prec in ("fp32", "bf16"):
        ms = []
        for name, head, params, crit in variants:
            m = model(head, params)
            opt = torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9)
            best = float("inf")
            with sp.precision(prec):
                for i in range(a.warmup + a.steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    opt.zero_grad(set_to_none=True)
                    crit(m(x), y)["loss"].backward()
                    opt.step()
                    e1.record()
                    e1.synchronize()
                    if i >= a.warmup:
                        best = min(best, e0.elapsed_time(e1))
            ms.append(best)
            del m, opt
            torch.cuda.empty_cache()
        base = min(ms[0], ms[-1])
        line = f"step {prec}  " + "  ".join(f"{name}: {tm:7.2f} ms ({tm / base:.3f})" for (name, *_), tm in zip(variants, ms))
        line += f"   spread {abs(ms[0] - ms[-1]) / base:.1%}"
        lines.append(line)
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="skip the cfg2 training steps")
    ap.add_argument("--only-fwd", action="store_true", help="run only the logits forward at top_k 0.1 (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from segmentation_pipeline_amd import _lib, ops
    assert torch.cuda.is_available(), "topk_loss_bench.py measures on the GPU"
    L = _lib.lib()

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def st():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ok(rc):
        assert rc == 0, L.m355_last_error()

    N, Cc, D, H, W = SHAPE
    S = D * H * W
    g = torch.Generator(device="cuda").manual_seed(0)
    z = torch.randn(SHAPE, generator=g, device="cuda") * 2
    prob = torch.softmax(z, dim=1)
    lab = torch.randint(0, Cc, (N, D, H, W), generator=g, device="cuda")
    t = torch.nn.functional.one_hot(lab, Cc).permute(0, 4, 1, 2, 3).float().contiguous()
    cw = torch.tensor([1.0, 2.0, 3.0, 4.0], device="cuda")
    dloss = torch.ones(1, device="cuda")
    out3, dx = torch.empty(3, device="cuda"), torch.empty_like(z)
    sums_h, sums_f, sums_k = (torch.empty(N * Cc * 4, device="cuda") for _ in range(3))
    e, state = torch.empty(N * S, device="cuda"), torch.empty(4, device="cuda")
    nws = max(int(L.m355_hybrid_loss_workspace(N, Cc, S)), int(L.m355_focal_tversky_workspace(N, Cc, S)),
              int(L.m355_topk_loss_workspace(N, Cc, S)))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")

    def hybrid_fwd():
        ok(L.m355_hybrid_loss_fwd(p(prob), p(t), N, Cc, S, 0.5, p(cw), 1, p(out3), p(sums_h), p(ws), nws, st()))

    def hybrid_bwd():
        ok(L.m355_hybrid_loss_bwd(p(prob), p(t), p(sums_h), p(dloss), N, Cc, S, 0.5, p(cw), 1, p(dx), st()))

    def ft_fwd():
        ok(L.m355_focal_tversky_fwd(p(z), p(t), N, Cc, S, 0.5, .5, .5, 1.0, 0.0, p(cw), None, 1, p(out3), p(sums_f), p(ws), nws,
                                    st()))

    def ft_bwd():
        ok(L.m355_focal_tversky_bwd(p(z), p(t), p(sums_f), p(dloss), N, Cc, S, 0.5, .5, .5, 1.0, 0.0, p(cw), None, 1, p(dx), st()))

    def topk_fwd(x, logits, top_k):
        k = ops.topk_count(N, S, top_k)
        return lambda: ok(L.m355_topk_loss_fwd(p(x), p(t), N, Cc, S, k, None, 0.5, p(cw), 1, logits, p(out3), p(sums_k), p(e),
                                               p(state), p(ws), nws, st()))

    def topk_bwd(x, logits):
        return lambda: ok(L.m355_topk_loss_bwd(p(x), p(t), p(e), p(sums_k), p(state), p(dloss), N, Cc, S, 0.5, p(cw), 1, logits,
                                               p(dx), st()))

    fractions = (0.1, 1.0)
    # (row, bytes of the new columns, yardstick, new columns, what primes the saved state of the backward rows)
    rows = [("prob fwd", 8 * N * Cc * S + 12 * N * S, ("hybrid", hybrid_fwd), [(f"top_k {f:g}", topk_fwd(prob, 0, f)) for f in fractions], None),
            ("logits fwd", 8 * N * Cc * S + 12 * N * S, ("focal Tversky logits", ft_fwd), [(f"top_k {f:g}", topk_fwd(z, 1, f)) for f in fractions], None)]
    for f in fractions:
        rows.append((f"prob bwd {f:g}", 12 * N * Cc * S + 4 * N * S, ("hybrid", hybrid_bwd), [(f"top_k {f:g}", topk_bwd(prob, 0))],
                     topk_fwd(prob, 0, f)))
        rows.append((f"logits bwd {f:g}", 12 * N * Cc * S + 4 * N * S, ("focal Tversky logits", ft_bwd), [(f"top_k {f:g}", topk_bwd(z, 1))],
                     topk_fwd(z, 1, f)))
    lines = [f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"# shape {'x'.join(map(str, SHAPE))}; minimum over {a.batches} batches of {a.calls} calls after {a.warmup} warm-up "
             "batches, per call;",
             "# the columns of a row interleaved, CUDA events around each batch; 'x yardstick' = time / the faster of the two",
             "# yardstick columns (the existing kernels, first and last); 'spread' = |first - last| / the faster one;",
             "# GB/s of the new columns count x and t read once, e written once and read twice (fwd); x, t, e read and dx",
             "# written (bwd); dice_weight 0.5, class weights 1..4, square_dice"]
    if a.only_fwd:
        fwd = topk_fwd(z, 1, 0.1)
        for _ in range(a.warmup + a.batches * a.calls):
            fwd()
        torch.cuda.synchronize()
        return
    print("\n".join(lines), flush=True)
    hybrid_fwd()
    ft_fwd()
    for what, nbytes, (yname, yfn), cols, prime in rows:
        if prime is not None:
            prime()
        cols = [(yname, yfn)] + cols + [(yname + " again", yfn)]
        ms = _time_interleaved([fn for _, fn in cols], a.batches, a.calls, a.warmup)
        base = min(ms[0], ms[-1])
        line = f"{what:15s}" + "".join(
            f"  {name}: {1e3 * tm:7.1f} us" + ("" if name.startswith(yname) else f" {nbytes / (tm * 1e-3) / 1e9:5.0f} GB/s")
            for (name, _), tm in zip(cols, ms))
        line += "   x yardstick: " + " ".join(f"{name} {tm / base:.2f}" for (name, _), tm in list(zip(cols, ms))[1:-1])
        line += f"   spread {abs(ms[0] - ms[-1]) / base:.1%}"
        lines.append(line)
        print(line, flush=True)

    # the log term alone in torch
    k = ops.topk_count(N, S, 0.1)
    w4 = cw.view(1, Cc, 1, 1, 1)

    def torch_fwd(x):
        lp = torch.log_softmax(x, dim=1)
        ce = -(w4 * t * lp).sum(1).flatten()
        return torch.topk(ce, k, sorted=False).values.sum() / (Cc * k)

    zg = z.clone().requires_grad_(True)

    def torch_fwd_bwd():
        zg.grad = None
        torch_fwd(zg).backward()
    with torch.no_grad():
        ms = _time_interleaved([lambda: torch_fwd(z)], a.batches, a.calls, a.warmup)
    ms += _time_interleaved([torch_fwd_bwd], a.batches, a.calls, a.warmup)
    line = (f"torch log term   log_softmax + weighted CE + torch.topk(k = {k}) + mean, on the device: fwd {1e3 * ms[0]:7.1f} us, "
            f"fwd + bwd {1e3 * ms[1]:7.1f} us")
    lines.append(line)
    print(line, flush=True)
    if not a.no_step:
        _step_times(a, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
