"""Times the Lovasz-softmax loss (csrc/lovasz_loss.hip, csrc/segmented_sort.hip) at cfg2's target shape
1 x 4 x 128^3, and the cfg2 training step with it.

  sort        m355_segmented_sort_u32 on 4 segments of 128^3 31-bit keys                 vs  torch.sort of int32 [4, 128^3]
  fwd / bwd   m355_lovasz_loss_fwd / _bwd (per_image False, classes 'present')           vs  m355_hybrid_loss_fwd / _bwd
  torch       Berman's formula in torch on the device (sort, gather, two cumsums, dot), forward and forward + backward:
              what a user would otherwise pay
  step        trainer-style step of the cfg2 network (forward, criterion, backward, SGD) in fp32 and bf16 with
              LovaszLoss(HybridLogisticDiceLoss()) next to the same step with HybridLogisticDiceLoss alone

    python tools/lovasz_loss_bench.py [--batches 12] [--calls 5] [--warmup 3] [--steps 5] [--no-step] [--out profiles/lovasz_loss_bench.txt]

The yardstick is hybrid_loss.hip, which this criterion leaves untouched: the code the previous revision built, timed in
the same process on the same tensors, first AND last in a row (the distance between its two columns is the spread of one
kernel against itself in this process order).  A timed batch is `calls` back-to-back calls between two CUDA events; the
figure is the minimum over the batches, per call.

Byte floors, per (class, voxel), at 6.3 TB/s: the key pass reads p and t and writes a key (12 B); a digit pass reads the
keys for its histogram (4 B) and reads and writes them to scatter (8 B), four passes; the scan pass reads the sorted keys
twice (tile counts, then F) and writes F (12 B); the backward reads p and t and writes dx (12 B) and makes two binary
searches in the sorted keys, which the Infinity Cache holds: 84 B in all, 0.70 GB at 1 x 4 x 128^3.
`--only-kernels` runs nothing but forward + backward, for a `rocprofv3 --kernel-trace --stats` run that splits the time
by kernel.
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (1, 4, 128, 128, 128)
HBM = 6.3e12    # achievable bytes / s


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
    """the cfg2 training step (bench.py's network and patch) per criterion, fp32 and bf16"""
    import torch
    from torch import nn

    import bench
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss, LovaszLoss
    from segmentation_pipeline_amd.models import ModularUNet
    from functools import partial
    cin, cout, filters, depth, patch = bench.WORKLOADS["cfg2"]
    x, _, y = bench.synth((1, cin) + tuple(patch), cout, 0, "cuda")

    def model():
        torch.manual_seed(0)
        return ModularUNet(cin, cout, filters, depth, block_params={'normalization_class': partial(nn.GroupNorm, 8)},
                           upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2}).cuda().train()
    variants = [("HybridLogisticDiceLoss", HybridLogisticDiceLoss()),
                ("LovaszLoss(HybridLogisticDiceLoss)", LovaszLoss(HybridLogisticDiceLoss(), 0.5)),
                ("LovaszLoss alone", LovaszLoss()),
                ("HybridLogisticDiceLoss, again", HybridLogisticDiceLoss())]
    for prec in ("fp32", "bf16"):
        ms = []
        for name, crit in variants:
            m = model()
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
        line = f"step {prec}  " + "  ".join(f"{name}: {tm:7.2f} ms ({tm / base:.3f})" for (name, _), tm in zip(variants, ms))
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
    ap.add_argument("--only-kernels", action="store_true", help="run only forward + backward (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from segmentation_pipeline_amd import _lib
    assert torch.cuda.is_available(), "lovasz_loss_bench.py measures on the GPU"
    L = _lib.lib()

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def st():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ok(rc):
        assert rc == 0, L.m355_last_error()

    N, Cc, D, H, W = SHAPE
    S = D * H * W
    R, M = Cc, N * S
    n = N * Cc * S
    g = torch.Generator(device="cuda").manual_seed(0)
    prob = torch.softmax(torch.randn(SHAPE, generator=g, device="cuda") * 2, dim=1)
    lab = torch.randint(0, Cc, (N, D, H, W), generator=g, device="cuda")
    t = torch.nn.functional.one_hot(lab, Cc).permute(0, 4, 1, 2, 3).float().contiguous()
    dloss = torch.ones(1, device="cuda")
    out3, out2, dx = torch.empty(3, device="cuda"), torch.empty(2, device="cuda"), torch.empty_like(prob)
    sums_h = torch.empty(N * Cc * 4, device="cuda")
    skeys, F = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    state = torch.empty(2 * R, dtype=torch.int32, device="cuda")
    keys = torch.randint(0, 1 << 31, (R, M), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
    sorted_keys = torch.empty_like(keys)
    nws = max(int(L.m355_hybrid_loss_workspace(N, Cc, S)), int(L.m355_lovasz_loss_workspace(N, Cc, S, 0)),
              int(L.m355_segmented_sort_workspace(R, M)))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")

    def hybrid_fwd():
        ok(L.m355_hybrid_loss_fwd(p(prob), p(t), N, Cc, S, 0.5, None, 1, p(out3), p(sums_h), p(ws), nws, st()))

    def hybrid_bwd():
        ok(L.m355_hybrid_loss_bwd(p(prob), p(t), p(sums_h), p(dloss), N, Cc, S, 0.5, None, 1, p(dx), st()))

    def lovasz_fwd():
        ok(L.m355_lovasz_loss_fwd(p(prob), p(t), N, Cc, S, 0, 0, None, p(out2), p(skeys), p(F), p(state), p(ws), nws, st()))

    def lovasz_bwd():
        ok(L.m355_lovasz_loss_bwd(p(prob), p(t), p(skeys), p(F), p(state), p(dloss), N, Cc, S, 0, p(dx), st()))

    def sort():
        ok(L.m355_segmented_sort_u32(p(keys), p(sorted_keys), R, M, 31, p(ws), nws, st()))

    if a.only_kernels:
        for _ in range(a.warmup + a.batches * a.calls):
            lovasz_fwd()
            lovasz_bwd()
        torch.cuda.synchronize()
        return
    lines = [f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"# shape {'x'.join(map(str, SHAPE))}; minimum over {a.batches} batches of {a.calls} calls after {a.warmup} warm-up "
             "batches, per call;",
             "# the columns of a row interleaved, CUDA events around each batch; 'floor' = the bytes the passes must move",
             f"# (see the tool's docstring) at {HBM / 1e12:.1f} TB/s; 'spread' = |first - last| of the yardstick / the faster one"]
    print("\n".join(lines), flush=True)
    hybrid_fwd()
    lovasz_fwd()
    sort()
    assert torch.equal(sorted_keys, torch.sort(keys, dim=1).values), "the sort differs from torch.sort"

    def row(what, cols, floors):
        ms = _time_interleaved([fn for _, fn in cols], a.batches, a.calls, a.warmup)
        line = f"{what:10s}" + "".join(
            f"  {name}: {1e3 * tm:8.1f} us" + (f" (floor {1e6 * floors[name] / HBM:6.1f} us, x {tm * 1e-3 * HBM / floors[name]:.1f})"
                                              if name in floors else "") for (name, _), tm in zip(cols, ms))
        if cols[0][0] + " again" == cols[-1][0]:
            line += f"   spread {abs(ms[0] - ms[-1]) / min(ms[0], ms[-1]):.1%}"
        lines.append(line)
        print(line, flush=True)
        return ms

    row("sort", [("torch.sort", lambda: torch.sort(keys, dim=1)), ("segmented_sort_u32", sort),
                 ("torch.sort again", lambda: torch.sort(keys, dim=1))], {"segmented_sort_u32": 4 * 12 * n})
    row("fwd", [("hybrid", hybrid_fwd), ("lovasz", lovasz_fwd), ("hybrid again", hybrid_fwd)], {"lovasz": (12 + 48 + 12) * n})
    row("bwd", [("hybrid", hybrid_bwd), ("lovasz", lovasz_bwd), ("hybrid again", hybrid_bwd)], {"lovasz": 12 * n})

    # Berman's formula in torch on the device
    def torch_fwd(x):
        xs, fg = x.transpose(0, 1).reshape(Cc, -1), t.transpose(0, 1).reshape(Cc, -1)
        errors = (fg - xs).abs()
        es, order = torch.sort(errors, dim=1, descending=True)
        fs = torch.gather(fg, 1, order)
        gts = fs.sum(1, keepdim=True)
        jac = 1 - (gts - fs.cumsum(1)) / (gts + (1 - fs).cumsum(1))
        jac = torch.cat([jac[:, :1], jac[:, 1:] - jac[:, :-1]], dim=1)
        return (es * jac).sum(1).mean()

    pg = prob.clone().requires_grad_(True)

    def torch_fwd_bwd():
        pg.grad = None
        torch_fwd(pg).backward()

    def lovasz_fwd_bwd():
        lovasz_fwd()
        lovasz_bwd()
    with torch.no_grad():
        ms_f = _time_interleaved([lambda: torch_fwd(prob), lovasz_fwd], a.batches, a.calls, a.warmup)
    ms_fb = _time_interleaved([torch_fwd_bwd, lovasz_fwd_bwd], a.batches, a.calls, a.warmup)
    lovasz_fwd()
    line = (f"torch      Berman's formula in torch on the device: fwd {1e3 * ms_f[0]:8.1f} us (lovasz {1e3 * ms_f[1]:8.1f} us, "
            f"x {ms_f[1] / ms_f[0]:.2f}), fwd + bwd {1e3 * ms_fb[0]:8.1f} us (lovasz {1e3 * ms_fb[1]:8.1f} us, x {ms_fb[1] / ms_fb[0]:.2f}); "
            f"loss {torch_fwd(prob).item():.7f} vs {out2[0].item():.7f}")
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
