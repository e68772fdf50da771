"""Times the focal Tversky loss (csrc/focal_tversky_loss.hip) next to the softmax loss it generalises, at
cfg2's output 1 x 4 x 128^3.

  prob fwd     m355_focal_tversky_fwd, gamma 0 / 2 / 2.5      vs  m355_hybrid_loss_fwd      8 B / element (x and t read once)
  prob bwd     m355_focal_tversky_bwd, gamma 0 / 2 / 2.5      vs  m355_hybrid_loss_bwd     12 B / element (x, t read, dx written)
  logits fwd   m355_focal_tversky_fwd on the logits           vs  m355_hybrid_loss_fwd      (the softmax forward stays in the
                                                                                            model either way: its output is
                                                                                            what prediction uses)
  logits bwd   m355_focal_tversky_bwd on the logits           vs  m355_hybrid_loss_bwd followed by m355_softmax_bwd, the two
                                                                  kernels it replaces: 24 B / element against 12

    python tools/focal_tversky_bench.py [--batches 12] [--calls 5] [--warmup 3] [--out profiles/focal_tversky_bench.txt]

The yardstick of every row is the existing kernel path on the same tensors in the same process: the columns of a row run
interleaved, the yardstick first AND last (the distance between its two columns is the spread of one kernel against itself
in this process order).  A timed batch is `calls` back-to-back calls between two CUDA events; the figure is the minimum over
the batches, per call.  With an integer gamma the prob kernels move the yardstick's bytes and add a few multiplies;
gamma = 2.5 pays for a powf per element (two in the backward).  The logits forward adds per element an expf, an expm1f and
its share of a logf.  67 MB of operands: the 256 MiB Infinity Cache holds them between calls, so the GB/s are not HBM rates.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from segmentation_pipeline_amd import _lib
    assert torch.cuda.is_available(), "focal_tversky_bench.py measures on the GPU"
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
    tw = torch.tensor([0.0, 1.0, 1.0, 1.0], device="cuda")
    dloss = torch.ones(1, device="cuda")
    out3, dx, dz = torch.empty(3, device="cuda"), torch.empty_like(z), torch.empty_like(z)
    sums_old, sums_new = torch.empty(N * Cc * 4, device="cuda"), torch.empty(N * Cc * 4, device="cuda")
    nws = max(int(L.m355_hybrid_loss_workspace(N, Cc, S)), int(L.m355_focal_tversky_workspace(N, Cc, S)))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")

    def old_fwd():
        ok(L.m355_hybrid_loss_fwd(p(prob), p(t), N, Cc, S, 0.5, p(cw), 0, p(out3), p(sums_old), p(ws), nws, st()))

    def old_bwd():
        ok(L.m355_hybrid_loss_bwd(p(prob), p(t), p(sums_old), p(dloss), N, Cc, S, 0.5, p(cw), 0, p(dx), st()))

    def old_bwd_and_head():      # what the logits backward replaces: dp, then the softmax head's dz from y and dp
        old_bwd()
        ok(L.m355_softmax_bwd(p(prob), p(dx), p(dz), N, Cc, 1, S, st()))

    def new_fwd(x, logits, gamma):
        return lambda: ok(L.m355_focal_tversky_fwd(p(x), p(t), N, Cc, S, 0.5, 0.3, 0.7, 0.75, gamma, p(cw), p(tw), logits, p(out3),
                                                   p(sums_new), p(ws), nws, st()))

    def new_bwd(x, logits, gamma):
        return lambda: ok(L.m355_focal_tversky_bwd(p(x), p(t), p(sums_new), p(dloss), N, Cc, S, 0.5, 0.3, 0.7, 0.75, gamma, p(cw),
                                                   p(tw), logits, p(dz), st()))

    gammas = (0.0, 2.0, 2.5)
    rows = [("prob fwd", 8 * N * Cc * S, [("hybrid (softmax)", old_fwd)] + [(f"gamma {g_:g}", new_fwd(prob, 0, g_)) for g_ in gammas]
             + [("hybrid again", old_fwd)], new_fwd(prob, 0, 0.0)),
            ("prob bwd", 12 * N * Cc * S, [("hybrid (softmax)", old_bwd)] + [(f"gamma {g_:g}", new_bwd(prob, 0, g_)) for g_ in gammas]
             + [("hybrid again", old_bwd)], new_fwd(prob, 0, 0.0)),
            ("logits fwd", 8 * N * Cc * S, [("hybrid (softmax)", old_fwd)] + [(f"gamma {g_:g}", new_fwd(z, 1, g_)) for g_ in gammas]
             + [("hybrid again", old_fwd)], new_fwd(z, 1, 0.0)),
            ("logits bwd", 12 * N * Cc * S, [("hybrid bwd + softmax bwd", old_bwd_and_head)]
             + [(f"gamma {g_:g}", new_bwd(z, 1, g_)) for g_ in gammas] + [("hybrid bwd + softmax bwd again", old_bwd_and_head)],
             new_fwd(z, 1, 0.0))]
    lines = [f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"# shape {'x'.join(map(str, SHAPE))}; minimum over {a.batches} batches of {a.calls} calls after {a.warmup} warm-up "
             "batches, per call;",
             "# the columns of a row interleaved, CUDA events around each batch; 'x yardstick' = time / the faster of the two",
             "# yardstick columns (the existing kernels, first and last); 'spread' = |first - last| / the faster one;",
             "# GB/s of the new columns count the bytes of one read of x and t (and one write of dx); the logits bwd yardstick",
             "# moves twice those",
             "# new columns: tversky_weight 0.5, alpha 0.3, beta 0.7, tversky_power 0.75, both weight vectors"]
    print("\n".join(lines), flush=True)
    for what, nbytes, cols, prime in rows:
        prime()                 # sums_new holds the sums of this row's mode; sums_old a forward's of the old loss
        old_fwd()
        ms = _time_interleaved([fn for _, fn in cols], a.batches, a.calls, a.warmup)
        base = min(ms[0], ms[-1])
        line = f"{what:10s}" + "".join(
            f"  {name}: {1e3 * tm:7.1f} us {(2 * nbytes if name.startswith('hybrid bwd +') else nbytes) / (tm * 1e-3) / 1e9:5.0f} GB/s"
            for (name, _), tm in zip(cols, ms))
        line += "   x yardstick: " + " ".join(f"{name} {tm / base:.2f}" for (name, _), tm in list(zip(cols, ms))[1:-1])
        line += f"   spread {abs(ms[0] - ms[-1]) / base:.1%}"
        lines.append(line)
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
