"""Times the fp32 normalisation backward behind a fused AvgPool3d(2, 2) in its two forms at the encoder
shapes of cfg2: 1 x 32 x 128^3, 1 x 64 x 64^3, 1 x 128 x 32^3, 1 x 256 x 16^3.

  two_step        m355_avgpool3d_2x_bwd_add into a dense tensor + m355_norm_act_bwd
  fused           m355_norm_act_bwd_pool
  norm_bwd_alone  m355_norm_act_bwd on the ready sum (what the pooled passes cost on top of the plain ones)

    python tools/pool_bwd_bench.py [--reps 30]

GroupNorm(8) + LeakyReLU; the skip gradient is a channel slice of a gradient three times as wide, as the decoder's concat
hands it over.  Device times: CUDA events around each call after warm-up, median (min) of the repeats in microseconds, in
the order two_step / fused / norm_bwd_alone / two_step / fused.  `bits_equal`: dx, dgamma, dbeta of the two forms compare
equal.  profiles/norm_bwd_fusion_ab.txt holds one run.
"""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from segmentation_pipeline_amd import _lib  # noqa: E402

LEVELS = [(32, 128), (64, 64), (128, 32), (256, 16)]   # (channels, edge)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    L = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ok(rc):
        assert rc == 0, L.m355_last_error()

    def bench(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        ts.sort()
        return "%.1f(%.1f)" % (ts[len(ts) // 2], ts[0])

    for Cc, E in LEVELS:
        S = E ** 3
        x = torch.randn(1, Cc, E, E, E, device="cuda")
        wide = torch.randn(1, 3 * Cc, E, E, E, device="cuda")
        dskip = wide[:, :Cc]
        dpool = torch.randn(1, Cc, E // 2, E // 2, E // 2, device="cuda")
        gamma, beta = torch.rand(Cc, device="cuda") + 0.5, torch.randn(Cc, device="cuda")
        d = _lib.NormDesc(1, Cc, S, 8, 2, 1e-5, 0.01, 0, 0, 0)
        mean, rstd = torch.empty(8, device="cuda"), torch.empty(8, device="cuda")
        ws = torch.empty(L.m355_norm_workspace(C.byref(d)), dtype=torch.uint8, device="cuda")
        ok(L.m355_norm_stats(C.byref(d), p(x), p(mean), p(rstd), None, None, 0.1, p(ws), ws.numel(), st()))
        tot, dx1, dx2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        dg1, db1, dg2, db2 = (torch.empty(Cc, device="cuda") for _ in range(4))

        def norm_only():
            ok(L.m355_norm_act_bwd(C.byref(d), p(x), p(tot), p(mean), p(rstd), p(gamma), p(beta), p(dx1), p(dg1), p(db1), 1,
                                   p(ws), ws.numel(), st()))

        def two_step():
            ok(L.m355_avgpool3d_2x_bwd_add(p(dpool), p(dskip), p(tot), 1, Cc, E, E, E, 0, 0, 0, st()))
            norm_only()

        def fused():
            ok(L.m355_norm_act_bwd_pool(C.byref(d), p(x), p(dskip), 0, p(dpool), 0, E, E, E, p(mean), p(rstd), p(gamma),
                                        p(beta), p(dx2), p(dg2), p(db2), 1, p(ws), ws.numel(), st()))

        r = [bench(f) for f in (two_step, fused, norm_only, two_step, fused)]
        same = torch.equal(dx1, dx2) and torch.equal(dg1, dg2) and torch.equal(db1, db2)
        print(f"C={Cc} {E}^3 us median(min): two_step {r[0]} fused {r[1]} norm_bwd_alone {r[2]} two_step {r[3]} fused {r[4]} "
              f"bits_equal={same}", flush=True)


if __name__ == "__main__":
    main()
