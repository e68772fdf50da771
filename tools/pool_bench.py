"""Times the four nn.MaxPool3d(2, 2) kernels (csrc/maxpool.hip) next to their AvgPool3d(2, 2) twins at the
encoder shapes of cfg2: 1 x 32 x 128^3, 1 x 64 x 64^3, 1 x 128 x 32^3, 1 x 256 x 16^3.

  fwd        m355_maxpool3d_2x_fwd (value + route byte)             vs  m355_avgpool3d_2x_fwd
  bwd+add    m355_maxpool3d_2x_bwd with the skip gradient           vs  m355_avgpool3d_2x_bwd_add
  c8 fwd     m355_maxpool3d_2x_fwd_h16 (bf16, value + route item)   vs  m355_avgpool3d_2x_fwd_h16
  c8 bwd     m355_maxpool3d_2x_bwd_h16 with dskip16 (bf16)          vs  m355_avgpool3d_2x_bwd_h16

    python tools/pool_bench.py [--reps 50] [--out profiles/maxpool_bench.txt]

Each kernel is reported as GB/s over the bytes it must move (every operand read or written once; the max-pool rows
include the route) and as a fraction of the avg twin's rate.  Device times: CUDA events around each call after warm-up,
median of the repeats.  Inputs are dense allocator tensors, so every kernel takes its widest path.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 32, 128, 128, 128), (1, 64, 64, 64, 64), (1, 128, 32, 32, 32), (1, 256, 16, 16, 16)]


def _time_events(fn, reps, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from segmentation_pipeline_amd import _lib
    L = _lib.lib()
    BF16 = _lib.COMPUTE_BF16

    def p(t):
        return C.c_void_p(t.data_ptr())

    def st():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ok(rc):
        assert rc == 0, L.m355_last_error()

    lines = [f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"# median of {a.reps} after {a.warmup} warm-up calls, CUDA events around each call; GB/s over the bytes the",
             "# kernel must move (max rows: route included); 'of avg' = max-pool rate / avg-pool twin's rate",
             f"{'shape':22s} {'kernel':8s} {'max ms':>8s} {'max GB/s':>9s} {'avg ms':>8s} {'avg GB/s':>9s} {'of avg':>7s}"]
    print("\n".join(lines), flush=True)
    for N, Cc, D, H, W in SHAPES:
        S, OS = D * H * W, D * H * W // 8
        g = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randn((N, Cc, D, H, W), generator=g, device="cuda")
        add = torch.randn((N, Cc, D, H, W), generator=g, device="cuda")
        dy = torch.randn((N, Cc, D // 2, H // 2, W // 2), generator=g, device="cuda")
        y, dx = torch.empty_like(dy), torch.empty_like(x)
        idx = torch.empty(dy.shape, dtype=torch.uint8, device="cuda")
        CB = (Cc + 7) // 8
        x16 = torch.randn((N, CB, S, 8), generator=g, device="cuda").bfloat16()
        ds16 = torch.randn((N, CB, S, 8), generator=g, device="cuda").bfloat16()
        dp16 = torch.randn((N, CB, OS, 8), generator=g, device="cuda").bfloat16()
        y16, dx16 = torch.empty_like(dp16), torch.empty_like(x16)
        idx8 = torch.empty((N, CB, OS, 8), dtype=torch.uint8, device="cuda")
        n, no = N * Cc * S, N * Cc * OS           # un-pooled / pooled elements (C is a multiple of 8 here)
        rows = [
            ("fwd",
             lambda: ok(L.m355_maxpool3d_2x_fwd(p(x), p(y), p(idx), N, Cc, D, H, W, 0, 0, st())), 4 * n + 4 * no + no,
             lambda: ok(L.m355_avgpool3d_2x_fwd(p(x), p(y), N, Cc, D, H, W, 0, 0, st())), 4 * n + 4 * no),
            ("bwd+add",
             lambda: ok(L.m355_maxpool3d_2x_bwd(p(dy), p(idx), p(add), p(dx), N, Cc, D, H, W, 0, 0, 0, st())), 8 * n + 4 * no + no,
             lambda: ok(L.m355_avgpool3d_2x_bwd_add(p(dy), p(add), p(dx), N, Cc, D, H, W, 0, 0, 0, st())), 8 * n + 4 * no),
            ("c8 fwd",
             lambda: ok(L.m355_maxpool3d_2x_fwd_h16(p(x16), p(y16), p(idx8), N, Cc, D, H, W, 0, 0, BF16, st())), 2 * n + 2 * no + no,
             lambda: ok(L.m355_avgpool3d_2x_fwd_h16(p(x16), p(y16), N, Cc, D, H, W, 0, 0, BF16, st())), 2 * n + 2 * no),
            ("c8 bwd",
             lambda: ok(L.m355_maxpool3d_2x_bwd_h16(p(dp16), p(idx8), p(ds16), p(dx16), N, Cc, D, H, W, 0, 0, 0, BF16, st())),
             4 * n + 2 * no + no,
             lambda: ok(L.m355_avgpool3d_2x_bwd_h16(p(dp16), p(ds16), p(dx16), N, Cc, D, H, W, 0, 0, 0, BF16, st())), 4 * n + 2 * no),
        ]
        for name, fmax, bmax, favg, bavg in rows:      # (forward rows first: they fill the routes the backward rows read)
            tm, ta = _time_events(fmax, a.reps, a.warmup), _time_events(favg, a.reps, a.warmup)
            rm, ra = bmax / (tm * 1e-3) / 1e9, bavg / (ta * 1e-3) / 1e9
            line = (f"{f'{N}x{Cc}x{D}x{H}x{W}':22s} {name:8s} {tm:8.4f} {rm:9.1f} {ta:8.4f} {ra:9.1f} {rm / ra:7.2f}")
            print(line, flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
