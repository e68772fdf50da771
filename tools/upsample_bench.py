"""Times the nearest and half-pixel trilinear 2x upsampling kernels (csrc/upsample.hip) next to the
align_corners=True kernels (csrc/elementwise.hip), which move the same bytes, at the two decoder levels of cfg2 that
carry the traffic: 1 x 128 x 32^3 -> 64^3 and 1 x 64 x 64^3 -> 128^3.

  fwd / bwd        m355_upsample_{trilinear2x, nearest2x, trilinear2x_hp}_{fwd, bwd}           fp32 NCDHW
  c8 fwd / c8 bwd  the same with _h16, bf16

    python tools/upsample_bench.py [--reps 50] [--warmup 10] [--out profiles/upsample_modes_bench.txt]

The three kernels of a row are timed interleaved in one process (one launch of each per round), CUDA events around each
launch, median of the rounds after the warm-up rounds.  GB/s over the bytes a kernel must move: the small tensor once and
the 2x tensor once.  'x old' = time / the align_corners=True kernel's time of the same row; the expectation is
nearest <= 1.00 and half-pixel <= 1.10.  Inputs are dense allocator tensors, so every kernel takes its widest path.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 128, 32, 32, 32), (1, 64, 64, 64, 64)]
FAMILIES = [("old", "m355_upsample_trilinear2x"), ("nearest", "m355_upsample_nearest2x"), ("half-px", "m355_upsample_trilinear2x_hp")]


def _time_interleaved(fns, reps, warmup):
    import torch
    times = [[] for _ in fns]
    for r in range(warmup + reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[k].append(e0.elapsed_time(e1))
    return [float(np.median(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
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

    def launch(name, src, dst, dims, extra):
        fn = getattr(L, name)

        def run():
            rc = fn(p(src), p(dst), *dims, 0, 0, *extra, st())
            assert rc == 0, L.m355_last_error()
        return run

    head = f"{'shape':18s} {'kernel':7s}" + "".join(f" {n + ' ms':>11s} {'GB/s':>7s}" for n, _ in FAMILIES) + \
           f" {'near x old':>11s} {'hp x old':>9s}"
    lines = [f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"# median of {a.reps} rounds after {a.warmup} warm-up rounds, the three kernels of a row interleaved, CUDA events",
             "# around each launch; GB/s over small tensor + 2x tensor, each moved once; 'x old' = time / old kernel's time",
             head]
    print("\n".join(lines), flush=True)
    for N, Cc, D, H, W in SHAPES:
        S, CB = D * H * W, (Cc + 7) // 8
        g = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randn((N, Cc, D, H, W), generator=g, device="cuda")
        dy = torch.randn((N, Cc, 2 * D, 2 * H, 2 * W), generator=g, device="cuda")
        y, dx = torch.empty_like(dy), torch.empty_like(x)
        x16 = torch.randn((N, CB, S, 8), generator=g, device="cuda").bfloat16()
        dy16 = torch.randn((N, CB, 8 * S, 8), generator=g, device="cuda").bfloat16()
        y16, dx16 = torch.empty_like(dy16), torch.empty_like(x16)
        dims, n = (N, Cc, D, H, W), N * Cc * S
        rows = [("fwd", "_fwd", x, y, (), 4 * 9 * n), ("bwd", "_bwd", dy, dx, (), 4 * 9 * n),
                ("c8 fwd", "_fwd_h16", x16, y16, (BF16,), 2 * 9 * n), ("c8 bwd", "_bwd_h16", dy16, dx16, (BF16,), 2 * 9 * n)]
        for name, suffix, src, dst, extra, nbytes in rows:
            t = _time_interleaved([launch(fam + suffix, src, dst, dims, extra) for _, fam in FAMILIES], a.reps, a.warmup)
            line = f"{f'{N}x{Cc}x{D}x{H}x{W}':18s} {name:7s}" + "".join(f" {v:11.4f} {nbytes / (v * 1e-3) / 1e9:7.0f}" for v in t) + \
                   f" {t[1] / t[0]:11.2f} {t[2] / t[0]:9.2f}"
            print(line, flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
