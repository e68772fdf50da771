#!/usr/bin/env python3
"""Per-level A/B of the k=2,s=2 ConvTranspose3d weight gradient through the C ABI: the fp32-MFMA entry point
(m355_conv_transpose3d_bwd_weight) against the split one (m355_conv_transpose3d_bwd_weight_x3, M355_COMPUTE_F32X3), in one
process, the old one timed first and last.  Each row is CALLS calls timed one by one with device events (median, min) and
the GB/s of the median on the algorithmic bytes (x + dy once each).  The levels are those of tools/convt_bench.py.
A level the split route refuses (m355_conv_transpose3d_x3_bwd_supported bit 1 clear) is reported as such.
usage: python tools/convt_grad_bench.py [--calls 40] [--all-levels]   (--all-levels: M355_F32X3_CONVT_BWD=2, the split
kernel also on the levels below the router's small-level floor -- how that floor was measured)"""
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from raw_ops import RawOps, _p  # noqa: E402
from convt_bench import LEVELS  # noqa: E402


def time_calls(fn, calls, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms)


def main():
    if "--all-levels" in sys.argv:
        os.environ["M355_F32X3_CONVT_BWD"] = "2"
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 40
    hip = RawOps("hip")
    L = hip.lib
    print(f"{'level':6s} {'Cin':>4s} {'Cout':>4s} {'S':>4s}  {'route':22s} {'median ms':>10s} {'min ms':>8s} {'GB/s':>7s}")
    for name, ci, co, sp in LEVELS:
        x = torch.randn(1, ci, sp, sp, sp, device="cuda")
        dy = torch.randn(1, co, 2 * sp, 2 * sp, 2 * sp, device="cuda")
        nbytes = 4.0 * (x.numel() + dy.numel())
        d = hip.conv_desc(x.shape, co, 2, 2, 0, compute=3)
        dw, db = torch.empty(ci, co, 2, 2, 2, device="cuda"), torch.empty(co, device="cuda")
        ws = torch.empty(max(int(L.m355_conv_transpose3d_x3_bwd_workspace(C.byref(d))), 16), dtype=torch.uint8, device="cuda")
        plan = (C.c_int32 * 4)()
        L.m355_conv_transpose3d_x3_bwd_plan(C.byref(d), 2, _p(dy), plan)
        supported = L.m355_conv_transpose3d_x3_bwd_supported(C.byref(d), _p(dy)) & 2

        def old():
            hip.convt_bwd_weight(x, dy, 2)

        def new():
            hip._chk(L.m355_conv_transpose3d_bwd_weight_x3(C.byref(d), _p(x), _p(dy), _p(dw), _p(db), _p(ws), ws.numel(),
                                                           hip._stream()), "bwd_weight_x3")
        rows = [("fp32 mfma (first)", old)]
        if supported:
            rows.append((f"x3 <{plan[1]}> {plan[2]} splits", new))
        rows.append(("fp32 mfma (last)", old))
        for what, fn in rows:
            med, mn = time_calls(fn, calls)
            print(f"{name:6s} {ci:4d} {co:4d} {sp:4d}  {what:22s} {med:10.4f} {mn:8.4f} {nbytes / med / 1e6:7.0f}", flush=True)
        if not supported:
            print(f"{name:6s} {'':14s}  x3: refused by the router (plan {tuple(plan)}): the fp32-MFMA kernel keeps the level")


if __name__ == "__main__":
    main()
