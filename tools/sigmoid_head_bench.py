"""Times the output convolution 32 -> 3 on 1 x 32 x 128^3 with the nn.Sigmoid head fused into its epilogue
(M355_CONV_SIGMOID) next to the pair it replaces, convolution + m355_sigmoid_fwd, in fp32
(conv3_valu_smallcout_kernel) and bf16 (c8 input; conv3_cout4_h16_kernel), and the stand-alone kernels alone.

    python tools/sigmoid_head_bench.py [--batches 12] [--calls 5] [--warmup 3] [--out profiles/sigmoid_head_bench.txt]

The variants of a row run interleaved in one process.  A timed batch is `calls` back-to-back calls between two CUDA
events; the figure is the minimum over the batches, per call (the method of tools/activation_bench.py).  Weights are
packed once (M355_CONV_W_PACKED), as ops.py does.  The fused call saves one write and one read of the 3 x 128^3 fp32
logits (25 MB each way); the stand-alone kernels move 8 bytes per element (forward) and 12 (backward).
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, CIN, COUT, D, H, W = 1, 32, 3, 128, 128, 128


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
    assert torch.cuda.is_available(), "sigmoid_head_bench.py measures on the GPU"
    L = _lib.lib()

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def st():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ok(rc):
        assert rc == 0, L.m355_last_error()

    S = D * H * W
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((N, CIN, D, H, W), generator=g, device="cuda")
    w = torch.randn((COUT, CIN, 3, 3, 3), generator=g, device="cuda") * 0.05
    b = torch.randn(COUT, generator=g, device="cuda")
    logits, y, y2 = (torch.empty((N, COUT, D, H, W), device="cuda") for _ in range(3))
    dy, dx = torch.randn((N, COUT, D, H, W), generator=g, device="cuda"), torch.empty((N, COUT, D, H, W), device="cuda")
    n_out = N * COUT * S
    lines = [f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"# output convolution {CIN} -> {COUT} on {N} x {CIN} x {D}^3; minimum over {a.batches} batches of {a.calls} calls after "
             f"{a.warmup} warm-up batches, per call;",
             "# the variants of a row interleaved, CUDA events around each batch; pair = convolution, then m355_sigmoid_fwd",
             f"{'mode':6s} {'kernel':30s} {'conv us':>9s} {'fused us':>9s} {'pair us':>9s} {'fused / pair':>13s} {'saved us':>9s}"]
    print("\n".join(lines), flush=True)
    for mode, compute in (("fp32", _lib.COMPUTE_F32), ("bf16", _lib.COMPUTE_BF16)):
        d = _lib.ConvDesc(N, CIN, COUT, D, H, W, 3, 1, 1, 0, 0, 0, compute, 0)
        assert L.m355_conv3d_fuses_sigmoid(C.byref(d)) == 1
        packed = torch.empty(int(L.m355_conv3d_packed_bytes(C.byref(d), 0)), dtype=torch.uint8, device="cuda")
        ok(L.m355_conv3d_pack(C.byref(d), 0, p(w), p(packed), st()))
        plain = _lib.ConvDesc(N, CIN, COUT, D, H, W, 3, 1, 1, 0, 0, 0, compute, _lib.CONV_W_PACKED)
        fused = _lib.ConvDesc(N, CIN, COUT, D, H, W, 3, 1, 1, 0, 0, 0, compute, _lib.CONV_W_PACKED | _lib.CONV_SIGMOID)
        if compute == _lib.COMPUTE_F32:
            ws = torch.empty(max(int(L.m355_conv3d_fwd_workspace(C.byref(d))), 16), dtype=torch.uint8, device="cuda")

            def conv(desc, out):
                return lambda: ok(L.m355_conv3d_fwd(C.byref(desc), p(x), p(packed), p(b), None, p(out), p(ws), ws.numel(), st()))
        else:
            x16 = torch.empty((N, (CIN + 7) // 8, S, 8), dtype=torch.bfloat16, device="cuda")
            ok(L.m355_act16_pack(p(x), p(x16), N, CIN, S, 0, 0, compute, st()))
            ws = torch.empty(max(int(L.m355_conv3d_h16_workspace(C.byref(d), 0)), 16), dtype=torch.uint8, device="cuda")

            def conv(desc, out):
                return lambda: ok(L.m355_conv3d_fwd_h16(C.byref(desc), p(x16), 0, p(packed), p(b), None, p(out), None, p(ws),
                                                        ws.numel(), st()))
        out12 = (C.c_int64 * 12)()
        entry = 0 if compute == _lib.COMPUTE_F32 else 4
        ptrs = (C.c_uint64 * 7)(x.data_ptr(), packed.data_ptr(), b.data_ptr(), 0, y.data_ptr(), 0, ws.data_ptr())
        ok(L.m355_conv3d_launch_plan(entry, C.byref(fused), (C.c_int64 * 2)(0, 0), ptrs, ws.numel(), out12))
        kernel = {3: "conv3_valu_smallcout_kernel", 8: "conv3_h16_kernel (one-shot)", 10: "conv3_cout4_h16_kernel"}.get(out12[0], f"variant {out12[0]}")
        conv_plain, conv_fused = conv(plain, logits), conv(fused, y)

        def pair():
            conv_plain()
            ok(L.m355_sigmoid_fwd(p(logits), p(y2), n_out, st()))
        conv_fused()
        pair()
        torch.cuda.synchronize()
        assert torch.equal(y, y2), "fused and unfused heads differ"
        t_conv, t_fused, t_pair = _time_interleaved([conv_plain, conv_fused, pair], a.batches, a.calls, a.warmup)
        line = (f"{mode:6s} {kernel:30s} {1e3 * t_conv:9.1f} {1e3 * t_fused:9.1f} {1e3 * t_pair:9.1f} {t_fused / t_pair:13.3f} "
                f"{1e3 * (t_pair - t_fused):9.1f}")
        lines.append(line)
        print(line, flush=True)
    t_fwd, t_bwd = _time_interleaved([lambda: ok(L.m355_sigmoid_fwd(p(logits), p(y2), n_out, st())),
                                      lambda: ok(L.m355_sigmoid_bwd(p(y2), p(dy), p(dx), n_out, st()))], a.batches, a.calls, a.warmup)
    for name, t, nbytes in (("m355_sigmoid_fwd", t_fwd, 8), ("m355_sigmoid_bwd", t_bwd, 12)):
        line = f"{name} over {n_out} elements: {1e3 * t:.1f} us, {nbytes * n_out / (t * 1e-3) / 1e9:.0f} GB/s over {nbytes} B / element"
        lines.append(line)
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
