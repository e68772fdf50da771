"""Times the binary cross-entropy + Dice loss (csrc/binary_loss.hip) next to the softmax loss it was
modelled on, and the thresholded counts next to the argmax counts, at cfg2's output 1 x 4 x 128^3.

  loss fwd    m355_binary_loss_fwd, prob and logits mode   vs  m355_hybrid_loss_fwd     8 B / element (x and t read once)
  loss bwd    m355_binary_loss_bwd, prob and logits mode   vs  m355_hybrid_loss_bwd    12 B / element (x, t read, dx written)
  counts      m355_eval_multilabel                         vs  m355_eval_scores        the same fp32 scores, a one-byte target
                                                                                        per score (multilabel) or per voxel

    python tools/binary_loss_bench.py [--batches 12] [--calls 5] [--warmup 3] [--out profiles/binary_loss_bench.txt]

The yardstick of every row is the existing kernel on the same tensors in the same process: the columns of a row run
interleaved, the yardstick first AND last (the distance between its two columns is the spread of one kernel against itself
in this process order).  A timed batch is `calls` back-to-back calls between two CUDA events; the figure is the minimum over
the batches, per call.  The new loss moves the bytes of the old one and adds per element one logf (prob mode) or two expf
and one log1pf (logits mode; the library's sigmoid needs expf(-z), the log-sigmoid pair expf(-|z|)); its backward adds one
division (prob) or two expf and two divisions (logits).  67 MB of operands: the 256 MiB Infinity Cache holds them between
calls, so the GB/s are not HBM rates.
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
    assert torch.cuda.is_available(), "binary_loss_bench.py measures on the GPU"
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
    prob = torch.softmax(z, dim=1)                  # a legal input of both losses
    lab = torch.randint(0, Cc, (N, D, H, W), generator=g, device="cuda")
    t = torch.nn.functional.one_hot(lab, Cc).permute(0, 4, 1, 2, 3).float().contiguous()
    cw = torch.tensor([1.0, 2.0, 3.0, 4.0], device="cuda")
    pw = torch.tensor([1.0, 5.0, 0.5, 2.0], device="cuda")
    dloss = torch.ones(1, device="cuda")
    out3, dx = torch.empty(3, device="cuda"), torch.empty_like(z)
    sums4, sums5 = torch.empty(N * Cc * 4, device="cuda"), torch.empty(N * Cc * 5, device="cuda")
    nws = max(int(L.m355_hybrid_loss_workspace(N, Cc, S)), int(L.m355_binary_loss_workspace(N, Cc, S)))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")

    def old_fwd():
        ok(L.m355_hybrid_loss_fwd(p(prob), p(t), N, Cc, S, 0.5, p(cw), 1, p(out3), p(sums4), p(ws), nws, st()))

    def old_bwd():
        ok(L.m355_hybrid_loss_bwd(p(prob), p(t), p(sums4), p(dloss), N, Cc, S, 0.5, p(cw), 1, p(dx), st()))

    def new_fwd(x, logits):
        return lambda: ok(L.m355_binary_loss_fwd(p(x), p(t), N, Cc, S, 0.5, p(cw), p(pw), 1, logits, p(out3), p(sums5), p(ws),
                                                 nws, st()))

    def new_bwd(x, logits):
        return lambda: ok(L.m355_binary_loss_bwd(p(x), p(t), p(sums5), p(dloss), N, Cc, S, 0.5, p(cw), p(pw), 1, logits, p(dx),
                                                 st()))

    # counts: the same fp32 scores [C, S]; eval_scores takes the argmax against a uint8 label map [S], eval_multilabel
    # thresholds every channel against a uint8 multi-hot target [C, S]
    scores = prob[0].contiguous()
    label_map = lab[0].to(torch.uint8).contiguous()
    multi_hot = t[0].to(torch.uint8).contiguous()
    sdesc = (_lib.EvalScoresDesc * 1)()
    sdesc[0].scores, sdesc[0].target = scores.data_ptr(), label_map.data_ptr()
    sdesc[0].size3[:] = (D, H, W)
    sdesc[0].target_kind, sdesc[0].target_dtype = _lib.EV_TARGET_MAP, _lib.EV_U8
    mdesc = (_lib.EvalMultilabelDesc * 1)()
    mdesc[0].scores, mdesc[0].target, mdesc[0].S, mdesc[0].target_dtype = scores.data_ptr(), multi_hot.data_ptr(), S, _lib.EV_U8
    dev_descs = torch.empty(256, dtype=torch.uint8, device="cuda")
    counts = torch.empty(Cc * 3, dtype=torch.int64, device="cuda")
    table = (C.c_int32 * (2 * Cc))(*(list(range(Cc)) * 2))
    labels = (C.c_int32 * Cc)(*range(Cc))
    thr = (C.c_float * Cc)(*([0.5] * Cc))

    def ev_scores():
        ok(L.m355_eval_scores(sdesc, 1, p(dev_descs), _lib.EV_F32, Cc, table, _lib.EV_MASK_NONE, 0, 0, labels, Cc, -2 ** 31,
                              p(counts), st()))

    def ev_multi():
        ok(L.m355_eval_multilabel(mdesc, 1, p(dev_descs), _lib.EV_F32, Cc, thr, p(counts), st()))

    rows = [("loss fwd", 8 * N * Cc * S, [("hybrid (softmax)", old_fwd), ("binary prob", new_fwd(prob, 0)),
                                          ("binary logits", new_fwd(z, 1)), ("hybrid again", old_fwd)]),
            ("loss bwd", 12 * N * Cc * S, [("hybrid (softmax)", old_bwd), ("binary prob", new_bwd(prob, 0)),
                                           ("binary logits", new_bwd(z, 1)), ("hybrid again", old_bwd)]),
            ("counts", None, [("eval_scores", ev_scores), ("eval_multilabel", ev_multi), ("eval_scores again", ev_scores)])]
    count_bytes = {"eval_scores": (4 * Cc + 1) * S, "eval_multilabel": 5 * Cc * S, "eval_scores again": (4 * Cc + 1) * S}
    lines = [f"# device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"# shape {'x'.join(map(str, SHAPE))}; minimum over {a.batches} batches of {a.calls} calls after {a.warmup} warm-up "
             "batches, per call;",
             "# the columns of a row interleaved, CUDA events around each batch; 'x yardstick' = time / the faster of the two",
             "# yardstick columns (the existing kernel, first and last); 'spread' = |first - last| / the faster one"]
    print("\n".join(lines), flush=True)
    for what, nbytes, cols in rows:
        new_fwd(prob, 0)()      # (sums5 / sums4 hold a forward's values whatever ran last)
        old_fwd()
        ms = _time_interleaved([fn for _, fn in cols], a.batches, a.calls, a.warmup)
        base = min(ms[0], ms[-1])
        line = f"{what:9s}" + "".join(
            f"  {name}: {1e3 * tm:7.1f} us {(nbytes or count_bytes[name]) / (tm * 1e-3) / 1e9:5.0f} GB/s" for (name, _), tm in zip(cols, ms))
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
