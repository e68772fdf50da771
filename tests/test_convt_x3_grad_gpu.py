"""The split (M355_COMPUTE_F32X3) weight gradient of the k2 s2 conv-transpose, convt_k2s2_bwd_weight_x3_kernel and its
reduce, called through m355_conv_transpose3d_bwd_weight_x3 and compared with the fp64 host oracle under the bounds
tests/test_convt_launch_plans_gpu.py holds the fp32-MFMA kernel to: per element |err| <= 3e-5 * T + TINY for dw and dbias,
T = the oracle on the absolute values of the operands (the sum of |terms| of that element).

Most of the shapes are below the router's small-level floor (512 voxels in the batch), so every case runs under
M355_F32X3_CONVT_BWD=2, the knob value that lifts the floor and nothing else; tests/test_convt_x3_grad_cpu.py checks what
the router answers without it.  The data gradient has no split kernel: its entry point is refused here as on the host.

Each shape runs with and without dbias, with x and dy as channel slices of wider canary-filled buffers (batch strides
that are not the dense ones), with dw, dbias and the workspace inside guard canaries, and twice (fixed-order reductions:
bit-identical).  W = 33 is refused (the kernel stages pairs of x-adjacent voxels) and asserted so; (2, 8, 8, 17, 30, 32) is
the second trip of the persistent loop with an uneven share in its place.

Measured on an MI355X (profiles/convt_grad_x3_ab.txt), worst err / bound over the five shapes: dw 0.0067 and dbias 0.0006
(both on (1, 320, 320, 2, 4, 8)); the hard operands 0.0045 / 0.0004 of their 1e-5 bound; the model's conv-transpose
gradients, split against fp32 MFMA, 0.0022 / 0.0001 of 6e-5 sum|terms|, every other gradient bit-identical.
"""
import ctypes as C

import pytest
import torch

from raw_ops import _p
from test_kernels_gpu import rnd

pytestmark = pytest.mark.gpu

TINY = 1e-30
EUNSUPPORTED = -2
X3, NONE = 2, 5
# N, Cin, Cout, D, H, W
SHAPES = [(2, 40, 24, 3, 5, 8),      # ragged channel tiles in both operands, voxel tail, a tile straddling two samples
          (2, 64, 64, 4, 8, 16),     # the u0 channel shape with everything aligned
          (1, 130, 70, 9, 20, 20),   # more than four m-tiles, Cout not a multiple of the column tile
          (1, 320, 320, 2, 4, 8),    # u3's widths: two tiles, one per workgroup
          (2, 8, 8, 17, 30, 32)]     # 32 640 voxels: the second trip of every persistent loop, with an uneven share
REFS = {}


def operands(shape):
    N, Cin, Cout, D, H, W = shape
    return rnd(N, Cin, D, H, W, seed=1), rnd(N, Cout, 2 * D, 2 * H, 2 * W, seed=5)


def reference(oracle, shape):
    """(dw, dbias, sum|terms| of dw, of dbias) of the fp64 host oracle, computed once per shape"""
    if shape not in REFS:
        x, dy = operands(shape)
        REFS[shape] = oracle.convt_bwd_weight(x, dy, 2, 2, 0, 0) + oracle.convt_bwd_weight(x.abs(), dy.abs(), 2, 2, 0, 0)
    return REFS[shape]


class X3Call:
    """m355_conv_transpose3d_bwd_weight_x3 on Slots: x and dy as channel slices, dw / dbias / workspace in canaries"""

    def __init__(self, hip, x, dy, with_bias, sliced=True):
        self.hip, self.L = hip, hip.lib
        N, Cin, D, H, W = x.shape
        Cout = dy.shape[1]
        lay = dict(c_pre=1, c_post=2) if sliced else dict(c_pre=0, c_post=0)
        self.x = hip.slot(x, extra=2 if sliced else 0, **lay)       # even batch stride, 8-byte aligned
        self.dy = hip.slot(dy, extra=4 if sliced else 0, **lay)     # batch stride % 4 == 0, 16-byte aligned
        self.d = hip.conv_desc(x.shape, Cout, 2, 2, 0, xbs=self.x.bs, ybs=self.dy.bs, compute=3)
        self.dw = hip.slot((Cin, Cout, 2, 2, 2), c_pre=0, c_post=0)
        self.db = hip.slot((1, Cout), c_pre=0, c_post=0) if with_bias else None
        self.ws_bytes = int(self.L.m355_conv_transpose3d_x3_bwd_workspace(C.byref(self.d)))
        self.ws = hip.slot((1, max(self.ws_bytes // 4, 4)), c_pre=0, c_post=0)

    def plan(self):
        out = (C.c_int32 * 4)()
        assert self.L.m355_conv_transpose3d_x3_bwd_plan(C.byref(self.d), 2, _p(self.dy), out) == 0
        return tuple(out)

    def supported(self):
        return self.L.m355_conv_transpose3d_x3_bwd_supported(C.byref(self.d), _p(self.dy))

    def run(self):
        rc = self.L.m355_conv_transpose3d_bwd_weight_x3(C.byref(self.d), _p(self.x), _p(self.dy), _p(self.dw), _p(self.db),
                                                        _p(self.ws), self.ws_bytes, self.hip._stream())
        torch.cuda.synchronize()
        return rc

    def outputs(self, what):
        self.ws.assert_guards_intact(what + " workspace")
        self.x.assert_unchanged(what + " x")
        self.dy.assert_unchanged(what + " dy")
        dw = self.dw.check_output(what + " dw")
        db = self.db.check_output(what + " dbias").view(-1) if self.db is not None else None
        return dw, db


def bounded(got, ref, bound, what):
    got, ref, bound = got.detach().cpu().double(), ref.detach().cpu().double(), bound.detach().cpu().double()
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    ratio = (got - ref).abs() / bound
    worst = float(ratio.max()) if not torch.isnan(ratio).any() else float("inf")
    print(f"{what}: worst err / bound {worst:.4f}")
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements over their bound, worst {worst:.3f}x"


@pytest.mark.parametrize("with_bias", [True, False], ids=["dbias", "no-dbias"])
@pytest.mark.parametrize("shape", SHAPES, ids=repr)
def test_weight_gradient_against_the_oracle(hip, oracle, tuning, shape, with_bias):
    tuning(M355_F32X3_CONVT_BWD=2)
    x, dy = operands(shape)
    ref_dw, ref_db, t, tb = reference(oracle, shape)
    call = X3Call(hip, x, dy, with_bias)
    fam, mt, nsplit, _ = call.plan()
    assert fam == X3 and mt == (4 if shape[1] > 64 else 2) and nsplit >= 1 and call.supported() == 2
    assert call.run() == 0, hip.lib.m355_last_error()
    dw, db = call.outputs(repr(shape))
    bounded(dw, ref_dw, 3e-5 * t + TINY, f"{shape} dw, {nsplit} splits")
    if with_bias:
        bounded(db, ref_db, 3e-5 * tb + TINY, f"{shape} dbias")
    again = X3Call(hip, x, dy, with_bias)
    assert again.run() == 0
    dw2, db2 = again.outputs(repr(shape) + " second call")
    assert torch.equal(dw, dw2) and (db is None or torch.equal(db, db2)), "not bit-identical: the reductions have a fixed order"
    # the dense layout gives the same bits: the slices change addresses only
    dense = X3Call(hip, x, dy, with_bias, sliced=False)
    assert dense.run() == 0
    dw3, db3 = dense.outputs(repr(shape) + " dense")
    assert torch.equal(dw, dw3) and (db is None or torch.equal(db, db3))
    # the data gradient has no split kernel: refused before any launch
    dx = hip.slot((shape[0], shape[1]) + shape[3:], c_pre=0, c_post=0)
    w = torch.zeros(shape[1], shape[2], 2, 2, 2, device="cuda")
    assert hip.lib.m355_conv_transpose3d_bwd_data_x3(C.byref(call.d), _p(call.dy), _p(w), _p(dx), None, 0, hip._stream()) == EUNSUPPORTED
    torch.cuda.synchronize()
    dx.assert_untouched("refused data gradient")


def test_odd_width_is_refused_and_nothing_is_written(hip, tuning):
    """W = 33: a pair of x-adjacent voxels would straddle two rows -> the fp32-MFMA kernel keeps the shape"""
    tuning(M355_F32X3_CONVT_BWD=2)
    shape = (2, 8, 8, 17, 30, 33)
    x, dy = operands(shape)
    call = X3Call(hip, x, dy, True, sliced=False)
    assert call.plan() == (NONE, 0, 0, 0) and call.supported() == 0 and call.ws_bytes == 0
    assert call.run() == EUNSUPPORTED
    call.dw.assert_untouched("refused call")
    call.db.assert_untouched("refused call")


def test_operands_a_bf16_rounding_would_destroy(hip, oracle, tuning):
    """All 24 significant bits in use, magnitudes 2^-20 .. 2^20 per channel on both operands, signed zeros: the three-way
    split is exact and six of its nine products are kept, so the error stays below 1e-5 * sum|terms| (one rounding of
    either operand to bf16 would cost 2^-9 of a term)."""
    tuning(M355_F32X3_CONVT_BWD=2)
    N, Cin, Cout, D, H, W = 2, 40, 24, 3, 6, 8
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, Cin, D, H, W, generator=g) * (2.0 ** torch.randint(-20, 21, (1, Cin, 1, 1, 1), generator=g).float())
    dy = torch.randn(N, Cout, 2 * D, 2 * H, 2 * W, generator=g) * (2.0 ** torch.randint(-20, 21, (1, Cout, 1, 1, 1), generator=g).float())
    x[0, 3, 1, 2, 5] = -0.0
    x[1, 0, 0, 0, 0] = 0.0
    dy[1, 2, 3, 4, 5] = -0.0
    dy[0, 0, 0, 0, 1] = 0.0
    ref_dw, ref_db = oracle.convt_bwd_weight(x, dy, 2, 2, 0, 0)
    t, tb = oracle.convt_bwd_weight(x.abs(), dy.abs(), 2, 2, 0, 0)
    call = X3Call(hip, x, dy, True)
    assert call.plan()[0] == X3 and call.run() == 0
    dw, db = call.outputs("hard operands")
    bounded(dw, ref_dw, 1e-5 * t + TINY, "hard operands dw")
    bounded(db, ref_db, 1e-5 * tb + TINY, "hard operands dbias")


def test_model_backward_takes_the_split_route_and_agrees_with_the_fp32_mfma_route(hip, oracle, tuning, monkeypatch):
    """One ModularUNet backward whose conv-transpose is the second shape (64 -> 64 channels at 4 x 8 x 16, N = 2), with the
    split weight gradient on (M355_F32X3_CONVT_BWD=2, as in the other tests of this file) and off (0).  The entry point
    is counted through a wrapper.  The conv-transpose's x and dy are the same tensors in both runs (nothing upstream of
    them reads dw), so its parameter gradients are two kernels' answers to one question: each is within 3e-5 * sum|terms|
    of the exact one, hence they are within 6e-5 * sum|terms| of each other, per element, sum|terms| from the oracle on
    the |x| and |dy| the model handed to ops.conv_transpose3d.  No other gradient depends on the kernel: 1e-5 of its
    maximum covers whatever run-to-run difference the other kernels have."""
    from functools import partial

    from torch import nn

    from segmentation_pipeline_amd import _lib, ops
    from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss
    from segmentation_pipeline_amd.models import ModularUNet

    L = _lib.lib()
    real = L.m355_conv_transpose3d_bwd_weight_x3
    calls, seen = [], {}

    def counted(*args):
        rc = real(*args)
        calls.append(rc)
        return rc
    monkeypatch.setattr(L, "m355_conv_transpose3d_bwd_weight_x3", counted)
    real_convt = ops.conv_transpose3d

    def recorded(x, *args, **kwargs):
        y = real_convt(x, *args, **kwargs)
        seen["x"] = x.detach().clone()
        y.register_hook(lambda g: seen.__setitem__("dy", g.detach().clone()))
        return y
    monkeypatch.setattr(ops, "conv_transpose3d", recorded)

    torch.manual_seed(0)
    model = ModularUNet(2, 3, [16, 64], 2, block_params={'normalization_class': partial(nn.GroupNorm, 8)},
                        upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2}).to("cuda").train()
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((2, 2, 8, 16, 32), generator=gen).cuda()
    lab = torch.randint(0, 3, (2, 8, 16, 32), generator=gen)
    y = torch.nn.functional.one_hot(lab, 3).permute(0, 4, 1, 2, 3).float().contiguous().cuda()

    def grads(knob):
        tuning(M355_F32X3_CONVT_BWD=knob)
        model.zero_grad(set_to_none=True)
        with ops.precision("fp32"):
            HybridLogisticDiceLoss()(model(x), y)["loss"].backward()
        torch.cuda.synchronize()
        return {k: v.grad.detach().clone() for k, v in model.named_parameters()}

    assert ops.FP32_SPLIT, "the fp32 mode maps to M355_COMPUTE_F32X3 unless M355_FP32_SPLIT=0"
    on = grads(2)
    assert calls == [0], f"the split entry point ran {len(calls)} times with status {calls}"
    assert tuple(seen["x"].shape) == (2, 64, 4, 8, 16) and tuple(seen["dy"].shape) == (2, 64, 8, 16, 32)
    t, tb = oracle.convt_bwd_weight(seen["x"].abs().cpu(), seen["dy"].abs().cpu(), 2, 2, 0, 0)
    off = grads(0)
    assert calls == [0], "M355_F32X3_CONVT_BWD=0: the split entry point is not called"
    up = {k: b for k, b in ((k, t if v.dim() == 5 else tb) for k, v in on.items() if "upsampling" in k)}
    assert len(up) == 2, list(up)
    for k in on:
        diff = (on[k] - off[k]).abs().cpu().double()
        if k in up:
            ratio = float((diff / (6e-5 * up[k].double() + TINY)).max())
            print(f"{k}: split against fp32 MFMA, worst |diff| / (6e-5 sum|terms|) {ratio:.4f}")
            assert ratio <= 1.0, (k, ratio)
        else:
            scale = off[k].abs().max().item()
            print(f"{k}: max|diff| {float(diff.max()):.3e}  max|grad| {scale:.3e}")
            assert float(diff.max()) <= 1e-5 * scale + TINY, (k, float(diff.max()), scale)
