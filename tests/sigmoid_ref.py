"""Test-side helpers of the nn.Sigmoid hypothesis head: the raw C-ABI wrappers of tests/raw_ops.py with the
M355_CONV_SIGMOID flag and the two stand-alone entry points added, and the CPU formulation of the models up to the logits
(oracle/torch_ref.py's blocks, the head and the loss applied by the caller)."""
import ctypes as C

import torch
import torch.nn.functional as F

from oracle import torch_ref as R
from raw_ops import RawOps, _p
from segmentation_pipeline_amd import _lib

# the values planted into the stand-alone kernels' input: the centre, the linear range, both saturated ends, and
# |v| > 88.7 where expf(-v) is +inf (v < 0: the result is +0) or 0; -104 is past the smallest fp32 denormal of exp(v)
PLANTED = (0.0, 1e-6, -1e-6, 1.0, -1.0, 20.0, -20.0, 88.0, -88.0, 90.0, -90.0, 104.0, -104.0)


class SigmoidOps(RawOps):
    """RawOps whose conv3d_fwd / conv3d_fwd_h16 take sigmoid=True (the descriptor then carries M355_CONV_SIGMOID; the
    wrapper asserts that the library offers the epilogue), plus m355_sigmoid_fwd / m355_sigmoid_bwd."""
    _head_flag = 0

    def conv_desc(self, *a, **kw):   # (every wrapper of the base class builds its descriptor here)
        d = RawOps.conv_desc(*a, **kw)
        d.flags |= self._head_flag
        return d

    def _with_head(self, call, d, sigmoid):
        if not sigmoid:
            return call()
        assert self.backend == "hip" and self.lib.m355_conv3d_fuses_sigmoid(C.byref(d)) == 1
        self._head_flag = _lib.CONV_SIGMOID
        try:
            return call()
        finally:
            self._head_flag = 0

    def conv3d_fwd(self, x, w, bias=None, add=None, sigmoid=False, **kw):
        d = RawOps.conv_desc(tuple(x.shape), w.shape[0], w.shape[2], kw.get("stride", 1), kw.get("pad", 1),
                             compute=kw.get("compute", 0))
        return self._with_head(lambda: super(SigmoidOps, self).conv3d_fwd(x, w, bias, add, **kw), d, sigmoid)

    def conv3d_fwd_h16(self, x16, Cin, spatial, w, bias=None, add=None, compute=1, sigmoid=False, **kw):
        d = RawOps.conv_desc((x16.shape[0], Cin) + tuple(spatial), w.shape[0], 3, 1, 1, compute=compute)
        return self._with_head(lambda: super(SigmoidOps, self).conv3d_fwd_h16(x16, Cin, spatial, w, bias, add, compute, **kw),
                               d, sigmoid)

    def sigmoid_fwd(self, x, out=None):
        """x: a dense tensor or 1-d view on this backend's device (its data pointer is what the kernel gets)"""
        y = torch.empty_like(x, memory_format=torch.contiguous_format) if out is None else out
        self._chk(self.lib.m355_sigmoid_fwd(_p(x), _p(y), x.numel(), self._stream()), "sigmoid_fwd")
        return y

    def sigmoid_bwd(self, y, dy, out=None):
        dx = torch.empty_like(y, memory_format=torch.contiguous_format) if out is None else out
        self._chk(self.lib.m355_sigmoid_bwd(_p(y), _p(dy), _p(dx), y.numel(), self._stream()), "sigmoid_bwd")
        return dx


def unet_logits(sd, spec: R.UNetSpec, x, training=True):
    """ModularUNet up to the output convolution (spec.hypothesis must be 'none')"""
    assert spec.hypothesis == "none"
    return R.unet_forward(sd, spec, x, training)


def nested_logits(sd, x, training=True):
    """NestedResUNet up to the output convolution: oracle/torch_ref.py's nested_res_unet_forward without its softmax"""
    down = lambda t: F.avg_pool3d(t, 2, 2, count_include_pad=False)   # noqa: E731
    up = lambda t: F.interpolate(t, scale_factor=2, mode="trilinear", align_corners=True)   # noqa: E731
    blk = lambda name, t, res=False: R.nested_block(sd, name, t, res, training)   # noqa: E731
    x0_0 = blk("conv0_0", x, True)
    x1_0 = blk("conv1_0", down(x0_0))
    x0_1 = blk("conv0_1", torch.cat((x0_0, up(x1_0)), 1), True)
    x2_0 = blk("conv2_0", down(x1_0))
    x1_1 = blk("conv1_1", torch.cat((x1_0, up(x2_0), down(x0_1)), 1))
    x0_2 = blk("conv0_2", torch.cat((x0_1, up(x1_1)), 1), True)
    x3_0 = blk("conv3_0", down(x2_0))
    x2_1 = blk("conv2_1", torch.cat((x2_0, up(x3_0), down(x1_1)), 1))
    x1_2 = blk("conv1_2", torch.cat((x1_1, up(x2_1), down(x0_2)), 1))
    x0_3 = blk("conv0_3", torch.cat((x0_2, up(x1_2)), 1), True)
    return F.conv3d(x0_3, sd["out_conv.weight"], sd["out_conv.bias"], padding=1)
