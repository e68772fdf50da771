"""nn.Sigmoid as hypothesis_class, the parts that need no device: the models construct and route the head (into the output
convolution where that is an nn.Conv3d, through ops.sigmoid otherwise), every other module keeps being refused by name, and
the library's host side answers for M355_CONV_SIGMOID exactly as it does for M355_CONV_SOFTMAX."""
import ctypes as C

import pytest
import torch
from torch import nn

from segmentation_pipeline_amd import _lib, ops
from segmentation_pipeline_amd.models import ModularUNet, NestedResUNet
from segmentation_pipeline_amd.models import modular_unet as MU
from test_conv_routes_cpu import BF16, EINVALID, EUNSUPPORTED, F16, F32, FWD, FWD_H16, SHAPES, desc, launch_plan


class _Recorder:
    """stands in for ops.conv3d and ops.sigmoid: records the head keywords, returns tensors of the right shape"""

    def __init__(self, monkeypatch):
        self.convs, self.sigmoids = [], 0
        monkeypatch.setattr(ops, "conv3d", self.conv3d)
        monkeypatch.setattr(ops, "sigmoid", self.sigmoid)

    def conv3d(self, x, weight, bias=None, **kw):
        self.convs.append({k: kw.get(k, False) for k in ("softmax", "sigmoid")})
        return torch.zeros((x.shape[0], weight.shape[0]) + tuple(x.shape[2:]))

    def sigmoid(self, x):
        self.sigmoids += 1
        return torch.sigmoid(x)


class _OutConv(nn.Module):
    """an output convolution that is no nn.Conv3d (run_conv reads weight / bias / stride / padding)"""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(out_channels, in_channels, 3, 3, 3))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.stride, self.padding = (1, 1, 1), (1, 1, 1)


def _unet(**kw):
    return ModularUNet(2, 3, [8, 16, 16], 3, hypothesis_class=nn.Sigmoid, hypothesis_params={}, **kw)


def test_models_construct_with_a_sigmoid_head():
    assert type(_unet().hypothesis) is nn.Sigmoid
    assert type(NestedResUNet(3, 2, 8, hypothesis_class=nn.Sigmoid, hypothesis_params={}).hypothesis) is nn.Sigmoid
    with pytest.raises(TypeError):      # the reference's default {"dim": 1} is torch's own error, here as there
        NestedResUNet(3, 2, 8, hypothesis_class=nn.Sigmoid)


def _tail(model, x):
    """what follows the last up block in ModularUNet._forward, through the model's own code: depth 1 has one block only,
    and that block is replaced by the identity"""
    model.down_blocks[0].forward = lambda t, **kw: t
    return model._forward(x)


def test_modular_unet_routes_the_head(monkeypatch):
    rec = _Recorder(monkeypatch)
    m = ModularUNet(8, 3, [8], 1, hypothesis_class=nn.Sigmoid, hypothesis_params={})
    p = _tail(m, torch.zeros(1, 8, 4, 4, 4))
    assert rec.convs == [{"softmax": False, "sigmoid": True}] and rec.sigmoids == 0 and p.shape == (1, 3, 4, 4, 4)
    # a non-Conv3d output convolution: plain conv, then ops.sigmoid
    rec.convs.clear()
    m = ModularUNet(8, 3, [8], 1, hypothesis_class=nn.Sigmoid, hypothesis_params={}, out_conv_class=_OutConv,
                    out_conv_params={'in_channels': 8, 'out_channels': 3})
    p = _tail(m, torch.zeros(1, 8, 4, 4, 4))
    assert rec.convs == [{"softmax": False, "sigmoid": False}] and rec.sigmoids == 1
    assert torch.equal(p, torch.full((1, 3, 4, 4, 4), 0.5))
    # the softmax head keeps its keyword
    rec.convs.clear()
    _tail(ModularUNet(8, 3, [8], 1), torch.zeros(1, 8, 4, 4, 4))
    assert rec.convs == [{"softmax": True, "sigmoid": False}] and rec.sigmoids == 1     # (no further ops.sigmoid call)


@pytest.mark.parametrize("cls,params", [(nn.LogSigmoid, {}), (nn.Hardsigmoid, {}), (nn.LogSoftmax, {"dim": 1})])
def test_other_heads_keep_raising_by_name(monkeypatch, cls, params):
    rec = _Recorder(monkeypatch)
    m = ModularUNet(8, 3, [8], 1, hypothesis_class=cls, hypothesis_params=params)
    with pytest.raises(NotImplementedError) as e:
        _tail(m, torch.zeros(1, 8, 4, 4, 4))
    msg = str(e.value)
    assert cls.__name__ in msg
    for supported in ("Softmax(dim=1)", "Sigmoid", "StochasticMatrix", "Identity"):
        assert supported in msg, msg
    assert rec.convs == [{"softmax": False, "sigmoid": False}] and rec.sigmoids == 0
    with pytest.raises(NotImplementedError):
        MU._run_hypothesis(cls(**params), torch.zeros(1, 3, 2, 2, 2))


def test_conv3d_refuses_both_heads():
    w = torch.zeros(3, 8, 3, 3, 3)
    with pytest.raises(ValueError, match="exclude"):
        ops.conv3d(torch.zeros(1, 8, 4, 4, 4), w, softmax=True, sigmoid=True)


# ------------------------------------------------------------------------------------------------ the library's host side
@pytest.mark.parametrize("compute", [F32, BF16, F16])
@pytest.mark.parametrize("shape", SHAPES)
def test_fuses_sigmoid_is_fuses_softmax(shape, compute):
    """one epilogue slot: the two queries agree, and a call with the flag is served exactly where they say so"""
    L = _lib.lib()
    d = desc(shape, compute)
    fuses = L.m355_conv3d_fuses_sigmoid(C.byref(d))
    assert fuses == L.m355_conv3d_fuses_softmax(C.byref(d))
    entry = FWD_H16 if compute in (BF16, F16) else FWD
    plain, soft = launch_plan(entry, d), launch_plan(entry, desc(shape, compute, flags=_lib.CONV_SOFTMAX))
    sig = launch_plan(entry, desc(shape, compute, flags=_lib.CONV_SIGMOID))
    assert (sig[0] == 0) == bool(fuses) and sig == soft          # the same launch as for the softmax flag
    assert plain[0] == 0 and family_of(d) == family_of(desc(shape, compute, flags=_lib.CONV_SIGMOID))   # m355_conv3d_plan
    assert L.m355_conv3d_fuses_sigmoid(None) == 0


def family_of(d):
    out = (C.c_int32 * 4)()
    assert _lib.lib().m355_conv3d_plan(C.byref(d), 0, out) == 0
    return tuple(out)


def test_some_shape_fuses_in_every_mode():
    """(so that the equality above is not 0 == 0 throughout)"""
    L = _lib.lib()
    for compute in (F32, BF16, F16):
        assert any(L.m355_conv3d_fuses_sigmoid(C.byref(desc(s, compute))) for s in SHAPES), compute


def test_head_flags_are_checked_before_any_launch():
    L = _lib.lib()
    fusing = next(s for s in SHAPES if L.m355_conv3d_fuses_sigmoid(C.byref(desc(s))))
    rc, _ = launch_plan(FWD, desc(fusing, flags=_lib.CONV_SOFTMAX | _lib.CONV_SIGMOID))
    assert rc == EINVALID and b"SIGMOID" in L.m355_last_error()
    assert _lib.CONV_SOFTMAX | _lib.CONV_SIGMOID == 2 | 4
    d = desc((2, 8, 8, 8, 8, 8), flags=_lib.CONV_SIGMOID)
    assert L.m355_conv3d_fuses_sigmoid(C.byref(d)) == 0
    rc, _ = launch_plan(FWD, d)
    assert rc == EUNSUPPORTED and b"SIGMOID" in L.m355_last_error() and b"m355_conv3d_fuses_sigmoid" in L.m355_last_error()
    # the entry point itself answers the same, before following a pointer
    p = C.c_void_p(1 << 20)
    assert L.m355_conv3d_fwd(C.byref(d), p, p, None, None, p, p, 1 << 30, None) == EUNSUPPORTED
    for compute in (BF16, F16):
        d16 = desc((2, 8, 8, 8, 8, 8), compute, flags=_lib.CONV_SIGMOID)
        assert launch_plan(FWD_H16, d16)[0] == EUNSUPPORTED and b"SIGMOID" in L.m355_last_error()


def test_stand_alone_kernels_check_their_arguments():
    L = _lib.lib()
    p = C.c_void_p(1 << 20)
    assert L.m355_sigmoid_fwd(None, p, 16, None) == EINVALID and b"sigmoid_fwd" in L.m355_last_error()
    assert L.m355_sigmoid_fwd(p, None, 16, None) == EINVALID
    assert L.m355_sigmoid_fwd(p, p, 0, None) == EINVALID and b"sigmoid_fwd" in L.m355_last_error()
    assert L.m355_sigmoid_fwd(p, p, -4, None) == EINVALID
    assert L.m355_sigmoid_bwd(p, None, p, 16, None) == EINVALID and b"sigmoid_bwd" in L.m355_last_error()
    assert L.m355_sigmoid_bwd(p, p, p, 0, None) == EINVALID
