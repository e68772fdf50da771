"""nn.ELU, nn.GELU (both approximations) and nn.SiLU as activation_class of Block3d: the Python mapping (_act_code) and the
host side of the normalisation family for the codes 3..6 (csrc/norm_host.hpp, csrc/activation.hpp).  Pure host code, no GPU:
the entry points are called with dummy non-null pointers and stop at their argument checks, as tests/test_norm_routes_cpu.py
does."""
import ctypes as C

import pytest
from torch import nn

from segmentation_pipeline_amd import _lib
from segmentation_pipeline_amd.models.components import Block3d, _act_code

EINVALID = -1
CASES = [(nn.ELU, {'alpha': 0.7, 'inplace': True}, 3), (nn.GELU, {}, 4), (nn.GELU, {'approximate': 'tanh'}, 5), (nn.SiLU, {}, 6)]
IDS = ["elu", "gelu", "gelu_tanh", "silu"]
# BatchNorm on a misaligning batch stride, GroupNorm on two network-level shapes, an odd one
DESCS = [(2, 8, 4 * 50 * 42, 0, 1), (1, 32, 64 ** 3, 8, 0), (2, 20, 2 * 2 * 819, 4, 0), (2, 5, 1, 0, 0)]


def desc(case, act):
    N, Cc, S, groups, k = case
    bs = [(Cc * S + k * j) if k else 0 for j in (1, 2, 3)]
    return _lib.NormDesc(N, Cc, S, groups, act, 1e-5, 0.7, *bs)


@pytest.mark.parametrize("cls,params,code", CASES, ids=IDS)
def test_block3d_constructs_and_maps_the_code(cls, params, code):
    block = Block3d(4, 8, activation_class=cls, activation_params=params)
    acts = [m for name, m in block.layers.named_children() if name.startswith("activation")]
    assert len(acts) == 2 and all(type(a) is cls for a in acts)
    got, param = _act_code(acts[0])
    assert got == code and isinstance(param, float)
    if cls is nn.ELU:
        assert param == 0.7
    relu = Block3d(4, 8, activation_class=nn.ReLU)
    assert list(block.state_dict().keys()) == list(relu.state_dict().keys())


def test_the_codes_are_the_headers():
    assert (_lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_LEAKY_RELU, _lib.ACT_ELU, _lib.ACT_GELU, _lib.ACT_GELU_TANH,
            _lib.ACT_SILU) == tuple(range(7))
    assert _act_code(nn.ELU()) == (3, 1.0) and _act_code(nn.GELU(approximate='none'))[0] == 4
    # the earlier three are untouched
    assert _act_code(nn.ReLU(inplace=True)) == (1, 0.0) and _act_code(nn.LeakyReLU(0.2)) == (2, 0.2)
    assert _act_code(nn.Identity()) == (0, 0.0) and _act_code(None) == (0, 0.0)


@pytest.mark.parametrize("make", [nn.Mish, nn.SELU, nn.PReLU, nn.Tanh, nn.CELU, nn.Softplus, nn.Hardswish, nn.ReLU6,
                                  lambda: nn.GELU(approximate='sigmoid')],
                         ids=["Mish", "SELU", "PReLU", "Tanh", "CELU", "Softplus", "Hardswish", "ReLU6", "GELU-unknown"])
def test_other_activations_still_fail_loudly(make):
    with pytest.raises(NotImplementedError, match="activation_class .* has no HIP kernel .*ELU, GELU, SiLU"):
        _act_code(make())
    with pytest.raises(NotImplementedError, match="activation_class"):
        Block3d(4, 8, activation_class=make, activation_params={})


@pytest.mark.parametrize("act", [3, 4, 5, 6])
@pytest.mark.parametrize("case", DESCS)
def test_plans_take_the_new_codes_and_do_not_depend_on_them(case, act):
    """m355_norm_plan answers for every pass, and its four numbers and m355_norm_workspace are those of ReLU: the activation
    changes no launch geometry and no workspace layout"""
    L = _lib.lib()
    d, d1 = desc(case, act), desc(case, 1)
    out, out1 = (C.c_int32 * 4)(), (C.c_int32 * 4)()
    for which in range(10):
        assert L.m355_norm_plan(C.byref(d), which, out) == 0, (which, L.m355_last_error())
        assert L.m355_norm_plan(C.byref(d1), which, out1) == 0
        assert tuple(out) == tuple(out1), which
    assert L.m355_norm_workspace(C.byref(d)) == L.m355_norm_workspace(C.byref(d1)) > 0


@pytest.mark.parametrize("act", [7, -1, 8])
def test_codes_outside_0_to_6_stay_invalid(act):
    L = _lib.lib()
    p, out = C.c_void_p(4096), (C.c_int32 * 4)()
    d = desc(DESCS[1], act)
    ref = C.byref(d)
    assert L.m355_norm_act_fwd(ref, p, p, p, p, p, None, p, None) == EINVALID and b"activation" in L.m355_last_error()
    assert L.m355_norm_plan(ref, 1, out) == EINVALID
    big = 1 << 40
    assert L.m355_norm_act_bwd(ref, p, p, p, p, p, p, p, p, p, 1, p, big, None) == EINVALID
    # the c8 backward checks the code itself
    assert L.m355_norm_act_bwd_c8(ref, p, 0, p, 0, None, 0, 64, 64, 64, p, p, p, p, p, 0, p, p, 1, 1.0, 1, p, big, None) == EINVALID
    assert b"activation" in L.m355_last_error()
