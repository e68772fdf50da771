"""The split (M355_COMPUTE_F32X3) conv-transpose gradients have entry points and queries of their own
(route_convt_x3_bwd, csrc/convt.hip): what they answer on the host, with no GPU (num_cus() is then 256), and that the
fp32 entry points' plan and workspace query answer what they did before.  The weight gradient has a split kernel
(convt_k2s2_bwd_weight_x3_kernel<2 | 4>); the data gradient has none and keeps the fp32-MFMA kernel at every level."""
import ctypes as C
import os
import re

import pytest

from segmentation_pipeline_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT, MFMA, X3, C8, H16, NONE = range(6)
EUNSUPPORTED = -2
K2S2 = (2, 2, 0, 0)
# name, (N, Cin, Cout, D, H, W): the conv-transpose levels of the cfg2 network (tools/convt_bench.py)
LEVELS = [("u0", (1, 64, 64, 64, 64, 64)), ("u1", (1, 128, 128, 32, 32, 32)), ("u2", (1, 256, 256, 16, 16, 16)),
          ("u3", (1, 320, 320, 8, 8, 8))]


def desc(shape, geom=K2S2, compute=3, xbs=0, ybs=0):
    return _lib.ConvDesc(*shape, *geom, xbs, ybs, compute, 0)


def x3_plan(d, which, y_side=None):
    out = (C.c_int32 * 4)()
    assert _lib.lib().m355_conv_transpose3d_x3_bwd_plan(C.byref(d), which, y_side, out) == 0
    return tuple(out)


def round_up(a, b):
    return -(-a // b) * b


@pytest.mark.parametrize("name,shape", LEVELS, ids=[n for n, _ in LEVELS])
def test_cfg2_levels_weight_gradient_on_the_split_route_data_gradient_not(name, shape):
    """all four levels measured faster on the split weight gradient (profiles/convt_grad_x3_ab.txt), so all four are
    supported; the plan names an instantiation that exists; the workspace is the slabs plus the bias partials computed
    from the plan's own split count"""
    L = _lib.lib()
    N, Cin, Cout, D, H, W = shape
    d = desc(shape)
    assert L.m355_conv_transpose3d_x3_bwd_supported(C.byref(d), None) == 2      # bit 1: weight gradient; bit 0: never
    assert x3_plan(d, 1) == (NONE, 0, 0, 0)
    fam, mt, nsplit, zero = x3_plan(d, 2)
    assert fam == X3 and zero == 0 and mt == (4 if Cin > 64 else 2)
    src = open(os.path.join(ROOT, "segmentation-pipeline_amd", "csrc", "conv3d_f32x3.hip")).read()
    assert str(mt) in re.findall(r"hipLaunchKernelGGL\(convt_k2s2_bwd_weight_x3_kernel<(\d+)>", src)
    # one residency: 3 (MT = 2) / 2 (MT = 4) workgroups per CU over the (16-channel o, 32 * MT-channel c) blocks
    blocks = -(-Cout // 16) * -(-Cin // (32 * mt))
    assert nsplit == min(max(1, (3 if mt == 2 else 2) * 256 // blocks), -(-(N * D * H * W) // 32))
    slabs, bias = round_up(nsplit * Cin * Cout * 8 * 4, 256), round_up(nsplit * Cout * 8, 256)
    assert L.m355_conv_transpose3d_x3_bwd_workspace(C.byref(d)) == slabs + bias


def test_small_level_floor_and_its_knob(tuning):
    """below 512 voxels in the batch (no level was measured there) the fp32-MFMA kernel keeps the shape;
    M355_F32X3_CONVT_BWD=2 lifts the floor and nothing else"""
    L = _lib.lib()
    small, at = desc((1, 64, 64, 4, 8, 8)), desc((1, 64, 64, 4, 8, 16))
    assert L.m355_conv_transpose3d_x3_bwd_supported(C.byref(small), None) == 0 and x3_plan(small, 2) == (NONE, 0, 0, 0)
    assert L.m355_conv_transpose3d_x3_bwd_supported(C.byref(at), None) == 2
    tuning(M355_F32X3_CONVT_BWD=2)
    assert L.m355_conv_transpose3d_x3_bwd_supported(C.byref(small), None) == 2 and x3_plan(small, 2) == (X3, 2, 8, 0)
    assert L.m355_conv_transpose3d_x3_bwd_supported(C.byref(desc((1, 64, 64, 4, 8, 9))), None) == 0    # odd W stays refused


def refused(d, y_side=None):
    """query, plan, workspace and both entry points agree that this descriptor / dy pointer has no split kernel; the entry
    points say so on the argument checks alone (pointers never dereferenced: they are not device memory)"""
    L = _lib.lib()
    ptr = C.c_void_p(4096)
    dy = C.c_void_p(y_side) if y_side is not None else ptr
    assert L.m355_conv_transpose3d_x3_bwd_supported(C.byref(d), dy) == 0
    assert x3_plan(d, 1, dy) == x3_plan(d, 2, dy) == (NONE, 0, 0, 0)
    assert L.m355_conv_transpose3d_bwd_data_x3(C.byref(d), dy, ptr, ptr, ptr, 1 << 40, None) == EUNSUPPORTED
    assert b"conv_transpose3d_bwd_data_x3" in L.m355_last_error()
    assert L.m355_conv_transpose3d_bwd_weight_x3(C.byref(d), ptr, dy, ptr, ptr, ptr, 1 << 40, None) == EUNSUPPORTED
    assert b"conv_transpose3d_bwd_weight_x3" in L.m355_last_error()


@pytest.mark.parametrize("geom", [(2, 2, 0, 1), (2, 1, 0, 0), (4, 2, 1, 0), (3, 2, 1, 1)])
def test_other_geometries_are_refused(geom):
    d = desc((1, 64, 64, 8, 8, 16), geom)
    refused(d)
    assert _lib.lib().m355_conv_transpose3d_x3_bwd_workspace(C.byref(d)) == 0


def test_dy_at_a_4_byte_offset_or_an_8_byte_one_is_refused():
    d = desc((1, 64, 64, 8, 8, 16))
    assert _lib.lib().m355_conv_transpose3d_x3_bwd_supported(C.byref(d), C.c_void_p(4096)) == 2
    refused(d, 4096 + 4)
    refused(d, 4096 + 8)      # the kernel loads dy as float4


def test_odd_batch_strides_are_refused():
    shape = (2, 64, 64, 8, 8, 16)
    dense_y, dense_x = 64 * 8 * 8 * 8 * 16, 64 * 8 * 8 * 16
    refused(desc(shape, ybs=dense_y + 1))
    refused(desc(shape, ybs=dense_y + 2))     # float4 rows: a multiple of 4
    refused(desc(shape, xbs=dense_x + 1))
    assert _lib.lib().m355_conv_transpose3d_x3_bwd_supported(C.byref(desc(shape, xbs=dense_x + 2, ybs=dense_y + 4)), None) == 2


def test_x_off_an_8_byte_boundary_is_refused_by_the_entry_point():
    """the query sees the dy pointer only; the x pointer is the entry point's own check, before any launch"""
    L = _lib.lib()
    d = desc((1, 64, 64, 8, 8, 16))
    ptr = C.c_void_p(4096)
    assert L.m355_conv_transpose3d_bwd_weight_x3(C.byref(d), C.c_void_p(4100), ptr, ptr, ptr, ptr, 1 << 40, None) == EUNSUPPORTED


def test_knob_off_and_other_compute_modes_are_refused(tuning):
    shape = (1, 64, 64, 8, 8, 16)
    for compute in (0, 1, 2):
        refused(desc(shape, compute=compute))
    tuning(M355_F32X3_CONVT_BWD=0)
    refused(desc(shape))
    assert _lib.lib().m355_conv_transpose3d_x3_bwd_workspace(C.byref(desc(shape))) == 0
    tuning(M355_F32X3_CONVT_BWD=1, M355_F32X3=0)
    refused(desc(shape))


def test_too_small_a_workspace_is_an_error_before_any_launch():
    L = _lib.lib()
    d = desc((1, 64, 64, 8, 8, 16))
    ptr = C.c_void_p(4096)
    need = L.m355_conv_transpose3d_x3_bwd_workspace(C.byref(d))
    nsplit = x3_plan(d, 2)[2]
    slabs = round_up(nsplit * 64 * 64 * 8 * 4, 256)
    EWORKSPACE = L.m355_conv_transpose3d_bwd_weight_x3(C.byref(d), ptr, ptr, ptr, ptr, ptr, need - 1, None)
    assert EWORKSPACE not in (0, EUNSUPPORTED) and b"workspace too small" in L.m355_last_error()
    assert L.m355_conv_transpose3d_bwd_weight_x3(C.byref(d), ptr, ptr, ptr, None, ptr, slabs - 1, None) == EWORKSPACE


@pytest.mark.parametrize("name,shape", LEVELS, ids=[n for n, _ in LEVELS])
def test_fp32_entry_points_plan_and_workspace_answer_as_before(name, shape, tuning):
    """m355_conv_transpose3d_plan and m355_conv_transpose3d_workspace: compute 3 moves the forward alone, whatever the
    new knob says, and the workspace is that of the two fp32-MFMA gradient routes"""
    L = _lib.lib()
    N, Cin, Cout, D, H, W = shape

    def answers():
        out = []
        for compute in (0, 3):
            d = desc(shape, compute=compute)
            plans = []
            for which in range(3):
                p = (C.c_int32 * 4)()
                assert L.m355_conv_transpose3d_plan(C.byref(d), which, None, p) == 0
                plans.append(tuple(p))
            out.append((plans, L.m355_conv_transpose3d_workspace(C.byref(d))))
        return out

    (p0, ws0), (p3, ws3) = base = answers()
    assert p0[0][0] == MFMA and p3[0][0] == X3 and p0[1:] == p3[1:] and p0[1][0] == p0[2][0] == MFMA and ws0 == ws3
    mt = 4 if Cin > 64 else 2
    nsplit = min(max(1, 2 * 256 // (-(-Cout // 16) * -(-Cin // (32 * mt)))), -(-(N * D * H * W) // 64))
    assert p0[2] == (MFMA, mt, nsplit, 0)
    slab_d = round_up(p0[1][3] * N * Cin * D * H * W * 4, 256) if p0[1][3] > 1 else 0
    dbias = Cout * -(-(8 * D * H * W) // 8192) * 8
    assert ws0 == max(round_up(nsplit * Cin * Cout * 8 * 4, 256) + round_up(max(dbias, nsplit * Cout * 8), 256), slab_d)
    for knob in (0, 2):
        tuning(M355_F32X3_CONVT_BWD=knob)
        assert answers() == base
