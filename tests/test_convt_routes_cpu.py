"""The conv-transpose routes (route_convt / route_convt_c8, csrc/convt.hip) answer consistently: the workspace queries, the
supported query and m355_conv_transpose3d_plan are numbers of the same route.  Pure host code, no GPU (num_cus() is then
256); tools/conv_routes.py --convt is the exhaustive table."""
import ctypes as C

import pytest

from segmentation_pipeline_amd import _lib

DIRECT, MFMA, X3, C8, H16, UNSUPPORTED = range(6)
EUNSUPPORTED = -2
GEOMS = [(2, 2, 0, 0), (2, 2, 0, 1), (2, 1, 0, 0), (4, 2, 1, 0), (3, 2, 1, 1)]   # k, stride, pad, out_pad
# N, Cin, Cout, D, H, W: network levels, ragged channels, Cin > 512, each side of the c8 gradients' channel limit, of the h16
# forward's 16384 voxels / 128 channels, of the c8 32-bit offsets (2^22 voxels) and of convt_fits_i32
SHAPES = [(1, 64, 64, 4, 4, 8), (2, 5, 7, 3, 5, 6), (1, 320, 48, 2, 2, 2), (1, 520, 8, 2, 2, 2), (2, 32, 16, 64, 64, 64),
          (1, 32, 128, 16, 16, 16), (1, 32, 129, 16, 16, 16), (1, 32, 136, 16, 16, 16), (1, 32, 137, 16, 16, 16),
          (1, 128, 32, 16, 32, 31), (1, 128, 32, 16, 32, 32), (1, 129, 32, 16, 32, 32), (1, 8, 8, 128, 128, 255),
          (1, 8, 8, 128, 128, 256), (1, 8, 8, 256, 256, 511), (1, 8, 8, 256, 256, 512)]
CASES = [s + GEOMS[0] for s in SHAPES] + [s + g for s in SHAPES[:4] for g in GEOMS[1:]]


def desc(case, compute=0):
    d = _lib.ConvDesc()
    d.N, d.Cin, d.Cout, d.D, d.H, d.W, d.k, d.stride, d.pad, d.out_pad = case
    d.compute = compute
    return d


def plan(d, which, y_side=None):
    out = (C.c_int32 * 4)()
    assert _lib.lib().m355_conv_transpose3d_plan(C.byref(d), which, y_side, out) == 0
    return tuple(out)


def round_up(a, b):
    return -(-a // b) * b


@pytest.mark.parametrize("case", CASES)
def test_workspace_is_the_larger_of_the_two_gradient_routes(case):
    """m355_conv_transpose3d_workspace == max(weight gradient's slabs + bias scratch, data gradient's slabs), each sized
    from the split counts the plan reports (a descriptor on the direct kernels: the bias gradient's partials alone)."""
    N, Cin, Cout, D, H, W, k, s, p, op = case
    d = desc(case)
    (fd, _, _, ksplit), (fw, _, nsplit, _) = plan(d, 1), plan(d, 2)
    assert fd == fw and fd in (DIRECT, MFMA)
    od = lambda n: (n - 1) * s - 2 * p + k + op
    dbias = Cout * -(-(od(D) * od(H) * od(W)) // 8192) * 8
    got = _lib.lib().m355_conv_transpose3d_workspace(C.byref(d))
    if fd == MFMA:
        slab_w = round_up(nsplit * Cin * Cout * 8 * 4, 256)
        slab_d = round_up(ksplit * N * Cin * D * H * W * 4, 256) if ksplit > 1 else 0
        assert got == max(slab_w + round_up(max(dbias, nsplit * Cout * 8), 256), slab_d)
    elif (k, s, p, op) != (2, 2, 0, 0):
        assert got == round_up(dbias, 256)
    else:   # k2 s2 past 2^31 elements per sample: direct kernels, the query still reserves the slabs
        assert got >= round_up(dbias, 256)


@pytest.mark.parametrize("case", CASES)
def test_plan_sides(case):
    """A y side at a 4-byte offset, or an odd y batch stride, puts all three fp32 entry points on the direct kernels; the
    aligned plans agree on MFMA-or-not between the two gradients, and the forward adds only its LDS limit (Cin <= 512);
    F32X3 moves the forward alone."""
    d = desc(case)
    aligned = [plan(d, w)[0] for w in range(3)]
    assert aligned[1] == aligned[2] and aligned[0] in ((aligned[1],) if case[1] <= 512 else (DIRECT,))
    assert all(plan(d, w, 4) == (DIRECT, 0, 0, 0) for w in range(3))
    d.y_batch_stride = case[2] * 8 * case[3] * case[4] * case[5] + 1
    assert all(plan(d, w)[0] == DIRECT for w in range(3))
    d3 = desc(case, 3)
    assert [plan(d3, w)[0] for w in range(3)] == [X3 if aligned[0] == MFMA else DIRECT] + aligned[1:]


@pytest.mark.parametrize("case", CASES)
def test_c8_supported_query_and_unsupported_status(case):
    """m355_conv_transpose3d_h16_bwd_supported agrees with the plans of the c8 gradients (which = 4, 5), its workspace is 0
    exactly when they have no kernel, and an unsupported descriptor gets M355_EUNSUPPORTED from the entry point on the
    argument checks alone (they come before any launch; the pointers are never dereferenced)."""
    L = _lib.lib()
    d = desc(case)
    fams = [plan(d, w)[0] for w in (3, 4, 5)]
    assert fams[0] in (C8, H16, UNSUPPORTED) and fams[1] in (H16, UNSUPPORTED) and fams[2] in (C8, UNSUPPORTED)
    supported = L.m355_conv_transpose3d_h16_bwd_supported(C.byref(d))
    assert supported == (fams[1] == H16) == (fams[2] == C8)
    assert (L.m355_conv_transpose3d_h16_bwd_workspace(C.byref(d)) > 0) == bool(supported)
    ptr = C.c_void_p(4096)
    if fams[0] == UNSUPPORTED:
        assert L.m355_conv_transpose3d_fwd_h16(C.byref(d), ptr, 0, ptr, None, ptr, 0, 1, None) == EUNSUPPORTED
        assert b"conv_transpose3d_fwd_h16" in L.m355_last_error()
    if not supported:
        assert L.m355_conv_transpose3d_bwd_data_h16(C.byref(d), ptr, 0, ptr, ptr, 0, 1, None) == EUNSUPPORTED
        assert L.m355_conv_transpose3d_bwd_weight_h16(C.byref(d), ptr, 0, ptr, 0, ptr, None, 1.0, 1, ptr, 1 << 40,
                                                      None) == EUNSUPPORTED


def test_c8_plans_follow_the_knobs(tuning):
    """M355_CONVT_H16=0 sends the large forward levels to the c8 kernel; M355_CONVT_WGS scales the persistent grids"""
    d = desc((2, 32, 16, 64, 64, 64) + GEOMS[0])
    assert plan(d, 3)[0] == H16
    base = plan(d, 4), plan(d, 5)
    tuning(M355_CONVT_H16=0)
    assert plan(d, 3)[0] == C8 and (plan(d, 4), plan(d, 5)) == base
    tuning(M355_CONVT_WGS=1)
    assert plan(d, 4)[2] * 2 == base[0][2] and plan(d, 5) == base[1]
    tuning(M355_CONVT_WGS=2)
    assert plan(d, 4) == base[0] and plan(d, 5)[2] == 2 * base[1][2]
