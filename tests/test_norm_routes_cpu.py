"""The normalisation plans (plan_norm / norm_pass, csrc/norm_host.hpp) answer consistently: m355_norm_workspace,
m355_norm_num_stats, m355_act16_partials_slots and m355_norm_plan are numbers of the same plan, and every entry point that
takes a workspace checks that very number.  Pure host code, no GPU: the entry points are called with dummy non-null pointers
and stop at their argument checks, nothing is launched.  tools/conv_routes.py --norm is the larger table."""
import ctypes as C

import pytest

from segmentation_pipeline_amd import _lib

EINVALID, EUNSUPPORTED, EWORKSPACE = -1, -2, -4
STATS, FWD, FWD_H16, FWD_C8, POOL_FWD, BWD1, BWD2, BWD2_H16, BWD1_C8, BWD2_C8 = range(10)
CHUNK, CHUNK_C8 = 16384, 4096
# (N, C, groups, (D, H, W), batch stride class k: 0 dense, else x / y / add = dense + k, 2k, 3k): BN, GN with 4 and 5 channels
# per group, InstanceNorm; S % 4 both ways; S, N * S and (C / groups) * S on each side of the two chunk sizes; a network level
CASES = [(2, 8, 0, (4, 50, 41), 0), (2, 8, 0, (4, 50, 42), 1), (1, 8, 0, (4, 26, 40), 0), (2, 8, 0, (8, 8, 8), 4),
         (1, 8, 8, (4, 32, 32), 0), (2, 8, 8, (1, 1, 4097), 4), (2, 32, 8, (4, 32, 32), 0), (1, 32, 8, (1, 17, 241), 0),
         (2, 20, 4, (2, 2, 819), 0), (1, 20, 4, (1, 29, 113), 1), (2, 20, 0, (2, 64, 64), 0), (1, 32, 8, (16, 32, 32), 4),
         (1, 16, 8, (128, 128, 128), 0), (2, 5, 0, (1, 1, 1), 0)]


def desc(case):
    N, Cc, groups, (D, H, W), k = case
    S = D * H * W
    bs = [(Cc * S + k * j) if k else 0 for j in (1, 2, 3)]
    return _lib.NormDesc(N, Cc, S, groups, 1, 1e-5, 0.0, *bs)


def plan(d, which):
    out = (C.c_int32 * 4)()
    assert _lib.lib().m355_norm_plan(C.byref(d), which, out) == 0, _lib.lib().m355_last_error()
    return tuple(out)


def round_up(a, b):
    return -(-a // b) * b


def grid_x(work, per_thread, cap):
    return max(1, min(-(-work // (256 * per_thread)), cap))


@pytest.mark.parametrize("case", CASES)
def test_workspace_is_the_largest_layout_end(case):
    """m355_norm_workspace == the largest (stat_m offset + stat_m bytes) over the backward layouts the plan reports, plus
    the slack the query has always had behind it (room for N * C pairs of doubles, rounded to 256, and 512 bytes); the
    statistics partials (16 bytes per chunk and statistic) fit in front of that end too."""
    N, Cc = case[0], case[1]
    d = desc(case)
    L = _lib.lib()
    nstats = L.m355_norm_num_stats(C.byref(d))
    ends = [plan(d, w)[3] + 8 * nstats for w in (BWD1, BWD2, BWD2_H16, BWD1_C8, BWD2_C8)]
    assert nstats * plan(d, STATS)[1] * 16 <= max(ends)
    assert L.m355_norm_workspace(C.byref(d)) == max(ends) + round_up(N * Cc * 16, 256) + 512
    assert all(plan(d, w)[3] == 0 for w in (STATS, FWD, FWD_H16, FWD_C8, POOL_FWD))


@pytest.mark.parametrize("case", CASES)
def test_plans_agree_with_the_descriptor_and_the_queries(case):
    """chunk counts, stat_m offsets, grids and vector verdicts of every pass, recomputed here from the descriptor"""
    N, Cc, groups, (D, H, W), k = case
    S = D * H * W
    d = desc(case)
    L = _lib.lib()
    nstats = Cc if groups == 0 else N * groups
    length, count = (S, N * S) if groups == 0 else (Cc // groups * S,) * 2
    assert L.m355_norm_num_stats(C.byref(d)) == nstats
    strides4 = k % 4 == 0
    nblk = -(-count // CHUNK)
    assert plan(d, STATS) == (int(length % 4 == 0 and S % 4 == 0 and strides4), nblk, nblk, 0)
    vec = int(S % 4 == 0 and strides4)
    assert plan(d, FWD) == (vec, 0, grid_x(S // 4 if vec else S, 4, 1024), 0)
    big = int(S >= 4096)
    assert plan(d, FWD_H16) == (big, 0, grid_x(S, 4 if big else 1, 2048), 0)
    assert plan(d, FWD_C8) == (0, 0, grid_x(S, 4, 2048), 0)
    assert plan(d, POOL_FWD) == (0, 0, grid_x(S // 8, 2, 1024), 0)
    nb32, nb16 = -(-S // CHUNK), -(-S // CHUNK_C8)
    off32, off16 = round_up(N * Cc * nb32 * 16, 256), round_up(N * Cc * nb16 * 16, 256)
    assert plan(d, BWD1) == (vec, nb32, nb32, off32)
    assert plan(d, BWD2) == (vec, 0, grid_x(S // 4 if vec else S, 4, 1024), off32)
    assert plan(d, BWD2_H16) == (0, 0, grid_x(S, 2, 1024), off32)
    assert plan(d, BWD1_C8) == (0, nb16, nb16, off16)
    assert plan(d, BWD2_C8) == (0, 0, grid_x(S, 2, 1024), off16)
    # the c8 statistics partials and the c8 backward cut a channel into the same 4096-voxel pieces
    assert L.m355_act16_partials_slots(S) == min(plan(d, BWD1_C8)[1], 1024)


@pytest.mark.parametrize("case", CASES)
def test_one_byte_short_workspace_is_refused(case):
    """every entry point that takes a workspace checks it against m355_norm_workspace: one byte less -> M355_EWORKSPACE,
    on the argument checks alone (they come before any launch; the pointers are never dereferenced)"""
    N, Cc, groups, (D, H, W), k = case
    d = desc(case)
    L = _lib.lib()
    ref, p = C.byref(d), C.c_void_p(4096)
    short = L.m355_norm_workspace(ref) - 1
    even = D % 2 == 0 and H % 2 == 0 and W % 2 == 0
    calls = {
        "norm_stats": (ref, p, p, p, None, None, 0.1, p, short, None),
        "norm_stats_from_partials": (ref, p, 3, p, p, None, None, 0.1, p, short, None),
        "norm_act_bwd": (ref, p, p, p, p, p, p, p, p, p, 1, p, short, None),
        "norm_act_bwd_h16": (ref, p, p, p, p, p, p, p, p, p, 1, p, 0, 1, p, short, None),
        "norm_act_bwd_reduce": (ref, p, p, p, p, p, p, p, p, 1, None, p, p, short, None),
        "norm_act_bwd_c8": (ref, p, 0, p, 0, p if even else None, 0, D, H, W, p, p, p, p, p, 0, p, p, 1, 1.0, 2, p, short, None),
        "norm_act_bwd_c8_reduce": (ref, p, 0, p, 0, p if even else None, 0, D, H, W, p, p, p, p, p, p, 1, None, 1.0, p, 1, p,
                                   short, None),
    }
    if groups == 0:   # (batch norm only: a GroupNorm descriptor is refused before the workspace is looked at)
        calls["norm_sums"] = (ref, p, None, 0, p, p, short, None)
        calls["norm_sums (partials)"] = (ref, None, p, 3, p, p, short, None)
    for name, args in calls.items():
        rc = getattr(L, "m355_" + name.split()[0])(*args)
        assert rc == EWORKSPACE and b"workspace" in L.m355_last_error(), (name, rc, L.m355_last_error())


def test_bad_descriptors_keep_their_status_codes():
    """C % groups != 0 -> M355_EINVALID_ARG from the plan query and from entry points of each file; a null descriptor and an
    unknown pass likewise; N > 65535 is M355_EUNSUPPORTED on the fp32 passes, and comes after a bad activation code"""
    L = _lib.lib()
    p, out = C.c_void_p(4096), (C.c_int32 * 4)()
    bad = _lib.NormDesc(1, 30, 64, 8, 0, 1e-5, 0.0, 0, 0, 0)
    ref = C.byref(bad)
    assert all(L.m355_norm_plan(ref, w, out) == EINVALID for w in range(10))
    assert b"divisible" in L.m355_last_error()
    assert L.m355_norm_stats(ref, p, p, p, None, None, 0.1, p, 1 << 40, None) == EINVALID
    assert L.m355_norm_act_fwd_h16(ref, p, p, p, p, p, None, None, p, 0, 1, None) == EINVALID
    assert L.m355_norm_act_fwd_c8(ref, p, 0, p, p, p, p, None, 0, p, 0, 1, None) == EINVALID
    assert L.m355_norm_act_bwd_c8_apply(ref, p, 0, p, 0, None, 0, 1, 8, 8, p, p, p, p, p, p, 0, 1, None) == EINVALID
    assert b"divisible" in L.m355_last_error()
    assert L.m355_norm_plan(None, 0, out) == EINVALID
    ok = _lib.NormDesc(1, 32, 64, 8, 0, 1e-5, 0.0, 0, 0, 0)
    assert L.m355_norm_plan(C.byref(ok), 10, out) == EINVALID and L.m355_norm_plan(C.byref(ok), -1, out) == EINVALID
    assert L.m355_norm_plan(C.byref(ok), 0, None) == EINVALID
    wide = _lib.NormDesc(65536, 32, 64, 8, 0, 1e-5, 0.0, 0, 0, 0)
    assert L.m355_norm_plan(C.byref(wide), FWD, out) == EUNSUPPORTED and L.m355_norm_plan(C.byref(wide), FWD_C8, out) == EINVALID
    assert L.m355_norm_act_fwd(C.byref(wide), p, p, p, p, p, None, p, None) == EUNSUPPORTED
    wide.act = 7
    assert L.m355_norm_act_fwd(C.byref(wide), p, p, p, p, p, None, p, None) == EINVALID
