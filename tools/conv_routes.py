#!/usr/bin/env python3
"""Every host answer of the conv3d route resolver (csrc/conv3d_route.hpp) for a fixed descriptor list under a fixed list of
tuning sets: one line per (tuning set, descriptor) with m355_conv3d_plan for which = 0, 1, 2, the workspace queries, the
packed-weight sizes, the statistics slots and the softmax answer; then the line count and a SHA-256 of the lines.

Pure host code: runs without a GPU (num_cus() is then 256, the MI355X's count).  A change that must not move any descriptor
to another route, workspace size or plan code gives the same hash before and after; M355_LIB_PATH points the run at
another build of the library.

--convt: the same for the conv-transpose routes (csrc/convt.hip): per line the three queries (workspace, h16_bwd_supported,
h16_bwd_workspace), m355_conv_transpose3d_plan for which = 0..5 with an aligned y side, and for which = 0..2 with a y side
at a 4-byte offset.  Two hashes: "queries" covers the three queries alone, so it can be compared with a library that
predates the plan query (it then is the only one printed), "routes" covers the whole lines.

--norm: the same for the normalisation plans (csrc/norm_host.hpp): per line m355_norm_num_stats, m355_norm_workspace,
m355_act16_partials_slots(S) -- the "queries" hash -- and m355_norm_plan for which = 0..9 -- with them the "routes" hash.

--resample: the same for the factor-2 resampling family (csrc/resample_host.hpp).  "queries": the return codes of the 17
entry points over argument tuples that are each REJECTED -- one fault or two out of null pointer, dimension <= 0, odd size,
bad compute mode, misaligned pointers, misaligned strides; a tuple that its entry point would accept is never built, because
the call would launch on the dummy pointers -- so this hash too compares with a library from before the plan query.
"routes": m355_resample_plan for valid shapes, strides and pointer alignments, both sides of every grid cap and of the
trilinear forward's kernel conditions.

--launch: the conv table once more ("queries": the default mode's lines and hash) and, "routes", m355_conv3d_launch_plan (csrc/
conv3d_route.hpp) for the ten launching entry points: over a thinned descriptor list with every guard volume, and over the
shapes of tests/test_conv_launch_plans_gpu.py with the facts a call adds to its descriptor varied one at a time -- each
pointer at +4 and +8 bytes, odd and padded batch strides, add / statistics / dbias present, the softmax and packed-weights
flags, each side of the 65535-sample limit of the pack behind the plain weight gradient -- under every tuning set.

usage: python tools/conv_routes.py [--convt | --norm | --resample | --launch] [--hash-only] [--jobs N] > routes.txt"""
import argparse
import ctypes as C
import hashlib
import itertools
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHANNELS = [1, 3, 4, 5, 8, 13, 16, 24, 32, 33, 40, 48, 64, 80, 96, 120, 128, 192, 256, 320, 384]
VOLUMES = [(8, 8, 8), (1, 5, 7), (8, 2, 32), (12, 9, 8), (6, 21, 16), (9, 10, 36), (17, 4, 62), (16, 16, 16), (32, 32, 32),
           (64, 64, 64), (96, 96, 96), (128, 128, 128), (32, 256, 256), (160, 160, 160)]
# each side of the 2^24, 2^26 and 2^27 voxel guards (channel counts <= 8 only)
GUARD_VOLUMES = [(256, 256, 255), (256, 256, 256), (256, 256, 1023), (256, 256, 1024), (512, 512, 511), (512, 512, 512)]
NON_K3 = [(1, 1, 0), (3, 2, 1), (2, 2, 0)]   # (k, stride, pad) of the direct kernels, on VOLUMES[:3]


def descriptors():
    """(N, Cin, Cout, D, H, W, k, stride, pad, compute)"""
    for vol, ci, co, n, comp in itertools.product(VOLUMES, CHANNELS, CHANNELS, (1, 2), range(4)):
        yield (n, ci, co) + vol + (3, 1, 1, comp)
    small = [c for c in CHANNELS if c <= 8]
    for vol, ci, co, n, comp in itertools.product(GUARD_VOLUMES, small, small, (1, 2), range(4)):
        yield (n, ci, co) + vol + (3, 1, 1, comp)
    for ksp, vol, ci, co, n, comp in itertools.product(NON_K3, VOLUMES[:3], CHANNELS, CHANNELS, (1, 2), range(4)):
        yield (n, ci, co) + vol + ksp + (comp,)


# ---- --convt ----
CONVT_GEOMS = [(2, 2, 0, 0), (2, 2, 0, 1), (2, 1, 0, 0), (4, 2, 1, 0), (3, 2, 1, 1)]   # (k, stride, pad, out_pad)
# (Cin, Cout, volume): each side of convt_fits_i32, of the c8 gradients' 32-bit offsets and channel limit, and of the
# h16 forward's 16384 voxels and 128 input channels
CONVT_GUARDS = [(8, 8, (256, 256, 511)), (8, 8, (256, 256, 512)), (8, 8, (128, 128, 255)), (8, 8, (128, 128, 256)),
                (256, 8, (128, 128, 255)), (256, 8, (128, 128, 256)),
                *[(32, co, (16, 16, 16)) for co in (128, 129, 136, 137)],
                *[(ci, 32, vol) for ci in (128, 129) for vol in ((16, 32, 31), (16, 32, 32), (16, 32, 33))]]


def convt_descriptors():
    """(N, Cin, Cout, D, H, W, k, stride, pad, out_pad, compute)"""
    for geom, vol, ci, co, n, comp in itertools.product(CONVT_GEOMS, VOLUMES, CHANNELS, CHANNELS, (1, 2), range(4)):
        yield (n, ci, co) + vol + geom + (comp,)
    for geom, (ci, co, vol), n, comp in itertools.product(CONVT_GEOMS[:2], CONVT_GUARDS, (1, 2), range(4)):
        yield (n, ci, co) + vol + geom + (comp,)


CONVT_TUNING_SETS = [{}, {"M355_CONVT_H16": "0"}, {"M355_CONVT_WGS": "1"}, {"M355_CONVT_WGS": "2"}, {"M355_F32X3": "0"},
                     {"M355_F32X3_CONVT": "0"}]


def run_convt_set(idx):
    """(index, line count, query-only text, whole text) of one conv-transpose tuning set."""
    env = CONVT_TUNING_SETS[idx]
    for k in [k for k in os.environ if k.startswith("M355_") and k != "M355_LIB_PATH"]:
        del os.environ[k]
    os.environ.update(env)
    from segmentation_pipeline_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # (not _lib.lib(): that insists on every symbol of this tree's header)
    for name in ("m355_conv_transpose3d_workspace", "m355_conv_transpose3d_h16_bwd_supported",
                 "m355_conv_transpose3d_h16_bwd_workspace", "m355_conv_transpose3d_plan"):
        if getattr(L, name, None) is not None:
            getattr(L, name).restype, getattr(L, name).argtypes = _lib.SIGNATURES[name]
    L.m355_reload_tuning()
    plan = getattr(L, "m355_conv_transpose3d_plan", None)   # None: a library from before the plan query
    tag = ",".join(f"{k[5:]}={v}" for k, v in sorted(env.items())) or "default"
    d = _lib.ConvDesc()
    ref = C.byref(d)
    out4 = (C.c_int32 * 4)()
    queries = [L.m355_conv_transpose3d_workspace, L.m355_conv_transpose3d_h16_bwd_supported,
               L.m355_conv_transpose3d_h16_bwd_workspace]
    qlines, lines = [], []
    for (d.N, d.Cin, d.Cout, d.D, d.H, d.W, d.k, d.stride, d.pad, d.out_pad, d.compute) in convt_descriptors():
        f = [tag, f"N{d.N} {d.Cin}->{d.Cout} {d.D}x{d.H}x{d.W} k{d.k}s{d.stride}p{d.pad}o{d.out_pad} c{d.compute}",
             "ws/h16_bwd/h16_bwd_ws=" + "/".join(str(q(ref)) for q in queries)]
        qlines.append(" ".join(f))
        if plan:
            for which, y_side in [(w, None) for w in range(6)] + [(w, 4) for w in range(3)]:
                rc = plan(ref, which, y_side, out4)
                f.append(f"plan{which}{'+4' if y_side else ''}={rc}:" + "/".join(str(v) for v in out4))
            lines.append(" ".join(f))
    return idx, len(qlines), "\n".join(qlines) + "\n", "\n".join(lines) + "\n" if plan else None


def convt_main(a):
    queries, routes, n, have_plan = hashlib.sha256(), hashlib.sha256(), 0, True
    with multiprocessing.get_context("spawn").Pool(a.jobs, maxtasksperchild=1) as pool:
        for idx, count, qtext, text in pool.imap(run_convt_set, range(len(CONVT_TUNING_SETS))):
            have_plan = have_plan and text is not None
            if a.hash_only:
                print(f"set {idx:2d} {count} queries {hashlib.sha256(qtext.encode()).hexdigest()}"
                      + (f" routes {hashlib.sha256(text.encode()).hexdigest()}" if text else ""), flush=True)
            else:
                sys.stdout.write(text or qtext)
            queries.update(qtext.encode())
            routes.update((text or "").encode())
            n += count
    print(f"lines {n} queries sha256 {queries.hexdigest()}" + (f" routes sha256 {routes.hexdigest()}" if have_plan else ""))


# ---- --norm ----
# (C, groups): BatchNorm (0), InstanceNorm (groups = C), GroupNorm with 4 and 5 channels per group
NORM_CHANNELS = [(8, 0), (20, 0), (32, 0), (8, 8), (8, 2), (32, 8), (20, 4), (40, 8)]
# S % 4 both ways; each side of the chunk sizes 4096 and 16384; N * S (BN, N = 2: 8191..8193) and (C / groups) * S (GN: 4 * 4096
# and 4097, 5 * 3276 and 3277) on each side of 16384; the 64^3, 128^3 and 32 x 256 x 256 levels
NORM_S = [1, 63, 64, 3276, 3277, 4095, 4096, 4097, 4100, 8191, 8192, 8193, 16383, 16384, 16385, 16388, 32768, 64 ** 3, 128 ** 3,
          32 * 256 * 256]
NORM_STRIDES = [0, 4, 1]   # batch strides: dense (0), dense + 4 k and dense + k elements for x, y, add (k = 1, 2, 3)
NORM_PASSES = 10


def norm_descriptors():
    """(N, C, groups, S, stride class)"""
    return itertools.product((1, 2), NORM_CHANNELS, NORM_S, NORM_STRIDES)


def norm_main(a):
    from segmentation_pipeline_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # (not _lib.lib(): that insists on every symbol, and a parent library has no m355_norm_plan)
    fns = {}
    for name in ("m355_norm_num_stats", "m355_norm_workspace", "m355_act16_partials_slots", "m355_norm_plan"):
        fns[name] = getattr(L, name, None)
        if fns[name] is not None:
            fns[name].restype, fns[name].argtypes = _lib.SIGNATURES[name]
    plan = fns["m355_norm_plan"]
    d = _lib.NormDesc()
    ref = C.byref(d)
    out4 = (C.c_int32 * 4)()
    qlines, lines = [], []
    for n, (c, g), s, k in norm_descriptors():
        d.N, d.C, d.groups, d.S, d.act, d.eps = n, c, g, s, 1, 1e-5
        d.x_batch_stride, d.y_batch_stride, d.add_batch_stride = [(c * s + k * j) if k else 0 for j in (1, 2, 3)]
        f = [f"N{n} C{c} g{g} S{s} bs+{k}", f"stats/ws/slots={fns['m355_norm_num_stats'](ref)}/"
             f"{fns['m355_norm_workspace'](ref)}/{fns['m355_act16_partials_slots'](s)}"]
        qlines.append(" ".join(f))
        if plan:
            for which in range(NORM_PASSES):
                rc = plan(ref, which, out4)
                f.append(f"plan{which}={rc}:" + "/".join(str(v) for v in out4))
            lines.append(" ".join(f))
    qtext, text = "\n".join(qlines) + "\n", "\n".join(lines) + "\n"
    if not a.hash_only:
        sys.stdout.write(text if plan else qtext)
    print(f"lines {len(qlines)} queries sha256 {hashlib.sha256(qtext.encode()).hexdigest()}"
          + (f" routes sha256 {hashlib.sha256(text.encode()).hexdigest()}" if plan else ""))


# ---- --resample ----
RS_BASE = dict(N=2, C=8, D=4, H=4, W=4, compute=1, bs=(0, 0, 0), ptr=(4096, 8192, 12288, 16384))
# (name, check it trips, the fields it sets): the alignment faults move EVERY pointer / stride, so that they fault whichever
# tensor an entry point looks at (the fp32 space / depth pair checks its full-resolution side only)
RS_FAULTS = [("null0", "n", dict(ptr=(0, 8192, 12288, 16384))), ("null-all", "n", dict(ptr=(0, 0, 0, 0))),
             *[(f"{k}=0", "d", {k: 0}) for k in "NCDHW"], ("C=-8", "d", dict(C=-8)),
             *[(f"{k}=5", "o", {k: 5}) for k in "DHW"],
             *[(f"compute={v}", "c", dict(compute=v)) for v in (0, 3, 7)],
             ("ptr+4", "a", dict(ptr=(4100, 8196, 12292, 16388))), ("bs=4099", "a", dict(bs=(4099, 4099, 4099)))]


def resample_faulty_calls():
    """(op, label, arguments) of calls that are rejected by construction: at least one fault of a kind the entry point checks"""
    from segmentation_pipeline_amd import _lib
    singles = [(f,) for f in RS_FAULTS]
    pairs = [(f, g) for f, g in itertools.combinations(RS_FAULTS, 2) if not set(f[2]) & set(g[2])]
    for op, (name, _, _, checks) in enumerate(_lib.RESAMPLE_OPS):
        for faults in singles + pairs:
            if not any(kind in checks for _, kind, _ in faults):
                continue   # e.g. an odd size alone on the trilinear ops: a valid call
            a = dict(RS_BASE)
            for _, _, fields in faults:
                a.update(fields)
            shape = tuple(a[k] for k in "NCDHW")
            yield op, "+".join(f[0] for f in faults), _lib.resample_args(op, shape, a["bs"], a["ptr"], a["compute"])


RS_VOLUMES = [(2, 2, 2), (2, 2, 6), (2, 4, 4), (4, 6, 8), (6, 2, 10), (8, 8, 8), (10, 36, 12), (16, 16, 18), (32, 32, 32),
              (36, 10, 130), (64, 64, 64), (128, 128, 128), (132, 132, 132), (2, 130, 132)]
# the trilinear ops take odd sizes; D = 1 / H = 1: no LDS tiling; W = 306 / 308: each side of the 48 KiB patch; the last
# four: each side of the quad kernel's 2^31 limit (N = 1, 2) and of the tiled kernel's N * C <= 65535
RS_TRI_VOLUMES = [(1, 2, 2), (2, 1, 4), (1, 1, 2), (2, 2, 3), (3, 5, 7), (2, 2, 306), (2, 2, 308), (2, 2, 310), (4, 4, 308),
                  (4095, 2048, 308), (4096, 2048, 308), (4095, 4096, 308), (4096, 4096, 308)]
RS_CHANNELS = [1, 3, 8, 9, 32]
RS_PADS = [0, 8, 1, 2]       # batch strides: dense (0), dense + pad * (slot + 1) elements
RS_OFFSETS = [0, 8, 4]       # bytes the pointers sit behind a 16-byte boundary (slot i: from slot i on, so each one moves alone too)


def resample_main(a):
    from segmentation_pipeline_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # (not _lib.lib(): a parent library has no m355_resample_plan)
    qlines = []
    for op, label, args in resample_faulty_calls():
        fn = getattr(L, "m355_" + _lib.RESAMPLE_OPS[op][0])
        fn.restype, fn.argtypes = _lib.SIGNATURES["m355_" + _lib.RESAMPLE_OPS[op][0]]
        rc = fn(*args)
        assert rc != 0, (op, label)
        qlines.append(f"{_lib.RESAMPLE_OPS[op][0]} {label} rc={rc}")
    qtext = "\n".join(qlines) + "\n"
    plan = getattr(L, "m355_resample_plan", None)
    lines = []
    if plan:
        plan.restype, plan.argtypes = _lib.SIGNATURES["m355_resample_plan"]
        out = (C.c_int64 * 8)()
        for op, (name, _, nstrides, checks) in enumerate(_lib.RESAMPLE_OPS):
            tri = "o" not in checks
            c8 = "c" in checks
            for (D, H, W), Cc, N, pad, off in itertools.product(RS_VOLUMES + (RS_TRI_VOLUMES if tri else []), RS_CHANNELS, (1, 2),
                                                                RS_PADS, RS_OFFSETS):
                if c8 and (pad % 8 or off):
                    continue   # rejected: covered by the queries
                # a padded stride: one the largest tensor of any op fits in (the upsampled one, channels rounded up to 8)
                big = 64 * (Cc + 7) * D * H * W
                bs = (C.c_int64 * 3)(*[(big + pad * (i + 1)) if pad and i < nstrides else 0 for i in range(3)])
                for first in range(3 if off else 1):
                    ptr = (C.c_uint64 * 4)(*[(1 << 20) * (i + 1) + (off if i >= first else 0) for i in range(4)])
                    rc = plan(op, N, Cc, D, H, W, bs, ptr, 1, out)
                    lines.append(f"{name} N{N} C{Cc} {D}x{H}x{W} bs+{pad} ptr+{off}@{first} plan={rc}:" + "/".join(str(v) for v in out))
    text = qtext + "\n".join(lines) + "\n"
    if not a.hash_only:
        sys.stdout.write(text if plan else qtext)
    print(f"lines {len(qlines)} queries sha256 {hashlib.sha256(qtext.encode()).hexdigest()}"
          + (f" routes ({len(lines)} more lines) sha256 {hashlib.sha256(text.encode()).hexdigest()}" if plan else ""))


def _e(**kw):
    return {k: str(v) for k, v in kw.items()}


# the default, every distinct dict that tests/*_gpu.py hands to the `tuning` fixture, and single knobs
TUNING_SETS = [
    {},
    # tests/test_fp16_overflow_gpu.py, tests/test_model_gpu.py
    _e(M355_CONV_SLOTS=5, M355_H16_ONESHOT=3), _e(M355_H16_ONESHOT=2, M355_CONV_KSPLIT=1),
    _e(M355_CONV_KSPLIT=2, M355_CONV_SLOTS=5, M355_H16_ONESHOT=3), _e(M355_CONV_NTW=1),
    _e(M355_CONV_PERSISTENT=2, M355_CONV_SLOTS=6, M355_H16_ONESHOT=3),
    # tests/test_strided_slots_gpu.py
    _e(M355_CONV_SLOTS=5), _e(M355_CONV_KSPLIT=2, M355_CONV_NTW=2), _e(M355_TILE16=1), _e(M355_F32X3_EDGE=1),
    _e(M355_F32X3_EDGE=1, M355_TILE16=1), _e(M355_CONV_KSPLIT=1), _e(M355_CONV_KSPLIT=1, M355_CONV_SLOTS=5),
    _e(M355_BWW_NSPLIT=3), _e(M355_BWW_NSPLIT=3, M355_TILE16=0), _e(M355_BWW_NSPLIT=1),
    # tests/test_kernels_gpu.py
    _e(M355_TILE16=0), _e(M355_CONV_SLOTS=7), _e(M355_CONV_SLOTS=5, M355_CONV_KSPLIT=2), _e(M355_CONV_SLOTS=3, M355_CONV_NTW=8),
    *[_e(M355_TILE16=t, **env) for t in (1, 0) for env in (
        _e(M355_CONV_SLOTS=5), _e(M355_CONV_NTW=1), _e(M355_CONV_NTW=2, M355_CONV_KSPLIT=3),
        _e(M355_CONV_NTW=4, M355_CONV_KSPLIT=1), _e(M355_BWW_NSPLIT=3), _e(M355_BWW_NSPLIT=1))],
    _e(M355_CONV_KSPLIT=2), _e(M355_CONV_KSPLIT=0),
    *[_e(M355_H16_W8=w8, M355_H16_ONESHOT=one, M355_CONV_KSPLIT=1) for w8, one in ((0, 3), (2, 3), (0, 1))],
    _e(M355_NO_SMALL=0, M355_CONV_KSPLIT=1, M355_CONV_NTW=4), _e(M355_NO_SMALL=1, M355_CONV_KSPLIT=1, M355_CONV_NTW=4),
    _e(M355_NO_SMALL=0),
    _e(M355_CONV_KSPLIT=1, M355_CONV_SLOTS=5, M355_H16_ONESHOT=3), _e(M355_CONV_SLOTS=3, M355_CONV_KSPLIT=2, M355_H16_ONESHOT=3),
    _e(M355_CONV_KSPLIT=1, M355_CONV_NTW=1), _e(M355_CONV_NTW=2, M355_CONV_SLOTS=7, M355_H16_ONESHOT=3, M355_CONV_KSPLIT=1),
    _e(M355_CONV_KSPLIT=3),
    *[_e(M355_H16_W8=w8, M355_H16_ONESHOT=3, **env) for w8 in (2, 0) for env in (
        _e(M355_CONV_KSPLIT=1), _e(M355_CONV_KSPLIT=1, M355_CONV_SLOTS=3), _e(M355_CONV_KSPLIT=2, M355_CONV_SLOTS=5))],
    _e(M355_CONVT_H16=1), _e(M355_CONVT_H16=0), _e(M355_BWW_NSPLIT=5),
    # single knobs
    _e(M355_SMALLCOUT_VALU=0), _e(M355_NO_SMALL=1), _e(M355_BWW_GEN=1), _e(M355_BWW_QUEUE=0), _e(M355_F32X3=0), _e(M355_F32X3=2),
    _e(M355_F32X3_BWW=0), _e(M355_FUSE_SOFTMAX=0), _e(M355_CONV_PERSISTENT=0), _e(M355_CONV_PERSISTENT=2),
    _e(M355_H16_ONESHOT=0), _e(M355_H16_W8=2),
]
TUNING_SETS = [dict(t) for t in dict.fromkeys(tuple(sorted(t.items())) for t in TUNING_SETS)]   # distinct, in order


QUERIES = ["m355_conv3d_plan", "m355_conv3d_fwd_workspace", "m355_conv3d_bwd_data_workspace", "m355_conv3d_bwd_weight_workspace",
           "m355_conv3d_h16_workspace", "m355_conv3d_packed_bytes", "m355_conv3d_bwd_weight_h16_workspace",
           "m355_conv3d_bwd_weight_c8_workspace", "m355_conv3d_stats_slots", "m355_conv3d_stats_slots_c8", "m355_conv3d_fuses_softmax",
           "m355_reload_tuning", "m355_conv3d_launch_plan"]


def open_set(idx):
    """(library with the tuning set's environment read, the set's tag): a process of its own per set, the library reads the
    environment.  (Not _lib.lib(): that insists on every symbol, and a parent library has no m355_conv3d_launch_plan.)"""
    env = TUNING_SETS[idx]
    for k in [k for k in os.environ if k.startswith("M355_") and k != "M355_LIB_PATH"]:
        del os.environ[k]
    os.environ.update(env)
    from segmentation_pipeline_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    for name in QUERIES:
        if getattr(L, name, None) is not None:
            getattr(L, name).restype, getattr(L, name).argtypes = _lib.SIGNATURES[name]
    L.m355_reload_tuning()
    return L, ",".join(f"{k[5:]}={v}" for k, v in sorted(env.items())) or "default"


def run_set(idx):
    """All lines of one tuning set."""
    from segmentation_pipeline_amd import _lib
    L, tag = open_set(idx)
    d = _lib.ConvDesc()
    ref = C.byref(d)
    out4 = (C.c_int32 * 4)()
    sizes = [L.m355_conv3d_fwd_workspace, L.m355_conv3d_bwd_data_workspace, L.m355_conv3d_bwd_weight_workspace]
    sizes_which = [L.m355_conv3d_h16_workspace, L.m355_conv3d_packed_bytes]
    tail = [L.m355_conv3d_bwd_weight_h16_workspace, L.m355_conv3d_bwd_weight_c8_workspace, L.m355_conv3d_stats_slots,
            L.m355_conv3d_stats_slots_c8, L.m355_conv3d_fuses_softmax]
    lines = []
    for (d.N, d.Cin, d.Cout, d.D, d.H, d.W, d.k, d.stride, d.pad, d.compute) in descriptors():
        f = [tag, f"N{d.N} {d.Cin}->{d.Cout} {d.D}x{d.H}x{d.W} k{d.k}s{d.stride}p{d.pad} c{d.compute}"]
        for which in (0, 1, 2):
            rc = L.m355_conv3d_plan(ref, which, out4)
            f.append(f"plan{which}={rc}:" + "/".join(str(v) for v in out4))
        f.append("ws=" + "/".join(str(q(ref)) for q in sizes))
        f += [name + "=" + "/".join(str(q(ref, w)) for w in (0, 1)) for name, q in zip(("h16ws", "packed"), sizes_which)]
        f.append("bww16/c8/slots/slots_c8/softmax=" + "/".join(str(q(ref)) for q in tail))
        lines.append(" ".join(f))
    text = "\n".join(lines) + "\n"
    return idx, len(lines), text


# ---- --launch ----
LAUNCH_CHANNELS = [1, 3, 4, 8, 24, 32, 40, 80, 120]
# tests/test_conv_launch_plans_gpu.py: volumes and (Cin, Cout)
LAUNCH_TEST_VOLUMES = [(6, 9, 36), (5, 7, 33), (8, 4, 32)]
LAUNCH_TEST_CHANNELS = [(3, 32), (32, 4), (40, 24), (32, 32), (8, 40)]
NPTR = 7   # first operand, w | second operand, bias | fp32 dy, add, output, statistics | dbias, workspace


def launch_descriptors():
    """the thinned list: (N, Cin, Cout, D, H, W, k, stride, pad, compute)"""
    for vol, ci, co, n, comp in itertools.product(VOLUMES, LAUNCH_CHANNELS, LAUNCH_CHANNELS, (1, 2), range(4)):
        yield (n, ci, co) + vol + (3, 1, 1, comp)
    small = [c for c in LAUNCH_CHANNELS if c <= 8]
    for vol, ci, co, n, comp in itertools.product(GUARD_VOLUMES, small, small, (1, 2), range(4)):
        yield (n, ci, co) + vol + (3, 1, 1, comp)
    for ksp, vol, ci, co, comp in itertools.product(NON_K3, VOLUMES[:3], LAUNCH_CHANNELS, LAUNCH_CHANNELS, range(4)):
        yield (2, ci, co) + vol + ksp + (comp,)


def launch_variations(cin, cout, S):
    """(label, flags, x / y batch stride of the descriptor, stride arguments, pointers) of one fact moved at a time"""
    base = [(i + 1) << 20 for i in range(NPTR)]
    mandatory = [p if i in (0, 1, 4, 6) else 0 for i, p in enumerate(base)]
    yield "plain", 0, (0, 0), (0, 0), mandatory
    for i in range(NPTR):
        for off in (4, 8):
            yield f"ptr{i}+{off}", 0, (0, 0), (0, 0), [p + (off if j == i else 0) for j, p in enumerate(base)]
    for present in range(1, 8):   # bit 0 add, bit 1 statistics | dbias, bit 2 bias | fp32 dy
        yield f"opt{present}", 0, (0, 0), (0, 0), [p if i in (0, 1, 4, 6) or (present >> {3: 0, 5: 1, 2: 2}[i]) & 1 else 0
                                                     for i, p in enumerate(base)]
    for pad in (1, 2, 4, 8):      # odd, even, float4 and c8-item padded batch strides
        yield f"bs+{pad}", 0, ((cin + 8) * S + pad, (cout + 8) * S + pad), (8 * (cin // 8 + 2) * S + pad, 8 * (cout // 8 + 2) * S + pad), mandatory
    yield "softmax", 2, (0, 0), (0, 0), mandatory
    yield "packed", 1, (0, 0), (0, 0), mandatory
    yield "softmax+add", 2, (0, 0), (0, 0), [p if i != 5 else 0 for i, p in enumerate(base)]


def run_launch_set(idx):
    """(index, line count of the queries, their text, line count of the routes, their text) of one tuning set"""
    from segmentation_pipeline_amd import _lib
    _, count, qtext = run_set(idx)
    L, tag = open_set(idx)
    plan = getattr(L, "m355_conv3d_launch_plan", None)
    if plan is None:
        return idx, count, qtext, 0, None
    d = _lib.ConvDesc()
    ref = C.byref(d)
    out = (C.c_int64 * 12)()
    lines = []
    bs0 = (C.c_int64 * 2)(0, 0)
    ptr0 = (C.c_uint64 * NPTR)(*[(i + 1) << 20 if i in (0, 1, 4, 6) else 0 for i in range(NPTR)])
    for (d.N, d.Cin, d.Cout, d.D, d.H, d.W, d.k, d.stride, d.pad, d.compute) in launch_descriptors():
        f = [tag, f"N{d.N} {d.Cin}->{d.Cout} {d.D}x{d.H}x{d.W} k{d.k}s{d.stride}p{d.pad} c{d.compute}"]
        for entry in range(10):
            rc = plan(entry, ref, bs0, ptr0, 1 << 62, out)
            f.append(f"e{entry}={rc}" + (":" + "/".join(str(v) for v in out) if rc == 0 else ""))
        lines.append(" ".join(f))
    d.k, d.stride, d.pad = 3, 1, 1
    shapes = [(n, ci, co) + vol for n in (2,) for vol in LAUNCH_TEST_VOLUMES for ci, co in LAUNCH_TEST_CHANNELS]
    shapes += [(n, 8, 8, 2, 4, 8) for n in (65535, 65536)]
    for (d.N, d.Cin, d.Cout, d.D, d.H, d.W), d.compute in itertools.product(shapes, range(4)):
        S = d.D * d.H * d.W
        for label, d.flags, (d.x_batch_stride, d.y_batch_stride), bs, ptrs in launch_variations(d.Cin, d.Cout, S):
            f = [tag, f"N{d.N} {d.Cin}->{d.Cout} {d.D}x{d.H}x{d.W} c{d.compute} {label}"]
            for entry in range(10):
                rc = plan(entry, ref, (C.c_int64 * 2)(*bs), (C.c_uint64 * NPTR)(*ptrs), 1 << 62, out)
                f.append(f"e{entry}={rc}" + (":" + "/".join(str(v) for v in out) if rc == 0 else ""))
            lines.append(" ".join(f))
        d.flags, d.x_batch_stride, d.y_batch_stride = 0, 0, 0
    return idx, count, qtext, len(lines), "\n".join(lines) + "\n"


def launch_main(a):
    queries, routes, n, m, have_plan = hashlib.sha256(), hashlib.sha256(), 0, 0, True
    with multiprocessing.get_context("spawn").Pool(a.jobs, maxtasksperchild=1) as pool:
        for idx, count, qtext, rcount, text in pool.imap(run_launch_set, range(len(TUNING_SETS))):
            have_plan = have_plan and text is not None
            if a.hash_only:
                print(f"set {idx:2d} {count} queries {hashlib.sha256(qtext.encode()).hexdigest()}"
                      + (f" {rcount} routes {hashlib.sha256(text.encode()).hexdigest()}" if text else ""), flush=True)
            else:
                sys.stdout.write(text or qtext)
            queries.update(qtext.encode())
            routes.update((text or "").encode())
            n, m = n + count, m + rcount
    print(f"lines {n} queries sha256 {queries.hexdigest()}" + (f" routes ({m} lines) sha256 {routes.hexdigest()}" if have_plan else ""))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hash-only", action="store_true", help="print no lines, only one hash per tuning set and the total")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--convt", action="store_true", help="the conv-transpose routes (two hashes: queries, routes)")
    ap.add_argument("--norm", action="store_true", help="the normalisation plans (two hashes: queries, routes)")
    ap.add_argument("--resample", action="store_true", help="the factor-2 resampling family (two hashes: queries, routes)")
    ap.add_argument("--launch", action="store_true", help="the conv launch plans (two hashes: queries = the default table, routes)")
    a = ap.parse_args()
    if a.launch:
        return launch_main(a)
    if a.resample:
        return resample_main(a)
    if a.convt:
        return convt_main(a)
    if a.norm:
        return norm_main(a)
    total, n = hashlib.sha256(), 0
    with multiprocessing.get_context("spawn").Pool(a.jobs, maxtasksperchild=1) as pool:
        for idx, count, text in pool.imap(run_set, range(len(TUNING_SETS))):
            if a.hash_only:
                print(f"set {idx:2d} {count} {hashlib.sha256(text.encode()).hexdigest()}", flush=True)
            else:
                sys.stdout.write(text)
            total.update(text.encode())
            n += count
    print(f"lines {n} sha256 {total.hexdigest()}")


if __name__ == "__main__":
    main()
