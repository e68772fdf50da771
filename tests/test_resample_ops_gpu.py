"""The factor-2 resampling family at the `ops` level: every public function, in the fp32 flow and both c8 flows, bit for bit
against the raw entry point it is supposed to call (through _lib.lib(), on the same device tensors) -- forward into a fresh
tensor and into a concat slot, with and without tracking; backward for dense, batch-expanded and sliced gradients; the skip
forms; the names of the autograd nodes; and which ops install the fp16 overflow word themselves."""
import contextlib
import ctypes as C
import types
from typing import Callable, NamedTuple

import pytest
import torch

from segmentation_pipeline_amd import _lib, ops

pytestmark = pytest.mark.gpu

N, GUARD, CANARY = 2, 3, -777.25
SPATIALS = [(2, 6, 10), (4, 4, 8)]        # W / 2 odd and W % 4 != 0, against the vector paths
FLOWS = ["fp32", "bf16", "fp16"]
COMPUTE = {"bf16": _lib.COMPUTE_BF16, "fp16": _lib.COMPUTE_F16}
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


class Op(NamedTuple):
    fn: Callable
    kind: str            # argument list of its entry points: "avg", "max" (route, add) or "plain" (source, destination)
    fwd: str
    bwd: str
    skip: bool           # the *_with_skip form: -> (input, result)
    C: int               # input channels: one full c8 block and a ragged one; the s2d pair 2 <-> 16
    cmul: int            # output channels = C * cmul // cdiv
    cdiv: int
    up: bool             # output spatial size: twice (True) or half the input's
    full_out: bool       # the entry points take the shape of the output (depth_to_space2), not of the input
    has_out: bool
    node32: str
    node_c8: str
    installs: bool       # its c8 function installs the fp16 overflow word itself


def _tri(mode):
    return lambda x, out=None: ops.upsample_trilinear2x(x, out, mode=mode)


_POOL = dict(C=12, cmul=1, cdiv=1, up=False, full_out=False, has_out=True)
_UP = dict(kind="plain", skip=False, C=12, cmul=1, cdiv=1, up=True, full_out=False, has_out=True, node32="_UpsampleFn",
           node_c8="_UpsampleC8Fn")
OPS = {
    "avgpool3d_2x": Op(ops.avgpool3d_2x, "avg", "avgpool3d_2x_fwd", "avgpool3d_2x_bwd", False, node32="_AvgPoolFn",
                       node_c8="_PoolC8Fn", installs=False, **_POOL),
    "avgpool3d_2x_with_skip": Op(ops.avgpool3d_2x_with_skip, "avg", "avgpool3d_2x_fwd", "avgpool3d_2x_bwd", True,
                                 node32="_PoolSkipFn", node_c8="_PoolC8Fn", installs=False, **_POOL),
    "maxpool3d_2x": Op(ops.maxpool3d_2x, "max", "maxpool3d_2x_fwd", "maxpool3d_2x_bwd", False, node32="_MaxPoolFn",
                       node_c8="_MaxPoolC8Fn", installs=True, **_POOL),
    "maxpool3d_2x_with_skip": Op(ops.maxpool3d_2x_with_skip, "max", "maxpool3d_2x_fwd", "maxpool3d_2x_bwd", True,
                                 node32="_MaxPoolSkipFn", node_c8="_MaxPoolC8Fn", installs=True, **_POOL),
    "upsample_trilinear2x": Op(ops.upsample_trilinear2x, fwd="upsample_trilinear2x_fwd", bwd="upsample_trilinear2x_bwd",
                               installs=False, **_UP),
    "upsample_nearest2x": Op(ops.upsample_nearest2x, fwd="upsample_nearest2x_fwd", bwd="upsample_nearest2x_bwd",
                             installs=True, **_UP),
    "upsample_trilinear2x_hp": Op(ops.upsample_trilinear2x_hp, fwd="upsample_trilinear2x_hp_fwd",
                                  bwd="upsample_trilinear2x_hp_bwd", installs=True, **_UP),
    # the same entry points through upsample_trilinear2x(mode=...)
    "upsample_trilinear2x[nearest]": Op(_tri("nearest"), fwd="upsample_nearest2x_fwd", bwd="upsample_nearest2x_bwd",
                                        installs=True, **_UP),
    "upsample_trilinear2x[trilinear_hp]": Op(_tri("trilinear_hp"), fwd="upsample_trilinear2x_hp_fwd",
                                             bwd="upsample_trilinear2x_hp_bwd", installs=True, **_UP),
    "space_to_depth2": Op(ops.space_to_depth2, "plain", "space_to_depth2", "depth_to_space2", False, 2, 8, 1, False, False,
                          False, "_S2DFn", "_S2DC8Fn", False),
    "depth_to_space2": Op(ops.depth_to_space2, "plain", "depth_to_space2", "space_to_depth2", False, 16, 1, 8, True, True,
                          True, "_S2DFn", "_S2DC8Fn", False),
}
CASES = [pytest.param(name, flow, sp, id=f"{name}-{flow}-" + "x".join(map(str, sp)))
         for name in OPS for flow in FLOWS for sp in SPATIALS]
# avgpool3d_2x_with_skip on a c8 activation that does not track has a case of its own below
NO_PLAIN_FORM = {("avgpool3d_2x_with_skip", "bf16"), ("avgpool3d_2x_with_skip", "fp16")}


# ------------------------------------------------------------------------------------------------ raw entry points
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _raw(name, pointers, shape, strides, compute):
    L = _lib.lib()
    args = list(pointers) + list(shape) + list(strides) + ([compute] if compute else [])
    args.append(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert getattr(L, "m355_" + name)(*args) == 0, (name, L.m355_last_error())


def raw_fwd(op, compute, x, y, route, shape):
    """x, y, route: dense device tensors (NCDHW fp32, or [N, CB, S, 8] c8)"""
    ptrs = (_p(x), _p(y), _p(route)) if op.kind == "max" else (_p(x), _p(y))
    _raw(op.fwd + ("_h16" if compute else ""), ptrs, shape, (0, 0), compute)


def raw_bwd(op, compute, g, add, dx, route, shape):
    h16 = "_h16" if compute else ""
    if op.kind == "max":
        _raw(op.bwd + h16, (_p(g), _p(route), _p(add), _p(dx)), shape, (0, 0, 0), compute)
    elif op.kind == "avg" and (compute or add is not None):
        _raw(op.bwd + (h16 or "_add"), (_p(g), _p(add), _p(dx)), shape, (0, 0, 0), compute)
    else:
        assert add is None
        _raw(op.bwd + h16, (_p(g), _p(dx)), shape, (0, 0), compute)


# ------------------------------------------------------------------------------------------------ shapes and tensors
def out_shape(op, xshape):
    n, c, d, h, w = xshape
    c = c * op.cmul // op.cdiv
    return (n, c, 2 * d, 2 * h, 2 * w) if op.up else (n, c, d // 2, h // 2, w // 2)


def c8_shape(shape):
    n, c, d, h, w = shape
    return (n, (c + 7) // 8, d * h * w, 8)


def _randn(shape, seed, flow):
    """seeded values on the device, in the flow's tensor type; exactly representable in its number format"""
    t = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return t.cuda() if flow == "fp32" else t.to(DT[flow]).cuda()


def same(a, b, Cc, flow):
    """bit for bit; of a c8 tensor the lanes of its channels (the lanes past C of a ragged last block are padding)"""
    if flow == "fp32":
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    a, b = a.contiguous().view(torch.int16).clone(), b.contiguous().view(torch.int16).clone()
    if Cc % 8:
        a[:, -1, :, Cc % 8:] = 0
        b[:, -1, :, Cc % 8:] = 0
    return torch.equal(a, b)


def _flow(flow):
    return contextlib.nullcontext() if flow == "fp32" else ops.precision(flow)


def make_input(x32, flow, track):
    """the op's input: an fp32 tensor, or the c8 activation packed from it; tracking or plain"""
    if flow == "fp32":
        return x32.clone().requires_grad_(track)
    if track:
        a = ops.pack_act16(x32.clone().requires_grad_(True), COMPUTE[flow])
        assert a.requires_grad
        return a
    with torch.no_grad():
        return ops.pack_act16(x32, COMPUTE[flow])


def call(op, x, out=None):
    res = op.fn(x, out) if op.has_out else op.fn(x)
    return res if op.skip else (None, res)


def tensor_of(y, flow):
    return y if flow == "fp32" else y.alias()


def handle(y, flow):
    """what autograd differentiates: the tensor, or a c8 activation's handle"""
    return y if flow == "fp32" else y.t


class Reference:
    """the raw forward of `op` on the seeded input of `spatial`: input, result and route, computed once per case"""

    def __init__(self, name, flow, spatial):
        self.op = op = OPS[name]
        self.flow, self.compute = flow, COMPUTE.get(flow, 0)
        self.xshape = (N, op.C) + tuple(spatial)
        self.oshape = out_shape(op, self.xshape)
        self.entry_shape = self.oshape if op.full_out else self.xshape
        self.x32 = _randn(self.xshape, 11, "fp32")
        if flow != "fp32":
            self.x32 = self.x32.to(DT[flow]).float()
        with _flow(flow):
            x = tensor_of(make_input(self.x32, flow, False), flow)
        self.y = self.empty(self.oshape)
        self.route = None
        if op.kind == "max":
            rshape = self.oshape if flow == "fp32" else c8_shape(self.xshape)[:2] + c8_shape(self.oshape)[2:]
            self.route = torch.zeros(rshape, dtype=torch.uint8, device="cuda")
        raw_fwd(op, self.compute, x, self.y, self.route, self.entry_shape)

    def empty(self, shape):
        if self.flow == "fp32":
            return torch.zeros(shape, device="cuda")
        return torch.zeros(c8_shape(shape), dtype=DT[self.flow], device="cuda")

    def backward(self, g, add=None):
        dx = self.empty(self.xshape)
        dense = torch.contiguous_format                   # (a copy: dense, and aligned as the allocator aligns)
        raw_bwd(self.op, self.compute, g.clone(memory_format=dense), None if add is None else add.clone(memory_format=dense),
                dx, self.route, self.entry_shape)
        return dx


def make_slot(ref, oshape=None):
    """(OutSlot, buffer, guards) at a non-zero channel offset of a wider canary-filled buffer: fp32 GUARD channels on each
    side, c8 one guard block on each side"""
    n, c = (oshape or ref.oshape)[:2]
    sp = tuple((oshape or ref.oshape)[2:])
    if ref.flow == "fp32":
        buf = torch.full((n, c + 2 * GUARD) + sp, CANARY, device="cuda")
        return ops.OutSlot(buf, GUARD, GUARD + c), buf, [buf[:, :GUARD], buf[:, GUARD + c:]]
    cb = (c + 7) // 8
    data = torch.full((n, cb + 2, sp[0] * sp[1] * sp[2], 8), CANARY, dtype=DT[ref.flow], device="cuda")
    buf16 = ops.Act16(data, 8 * (cb + 2), sp, ref.compute)
    return ops.OutSlot(None, 8, 8 + c, buf16=buf16), data, [data[:, :1], data[:, cb + 1:]]


def intact(guards):
    return all(bool((g == torch.full((), CANARY, dtype=g.dtype, device=g.device)).all()) for g in guards)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name, flow, spatial", CASES)
def test_forward_is_the_raw_entry_point(name, flow, spatial):
    ref = Reference(name, flow, spatial)
    op = ref.op
    with _flow(flow):
        for track in (False, True):
            if not track and (name, flow) in NO_PLAIN_FORM:
                continue
            for slotted in (False, True) if op.has_out else (False,):
                out, buf, guards = make_slot(ref) if slotted else (None, None, [])
                with torch.set_grad_enabled(track):
                    x = make_input(ref.x32, flow, track)
                    skip, y = call(op, x, out)
                where = (track, slotted)
                assert same(tensor_of(y, flow), ref.y, ref.oshape[1], flow), where
                node = handle(y, flow).grad_fn if handle(y, flow) is not None else None
                if track:
                    assert type(node).__name__ == (op.node32 if flow == "fp32" else op.node_c8) + "Backward", where
                else:
                    assert node is None and (flow == "fp32" or y.t is None), where
                if op.skip:       # the input as it continues: the same storage
                    assert tensor_of(skip, flow).data_ptr() == tensor_of(x, flow).data_ptr(), where
                    assert not track or handle(skip, flow).data_ptr() == handle(x, flow).data_ptr(), where
                    assert same(tensor_of(skip, flow), tensor_of(x, flow), op.C, flow), where
                if not slotted:
                    continue
                assert intact(guards), where
                if flow == "fp32" and op.skip:            # the fp32 skip forms ignore `out`
                    assert intact([buf]) and y.data_ptr() != buf[:, GUARD:].data_ptr(), where
                elif flow == "fp32":
                    assert y.data_ptr() == buf[:, GUARD:].data_ptr() and y.stride() == buf[:, GUARD:GUARD + y.shape[1]].stride()
                else:                                     # the returned activation IS the slot
                    assert y.data.data_ptr() == buf.data_ptr() and y.cb0 == 1 and y.shape == ref.oshape, where
                    assert y.ptr().value == buf[:, 1:].data_ptr(), where


# every op with an `out`, but the fp32 skip forms, which ignore it (forward test), and the c8 average pool (case below)
WRONG_SLOT = [(n, f) for n, op in OPS.items() if op.has_out for f in FLOWS
              if not (f == "fp32" and op.skip) and not (f != "fp32" and n == "avgpool3d_2x")]


@pytest.mark.parametrize("name, flow", WRONG_SLOT)
def test_a_slot_of_the_wrong_shape_is_refused(name, flow):
    ref = Reference(name, flow, SPATIALS[1])
    n, c, d, h, w = ref.oshape
    out, buf, _ = make_slot(ref, (n, c, d, h, w + 2))
    track = (name, flow) in NO_PLAIN_FORM
    with _flow(flow), torch.set_grad_enabled(track):
        with pytest.raises(_lib.M355Error, match="slot shape"):
            call(ref.op, make_input(ref.x32, flow, track), out)
    assert intact([buf])


# (this case pins a unification of this file's pull request: before it, the c8 average pool took its slot unchecked)
@pytest.mark.parametrize("flow", ["bf16", "fp16"])
def test_c8_avgpool_checks_its_slot(flow):
    ref = Reference("avgpool3d_2x", flow, SPATIALS[1])
    n, c, d, h, w = ref.oshape
    out, buf, _ = make_slot(ref, (n, c, d, h, w + 2))
    with _flow(flow), torch.no_grad():
        with pytest.raises(_lib.M355Error, match="slot shape"):
            ops.avgpool3d_2x(make_input(ref.x32, flow, False), out)
    assert intact([buf])


# (this case pins a unification of this file's pull request: before it, only the max pool's skip form accepted a c8
# activation that does not track)
@pytest.mark.parametrize("flow", ["bf16", "fp16"])
def test_c8_avgpool_with_skip_without_tracking(flow):
    ref = Reference("avgpool3d_2x_with_skip", flow, SPATIALS[0])
    with _flow(flow), torch.no_grad():
        x = make_input(ref.x32, flow, False)
        for slotted in (False, True):
            out, buf, guards = make_slot(ref) if slotted else (None, None, [])
            skip, y = ops.avgpool3d_2x_with_skip(x, out)
            assert skip is x and y.t is None and same(y.alias(), ref.y, ref.oshape[1], flow) and intact(guards)
            assert not slotted or y.data.data_ptr() == buf.data_ptr()


@pytest.mark.parametrize("name", ["space_to_depth2", "depth_to_space2"])
def test_fp32_s2d_pair_on_views_that_are_only_4_byte_aligned(name):
    """the full-resolution side one element into its allocation: compacted on input (the input of space_to_depth2, the
    gradient of depth_to_space2), produced in a fresh tensor and copied into the slot on output (depth_to_space2)"""
    ref = Reference(name, "fp32", SPATIALS[0])
    op = ref.op

    def shifted(t, fill=None):
        base = torch.full((t.numel() + 2,), CANARY, device="cuda")
        v = base[1:t.numel() + 1].view(t.shape)
        if fill is not None:
            v.copy_(fill)
        return base, v
    if name == "space_to_depth2":
        _, x = shifted(ref.x32, ref.x32)
        x.requires_grad_(True)
        y = op.fn(x)
        g = _randn(ref.oshape, 5, "fp32")
    else:
        n, c = ref.oshape[:2]
        base, buf = shifted(torch.empty((n, c + 2 * GUARD) + ref.oshape[2:]))
        x = ref.x32.clone().requires_grad_(True)
        y = op.fn(x, ops.OutSlot(buf, GUARD, GUARD + c))
        assert y.data_ptr() == buf[:, GUARD:].data_ptr() and y.data_ptr() % 8 == 4
        assert intact([base[:1], base[-1:], buf[:, :GUARD], buf[:, GUARD + c:]])
        _, g = shifted(torch.empty(ref.oshape), _randn(ref.oshape, 5, "fp32"))
    assert same(y, ref.y, ref.oshape[1], "fp32")
    assert same(torch.autograd.grad(y, x, g)[0], ref.backward(g), op.C, "fp32")


# ------------------------------------------------------------------------------------------------ backward
def gradient(shape, layout, seed, flow):
    """a gradient of `shape` (c8: [N, CB, S, 8]) in one of the layouts autograd hands over"""
    n, c = shape[:2]
    if layout == "dense":
        return _randn(shape, seed, flow)
    if layout == "expanded":                              # stride 0 along the batch: what y.sum(dim=0) hands back
        return _randn((1,) + tuple(shape[1:]), seed, flow).expand(shape)
    guard = GUARD if flow == "fp32" else 1                # a channel slice / a block slice of a wider buffer
    return _randn((n, c + 2 * guard) + tuple(shape[2:]), seed, flow)[:, guard:guard + c]


@pytest.mark.parametrize("name, flow, spatial", CASES)
def test_backward_is_the_raw_entry_point(name, flow, spatial):
    ref = Reference(name, flow, spatial)
    op = ref.op
    gshape = ref.oshape if flow == "fp32" else c8_shape(ref.oshape)
    sshape = ref.xshape if flow == "fp32" else c8_shape(ref.xshape)
    with _flow(flow):
        x = make_input(ref.x32, flow, True)
        skip, y = call(op, x)
        leaf, yt = handle(x, flow), handle(y, flow)
        for layout in ("dense", "expanded", "slice"):
            g = gradient(gshape, layout, 21, flow)
            assert layout == "dense" or not g.is_contiguous()
            dx = torch.autograd.grad(yt, leaf, g, retain_graph=True)[0]
            assert same(dx, ref.backward(g), op.C, flow), layout
            if not op.skip:
                continue
            # both gradients: one pass with `add`
            gs = gradient(sshape, layout, 22, flow)
            dx = torch.autograd.grad([handle(skip, flow), yt], leaf, [gs, g], retain_graph=True)[0]
            assert same(dx, ref.backward(g, gs), op.C, flow), layout
        if op.skip:
            # the skip gradient alone: autograd hands the function zeros for the pooled output, and the sum is the skip
            # gradient again (no element of it is a zero, whose sign the sum could change)
            gs = gradient(sshape, "dense", 23, flow)
            dx = torch.autograd.grad(handle(skip, flow), leaf, gs, retain_graph=True)[0]
            assert same(dx, gs, op.C, flow)


@pytest.mark.parametrize("cls", ["_PoolSkipFn", "_MaxPoolSkipFn", "_PoolC8Fn", "_MaxPoolC8Fn"])
def test_skip_gradient_without_a_pool_gradient_is_handed_back_as_it_is(cls):
    """backward(skip gradient, None) -- what autograd passes with set_materialize_grads(False) -- launches nothing and
    returns that very tensor for the input"""
    shape = (N, 12) + SPATIALS[1]
    ctx = types.SimpleNamespace(shape=shape, info=shape + (_lib.COMPUTE_BF16,), idx=None, idx8=None, route=None)
    g = torch.ones(c8_shape(shape) if "C8" in cls else shape, device="cuda")
    got = getattr(ops, cls).backward(ctx, g, None)
    got = got if isinstance(got, tuple) else (got,)
    assert got[0] is g and all(v is None for v in got[1:])


# ------------------------------------------------------------------------------------------------ overflow word
OVERFLOW_OPS = ["avgpool3d_2x_with_skip", "maxpool3d_2x_with_skip", "upsample_trilinear2x", "upsample_nearest2x",
                "upsample_trilinear2x_hp", "space_to_depth2", "depth_to_space2"]


@pytest.mark.parametrize("name", OVERFLOW_OPS)
def test_which_c8_functions_install_the_fp16_overflow_word(name, monkeypatch):
    """pack -> op -> backward on its own, fp16, from a state in which no word is installed.  The gradients saturate the
    backward's sums: dskip = dpool = 60000 in one voxel for the pools, 10000 everywhere for the single-gradient ops (eight
    of them exceed 65504).  Bit 0 is reported by exactly the ops that install the word themselves (max pool, nearest,
    half-pixel trilinear); the others leave that to a neighbouring node of the model, and on their own report nothing.
    The package's word is put back, and read before and after, so the test leaves it clear."""
    for attr in ("_fp16_target", "_fp16_clean_checks"):
        monkeypatch.setattr(ops, attr, getattr(ops, attr))
    op, L, dev = OPS[name], _lib.lib(), torch.cuda.current_device()
    ops.fp16_overflow()                                   # whatever earlier tests left
    assert ops.fp16_overflow() == 0
    before = dict(ops._overflow_words)
    compute, spatial = COMPUTE["fp16"], (2, 2, 4)
    xshape = (1, op.C) + spatial
    oshape = out_shape(op, xshape)
    x = torch.zeros(xshape)
    x[0, 1, 1, 0, 2] = 5.0                                # the maximum of its window
    try:
        assert L.m355_overflow_flag_set(None, dev) == 0
        ops._overflow_words.clear()
        with ops.precision("fp16"):
            a = ops.pack_act16(x.cuda().requires_grad_(True), compute)
            skip, y = call(op, a)
            assert bool(ops._overflow_words) == op.installs
            if op.skip:
                dpool, dskip = torch.zeros(oshape), torch.zeros(xshape)
                dpool[0, 1, 0, 0, 1] = dskip[0, 1, 1, 0, 2] = 60000.0
                with torch.no_grad():
                    grads = [ops.pack_act16(dskip.cuda(), compute).data, ops.pack_act16(dpool.cuda(), compute).data]
                dx16 = torch.autograd.grad([skip.t, y.t], a.t, grads)[0]
            else:
                dx16 = torch.autograd.grad(y.t, a.t, torch.full(c8_shape(oshape), 10000.0, dtype=torch.float16, device="cuda"))[0]
            word = ops.fp16_overflow()
        assert word == (1 if op.installs else 0), word
    finally:
        ops._overflow_words.clear()
        ops._overflow_words.update(before)
        assert L.m355_overflow_flag_set(_p(before.get(dev)), dev) == 0
    assert ops.fp16_overflow() == 0
