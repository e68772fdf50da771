"""torch.autograd bindings of the HIP kernels (one Function per op family).

PyTorch is plumbing here: device memory (caching allocator), the current HIP
stream, and the autograd graph.  Every tensor op on the hot path is a call
through the C ABI of libm355seg.so; nothing falls back to torch or to the CPU.
"""
import ctypes as C
import math
import os
import weakref
from dataclasses import dataclass
from operator import itemgetter
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import ACT_LEAKY_RELU, ACT_NONE, ACT_RELU, ConvDesc, NormDesc, check

# Arithmetic of the 3x3x3 convolutions:
#   "fp32" (default)  fp32 tensors, fp32 results.  The 3x3x3 convolutions with >= 8 input and > 4 output channels (forward / data
#                     gradient; weight gradient: > 4 channels on both sides) and the k2 s2 conv-transpose forward run on the bf16 matrix pipe: every operand is split EXACTLY into three bf16
#                     values (8 + 8 + 8 significant bits) and six plane products per fp32 product are accumulated in fp32
#                     (M355_COMPUTE_F32X3, csrc/conv3d_f32x3.hip) -- measured against fp64 as accurate as the fp32 MFMA
#                     kernels (the error of both is the fp32 accumulation's), 1.5-1.7x their rate; the output conv and the
#                     edge layers' weight gradients run the fp32 MFMA / vector-ALU kernels.  Every 1e-4 parity claim refers to this mode.
#                     M355_FP32_SPLIT=0 in the environment maps "fp32" to "fp32_mfma".
#   "fp32_mfma"       every convolution on v_mfma_f32_32x32x2_f32 (M355_COMPUTE_F32): the same tensors, layouts and flow,
#                     only the conv kernels differ; results differ from "fp32" by summation-order noise.
#   "bf16" / "fp16"   operands rounded to 16 bits, fp32 accumulate (BASELINE cfg3 / cfg5).
# In the 16-bit modes the forward / data-gradient / weight-gradient kernels of the 3x3x3 stride-1 convolutions with
# more than 4 channels on both sides read the c8 activation layout (include/m355seg.h); the
# edge layers go through the fp32-tensor entry points, which round the operands while staging them (Cin <= 4
# forward) or take the vector-ALU fp32 path (Cout <= 4).  Normalisation, pooling, conv-transpose, softmax and loss
# kernels always compute in fp32.
# Under torch.no_grad() the activations between conv -> norm/act -> conv (-> pool) live ONLY in c8 (`Act16`):
# no fp32 copy is written or read.
FP32_SPLIT = os.environ.get("M355_FP32_SPLIT", "1") != "0"
_COMPUTE = {"fp32": _lib.COMPUTE_F32X3 if FP32_SPLIT else _lib.COMPUTE_F32, "fp32_mfma": _lib.COMPUTE_F32,
            "bf16": _lib.COMPUTE_BF16, "fp16": _lib.COMPUTE_F16}
_DT16 = {_lib.COMPUTE_BF16: torch.bfloat16, _lib.COMPUTE_F16: torch.float16}
_compute_mode = "fp32"


def set_precision(mode: str):
    global _compute_mode
    if mode not in _COMPUTE:
        raise ValueError(f"precision must be one of {sorted(_COMPUTE)}, not {mode!r}")
    _compute_mode = mode


def get_precision() -> str:
    return _compute_mode


def is_fp32() -> bool:
    """fp32 tensors between the layers ("fp32" / "fp32_mfma")"""
    return _COMPUTE[_compute_mode] not in _DT16


class precision:
    """Context manager: `with ops.precision("bf16"): y = model(x)`."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = get_precision()
        set_precision(self.mode)

    def __exit__(self, *exc):
        set_precision(self.prev)


# Optional instrumentation used by bench.py: when set to a list, every conv launch appends
# (tag, flops, start_event, end_event, plan, algorithmic bytes) recorded on the launch stream.
CONV_PROFILE: Optional[list] = None
# restrict CONV_PROFILE to launches whose (tag, plan) is in this set: bench.py event-times only the dominant kernel
# inside its timed region (two timing events around each of the ~56 conv launches of a step are a measurable
# perturbation of a 12 ms step)
CONV_PROFILE_KEYS: Optional[set] = None
# ... and only every CONV_PROFILE_EVERY-th of those launches (a stride coprime with their count per step walks through
# all layers over a few steps)
CONV_PROFILE_EVERY = 1
_prof_seen = 0


def _conv_bytes(N, Cin, Cout, voxels, taps, in_elem, out_elem):
    """algorithmic HBM bytes of one conv launch: input once + output once + weights once"""
    return float(N) * voxels * (Cin * in_elem + Cout * out_elem) + 4.0 * Cin * Cout * taps


def _conv_launch(tag, d, which, in_elem, out_elem, fn, *args):
    """THE launch of a convolution: `fn(*args)`, an entry point of the library, checked.  While CONV_PROFILE is a list and
    the gates let this launch through, it is recorded between two events.  d: the descriptor before any flag is set, which
    gives the shape of the record (N, Cin, Cout, k and the output voxels: flops and bytes) and its plan,
    m355_conv3d_plan(d, which) -- which = None: the record carries no plan (the weight gradient from c8 operands);
    in_elem / out_elem: bytes per element the flow reports.  With profiling off nothing of the record is computed."""
    prof = CONV_PROFILE
    if prof is not None:
        plan = conv_plan(d, which) if which is not None else None
        if CONV_PROFILE_KEYS is not None and (tag, plan) not in CONV_PROFILE_KEYS:
            prof = None
        elif CONV_PROFILE_EVERY > 1:
            global _prof_seen
            _prof_seen += 1
            if _prof_seen % CONV_PROFILE_EVERY:
                prof = None
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    rc = fn(*args)
    if rc:
        check(rc, fn.__name__[len("m355_"):])
    if prof is not None:
        e1.record()
        taps = d.k ** 3
        voxels = 1
        for n in (d.D, d.H, d.W):
            voxels *= (n + 2 * d.pad - d.k) // d.stride + 1
        prof.append((tag, 2.0 * taps * d.Cin * d.Cout * d.N * voxels, e0, e1, plan,
                     _conv_bytes(d.N, d.Cin, d.Cout, voxels, taps, in_elem, out_elem)))


# ----------------------------------------------------------------- helpers
# torch.cuda.current_stream() builds a Stream object through three layers of Python (device-index parsing, availability
# checks): ~8 us a call, once per launch -- a quarter of the host time of a forward where the step is host-bound
# (msseg2 in the 16-bit modes: ~120 launches in 3.4 ms).  The raw handle of the current stream is one C call.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    if _raw_stream is not None and _cur_device is not None:
        return C.c_void_p(_raw_stream(_cur_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _require(*tensors, dtype=torch.float32):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.M355Error(
                "segmentation_pipeline_amd ops run only on the GPU through libm355seg.so "
                f"(got a {t.device} tensor); there is no CPU fallback")
        if t.dtype != dtype:
            raise _lib.M355Error(f"expected {dtype}, got {t.dtype}")


def _workspace(nbytes, device):
    # (every conv launch asks for its workspace here first: the one place that hands the library its work-queue pool)
    if device.index not in _lib._queue_pools:
        _lib.ensure_queue_pool(device)
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _dense_channels(t):
    """Return (tensor, batch_stride) for a 5-D tensor whose (C, D, H, W) block is
    dense and whose samples do not overlap (batch stride >= C*S); channel slices of a
    concat buffer qualify.  Anything else is compacted -- a batch-expanded gradient
    (stride 0, what `y.sum(dim=0)` hands back) among them: 0 means "dense" in the C ABI."""
    N, Cc, D, H, W = t.shape
    st = t.stride()
    S = D * H * W
    ok = ((W == 1 or st[4] == 1) and (H == 1 or st[3] == W) and (D == 1 or st[2] == H * W)
          and (Cc == 1 or st[1] == S) and (N == 1 or st[0] >= Cc * S))
    if not ok:
        t = t.contiguous()
        return t, Cc * S
    return t, (st[0] if N > 1 else Cc * S)


def _pairs_ok(t, bs):
    """m355_norm_act_pool_fwd and the fp32 space-to-depth pair move x pairs: they want an 8-byte aligned pointer and an
    even batch stride (m355seg.h).  Channel slices of an allocator-aligned buffer always qualify; a caller's view at an odd
    element offset does not."""
    return t.data_ptr() % 8 == 0 and (t.shape[0] == 1 or bs % 2 == 0)


def _pairs_in(t, bs):
    """(tensor, batch stride) of an INPUT of those kernels: a view they would reject is compacted first"""
    if _pairs_ok(t, bs):
        return t, bs
    t = t.clone(memory_format=torch.contiguous_format)
    return t, t[0].numel()


def _pairs_out(y, bs):
    """(tensor to write, batch stride) for an OUTPUT of those kernels: a destination they would reject is produced in a
    fresh tensor, which the caller copies into `y` afterwards (`written is not y`)"""
    if _pairs_ok(y, bs):
        return y, bs
    t = torch.empty(y.shape, dtype=y.dtype, device=y.device)
    return t, t[0].numel()


class OutSlot:
    """A destination inside a pre-allocated concat buffer.

    Wrapped in a plain object so autograd does not see the buffer as an input:
    producers write straight into their channel slice (no torch.cat copy, no
    CopySlices nodes) and return a fresh tensor aliasing the slice.
    """

    def __init__(self, buf: Optional[torch.Tensor], c0: int, c1: int, buf16=None):
        # buf16: the c8 twin of the buffer (an `Act16` spanning all its channels) in the 16-bit no-grad flow;
        # `buf` may then be None (nothing is kept in fp32)
        self.buf, self.c0, self.c1, self.buf16 = buf, c0, c1, buf16

    def view(self):
        return self.buf[:, self.c0:self.c1]

    def act16(self):
        return None if self.buf16 is None else self.buf16.slot(self.c0, self.c1)


class Concat:
    """Channel concatenation of tensors that already live in adjacent slices of
    `buf` (models/modular_unet.py:97: torch.cat([x_up, x_skip], dim=1))."""

    def __init__(self, buf, parts: Sequence):
        # buf: the fp32 concat buffer, or an `Act16` (c8 flow of the 16-bit modes under no_grad)
        self.buf, self.parts = buf, list(parts)
        assert sum(p.shape[1] for p in self.parts) == buf.shape[1]

    @property
    def shape(self):
        return self.buf.shape


def _alloc_out(out: Optional[OutSlot], shape, like):
    if out is None:
        return torch.empty(shape, dtype=like.dtype, device=like.device)
    v = out.view()
    if tuple(v.shape) != tuple(shape):
        raise _lib.M355Error(f"output slot shape {tuple(v.shape)} != op output shape {tuple(shape)}")
    # fresh tensor object aliasing the slice (see OutSlot)
    return torch.as_strided(out.buf, v.shape, v.stride(), v.storage_offset())


# ----------------------------------------------------- c8 activations (16-bit modes)
def h16_flow() -> int:
    """The 16-bit compute code when activations should flow in the c8 layout (a 16-bit precision mode; with autograd
    recording the c8-only training flow, H16_TRAIN_C8ONLY), else 0."""
    c = _COMPUTE[_compute_mode]
    if c not in _DT16:
        return 0
    if not torch.is_grad_enabled():
        return c
    # with autograd: the c8-only training flow (`_*C8Fn` below) -- since round 4 under synchronised batch norm too
    # (m355_norm_act_bwd_c8_reduce / _apply: the backward split around the all-reduce, on c8 tensors)
    return c if H16_TRAIN_C8ONLY else 0


class Act16:
    """An activation in the c8 layout: `data` is [N, CB_total, S, 8] (bf16 / fp16); this activation
    occupies the channel blocks [cb0, cb0 + ceil(C / 8)) of it (a slot of a concat buffer, or all of it)."""

    def __init__(self, data: torch.Tensor, C: int, spatial, compute: int, cb0: int = 0, t: Optional[torch.Tensor] = None):
        self.data, self.C, self.spatial, self.compute, self.cb0 = data, int(C), tuple(spatial), compute, cb0
        # c8-only TRAINING flow: the autograd handle of this activation -- a [N, CB, S, 8] tensor aliasing exactly its
        # channel blocks of `data` (produced by one of the `_*C8Fn` functions below); None outside autograd
        self.t = t

    @property
    def requires_grad(self):
        return self.t is not None and self.t.requires_grad

    @property
    def CB(self):
        return (self.C + 7) // 8

    def alias(self):
        """a fresh [N, CB, S, 8] tensor over exactly this activation's blocks (no autograd history)"""
        d = self.data
        N, CBt, S = d.shape[0], d.shape[1], d.shape[2]
        return torch.as_strided(d.detach(), (N, self.CB, S, 8), (CBt * S * 8, S * 8, 8, 1), d.storage_offset() + self.cb0 * S * 8)

    @staticmethod
    def empty(N, C, spatial, compute, device):
        S = spatial[0] * spatial[1] * spatial[2]
        return Act16(torch.empty((N, (C + 7) // 8, S, 8), dtype=_DT16[compute], device=device), C, spatial, compute)

    @property
    def shape(self):
        return (self.data.shape[0], self.C) + self.spatial

    @property
    def device(self):
        return self.data.device

    @property
    def S(self):
        return self.data.shape[2]

    def ptr(self):
        return C.c_void_p(self.data.data_ptr() + self.cb0 * self.S * 16)

    def batch_stride(self):
        return self.data.shape[1] * self.S * 8

    def with_t(self, t):
        """this activation with `t` as its autograd handle"""
        return Act16(self.data, self.C, self.spatial, self.compute, self.cb0, t)

    def slot(self, c0, c1):
        if c0 % 8:
            raise _lib.M355Error(f"a c8 slot must start at a multiple of 8 channels (got {c0})")
        return Act16(self.data, c1 - c0, self.spatial, self.compute, self.cb0 + c0 // 8)

    def to_f32(self):
        if torch.is_grad_enabled() and self.requires_grad:      # c8 training flow: differentiable (fallback ops)
            return _UnpackFn.apply(self.t, self)
        N = self.data.shape[0]
        x = torch.empty((N, self.C) + self.spatial, dtype=torch.float32, device=self.device)
        check(_lib.lib().m355_act16_unpack(self.ptr(), _p(x), N, self.C, self.S, self.batch_stride(), 0, self.compute,
                                           _stream()), "act16_unpack")
        return x


def _c8_out_slot(x: Act16, out: Optional["OutSlot"], spatial, C: Optional[int] = None) -> Act16:
    """the c8 output of an op on `x` (C channels, default x.C): its slot of the concat buffer, shape-checked, else a fresh
    activation"""
    shape = (x.shape[0], x.C if C is None else C) + tuple(spatial)
    y16 = out.act16() if out is not None else None
    if y16 is None:
        return Act16.empty(shape[0], shape[1], shape[2:], x.compute, x.device)
    if y16.shape != shape:
        raise _lib.M355Error(f"c8 slot shape {y16.shape} != op output shape {shape}")
    return y16


def _c8_grad(N, C, S, compute, device) -> torch.Tensor:
    """a dense c8 gradient tensor [N, ceil(C / 8), S, 8] for a backward kernel to fill"""
    return torch.empty((N, (C + 7) // 8, S, 8), dtype=_DT16[compute], device=device)


def pack_act16(x: torch.Tensor, compute: int, out: Optional[Act16] = None) -> Act16:
    """fp32 NCDHW tensor -> c8 (into `out`, a slot of matching shape, or a fresh buffer)."""
    if torch.is_grad_enabled() and x.requires_grad and h16_flow():   # c8 training flow: differentiable (fallback ops)
        N, Cc = x.shape[:2]
        if out is None:
            out = Act16.empty(N, Cc, x.shape[2:], compute, x.device)
        elif out.shape != tuple(x.shape):
            raise _lib.M355Error(f"c8 slot shape {out.shape} != tensor shape {tuple(x.shape)}")
        t = _PackFn.apply(x, out)
        return Act16(out.data, out.C, out.spatial, out.compute, out.cb0, t)
    _require(x)
    x, xbs = _dense_channels(x)
    N, Cc = x.shape[:2]
    if out is None:
        out = Act16.empty(N, Cc, x.shape[2:], compute, x.device)
    elif out.shape != tuple(x.shape):
        raise _lib.M355Error(f"c8 slot shape {out.shape} != tensor shape {tuple(x.shape)}")
    check(_lib.lib().m355_act16_pack(_p(x), out.ptr(), N, Cc, out.S, xbs, out.batch_stride(), compute, _stream()),
          "act16_pack")
    return out


def as_f32(x):
    """fp32 NCDHW view of an activation (c8 activations are converted: the fallback for ops without a c8 kernel)."""
    return x.to_f32() if isinstance(x, Act16) else x


# Packed weights are cached per parameter VERSION: the kernels want the filter re-laid-out ([c][tap][o], 16-bit for
# the 16-bit modes, flipped / transposed for the data gradient) and the library used to repack before every
# launch (234 launches per profiled run).  Weights only change at optimizer.step(), which bumps `_version`.
PACK_CACHE = True
# 16-bit precision modes, training: the conv input / output gradient is packed to c8 once in the autograd function, and
# forward, data gradient and weight gradient run on the c8 entry points.  H16_TRAIN_C8ONLY: also keep activations AND
# activation gradients of ModularUNet / Block3d only in c8 while training (round 3: the fp32 tensors the twin flow keeps
# beside the c8 ones bound the 16-bit step); False: the round-2 twin flow
H16_TRAIN_C8ONLY = os.environ.get("M355_TRAIN_C8ONLY", "1") != "0"
_bn_sync_group = None      # (defined properly with batch_norm_sync below)

# fp16 carries activation gradients multiplied by a power of two (include/m355seg.h, "grad_scale"); bf16 has fp32's exponent
# range: always 1.  The scale belongs to ONE backward pass: every node of the c8 training flow holds the `GradScale` cell of
# the forward pass that created it (`grad_scale_scope`, opened by the models' forward), the node where the gradient ENTERS
# the flow (the output convolution's backward, `_UnpackFn`) resolves the value, every other node of that pass reads it --
# two models forwarded before either backward, or an ensemble member of another size, never see each other's scale
# (round 3 kept one process-wide number, set as a side effect of the softmax out conv's forward).
# FP16_GRAD_SCALE = "auto": the value is CALIBRATED on the gradient that enters: 2^round(log2(target / max|dL/dlogits|)),
# measured once per (head, shape) -- one host read -- and again after an overflow; so a mean-reduced loss (gradient
# ~1 / (N * voxels)), a sum-reduced one (~1) and a StochasticMatrix head all travel at max|g| ~ `target` = 16, three decimal
# orders below the fp16 maximum (normalisation backward multiplies by rstd) and four above its normal minimum.  While a
# hipGraph is being captured nothing can be read: the cached calibration is used, or the size-derived estimate
# 2^(floor(log2(N * voxels)) + 3) of a mean-type loss.  A number fixes the scale.
# Overflow: the kernels OR into a device word (m355_overflow_flag_set) when a scaled gradient had to be clamped or a
# parameter gradient came out non-finite; `fp16_overflow()` reads and clears it -- trainer.train_step then skips the
# optimizer step, and the next backward re-calibrates with a 4x lower target.
FP16_GRAD_SCALE = "auto"
FP16_CHECK_OVERFLOW = True          # trainer.train_step: read the overflow word after every fp16 backward (one host sync)
_FP16_TARGET_MAX = 16.0
_fp16_target = _FP16_TARGET_MAX     # max|g| * scale aimed at by the calibration (lowered after an overflow)
_fp16_clean_checks = 0
_fp16_calibration = {}              # (head id, gradient shape) -> scale
_last_scale = 2.0 ** 16             # the most recently resolved fp16 scale (ops.grad_scale: tests, reporting)


class GradScale:
    """the loss scale of one forward / backward pass of the c8 training flow"""
    __slots__ = ("value", "auto")

    def __init__(self):
        self.value = None     # resolved where the gradient enters the flow
        self.auto = None      # size-derived estimate, recorded by the head's forward

    def get(self, compute) -> float:
        if compute != _lib.COMPUTE_F16:
            return 1.0
        if self.value is not None:
            return self.value
        return self.auto if self.auto is not None else _last_scale

    def resolve(self, compute, grad: torch.Tensor, key) -> float:
        """called by an entry node with the fp32 gradient that is about to be packed"""
        global _last_scale
        if compute != _lib.COMPUTE_F16:
            return 1.0
        if self.value is None:
            if FP16_GRAD_SCALE != "auto":
                self.value = float(FP16_GRAD_SCALE)
            else:
                cal = _fp16_calibration.get(key)
                if cal is None and not torch.cuda.is_current_stream_capturing():
                    import math
                    amax = float(grad.detach().abs().max())
                    if math.isfinite(amax) and amax > 0.0:
                        cal = 2.0 ** min(24, max(-8, round(math.log2(_fp16_target / amax))))
                        _fp16_calibration[key] = cal
                if cal is None:
                    cal = self.auto if self.auto is not None else _last_scale
                self.value = cal
            _last_scale = self.value
        return self.value


_gs_default = GradScale()
_gs_current = None


def _gs() -> GradScale:
    """the cell of the forward pass being recorded (outside a `grad_scale_scope`: one process-wide cell, as in round 3)"""
    return _gs_current if _gs_current is not None else _gs_default


class grad_scale_scope:
    """`with grad_scale_scope():` around ONE forward pass (ModularUNet / NestedResUNet open it themselves): the c8 nodes
    created inside share a fresh GradScale cell.  Nested scopes (a model called by an ensemble that is itself inside a
    scope) keep the outer cell -- one loss, one scale."""

    def __enter__(self):
        global _gs_current
        self.prev = _gs_current
        if _gs_current is None:
            _gs_current = GradScale()
        return _gs_current

    def __exit__(self, *exc):
        global _gs_current
        _gs_current = self.prev


def grad_scale(compute) -> float:
    """the fp16 loss scale most recently resolved (1.0 for bf16)"""
    return _last_scale if compute == _lib.COMPUTE_F16 else 1.0


def _auto_grad_scale(n_elements) -> float:
    import math
    return 2.0 ** min(24, max(0, int(math.floor(math.log2(max(1, n_elements)))) + 3))


_overflow_words = {}   # device index -> int32 device word handed to the library (m355_overflow_flag_set)


def _overflow_word(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    w = _overflow_words.get(idx)
    if w is None and not torch.cuda.is_current_stream_capturing():
        w = torch.zeros(1, dtype=torch.int32, device=device)
        check(_lib.lib().m355_overflow_flag_set(_p(w), idx), "overflow_flag_set")
        _overflow_words[idx] = w
    return w


class _DeferredOverflow:
    """the overflow word of the LAST step on its way to the host (pinned copy + event): read when it has arrived, never
    waited for -- the scale adaptation may lag a step, the decision to skip does not (it is taken on the device)"""

    def __init__(self):
        self.host = None
        self.event = None
        self.armed = False


_deferred = {}      # device index -> _DeferredOverflow


def _adapt_after_overflow(hit: int):
    global _fp16_target, _fp16_clean_checks
    if hit:
        _fp16_calibration.clear()
        _fp16_target = max(_fp16_target / 4.0, 2.0 ** -6)
        _fp16_clean_checks = 0
    else:
        _fp16_clean_checks += 1
        if _fp16_clean_checks >= 200 and _fp16_target < _FP16_TARGET_MAX:
            _fp16_target = min(_FP16_TARGET_MAX, _fp16_target * 2.0)
            _fp16_calibration.clear()
            _fp16_clean_checks = 0


def fp16_found_inf(device) -> Optional[torch.Tensor]:
    """The overflow word as the `found_inf` tensor of torch's fused optimizers (float32, 1.0 = skip this step), WITHOUT a
    host synchronisation: torch.optim.SGD / Adam / AdamW built with fused=True take it (`optimizer.found_inf`, the protocol
    torch.cuda.amp.GradScaler uses) and leave parameters and optimizer state untouched on the device when it is set.  The
    word is cleared on the device; its value travels to the host asynchronously and lowers the loss-scale target when it
    has arrived (usually before the next backward).  None when no fp16 pass has run on this device."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    w = _overflow_words.get(idx)
    if w is None:
        return None
    d = _deferred.get(idx)
    if d is None:
        d = _deferred[idx] = _DeferredOverflow()
        d.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        d.event = torch.cuda.Event()
    elif d.armed and d.event.query():          # last step's word has arrived
        _adapt_after_overflow(int(d.host[0]))
        d.armed = False
    found = (w != 0).to(torch.float32).reshape(())       # 0-dim, as torch.cuda.amp.GradScaler hands it over
    if not d.armed:
        d.host.copy_(w, non_blocking=True)
        d.event.record()
        d.armed = True
    w.zero_()
    return found


def fp16_overflow(device=None) -> int:
    """Read and clear the overflow word of the fp16 training flow (one host synchronisation): non-zero when, since the last
    call, a loss-scaled gradient was clamped to the fp16 range (bit 0) or a parameter gradient came out non-finite (bit 1).  The caller
    skips its optimizer step; the next backward re-calibrates the scale with a 4x lower target (raised again, 2x per 200
    clean checks)."""
    hit = 0
    for idx, w in _overflow_words.items():
        if device is not None and device.index not in (None, idx):
            continue
        v = int(w.item())
        if v:
            w.zero_()
            hit |= v
    _adapt_after_overflow(hit)
    return hit
# an encoder block's last norm + activation pass also emits the AvgPool3d(2, 2) the next level consumes
FUSE_POOL = os.environ.get("M355_FUSE_POOL", "1") != "0"
# ... and its backward sums the skip gradient and the un-pooled gradient inside the two normalisation-backward passes
# (m355_norm_act_bwd_pool); 0: m355_avgpool3d_2x_bwd[_add] writes the sum first, the launches before that entry existed
FUSE_POOL_BWD = os.environ.get("M355_FUSE_POOL_BWD", "1") != "0"
# how often a backward took a fused path since import (the tests read and reset it)
fused_bwd_counts = {"pool": 0}


# Parameters that own packed forms (id -> weak reference).  optimizer.step changes every one of them at once; the first
# conv that then finds its weight stale re-packs ALL stale registered forms in one launch (m355_conv3d_pack_batch)
# instead of ~37 small packs spread over the step, each on the critical path in front of its conv.
_pack_registry = {}
PACK_BATCH = os.environ.get("M355_PACK_BATCH", "1") != "0"
# While a train step is being CAPTURED into a hipGraph the batched re-pack must contain exactly the captured model's
# forms: `pack_scope(params)` marks them stale (so the re-pack kernel is part of the captured step whatever ran before --
# another model's eager forward between this model's last optimizer step and the capture refreshes ALL stale registered
# forms, and a capture that then finds its weights "fresh" would replay with the packed weights of the capture step
# forever) and keeps other models' forms out of the graph.
_pack_scope = None


class pack_scope:
    def __init__(self, params):
        self.ids = {id(p) for p in params}
        self.params = list(params)

    def __enter__(self):
        global _pack_scope
        self.prev, _pack_scope = _pack_scope, self.ids
        for p in self.params:
            cache = getattr(p, "_m355_packed", None)
            if cache is not None:
                p._m355_packed = (-1, cache[1], cache[2])
        return self

    def __exit__(self, *exc):
        global _pack_scope
        _pack_scope = self.prev


def _repack_stale(L, device):
    """Refresh, in place and with one launch, every cached packed form whose parameter has a new version."""
    items = []
    for key, ref in list(_pack_registry.items()):
        if _pack_scope is not None and key not in _pack_scope:
            continue
        w = ref()
        cache = getattr(w, "_m355_packed", None) if w is not None else None
        if cache is None or cache[1] != w.data_ptr() or w.device != device:
            if w is None or cache is None or cache[1] != w.data_ptr():
                del _pack_registry[key]   # gone, or its storage moved: the per-weight path starts a new cache
            continue
        if cache[0] == w._version:
            continue
        for (which, *_), (buf, d) in cache[2].items():
            items.append(_lib.PackItem(d, which, w.data_ptr(), buf.data_ptr()))
        w._m355_packed = (w._version, cache[1], cache[2])
    if items:
        arr = (_lib.PackItem * len(items))(*items)
        check(L.m355_conv3d_pack_batch(C.cast(arr, C.c_void_p), len(items), _stream()), "conv3d_pack_batch")


def _packed_weight(weight, d, which):
    """-> (pointer argument, flags) for a conv entry point: the cached packed form of `weight` for descriptor
    `d` (which: 0 forward, 1 data gradient) with M355_CONV_W_PACKED, or the plain weight with flags 0."""
    if not PACK_CACHE:
        return weight, 0
    L = _lib.lib()
    ver, ptr = weight._version, weight.data_ptr()
    cache = getattr(weight, "_m355_packed", None)
    if (cache is not None and cache[0] != ver and cache[1] == ptr and PACK_BATCH and id(weight) in _pack_registry):
        _repack_stale(L, weight.device)   # a parameter after optimizer.step: all stale forms of all parameters at once
        cache = weight._m355_packed
    if cache is None or cache[0] != ver or cache[1] != ptr:
        cache = (ver, ptr, {})
        try:
            weight._m355_packed = cache
        except (AttributeError, RuntimeError):
            return weight, 0
    # The packed layout depends on the channel counts, the arithmetic and the kernel family only -- not on the spatial
    # extent or the batch: ONE buffer per (direction, family) serves every input shape (variable-size validation
    # volumes used to add a full copy of every weight per distinct shape, all re-packed after each optimizer.step).
    small = 1 if (which == 0 and d.Cout <= 4 and conv_plan(d, 0)[0] == 2) else 0   # Cout <= 4 forward: its own layout
    key = (which, d.Cin, d.Cout, d.compute, small)
    ent = cache[2].get(key)
    if ent is None:
        nbytes = L.m355_conv3d_packed_bytes(C.byref(d), which)
        if nbytes == 0:
            return weight, 0
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=weight.device)
        check(L.m355_conv3d_pack(C.byref(d), which, _p(weight), _p(buf), _stream()), "conv3d_pack")
        d0 = ConvDesc(d.N, d.Cin, d.Cout, d.D, d.H, d.W, d.k, d.stride, d.pad, d.out_pad, 0, 0, d.compute, 0)
        ent = cache[2][key] = (buf, d0)
        if weight.is_leaf and isinstance(weight, torch.nn.Parameter):   # (derived weights -- blur / WS -- are new tensors every step)
            _pack_registry[id(weight)] = weakref.ref(weight)
    return ent[0], _lib.CONV_W_PACKED


def _c8_twin(t, compute):
    """the c8 twin a producer pass attached to this fp32 tensor (norm_act forward / backward in the 16-bit
    training flow), if it describes exactly this tensor"""
    rec = getattr(t, "_m355_c8", None)
    if rec is None:
        return None
    tw, version = rec
    if (version == t._version and tw.compute == compute and tw.shape == tuple(t.shape) and tw.device == t.device):
        return tw
    return None   # (an in-place op on the fp32 tensor since the twin was written bumps _version: the twin is stale)


def _with_flags(d, flags):
    if flags == d.flags:
        return d
    return ConvDesc(d.N, d.Cin, d.Cout, d.D, d.H, d.W, d.k, d.stride, d.pad, d.out_pad, d.x_batch_stride,
                    d.y_batch_stride, d.compute, flags)


def _c8_channel_partials(x16: Act16, stats: dict):
    """statistics partials of a c8 tensor (pre-norm output of a conv without fused statistics)"""
    L = _lib.lib()
    N, Cc = x16.shape[:2]
    slots = int(L.m355_act16_partials_slots(x16.S))
    part = torch.empty((N, slots, Cc, 2), dtype=torch.float32, device=x16.device)
    check(L.m355_act16_channel_partials(x16.ptr(), x16.batch_stride(), N, Cc, x16.S, x16.compute, _p(part), _stream()),
          "act16_channel_partials")
    stats["partials"], stats["slots"] = part, slots


def _head_flag(d, softmax, sigmoid):
    """-> the descriptor flag of the hypothesis head the conv epilogue of `d` applies itself; 0: no head asked for, or the
    kernel variant has no epilogue (`_head_fwd` then runs as a pass of its own)"""
    L = _lib.lib()
    if softmax and L.m355_conv3d_fuses_softmax(C.byref(d)) != 0:
        return _lib.CONV_SOFTMAX
    if sigmoid and L.m355_conv3d_fuses_sigmoid(C.byref(d)) != 0:
        return _lib.CONV_SIGMOID
    return 0


def _head_fwd(x, softmax, inner=1, diag_bias=0.0):
    """nn.Softmax(dim=1) of the logits `x` (softmax; inner / diag_bias: StochasticMatrix) or nn.Sigmoid of them, as a pass"""
    x = x.contiguous()
    y = torch.empty_like(x)
    if softmax:
        N, Ctot = x.shape[0], x.shape[1]
        check(_lib.lib().m355_softmax_fwd(_p(x), _p(y), N, Ctot // inner, inner, x.numel() // (N * Ctot), float(diag_bias),
                                          _stream()), "softmax_fwd")
    else:
        check(_lib.lib().m355_sigmoid_fwd(_p(x), _p(y), x.numel(), _stream()), "sigmoid_fwd")
    return y


def _head_bwd(y, dy, softmax, inner=1):
    """dlogits from the saved head output: y * (dy - sum_c y dy) (softmax) or dy * y * (1 - y) (sigmoid)"""
    y, dy = y.contiguous(), dy.contiguous()
    dx = torch.empty_like(y)
    if softmax:
        N, Ctot = y.shape[0], y.shape[1]
        check(_lib.lib().m355_softmax_bwd(_p(y), _p(dy), _p(dx), N, Ctot // inner, inner, y.numel() // (N * Ctot), _stream()),
              "softmax_bwd")
    else:
        check(_lib.lib().m355_sigmoid_bwd(_p(y), _p(dy), _p(dx), y.numel(), _stream()), "sigmoid_bwd")
    return dx


def _conv3d_act16(x16: Act16, weight, bias, add, stats, out16: Optional[Act16], softmax=False, sigmoid=False):
    """3x3x3 / s1 / p1 forward on a c8 input, the one launch sequence of the no-grad c8 flow and of `_Conv3dC8Fn`.
    out16: the result (a pre-norm tensor) is written there by the conv epilogue, as c8 too; None: a fresh fp32 tensor,
    with `add` fused and nn.Softmax(dim=1) / nn.Sigmoid applied (the conv's epilogue where the kernel variant has one and
    neither `add` nor `stats` is in the way, else a separate pass).  `weight` is contiguous.  -> (result, descriptor)"""
    L = _lib.lib()
    _require(weight, bias, add)
    N, Cin, D, H, W = x16.shape
    Cout = weight.shape[0]
    d = _conv_desc(N, Cin, Cout, D, H, W, 3, 1, 1, 0, 0, compute=x16.compute)
    wbuf, flags = _packed_weight(weight, d, 0)
    head = softmax or sigmoid
    fused = _head_flag(d, softmax, sigmoid) if (head and out16 is None and add is None and stats is None) else 0
    dk = _with_flags(d, flags | fused)
    ws = _workspace(L.m355_conv3d_h16_workspace(C.byref(d), 0), x16.device)
    part = None
    slots = 0
    if stats is not None:
        slots = L.m355_conv3d_stats_slots(C.byref(d)) if out16 is None else L.m355_conv3d_stats_slots_c8(C.byref(d))
    if slots > 0:
        part = torch.empty((N, slots, Cout, 2), dtype=torch.float32, device=x16.device)
        stats["partials"], stats["slots"] = part, slots
    if out16 is not None:
        y = out16
        _conv_launch("conv3d_fwd", d, 0, 2, 2, L.m355_conv3d_fwd_h16_c8, C.byref(dk), x16.ptr(),
                     x16.batch_stride(), _p(wbuf), _p(bias), y.ptr(), y.batch_stride(), _p(part), _p(ws), ws.numel(), _stream())
        if stats is not None and slots == 0:
            _c8_channel_partials(y, stats)
        return y, d
    if add is not None:
        add = add.contiguous()
    y = torch.empty((N, Cout, D, H, W), dtype=torch.float32, device=x16.device)
    _conv_launch("conv3d_fwd", d, 0, 2, 4, L.m355_conv3d_fwd_h16, C.byref(dk), x16.ptr(), x16.batch_stride(),
                 _p(wbuf), _p(bias), _p(add), _p(y), _p(part), _p(ws), ws.numel(), _stream())
    if head and not fused:
        y = _head_fwd(y, softmax)
    return y, d


# ------------------------------------------------- c8-only TRAINING flow (16-bit modes, autograd on)
# Activations and their gradients are [N, CB, S, 8] 16-bit tensors (the c8 layout) on BOTH sides of every function:
# forward kernels as in the no-grad flow, backward kernels from csrc/train16.hip / convt.hip (include/m355seg.h,
# "c8-only TRAINING flow").  An `Act16` carries the autograd handle `t` of its tensor; the functions read their
# operands through the `Act16` objects in `meta` (pointers, batch strides) and take the handles only as graph edges.
def _c8t(t):
    """(tensor, batch stride) of a [N, CB, S, 8] c8 tensor whose samples are dense -- a slot alias or a slice of a
    gradient buffer along the block axis; anything else (overlapping samples, such as a batch-expanded gradient with
    stride 0, included) is compacted first"""
    N, CB, S, _ = t.shape
    st = t.stride()
    if (st[3] != 1 or st[2] != 8 or (CB > 1 and st[1] != S * 8)
            or (N > 1 and (st[0] % 8 or st[0] < CB * S * 8))):
        t = t.contiguous()
        return t, CB * S * 8
    return t, (st[0] if N > 1 else CB * S * 8)


def _pack_scaled(x, compute, scale):
    """fp32 NCDHW gradient -> dense c8 tensor, multiplied by the loss scale of the mode"""
    x, xbs = _dense_channels(x)
    N, Cc = x.shape[:2]
    S = x.shape[2] * x.shape[3] * x.shape[4]
    out = _c8_grad(N, Cc, S, compute, x.device)
    check(_lib.lib().m355_act16_pack_scaled(_p(x), _p(out), N, Cc, S, xbs, 0, compute, float(scale), _stream()),
          "act16_pack_scaled")
    return out


def _unpack_scaled(t, Cc, spatial, compute, scale):
    t, bs = _c8t(t)
    N, S = t.shape[0], t.shape[2]
    x = torch.empty((N, Cc) + tuple(spatial), dtype=torch.float32, device=t.device)
    check(_lib.lib().m355_act16_unpack_scaled(_p(t), _p(x), N, Cc, S, bs, 0, compute, float(scale), _stream()),
          "act16_unpack_scaled")
    return x


class _PackFn(torch.autograd.Function):
    """fp32 NCDHW -> c8 (the generic entry of a tensor into the c8 training flow); backward: the c8 gradient back to
    fp32, loss scale removed"""

    @staticmethod
    def forward(ctx, x, out: Act16):
        _require(x)
        xd, xbs = _dense_channels(x)
        N, Cc = xd.shape[:2]
        check(_lib.lib().m355_act16_pack(_p(xd), out.ptr(), N, Cc, out.S, xbs, out.batch_stride(), out.compute, _stream()),
              "act16_pack")
        ctx.info = (Cc, out.spatial, out.compute)
        ctx.gs = _gs()
        return out.alias()

    @staticmethod
    def backward(ctx, dy16):
        Cc, spatial, compute = ctx.info
        return _unpack_scaled(dy16, Cc, spatial, compute, 1.0 / ctx.gs.get(compute)), None


class _UnpackFn(torch.autograd.Function):
    """c8 -> fp32 NCDHW (ops without a c8 kernel: trilinear upsampling, dropout, space-to-depth ...); backward: the fp32
    gradient enters the c8 flow (loss scale applied)"""

    @staticmethod
    def forward(ctx, t, a: Act16):
        N = a.data.shape[0]
        x = torch.empty((N, a.C) + a.spatial, dtype=torch.float32, device=a.device)
        check(_lib.lib().m355_act16_unpack(a.ptr(), _p(x), N, a.C, a.S, a.batch_stride(), 0, a.compute, _stream()),
              "act16_unpack")
        ctx.compute = a.compute
        ctx.gs = _gs()
        if a.compute == _lib.COMPUTE_F16:
            _overflow_word(a.device)
        return x

    @staticmethod
    def backward(ctx, dy):
        # (a gradient ENTERS the c8 flow here: this node may be the one that fixes the scale of the pass)
        scale = ctx.gs.resolve(ctx.compute, dy, ("unpack", tuple(dy.shape)))
        return _pack_scaled(dy, ctx.compute, scale), None


@dataclass
class _C8ConvMeta:
    x16: "Act16"                      # the whole (possibly concatenated) conv input
    part_blocks: Sequence[int]        # channel blocks of each autograd part of it
    out16: Optional["Act16"] = None   # c8 destination; None: fp32 NCDHW result (the out conv), optionally with its head
    softmax: bool = False
    sigmoid: bool = False
    stats: Optional[dict] = None
    has_add: bool = False


class _Conv3dC8Fn(torch.autograd.Function):
    """3x3x3 / s1 / p1 convolution of the c8 training flow: c8 in -> c8 out (pre-norm tensor, statistics fused), or
    -> fp32 (+ softmax) for the output convolution.  Backward: weight / bias gradient from the two c8 operands
    (m355_conv3d_bwd_weight_c8), data gradient c8 -> c8 (m355_conv3d_bwd_data_h16_c8) sliced per concat part."""

    @staticmethod
    def forward(ctx, weight, bias, add, meta: _C8ConvMeta, *part_ts):
        x16 = meta.x16
        weight = weight.contiguous()
        out, d = _conv3d_act16(x16, weight, bias, add, meta.stats, meta.out16, meta.softmax, meta.sigmoid)
        if meta.out16 is not None:
            out = meta.out16.alias()
        elif x16.compute == _lib.COMPUTE_F16:     # the head of an fp16 pass: size-derived estimate (capture fallback)
            _gs().auto = _auto_grad_scale(d.N * d.D * d.H * d.W)
            _overflow_word(x16.device)
        ctx.meta, ctx.desc = meta, d
        ctx.gs = _gs()
        ctx.has_bias = bias is not None
        xa = x16.alias()
        if meta.softmax or meta.sigmoid:
            ctx.save_for_backward(xa, weight, out)
        else:
            ctx.save_for_backward(xa, weight)
        return out

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        meta, d = ctx.meta, ctx.desc
        compute = d.compute
        if meta.softmax or meta.sigmoid:
            xa, weight, y = ctx.saved_tensors
            dy = _head_bwd(y, dy, meta.softmax)
        else:
            xa, weight = ctx.saved_tensors
        dadd = dy if (meta.has_add and ctx.needs_input_grad[2]) else None
        if meta.out16 is None:   # the gradient enters the c8 flow here: this node fixes the scale of the pass
            key = (id(weight), tuple(dy.shape), "sigmoid") if meta.sigmoid else (id(weight), tuple(dy.shape))
            scale = ctx.gs.resolve(compute, dy, key)
            dy16 = _pack_scaled(dy, compute, scale)
        else:
            scale = ctx.gs.get(compute)
            dy16 = dy
        dy16, dybs = _c8t(dy16)
        xa, xbs = _c8t(xa)
        need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and ctx.has_bias
        need_x = any(ctx.needs_input_grad[4:])
        S = d.D * d.H * d.W
        dw = db = None
        if need_w or need_b:
            dw = torch.empty_like(weight)
            db = torch.empty(d.Cout, dtype=weight.dtype, device=weight.device) if ctx.has_bias else None
            ws = _workspace(L.m355_conv3d_bwd_weight_c8_workspace(C.byref(d)), weight.device)
            _conv_launch("conv3d_bwd_weight", d, None, 2, 2, L.m355_conv3d_bwd_weight_c8, C.byref(d), _p(xa), xbs,
                         _p(dy16), dybs, _p(dw), _p(db), 1.0 / scale, _p(ws), ws.numel(), _stream())
        dparts: List[Optional[torch.Tensor]] = [None] * len(meta.part_blocks)
        if need_x:
            dx16 = _c8_grad(d.N, d.Cin, S, compute, weight.device)
            wbuf, flags = _packed_weight(weight, d, 1)
            ws = _workspace(L.m355_conv3d_h16_workspace(C.byref(d), 1), weight.device)
            _conv_launch("conv3d_bwd_data", d, 1, 2, 2, L.m355_conv3d_bwd_data_h16_c8, C.byref(_with_flags(d, flags)),
                         _p(dy16), dybs, _p(wbuf), _p(dx16), 0, _p(ws), ws.numel(), _stream())
            b0 = 0
            for i, nb in enumerate(meta.part_blocks):
                if ctx.needs_input_grad[4 + i]:
                    dparts[i] = dx16 if len(meta.part_blocks) == 1 else dx16[:, b0:b0 + nb]
                b0 += nb
        return (dw if need_w else None, db if need_b else None, dadd, None, *dparts)


def _conv3d_c8_train(x16: Act16, parts, weight, bias, add, stats, out16, softmax, sigmoid):
    """`_conv3d_act16` while autograd records (c8 training flow)"""
    if parts is None:
        parts = [x16]
    if any(p.C % 8 for p in parts[:-1]):
        raise _lib.M355Error("c8 training flow: concat parts must be whole channel blocks")
    meta = _C8ConvMeta(x16, [p.CB for p in parts], out16=out16, softmax=softmax, sigmoid=sigmoid, stats=stats,
                       has_add=add is not None)
    out = _Conv3dC8Fn.apply(weight, bias, add, meta, *[p.t for p in parts])
    return out if out16 is None else out16.with_t(out)


@dataclass
class _C8NormMeta:
    x16: "Act16"
    add16: Optional["Act16"]
    out16: Optional["Act16"]
    cfg: "NormCfg"
    pool: bool = False
    pooled16: Optional["Act16"] = None


class _NormActC8Fn(torch.autograd.Function):
    """normalisation + activation (+ residual add) of the c8 training flow, c8 -> c8; optionally nn.AvgPool3d(2, 2) of
    the result as a second output (an encoder block's output feeds the skip connection and the next level).  Backward:
    ONE call of m355_norm_act_bwd_c8, which also sums the skip-path and the un-pooled gradient."""

    @staticmethod
    def forward(ctx, x_t, gamma, beta, add_t, meta: _C8NormMeta):
        L = _lib.lib()
        x, cfg = meta.x16, meta.cfg
        _require(gamma, beta)
        N, Cc, spatial, S = x.shape[0], x.C, x.spatial, x.S
        out16 = meta.out16
        d = NormDesc(N, Cc, S, cfg.groups, cfg.act, cfg.eps, cfg.slope, 0, 0, 0)
        use_batch = cfg.groups > 0 or cfg.training or cfg.running_mean is None
        if use_batch and not (cfg.stats and cfg.stats.get("partials") is not None):
            cfg.stats = {} if cfg.stats is None else cfg.stats
            _c8_channel_partials(x, cfg.stats)
        mean, rstd, use_batch = _norm_statistics(L, d, None, cfg, N, Cc, device=x.device)
        a16 = meta.add16
        check(L.m355_norm_act_fwd_c8(C.byref(d), x.ptr(), x.batch_stride(), _p(mean), _p(rstd), _p(gamma), _p(beta),
                                     a16.ptr() if a16 is not None else None, a16.batch_stride() if a16 is not None else 0,
                                     out16.ptr(), out16.batch_stride(), x.compute, _stream()), "norm_act_fwd_c8")
        ctx.desc, ctx.batch_stats, ctx.has_add, ctx.has_affine = d, use_batch, a16 is not None, gamma is not None
        ctx.compute, ctx.spatial = x.compute, spatial
        ctx.gs = _gs()
        ctx.sync = cfg.sync             # synchronised batch norm: (process group, element count over all ranks)
        ctx.save_for_backward(x.alias(), mean, rstd, gamma, beta)
        if not meta.pool:
            return out16.alias()
        D, H, W = spatial
        p16 = meta.pooled16
        check(L.m355_avgpool3d_2x_fwd_h16(out16.ptr(), p16.ptr(), N, Cc, D, H, W, out16.batch_stride(), p16.batch_stride(),
                                          x.compute, _stream()), "avgpool3d_2x_fwd_h16")
        return out16.alias(), p16.alias()

    @staticmethod
    def backward(ctx, dy16, dpool16=None):
        L = _lib.lib()
        xa, mean, rstd, gamma, beta = ctx.saved_tensors
        d = ctx.desc
        compute = ctx.compute
        xa, xbs = _c8t(xa)
        dyb = dpb = 0
        if dy16 is not None:
            dy16, dyb = _c8t(dy16)
        if dpool16 is not None:
            dpool16, dpb = _c8t(dpool16)
        dx16 = torch.empty((d.N, (d.C + 7) // 8, d.S, 8), dtype=_DT16[compute], device=xa.device)
        dgamma = torch.empty(d.C, dtype=torch.float32, device=xa.device) if ctx.has_affine else None
        dbeta = torch.empty(d.C, dtype=torch.float32, device=xa.device) if ctx.has_affine else None
        ws = _workspace(L.m355_norm_workspace(C.byref(d)), xa.device)
        D, H, W = ctx.spatial
        training, unscale = 1 if ctx.batch_stats else 0, 1.0 / ctx.gs.get(compute)
        if ctx.sync is not None:        # the two halves around the all-reduce of the per-channel gradient means
            import torch.distributed as dist
            group, total = ctx.sync
            stat_m = torch.empty(2 * d.C, dtype=torch.float32, device=xa.device)
            check(L.m355_norm_act_bwd_c8_reduce(C.byref(d), _p(xa), xbs, _p(dy16), dyb, _p(dpool16), dpb, D, H, W, _p(mean),
                                                _p(rstd), _p(gamma), _p(beta), _p(dgamma), _p(dbeta), training, _p(total),
                                                unscale, _p(stat_m), compute, _p(ws), ws.numel(), _stream()),
                  "norm_act_bwd_c8_reduce")
            dist.all_reduce(stat_m, group=group)
            check(L.m355_norm_act_bwd_c8_apply(C.byref(d), _p(xa), xbs, _p(dy16), dyb, _p(dpool16), dpb, D, H, W, _p(mean),
                                               _p(rstd), _p(gamma), _p(beta), _p(stat_m), _p(dx16), 0, compute, _stream()),
                  "norm_act_bwd_c8_apply")
        else:
            check(L.m355_norm_act_bwd_c8(C.byref(d), _p(xa), xbs, _p(dy16), dyb, _p(dpool16), dpb, D, H, W, _p(mean), _p(rstd),
                                         _p(gamma), _p(beta), _p(dx16), 0, _p(dgamma), _p(dbeta), training, unscale, compute,
                                         _p(ws), ws.numel(), _stream()), "norm_act_bwd_c8")
        dadd = dy16 if (ctx.has_add and ctx.needs_input_grad[3]) else None
        # (x_t is None for the output of a convolution without history -- frozen weight and bias on the network input: autograd
        # refuses a gradient for an input that was not a tensor)
        return dx16 if ctx.needs_input_grad[0] else None, dgamma, dbeta, dadd, None


def _norm_act_c8_train(x: Act16, gamma, beta, add, cfg: "NormCfg", pool=False):
    out16 = cfg.out.act16() if cfg.out is not None else None
    if out16 is not None and out16.shape != x.shape:
        raise _lib.M355Error(f"c8 slot shape {out16.shape} != op output shape {x.shape}")
    add16 = None
    if add is not None:
        add16 = add if isinstance(add, Act16) else pack_act16(add, x.compute)
    if out16 is None:
        out16 = Act16.empty(x.shape[0], x.C, x.spatial, x.compute, x.device)
    pooled16 = None
    if pool:
        D, H, W = x.spatial
        pooled16 = Act16.empty(x.shape[0], x.C, (D // 2, H // 2, W // 2), x.compute, x.device)
    meta = _C8NormMeta(x, add16, out16, cfg, pool, pooled16)
    res = _NormActC8Fn.apply(x.t, gamma, beta, add16.t if add16 is not None else None, meta)
    o = meta.out16
    if pool:
        y = Act16(o.data, o.C, o.spatial, o.compute, o.cb0, res[0])
        p = meta.pooled16
        return y, Act16(p.data, p.C, p.spatial, p.compute, p.cb0, res[1])
    return Act16(o.data, o.C, o.spatial, o.compute, o.cb0, res)


def _convt_c8_fwd(x: Act16, weight, bias, y16: Act16):
    """The c8 -> c8 launch of nn.ConvTranspose3d(kernel_size=2, stride=2) into y16; returns the descriptor."""
    _require(weight, bias)
    N, Cin, D, H, W = x.shape
    d = _conv_desc(N, Cin, weight.shape[1], D, H, W, 2, 2, 0, 0, 0)
    check(_lib.lib().m355_conv_transpose3d_fwd_h16(C.byref(d), x.ptr(), x.batch_stride(), _p(weight), _p(bias), y16.ptr(),
                                                   y16.batch_stride(), x.compute, _stream()), "conv_transpose3d_fwd_h16")
    return d


class _ConvTC8Fn(torch.autograd.Function):
    """nn.ConvTranspose3d(kernel_size=2, stride=2) of the c8 training flow: c8 -> c8 straight into its concat slot;
    backward on the 16-bit MFMA from c8 operands where the library has the kernels (Cout <= 128), else through the
    fp32 kernels (the deepest levels: a few MB)."""

    @staticmethod
    def forward(ctx, x_t, weight, bias, x: Act16, y16: Act16):
        weight = weight.contiguous()
        ctx.desc, ctx.compute, ctx.has_bias = _convt_c8_fwd(x, weight, bias, y16), x.compute, bias is not None
        ctx.gs = _gs()
        ctx.save_for_backward(x.alias(), weight)
        return y16.alias()

    @staticmethod
    def backward(ctx, dy16):
        L = _lib.lib()
        xa, weight = ctx.saved_tensors
        d, compute = ctx.desc, ctx.compute
        scale = ctx.gs.get(compute)
        dy16, dybs = _c8t(dy16)
        xa, xbs = _c8t(xa)
        S = d.D * d.H * d.W
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        dx16 = dw = db = None
        if L.m355_conv_transpose3d_h16_bwd_supported(C.byref(d)):
            if need_x:
                dx16 = _c8_grad(d.N, d.Cin, S, compute, weight.device)
                check(L.m355_conv_transpose3d_bwd_data_h16(C.byref(d), _p(dy16), dybs, _p(weight), _p(dx16), 0, compute,
                                                           _stream()), "conv_transpose3d_bwd_data_h16")
            if need_w:
                dw = torch.empty_like(weight)
                db = torch.empty(d.Cout, dtype=weight.dtype, device=weight.device) if ctx.has_bias else None
                ws = _workspace(L.m355_conv_transpose3d_h16_bwd_workspace(C.byref(d)), weight.device)
                check(L.m355_conv_transpose3d_bwd_weight_h16(C.byref(d), _p(xa), xbs, _p(dy16), dybs, _p(dw), _p(db),
                                                             1.0 / scale, compute, _p(ws), ws.numel(), _stream()),
                      "conv_transpose3d_bwd_weight_h16")
        else:
            dy = _unpack_scaled(dy16, d.Cout, (2 * d.D, 2 * d.H, 2 * d.W), compute, 1.0 / scale)
            ws = _workspace(L.m355_conv_transpose3d_workspace(C.byref(d)), weight.device)
            if need_x:
                dx = torch.empty((d.N, d.Cin, d.D, d.H, d.W), dtype=torch.float32, device=weight.device)
                check(L.m355_conv_transpose3d_bwd_data(C.byref(d), _p(dy), _p(weight), _p(dx), _p(ws), ws.numel(), _stream()),
                      "conv_transpose3d_bwd_data")
                dx16 = _pack_scaled(dx, compute, scale)
            if need_w:
                x = _unpack_scaled(xa, d.Cin, (d.D, d.H, d.W), compute, 1.0)
                dw = torch.empty_like(weight)
                db = torch.empty(d.Cout, dtype=weight.dtype, device=weight.device) if ctx.has_bias else None
                check(L.m355_conv_transpose3d_bwd_weight(C.byref(d), _p(x), _p(dy), _p(dw), _p(db), _p(ws), ws.numel(),
                                                         _stream()), "conv_transpose3d_bwd_weight")
        return dx16, dw, db, None, None


def _act16_tracks(*xs):
    """autograd is recording and one of these c8 activations carries a gradient"""
    return torch.is_grad_enabled() and any(isinstance(x, Act16) and x.requires_grad for x in xs)


def _tracks_any(*ts):
    """one of these tensors (parameters: weight, bias; a fused fp32 `add`) requires grad -- a frozen weight with a
    trainable bias still needs the autograd function"""
    return any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


# ------------------------------------------------------------------ conv3d
@dataclass
class _ConvMeta:
    k: int
    stride: int
    pad: int
    catbuf: Optional[torch.Tensor] = None
    out: Optional[OutSlot] = None
    tag: str = "conv3d"
    stats: Optional[dict] = None   # filled with {"partials", "slots"} when the statistics are fused
    softmax: bool = False          # Softmax(dim=1) over the output channels fused into this op (out conv + hypothesis)
    sigmoid: bool = False          # ... or Sigmoid, per element
    h16_train: int = 0             # set by the forward: the 16-bit compute code when the c8 training flow ran


def _conv_desc(N, Cin, Cout, D, H, W, k, stride, pad, xbs, ybs, out_pad=0, compute=0):
    return ConvDesc(N, Cin, Cout, D, H, W, k, stride, pad, out_pad, xbs, ybs, compute, 0)


def conv_plan(desc, which=0):
    """(mfma, ntw, gx, ksplit) of the kernel variant the library picks (profiling only)."""
    out = (C.c_int32 * 4)()
    check(_lib.lib().m355_conv3d_plan(C.byref(desc), which, out), "conv3d_plan")
    return tuple(out)


class _Conv3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, bias, add, meta: _ConvMeta, *parts):
        L = _lib.lib()
        x = meta.catbuf if meta.catbuf is not None else parts[0]
        _require(x, weight, bias, add)
        x, xbs = _dense_channels(x)
        weight = weight.contiguous()
        N, Cin, D, H, W = x.shape
        Cout, k = weight.shape[0], meta.k
        od = lambda n: (n + 2 * meta.pad - k) // meta.stride + 1
        oshape = (N, Cout, od(D), od(H), od(W))
        y = _alloc_out(meta.out, oshape, x)
        y, ybs = _dense_channels(y)
        if add is not None:
            add, abs_ = _dense_channels(add)
            if abs_ != ybs:
                add = add.contiguous()
                if ybs != Cout * oshape[2] * oshape[3] * oshape[4]:
                    raise _lib.M355Error("conv3d: a fused `add` needs the output's batch stride (write to a dense "
                                         "tensor and copy_into the slot instead)")
        d = _conv_desc(N, Cin, Cout, D, H, W, k, meta.stride, meta.pad, xbs, ybs, compute=_COMPUTE[_compute_mode])
        wbuf, flags = _packed_weight(weight, d, 0)
        head = meta.softmax or meta.sigmoid
        fused = _head_flag(d, meta.softmax, meta.sigmoid) if head else 0
        dk = _with_flags(d, flags | fused)
        # 16-bit training flow: the conv input is packed to c8 ONCE here (the library would stage the same copy
        # internally), consumed by the forward kernel and kept for the weight gradient (m355_conv3d_bwd_weight_h16
        # reads both operands as c8); the fp32 input is then not saved at all
        x16 = None
        if (d.compute in _DT16 and k == 3 and meta.stride == 1 and meta.pad == 1
                and Cin > 4 and Cout > 4 and not meta.softmax and not meta.sigmoid and D * H * W * 64 < 2 ** 31
                and ctx.needs_input_grad[0]):
            x16 = _c8_twin(x, d.compute)
            if x16 is None:
                x16 = pack_act16(x, d.compute)
            meta.h16_train = d.compute
        ws = _workspace(L.m355_conv3d_h16_workspace(C.byref(d), 0) if x16 is not None
                        else L.m355_conv3d_fwd_workspace(C.byref(d)), x.device)
        # statistics of the following normalisation fused into the conv epilogue (per-wave partials)
        slots = L.m355_conv3d_stats_slots(C.byref(d)) if meta.stats is not None else 0
        part = None
        if slots > 0:
            part = torch.empty((N, slots, Cout, 2), dtype=torch.float32, device=x.device)
            meta.stats["partials"], meta.stats["slots"] = part, slots
        if x16 is not None:
            _conv_launch("conv3d_fwd", d, 0, 4, 4, L.m355_conv3d_fwd_h16, C.byref(dk), x16.ptr(), x16.batch_stride(),
                         _p(wbuf), _p(bias), _p(add), _p(y), _p(part), _p(ws), ws.numel(), _stream())
        elif part is not None:
            _conv_launch("conv3d_fwd", d, 0, 4, 4, L.m355_conv3d_fwd_stats, C.byref(dk), _p(x), _p(wbuf), _p(bias),
                         _p(add), _p(y), _p(part), _p(ws), ws.numel(), _stream())
        else:
            _conv_launch("conv3d_fwd", d, 0, 4, 4, L.m355_conv3d_fwd, C.byref(dk), _p(x), _p(wbuf), _p(bias), _p(add),
                         _p(y), _p(ws), ws.numel(), _stream())
        if head and not fused:   # kernel variants without the fused epilogue: a separate pass
            y = _head_fwd(y, meta.softmax)
        ctx.meta, ctx.desc = meta, d
        ctx.has_bias, ctx.has_add = bias is not None, add is not None
        ctx.part_channels = [p.shape[1] for p in parts]
        ctx.x16 = None
        if meta.softmax or meta.sigmoid:
            ctx.save_for_backward(x, weight, y)
        elif x16 is not None:
            ctx.x16 = (x16.C, x16.spatial, x16.compute)
            ctx.x_meta = (x.dtype, x.device)
            ctx.save_for_backward(x16.data, weight)
        else:
            ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        meta = ctx.meta
        d = ctx.desc
        if meta.softmax or meta.sigmoid:
            x, weight, y = ctx.saved_tensors
            dy = _head_bwd(y, dy, meta.softmax)
        else:
            x, weight = ctx.saved_tensors
        dy, dybs = _dense_channels(dy)
        if dybs != d.y_batch_stride:
            d = _conv_desc(d.N, d.Cin, d.Cout, d.D, d.H, d.W, d.k, d.stride, d.pad, d.x_batch_stride, dybs, compute=d.compute)
        need_w, need_b, need_add = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        need_x = any(ctx.needs_input_grad[4:])
        dw = db = dadd = None
        dparts: List[Optional[torch.Tensor]] = [None] * len(ctx.part_channels)
        x16 = dy16 = None
        if ctx.x16 is not None:   # 16-bit training flow: `x` is the saved c8 conv input; dy is packed once for both gradients
            x16 = Act16(x, *ctx.x16)
            x_dtype, x_device = ctx.x_meta
            dy16 = _c8_twin(dy, x16.compute)
            if dy16 is None:
                dy16 = pack_act16(dy, x16.compute)
        else:
            x_dtype, x_device = x.dtype, x.device
        # (the records of this function count 4-byte elements on both sides, whichever operands the kernels read)
        if need_w or (need_b and ctx.has_bias):
            dw = torch.empty_like(weight)
            db = torch.empty(d.Cout, dtype=weight.dtype, device=weight.device) if ctx.has_bias else None
            if x16 is not None:
                ws = _workspace(L.m355_conv3d_bwd_weight_h16_workspace(C.byref(d)), x_device)
                _conv_launch("conv3d_bwd_weight", d, None, 4, 4, L.m355_conv3d_bwd_weight_h16, C.byref(d), x16.ptr(),
                             x16.batch_stride(), dy16.ptr(), dy16.batch_stride(), _p(dy) if db is not None else None,
                             _p(dw), _p(db), _p(ws), ws.numel(), _stream())
            else:
                ws = _workspace(L.m355_conv3d_bwd_weight_workspace(C.byref(d)), x_device)
                _conv_launch("conv3d_bwd_weight", d, 2, 4, 4, L.m355_conv3d_bwd_weight, C.byref(d), _p(x), _p(dy),
                             _p(dw), _p(db), _p(ws), ws.numel(), _stream())
        if need_x:
            # gradient w.r.t. the (possibly concatenated) input, dense, then sliced per part
            dx = torch.empty((d.N, d.Cin, d.D, d.H, d.W), dtype=x_dtype, device=x_device)
            dd = _conv_desc(d.N, d.Cin, d.Cout, d.D, d.H, d.W, d.k, d.stride, d.pad, 0, d.y_batch_stride, compute=d.compute)
            wbuf, flags = _packed_weight(weight, dd, 1)
            ddk = _with_flags(dd, flags)
            if dy16 is not None:
                ws = _workspace(L.m355_conv3d_h16_workspace(C.byref(dd), 1), x_device)
                _conv_launch("conv3d_bwd_data", dd, 1, 4, 4, L.m355_conv3d_bwd_data_h16, C.byref(ddk), dy16.ptr(),
                             dy16.batch_stride(), _p(wbuf), _p(dx), _p(ws), ws.numel(), _stream())
            else:
                ws = _workspace(L.m355_conv3d_bwd_data_workspace(C.byref(dd)), x_device)
                _conv_launch("conv3d_bwd_data", dd, 1, 4, 4, L.m355_conv3d_bwd_data, C.byref(ddk), _p(dy), _p(wbuf),
                             _p(dx), _p(ws), ws.numel(), _stream())
            c0 = 0
            for i, cc in enumerate(ctx.part_channels):
                if ctx.needs_input_grad[4 + i]:
                    dparts[i] = dx if len(ctx.part_channels) == 1 else dx[:, c0:c0 + cc]
                c0 += cc
        if need_add and ctx.has_add:
            dadd = dy
        return (dw if need_w else None, db if need_b else None, dadd, None, *dparts)


def conv3d(x, weight, bias=None, add=None, stride=1, padding=1, out: Optional[OutSlot] = None,
           stats: Optional[dict] = None, c8_out: bool = False, softmax: bool = False, sigmoid: bool = False):
    """nn.Conv3d forward (cubic kernel).  `x` is a tensor or a `Concat`; `add` is fused
    into the epilogue (y = conv(x) + bias + add).  `stats`: an empty dict asks the kernel to also
    emit the partial sums the following normalisation needs (filled in when the kernel variant
    supports it; pass it on as `NormCfg.stats`).  `c8_out`: in the c8 flow (x is an `Act16`) return the result
    as an `Act16` written by the conv epilogue (for the normalisation pass that follows).  `softmax`: apply
    nn.Softmax(dim=1) to the result (fused into the conv epilogue where the kernel variant allows); `sigmoid`: apply
    nn.Sigmoid to it, the same way.  The two exclude each other."""
    if softmax and sigmoid:
        raise ValueError("conv3d: softmax and sigmoid exclude each other (one hypothesis head per output convolution)")
    head = softmax or sigmoid
    k = weight.shape[2]
    if not (weight.shape[2] == weight.shape[3] == weight.shape[4]):
        raise NotImplementedError("only cubic kernels are supported")
    c8_parts = None
    if isinstance(x, Concat) and isinstance(x.buf, Act16):
        c8_parts, x = x.parts, x.buf
    if out is not None and out.buf16 is not None:   # c8 flow: the destination slot only exists in c8
        return pack_act16(conv3d(x, weight, bias, add, stride, padding, None, stats), out.buf16.compute, out.act16())
    if isinstance(x, Act16):
        if k == 3 and stride == 1 and padding == 1:
            # (a conv with a fused fp32 `add`, or with a head, keeps its result in fp32)
            out16 = _c8_out_slot(x, None, x.spatial, C=weight.shape[0]) if (c8_out and not head and add is None) else None
            add32 = as_f32(add) if add is not None else None
            if torch.is_grad_enabled() and (_tracks_any(weight, bias, add) or _act16_tracks(x, add, *(c8_parts or ()))):
                return _conv3d_c8_train(x, c8_parts, weight, bias, add32, stats, out16, softmax, sigmoid)   # c8 training flow
            return _conv3d_act16(x, weight.contiguous(), bias, add32, stats, out16, softmax, sigmoid)[0]
        if c8_parts is not None and _act16_tracks(*c8_parts):
            raise NotImplementedError("c8 training flow: only 3x3x3 / stride 1 / padding 1 convolutions read a concat buffer")
        x = x.to_f32()
    if isinstance(x, Concat):
        meta = _ConvMeta(k, stride, padding, catbuf=x.buf, out=out, stats=stats, softmax=softmax, sigmoid=sigmoid)
        y = _Conv3dFn.apply(weight, bias, add, meta, *x.parts)
    else:
        meta = _ConvMeta(k, stride, padding, out=out, stats=stats, softmax=softmax, sigmoid=sigmoid)
        y = _Conv3dFn.apply(weight, bias, add, meta, x)
    if meta.h16_train and add is None:
        # 16-bit training flow: the normalisation that follows may emit its input gradient (= this conv's output
        # gradient) as c8 in the same pass (m355_norm_act_bwd_h16) -- not with a fused residual `add`, whose
        # gradient is the same tensor and goes elsewhere
        y._m355_c8_grad = meta.h16_train
    return y


# -------------------------------------------------------- conv-transpose3d
class _ConvT3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, meta):
        L = _lib.lib()
        _require(x, weight, bias)
        k, stride, pad, out_pad, out = meta
        x, xbs = _dense_channels(x)
        weight = weight.contiguous()
        N, Cin, D, H, W = x.shape
        Cout = weight.shape[1]
        od = lambda n: (n - 1) * stride - 2 * pad + k + out_pad
        oshape = (N, Cout, od(D), od(H), od(W))
        y = _alloc_out(out, oshape, x)
        y, ybs = _dense_channels(y)
        # (the fp32 entry points honour M355_COMPUTE_F32X3 -- the k2 s2 forward on the split kernels -- and ignore the 16-bit codes)
        d = _conv_desc(N, Cin, Cout, D, H, W, k, stride, pad, xbs, ybs, out_pad, compute=_COMPUTE[_compute_mode])
        ws = _workspace(L.m355_conv_transpose3d_workspace(C.byref(d)), x.device)
        check(L.m355_conv_transpose3d_fwd(C.byref(d), _p(x), _p(weight), _p(bias), _p(y), _p(ws), ws.numel(),
                                          _stream()), "conv_transpose3d_fwd")
        ctx.desc, ctx.has_bias = d, bias is not None
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        x, weight = ctx.saved_tensors
        d = ctx.desc
        dy, dybs = _dense_channels(dy)
        d = _conv_desc(d.N, d.Cin, d.Cout, d.D, d.H, d.W, d.k, d.stride, d.pad, d.x_batch_stride, dybs, d.out_pad, compute=d.compute)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((d.N, d.Cin, d.D, d.H, d.W), dtype=x.dtype, device=x.device)
            dd = _conv_desc(d.N, d.Cin, d.Cout, d.D, d.H, d.W, d.k, d.stride, d.pad, 0, dybs, d.out_pad, compute=d.compute)
            ws = _workspace(L.m355_conv_transpose3d_workspace(C.byref(dd)), x.device)
            check(L.m355_conv_transpose3d_bwd_data(C.byref(dd), _p(dy), _p(weight), _p(dx), _p(ws), ws.numel(),
                                                   _stream()), "conv_transpose3d_bwd_data")
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw = torch.empty_like(weight)
            db = torch.empty(d.Cout, dtype=weight.dtype, device=weight.device) if ctx.has_bias else None
            # M355_COMPUTE_F32X3: the split kernel where the library has one for this descriptor and this dy (bit 1)
            rc = _lib.M355_EUNSUPPORTED
            if d.compute == _lib.COMPUTE_F32X3 and L.m355_conv_transpose3d_x3_bwd_supported(C.byref(d), _p(dy)) & 2:
                ws = _workspace(L.m355_conv_transpose3d_x3_bwd_workspace(C.byref(d)), x.device)
                rc = L.m355_conv_transpose3d_bwd_weight_x3(C.byref(d), _p(x), _p(dy), _p(dw), _p(db), _p(ws), ws.numel(),
                                                           _stream())
                if rc != _lib.M355_EUNSUPPORTED:
                    check(rc, "conv_transpose3d_bwd_weight_x3")
            if rc == _lib.M355_EUNSUPPORTED:
                ws = _workspace(L.m355_conv_transpose3d_workspace(C.byref(d)), x.device)
                check(L.m355_conv_transpose3d_bwd_weight(C.byref(d), _p(x), _p(dy), _p(dw), _p(db), _p(ws),
                                                         ws.numel(), _stream()), "conv_transpose3d_bwd_weight")
        return dx, dw, db, None


def conv_transpose3d(x, weight, bias=None, stride=2, padding=0, output_padding=0, out: Optional[OutSlot] = None):
    """nn.ConvTranspose3d forward (cubic kernel, weight [Cin, Cout, k, k, k])."""
    k = weight.shape[2]
    if isinstance(x, Act16):
        if k == 2 and stride == 2 and padding == 0 and output_padding == 0:   # c8 -> c8 kernel
            D, H, W = x.spatial
            y16 = _c8_out_slot(x, out, (2 * D, 2 * H, 2 * W), C=weight.shape[1])
            if torch.is_grad_enabled() and (_tracks_any(weight, bias) or x.requires_grad):
                return y16.with_t(_ConvTC8Fn.apply(x.t, weight, bias, x, y16))
            _convt_c8_fwd(x, weight.contiguous(), bias, y16)
            return y16
        y = _ConvT3dFn.apply(x.to_f32(), weight, bias, (k, stride, padding, output_padding, None))
        return _into_c8_slot(y, out, x.compute)
    return _ConvT3dFn.apply(x, weight, bias, (k, stride, padding, output_padding, out))


# ----------------------------------------------------------- norm + activation
@dataclass
class NormCfg:
    groups: int            # 0 = batch norm
    eps: float
    act: int = ACT_NONE
    slope: float = 0.01
    training: bool = True  # BN: use batch statistics (and update running stats)
    momentum: float = 0.1
    running_mean: Optional[torch.Tensor] = None
    running_var: Optional[torch.Tensor] = None
    out: Optional[OutSlot] = None
    stats: Optional[dict] = None   # partial sums from the producing conv (ops.conv3d(..., stats=...))
    c8: int = 0                    # 16-bit no-grad flow: emit the result ONLY in the c8 layout (compute code)
    # 16-bit TRAINING flow on fp32 tensors (the twin flow), set by norm_act() / its autograd function:
    dx_twin: int = 0               # compute code when the conv that produced x wants its output gradient as c8 too
    twin: Optional["Act16"] = None  # c8 twin of the fp32 result, handed from the forward to norm_act()
    sync: Optional[tuple] = None   # synchronised batch norm: (process group, device-side total element count)


# Synchronised batch norm: while a process group is set here (distributed.PatchParallel(sync_batch_norm=True) does so
# around the forward), BatchNorm layers in training mode take their statistics over the batch of ALL ranks -- the
# reference is one process normalising the whole batch (segmentation_trainer.py:189-262).  Two small all-reduces per
# layer and step: the per-channel sums forward, the per-channel gradient means backward.
class batch_norm_sync:
    """Context manager: BatchNorm training statistics over all ranks of `group` (None = off)."""

    def __init__(self, group):
        self.group = group

    def __enter__(self):
        global _bn_sync_group
        self.prev, _bn_sync_group = _bn_sync_group, self.group
        return self

    def __exit__(self, *exc):
        global _bn_sync_group
        _bn_sync_group = self.prev
        return False


def _norm_statistics(L, d, x, cfg, N, Cc, device=None):
    """mean / rstd of the normalisation: from the conv epilogue partials, from x, or from BN running stats."""
    device = x.device if device is None else device
    ns = L.m355_norm_num_stats(C.byref(d))
    mean = torch.empty(ns, dtype=torch.float32, device=device)
    rstd = torch.empty(ns, dtype=torch.float32, device=device)
    use_batch = cfg.groups > 0 or cfg.training or cfg.running_mean is None
    fused = cfg.stats.get("partials") if cfg.stats else None
    if fused is not None and tuple(fused.shape) != (N, cfg.stats["slots"], Cc, 2):
        raise _lib.M355Error(f"norm_act: statistics partials {tuple(fused.shape)} do not belong to this tensor")
    upd = cfg.groups == 0 and cfg.training and use_batch
    cfg.sync = None
    if upd and _bn_sync_group is not None:
        import torch.distributed as dist
        ws = _workspace(L.m355_norm_workspace(C.byref(d)), device)
        sums = torch.empty(2 * Cc + 1, dtype=torch.float64, device=device)   # {sum, sum of squares} per channel, count
        check(L.m355_norm_sums(C.byref(d), _p(x) if fused is None else None, _p(fused),
                               int(cfg.stats["slots"]) if fused is not None else 0, _p(sums), _p(ws), ws.numel(),
                               _stream()), "norm_sums")
        dist.all_reduce(sums, group=_bn_sync_group)
        check(L.m355_norm_stats_from_sums(C.byref(d), _p(sums), _p(mean), _p(rstd), _p(cfg.running_mean),
                                          _p(cfg.running_var), float(cfg.momentum), _stream()), "norm_stats_from_sums")
        cfg.sync = (_bn_sync_group, sums[2 * Cc:])
        return mean, rstd, use_batch
    if use_batch and fused is not None:
        ws = _workspace(L.m355_norm_workspace(C.byref(d)), device)
        check(L.m355_norm_stats_from_partials(C.byref(d), _p(fused), int(cfg.stats["slots"]), _p(mean), _p(rstd),
                                              _p(cfg.running_mean) if upd else None,
                                              _p(cfg.running_var) if upd else None,
                                              float(cfg.momentum), _p(ws), ws.numel(), _stream()),
              "norm_stats_from_partials")
    elif use_batch:
        ws = _workspace(L.m355_norm_workspace(C.byref(d)), x.device)
        check(L.m355_norm_stats(C.byref(d), _p(x), _p(mean), _p(rstd),
                                _p(cfg.running_mean) if upd else None,
                                _p(cfg.running_var) if upd else None,
                                float(cfg.momentum), _p(ws), ws.numel(), _stream()), "norm_stats")
    else:
        check(L.m355_norm_stats_from_running(C.byref(d), _p(cfg.running_mean), _p(cfg.running_var),
                                             _p(mean), _p(rstd), _stream()), "norm_stats_from_running")
    return mean, rstd, use_batch


def _norm_act_c8(x, gamma, beta, add, cfg: NormCfg) -> Act16:
    """norm + activation (+ residual) whose ONLY output is c8 (16-bit no-grad flow).  x: the fp32 conv output
    (read once, 2 bytes per element written) or the c8 pre-norm tensor of m355_conv3d_fwd_h16_c8 (2 + 2 bytes)."""
    L = _lib.lib()
    _require(gamma, beta)
    x_c8 = isinstance(x, Act16)
    if x_c8:
        N, Cc, spatial, S, xbs = x.shape[0], x.C, x.spatial, x.S, 0
    else:
        _require(x)
        x, xbs = _dense_channels(x)
        N, Cc, spatial = x.shape[0], x.shape[1], tuple(x.shape[2:])
        S = spatial[0] * spatial[1] * spatial[2]
    out16 = cfg.out.act16() if cfg.out is not None else None
    if out16 is None:
        out16 = Act16.empty(N, Cc, spatial, cfg.c8, gamma.device if gamma is not None else (x.device))
    elif out16.shape != (N, Cc) + tuple(spatial):
        raise _lib.M355Error(f"c8 slot shape {out16.shape} != op output shape {(N, Cc) + tuple(spatial)}")
    abs_ = 0
    if add is not None and not x_c8:
        add, abs_ = _dense_channels(as_f32(add))
        _require(add)
    d = NormDesc(N, Cc, S, cfg.groups, cfg.act, cfg.eps, cfg.slope, xbs, 0, abs_)
    if x_c8:
        use_batch = cfg.groups > 0 or cfg.training or cfg.running_mean is None
        if use_batch and not (cfg.stats and cfg.stats.get("partials") is not None):
            cfg.stats = {} if cfg.stats is None else cfg.stats
            _c8_channel_partials(x, cfg.stats)
        mean, rstd, _ = _norm_statistics(L, d, None, cfg, N, Cc, device=x.device)
        add16 = None
        if add is not None:
            add16 = add if isinstance(add, Act16) else pack_act16(add, cfg.c8)
        check(L.m355_norm_act_fwd_c8(C.byref(d), x.ptr(), x.batch_stride(), _p(mean), _p(rstd), _p(gamma), _p(beta),
                                     add16.ptr() if add16 is not None else None,
                                     add16.batch_stride() if add16 is not None else 0, out16.ptr(),
                                     out16.batch_stride(), cfg.c8, _stream()), "norm_act_fwd_c8")
        return out16
    mean, rstd, _ = _norm_statistics(L, d, x, cfg, N, Cc)
    check(L.m355_norm_act_fwd_h16(C.byref(d), _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(add), None,
                                  out16.ptr(), out16.batch_stride(), cfg.c8, _stream()), "norm_act_fwd_h16")
    return out16


def _norm_backward(L, d, x, dy, mean, rstd, gamma, beta, dx, dgamma, dbeta, batch_stats, sync, dx16=None, compute=0):
    """The normalisation backward; with `sync` (synchronised batch norm) as its two halves around the all-reduce of the
    per-channel gradient means."""
    ws = _workspace(L.m355_norm_workspace(C.byref(d)), x.device)
    training = 1 if batch_stats else 0
    if sync is not None:
        import torch.distributed as dist
        group, total = sync
        stat_m = torch.empty(2 * d.C, dtype=torch.float32, device=x.device)
        check(L.m355_norm_act_bwd_reduce(C.byref(d), _p(x), _p(dy), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dgamma),
                                         _p(dbeta), training, _p(total), _p(stat_m), _p(ws), ws.numel(), _stream()),
              "norm_act_bwd_reduce")
        dist.all_reduce(stat_m, group=group)
        check(L.m355_norm_act_bwd_apply(C.byref(d), _p(x), _p(dy), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(stat_m),
                                        _p(dx), dx16.ptr() if dx16 is not None else None,
                                        dx16.batch_stride() if dx16 is not None else 0, compute, _stream()),
              "norm_act_bwd_apply")
    elif dx16 is not None:
        check(L.m355_norm_act_bwd_h16(C.byref(d), _p(x), _p(dy), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dx),
                                      _p(dgamma), _p(dbeta), training, dx16.ptr(), dx16.batch_stride(), compute,
                                      _p(ws), ws.numel(), _stream()), "norm_act_bwd_h16")
    else:
        check(L.m355_norm_act_bwd(C.byref(d), _p(x), _p(dy), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dx),
                                  _p(dgamma), _p(dbeta), training, _p(ws), ws.numel(), _stream()), "norm_act_bwd")


class _NormActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, add, cfg: NormCfg):
        L = _lib.lib()
        _require(x, gamma, beta, add)
        x, xbs = _dense_channels(x)
        N, Cc = x.shape[0], x.shape[1]
        S = x.shape[2] * x.shape[3] * x.shape[4]
        if xbs != Cc * S:  # keep the saved input dense so the backward writes a dense dx
            x, xbs = x.contiguous(), Cc * S
        y = _alloc_out(cfg.out, x.shape, x)
        y, ybs = _dense_channels(y)
        abs_ = 0
        if add is not None:
            add, abs_ = _dense_channels(add)
        d = NormDesc(N, Cc, S, cfg.groups, cfg.act, cfg.eps, cfg.slope, xbs, ybs, abs_)
        mean, rstd, use_batch = _norm_statistics(L, d, x, cfg, N, Cc)
        # 16-bit training flow on fp32 tensors (the twin flow): a dense output also leaves as a c8 twin for the convolution that
        # usually consumes it (handed over through `cfg.twin`, attached to the returned tensor by norm_act());
        # ctx.dx_twin: the convolution that produced x wants its output gradient in c8 as well (see backward)
        compute = _COMPUTE[_compute_mode]
        ctx.dx_twin = cfg.dx_twin
        cfg.twin = None
        if compute in _DT16 and cfg.out is None and ybs == Cc * S and Cc > 4:
            cfg.twin = Act16.empty(N, Cc, tuple(x.shape[2:]), compute, x.device)
            check(L.m355_norm_act_fwd_h16(C.byref(d), _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(add), _p(y),
                                          cfg.twin.ptr(), cfg.twin.batch_stride(), compute, _stream()), "norm_act_fwd_h16")
        else:
            check(L.m355_norm_act_fwd(C.byref(d), _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(add), _p(y),
                                      _stream()), "norm_act_fwd")
        ctx.desc, ctx.batch_stats, ctx.has_add = d, use_batch, add is not None
        ctx.has_affine, ctx.sync = gamma is not None, cfg.sync
        ctx.save_for_backward(x, mean, rstd, gamma, beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        x, mean, rstd, gamma, beta = ctx.saved_tensors
        d0 = ctx.desc
        dy, dybs = _dense_channels(dy)
        d = NormDesc(d0.N, d0.C, d0.S, d0.groups, d0.act, d0.eps, d0.act_slope, d0.x_batch_stride, dybs, 0)
        dx = torch.empty_like(x)  # x was saved dense
        dgamma = torch.empty(d0.C, dtype=torch.float32, device=x.device) if ctx.has_affine else None
        dbeta = torch.empty(d0.C, dtype=torch.float32, device=x.device) if ctx.has_affine else None
        if ctx.dx_twin:   # dx is the output gradient of an h16-flow convolution: emit it as c8 too, in the same pass
            dx16 = Act16.empty(d0.N, d0.C, tuple(x.shape[2:]), ctx.dx_twin, x.device)
            _norm_backward(L, d, x, dy, mean, rstd, gamma, beta, dx, dgamma, dbeta, ctx.batch_stats, ctx.sync, dx16,
                           ctx.dx_twin)
            dx._m355_c8 = (dx16, dx._version)
        else:
            _norm_backward(L, d, x, dy, mean, rstd, gamma, beta, dx, dgamma, dbeta, ctx.batch_stats, ctx.sync)
        dadd = dy if (ctx.has_add and ctx.needs_input_grad[3]) else None
        return dx, dgamma, dbeta, dadd, None


class _NormActPoolFn(torch.autograd.Function):
    """norm + activation with AvgPool3d(2, 2) of the result as a second output (m355_norm_act_pool_fwd): the last
    pass of an encoder block also produces the next level's input, so the pool never re-reads the activated tensor.
    Backward: the two incoming gradients (skip path, pooled path) are summed inside the two passes of the normalisation
    backward (m355_norm_act_bwd_pool).  With FUSE_POOL_BWD off, and for synchronised batch norm (two halves around an
    all-reduce), the pool-backward pass writes the sum first (m355_avgpool3d_2x_bwd_add), then the usual backward."""

    @staticmethod
    def forward(ctx, x, gamma, beta, cfg: NormCfg):
        L = _lib.lib()
        _require(x, gamma, beta)
        x, xbs = _dense_channels(x)
        N, Cc, D, H, W = x.shape
        S = D * H * W
        if xbs != Cc * S:
            x, xbs = x.contiguous(), Cc * S
        x, xbs = _pairs_in(x, xbs)
        y = _alloc_out(cfg.out, x.shape, x)
        y, ybs = _dense_channels(y)
        yw, ywbs = _pairs_out(y, ybs)
        pooled = torch.empty((N, Cc, D // 2, H // 2, W // 2), dtype=x.dtype, device=x.device)
        d = NormDesc(N, Cc, S, cfg.groups, cfg.act, cfg.eps, cfg.slope, xbs, ywbs, 0)
        mean, rstd, use_batch = _norm_statistics(L, d, x, cfg, N, Cc)
        check(L.m355_norm_act_pool_fwd(C.byref(d), _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(yw), _p(pooled), 0,
                                       D, H, W, _stream()), "norm_act_pool_fwd")
        if yw is not y:
            y.copy_(yw)
        ctx.desc, ctx.batch_stats, ctx.has_affine, ctx.dims = d, use_batch, gamma is not None, (D, H, W)
        ctx.sync = cfg.sync
        ctx.save_for_backward(x, mean, rstd, gamma, beta)
        return y, pooled

    @staticmethod
    def backward(ctx, dy, dpool):
        L = _lib.lib()
        x, mean, rstd, gamma, beta = ctx.saved_tensors
        d0 = ctx.desc
        D, H, W = ctx.dims
        if dpool is not None and FUSE_POOL_BWD and ctx.sync is None:
            # gradient of the activated tensor = skip-path gradient + un-pooled gradient, formed inside both passes
            dpool, gpbs = _dense_channels(dpool)
            gsbs = 0
            if dy is not None:
                dy, gsbs = _dense_channels(dy)
            dx = torch.empty_like(x)
            dgamma = torch.empty(d0.C, dtype=torch.float32, device=x.device) if ctx.has_affine else None
            dbeta = torch.empty(d0.C, dtype=torch.float32, device=x.device) if ctx.has_affine else None
            ws = _workspace(L.m355_norm_workspace(C.byref(d0)), x.device)
            check(L.m355_norm_act_bwd_pool(C.byref(d0), _p(x), _p(dy), gsbs, _p(dpool), gpbs, D, H, W, _p(mean), _p(rstd),
                                           _p(gamma), _p(beta), _p(dx), _p(dgamma), _p(dbeta), 1 if ctx.batch_stats else 0,
                                           _p(ws), ws.numel(), _stream()), "norm_act_bwd_pool")
            fused_bwd_counts["pool"] += 1
            return dx, dgamma, dbeta, None
        if dpool is not None:   # the two-step form: the sum in one pass of its own
            dpool, gpbs = _dense_channels(dpool)
            tot = torch.empty_like(x)
            if dy is None:
                check(L.m355_avgpool3d_2x_bwd(_p(dpool), _p(tot), d0.N, d0.C, D, H, W, gpbs, 0, _stream()), "avgpool3d_2x_bwd")
            else:
                dy, gsbs = _dense_channels(dy)
                check(L.m355_avgpool3d_2x_bwd_add(_p(dpool), _p(dy), _p(tot), d0.N, d0.C, D, H, W, gpbs, gsbs, 0,
                                                  _stream()), "avgpool3d_2x_bwd_add")
            dy = tot
        dy, dybs = _dense_channels(dy)
        d = NormDesc(d0.N, d0.C, d0.S, d0.groups, d0.act, d0.eps, d0.act_slope, d0.x_batch_stride, dybs, 0)
        dx = torch.empty_like(x)
        dgamma = torch.empty(d0.C, dtype=torch.float32, device=x.device) if ctx.has_affine else None
        dbeta = torch.empty(d0.C, dtype=torch.float32, device=x.device) if ctx.has_affine else None
        _norm_backward(L, d, x, dy, mean, rstd, gamma, beta, dx, dgamma, dbeta, ctx.batch_stats, ctx.sync)
        return dx, dgamma, dbeta, None


def norm_act_pool(x, gamma, beta, cfg: NormCfg):
    """act(norm(x)) AND AvgPool3d(2, 2) of it from one pass -> (y, pooled); fp32 tensors, even spatial sizes."""
    return _NormActPoolFn.apply(x, gamma, beta, cfg)


def norm_act(x, gamma, beta, cfg: NormCfg, add=None, pool=False):
    """normalization_class + activation_class of Block3d (components.py:52-55), optionally
    fused with the residual sum (components.py:67-68): act(norm(x)) + add.  With `cfg.c8` set (16-bit
    precision mode under no_grad) the result is an `Act16` and nothing is written in fp32."""
    if cfg.c8 and torch.is_grad_enabled():                                   # c8 training flow
        if not isinstance(x, Act16):     # the pre-norm tensor of a conv without a c8 kernel (strided / Blur): joins here
            x = pack_act16(x, cfg.c8)
        return _norm_act_c8_train(x, gamma, beta, add, cfg, pool=pool)
    if pool:
        raise _lib.M355Error("norm_act(pool=True) is the c8 training flow's fused pool; use norm_act_pool for fp32 tensors")
    if cfg.c8 and not torch.is_grad_enabled():
        return _norm_act_c8(x, gamma, beta, add, cfg)
    x = as_f32(x)
    cfg.dx_twin = getattr(x, "_m355_c8_grad", 0) if torch.is_grad_enabled() else 0
    y = _NormActFn.apply(x, gamma, beta, as_f32(add) if add is not None else None, cfg)
    if cfg.twin is not None:
        # the twin describes y as written by this pass: recorded with y's version, so an in-place op on y voids it
        y._m355_c8 = (cfg.twin, y._version)
        cfg.twin = None
    return y


# ------------------------------------------- factor-2 resampling: pool / upsample / space-to-depth
# One row per op says in data what its entry points are called and take; the fp32 flow and the c8 flow have one autograd
# function body each (_Resample2xFn, _Resample2xC8Fn), and _resample_launch is the one place that builds a call.  The C
# side's counterpart is the row per entry point of csrc/resample_host.hpp.
class _Resample2x(NamedTuple):
    fwd: str                      # the entry points m355_<fwd> / m355_<bwd>, in the c8 flow m355_<fwd>_h16 / m355_<bwd>_h16;
    bwd: str                      # space-to-depth and depth-to-space: each is the other's backward
    chan: tuple                   # output shape from the input's (N, C, D, H, W): C * chan[0] // chan[1] channels ...
    up: bool                      # ... at twice (True) or half the spatial size
    nodes: tuple                  # autograd function of the fp32 flow, of its *_with_skip form, of the c8 flow
    full_out: bool = False        # the entry points take the (N, C, D, H, W) of the output, not of the input: depth-to-space,
    #                               whose full-resolution side (the one the s2d pair's entry points describe) is its output
    route: bool = False           # the forward writes a route byte per output element for the backward to gather through:
    #                               uint8 [N, C, D/2, H/2, W/2], in c8 [N, CB, S_out, 8]; null when nothing will run backward
    add: Optional[str] = None     # not None: the backward takes the skip gradient as `add`, with a batch stride of its own (null
    #                               without one); the suffix of the fp32 entry point that does (avg pool: one of its own)
    pairs: bool = False           # the fp32 kernels move x pairs of the full-resolution side: _pairs_in / _pairs_out
    overflow: bool = False        # the c8 function installs the fp16 overflow word, in which its backward's sums report their
    #                               saturation, itself: the op is also used on its own (pack -> op -> backward).  The others (avg
    #                               pool, align_corners=True trilinear, the s2d pair, which sums nothing) leave that to a
    #                               neighbouring node of the model (_UnpackFn, the c8 conv)


# entry point -> (picks its pointer arguments, in its order, out of (tensor 0, tensor 1, tensor 2, route); its number of batch
# strides; its symbol): the argument orders of the family are written down once, in _lib's mirror of the C table
_RESAMPLE_ARGS = {name: (itemgetter(*order), nstrides, "m355_" + name)
                  for name, order, nstrides, _ in _lib.RESAMPLE_OPS + list(_lib.UPSAMPLE2X_OPS.values())}


def _resample_launch(row, bwd, c8, pointers, shape, strides, compute=0):
    """Call the forward or backward entry point of `row`, c8: its _h16 form.  pointers: (tensor 0, tensor 1, tensor 2, route)
    as c_void_p or None, the tensors in the order of their batch `strides`: (x, y) forward, (dy, dx) backward, (dy, add, dx)
    where the backward takes an `add`.  shape: the (N, C, D, H, W) the entry point takes."""
    name = row.bwd if bwd else row.fwd
    if c8:
        name += "_h16"
    elif bwd and row.add:     # fp32 avg pool: the sum with `add` is an entry point of its own, the plain one has no such argument
        if pointers[1] is None:
            pointers, strides = (pointers[0], pointers[2]), (strides[0], strides[2])
        else:
            name += row.add
    pick, nstrides, symbol = _RESAMPLE_ARGS[name]
    check(getattr(_lib.lib(), symbol)(*pick(pointers), *shape, *strides[:nstrides], *((compute,) if c8 else ()), _stream()),
          name)


def _out_shape(row, xshape):
    N, Cc, D, H, W = xshape
    Cc = Cc * row.chan[0] // row.chan[1]
    return (N, Cc, 2 * D, 2 * H, 2 * W) if row.up else (N, Cc, D // 2, H // 2, W // 2)


def _tracks(x):
    return torch.is_grad_enabled() and x.requires_grad


class _Resample2xFn(torch.autograd.Function):
    """The fp32 flow of the family: x -> y, a fresh tensor or the concat slot `out`.
    with_skip: x ALSO continues as a skip connection (models/modular_unet.py:90-92).  Returns (skip alias, y), `out` is
    ignored; the backward receives both gradients together and sums them in its one pass (`add`) -- autograd would
    otherwise add them with a separate torch kernel.
    route: autograd was recording at .apply and x carries a gradient (inside forward grad mode is always off, and
    ctx.needs_input_grad stays True under no_grad for a tensor that requires grad).  The route tensor comes from the caching
    allocator and lives on ctx; it is not allocated when nothing will run backward."""

    @staticmethod
    def forward(ctx, x, row, out, with_skip, route):
        _require(x)
        xd, xbs = _dense_channels(x)
        xshape = tuple(xd.shape)
        oshape = _out_shape(row, xshape)
        y = _alloc_out(None if with_skip else out, oshape, x)
        y, ybs = _dense_channels(y)
        full = oshape if row.full_out else xshape
        yw, ywbs = y, ybs
        if row.pairs:     # (the FULL-resolution side must be 8-byte aligned with an even stride)
            if row.full_out:
                yw, ywbs = _pairs_out(y, ybs)
            else:
                xd, xbs = _pairs_in(xd, xbs)
        idx = torch.empty(oshape, dtype=torch.uint8, device=x.device) if route else None
        _resample_launch(row, False, False, (_p(xd), _p(yw), None, _p(idx)), full, (xbs, ywbs))
        if yw is not y:
            y.copy_(yw)
        ctx.row, ctx.shape, ctx.full, ctx.route = row, xshape, full, idx
        return (x.view_as(x), y) if with_skip else y

    @staticmethod
    def backward(ctx, *grads):
        g_skip, g = grads if len(grads) == 2 else (None, grads[0])
        if g is None:
            return g_skip, None, None, None, None
        row = ctx.row
        g, gbs = _dense_channels(g)
        dx = torch.empty(ctx.shape, dtype=g.dtype, device=g.device)
        if row.add is None:
            if row.pairs and row.full_out:    # the gradient is the full-resolution side
                g, gbs = _pairs_in(g, gbs)
            pointers, strides = (_p(g), _p(dx), None, None), (gbs, 0)
        else:
            sbs = 0
            if g_skip is not None:
                g_skip, sbs = _dense_channels(g_skip)
            pointers, strides = (_p(g), _p(g_skip), _p(dx), _p(ctx.route)), (gbs, sbs, 0)
        _resample_launch(row, True, False, pointers, ctx.full, strides)
        return dx, None, None, None, None


def _resample_c8_fwd(row, x: "Act16", y16: "Act16", route=None):
    """the c8 -> c8 forward launch: of the no-grad flow as it is, and of _Resample2xC8Fn"""
    _resample_launch(row, False, True, (x.ptr(), y16.ptr(), None, _p(route)), y16.shape if row.full_out else x.shape,
                     (x.batch_stride(), y16.batch_stride()), x.compute)


class _Resample2xC8Fn(torch.autograd.Function):
    """The c8 training flow of the family: c8 -> c8 straight into `y16`, a fresh activation or a concat slot; the backward
    runs the c8 kernel on the c8 gradient.  with_skip: also returns the input as it continues into the skip connection, so
    that the backward receives both gradients and sums them in its one pass."""

    @staticmethod
    def forward(ctx, x_t, row, x: "Act16", y16: "Act16", with_skip):
        route = torch.empty((x.shape[0], x.CB, y16.S, 8), dtype=torch.uint8, device=x.device) if row.route else None
        _resample_c8_fwd(row, x, y16, route)
        ctx.row, ctx.route = row, route
        ctx.info = (x.shape, y16.shape if row.full_out else x.shape, x.compute)
        if row.overflow and x.compute == _lib.COMPUTE_F16:
            _overflow_word(x.device)
        return (x_t.view_as(x_t), y16.alias()) if with_skip else y16.alias()

    @staticmethod
    def backward(ctx, *grads):
        g_skip, g = grads if len(grads) == 2 else (None, grads[0])
        if g is None:
            return g_skip, None, None, None, None
        row = ctx.row
        (N, Cc, D, H, W), full, compute = ctx.info
        g, gbs = _c8t(g)
        dx16 = _c8_grad(N, Cc, D * H * W, compute, g.device)
        if row.add is None:
            pointers, strides = (_p(g), _p(dx16), None, None), (gbs, 0)
        else:
            sbs = 0
            if g_skip is not None:
                g_skip, sbs = _c8t(g_skip)
            pointers, strides = (_p(g), _p(g_skip), _p(dx16), _p(ctx.route)), (gbs, sbs, 0)
        _resample_launch(row, True, True, pointers, full, strides, compute)
        return dx16, None, None, None, None


# autograd names its nodes after the class: one name per op and flow, as the graphs of the models are read
class _AvgPoolFn(_Resample2xFn):
    """nn.AvgPool3d(2, 2)"""


class _PoolSkipFn(_Resample2xFn):
    """nn.AvgPool3d(2, 2) of a tensor that also continues as a skip connection"""


class _PoolC8Fn(_Resample2xC8Fn):
    """nn.AvgPool3d(2, 2) c8 -> c8, with or without the skip output"""


class _MaxPoolFn(_Resample2xFn):
    """nn.MaxPool3d(2, 2) (csrc/maxpool.hip): the route byte is the window position 0..7 of torch's argmax, ties / NaN
    included; the backward is a gather through it"""


class _MaxPoolSkipFn(_Resample2xFn):
    """nn.MaxPool3d(2, 2) of a tensor that also continues as a skip connection"""


class _MaxPoolC8Fn(_Resample2xC8Fn):
    """nn.MaxPool3d(2, 2) c8 -> c8, with or without the skip output; the route is one byte per lane of the pooled items"""


class _UpsampleFn(_Resample2xFn):
    """nn.Upsample(scale_factor=2), all three conventions"""


class _UpsampleC8Fn(_Resample2xC8Fn):
    """nn.Upsample(scale_factor=2) c8 -> c8; backward: the gather-form kernel on the c8 gradient"""


class _S2DFn(_Resample2xFn):
    """space-to-depth or depth-to-space by 2"""


class _S2DC8Fn(_Resample2xC8Fn):
    """space-to-depth or depth-to-space by 2 on c8 activations"""


_AVGPOOL = _Resample2x("avgpool3d_2x_fwd", "avgpool3d_2x_bwd", (1, 1), False, (_AvgPoolFn, _PoolSkipFn, _PoolC8Fn), add="_add")
_MAXPOOL = _Resample2x("maxpool3d_2x_fwd", "maxpool3d_2x_bwd", (1, 1), False, (_MaxPoolFn, _MaxPoolSkipFn, _MaxPoolC8Fn),
                       route=True, add="", overflow=True)
# nn.Upsample(scale_factor=2) by `mode`: align_corners=True trilinear (csrc/elementwise.hip), nearest and half-pixel
# (align_corners=False) trilinear (csrc/upsample.hip)
_UPSAMPLE = {
    mode: _Resample2x(stem + "_fwd", stem + "_bwd", (1, 1), True, (_UpsampleFn, None, _UpsampleC8Fn), overflow=overflow)
    for mode, stem, overflow in (("trilinear", "upsample_trilinear2x", False), ("nearest", "upsample_nearest2x", True),
                                 ("trilinear_hp", "upsample_trilinear2x_hp", True))}
_S2D = _Resample2x("space_to_depth2", "depth_to_space2", (8, 1), False, (_S2DFn, None, _S2DC8Fn), pairs=True)
_D2S = _Resample2x("depth_to_space2", "space_to_depth2", (1, 8), True, (_S2DFn, None, _S2DC8Fn), full_out=True, pairs=True)


def _resample2x(row, x, out=None, with_skip=False):
    """A public function of the family: pick the flow, obtain the output, then the autograd function -- or, for a c8
    activation that does not track, the plain launch.  -> y, with_skip: (x as it continues into the skip connection, y)"""
    if not isinstance(x, Act16):
        return row.nodes[1 if with_skip else 0].apply(x, row, out, with_skip, row.route and _tracks(x))
    tracks = _act16_tracks(x)
    if with_skip and not tracks:
        return x, _resample2x(row, x, out)
    oshape = _out_shape(row, x.shape)
    y16 = _c8_out_slot(x, out, oshape[2:], oshape[1])
    if not tracks:
        _resample_c8_fwd(row, x, y16)
        return y16
    res = row.nodes[2].apply(x.t, row, x, y16, with_skip)
    return (x.with_t(res[0]), y16.with_t(res[1])) if with_skip else y16.with_t(res)


def avgpool3d_2x_with_skip(x, out: Optional[OutSlot] = None):
    """-> (x as it continues into the skip connection, AvgPool3d(2, 2)(x)); see _Resample2xFn.  `out` (c8 flow): the pooled
    tensor is written into this concat slot."""
    return _resample2x(_AVGPOOL, x, out, True)


def avgpool3d_2x(x, out: Optional[OutSlot] = None):
    """nn.AvgPool3d(kernel_size=2, stride=2, count_include_pad=False); c8 -> c8 in the 16-bit flows."""
    return _resample2x(_AVGPOOL, x, out)


def maxpool3d_2x_with_skip(x, out: Optional[OutSlot] = None):
    """-> (x as it continues into the skip connection, MaxPool3d(2, 2)(x)); see _Resample2xFn.  `out` (c8 flow): the
    pooled tensor is written into this concat slot."""
    return _resample2x(_MAXPOOL, x, out, True)


def maxpool3d_2x(x, out: Optional[OutSlot] = None):
    """nn.MaxPool3d(kernel_size=2, stride=2), torch's tie / NaN routing; c8 -> c8 in the 16-bit flows."""
    return _resample2x(_MAXPOOL, x, out)


def upsample_trilinear2x(x, out: Optional[OutSlot] = None, mode: str = "trilinear"):
    """nn.Upsample(scale_factor=2, mode='trilinear', align_corners=True); c8 -> c8 in the 16-bit flows.
    mode: 'trilinear' (this default), or 'nearest' / 'trilinear_hp' = upsample_nearest2x / upsample_trilinear2x_hp."""
    if mode not in _UPSAMPLE:
        raise ValueError(f"upsample mode {mode!r} not in {sorted(_UPSAMPLE)}")
    return _resample2x(_UPSAMPLE[mode], x, out)


def upsample_nearest2x(x, out: Optional[OutSlot] = None):
    """nn.Upsample(scale_factor=2, mode='nearest') (= 'nearest-exact' at this factor): the forward copies bits, the
    backward sums each 2x2x2 block; c8 -> c8 in the 16-bit flows."""
    return _resample2x(_UPSAMPLE["nearest"], x, out)


def upsample_trilinear2x_hp(x, out: Optional[OutSlot] = None):
    """nn.Upsample(scale_factor=2, mode='trilinear', align_corners=False): the half-pixel convention (weights 0.25 / 0.75,
    edges clamped); c8 -> c8 in the 16-bit flows."""
    return _resample2x(_UPSAMPLE["trilinear_hp"], x, out)


def space_to_depth2(x):
    """[N, C, D, H, W] -> [N, 8C, D/2, H/2, W/2], channel c*8 + (pz*4 + py*2 + px).  A c8 activation stays c8 (the packed
    channels of input channel c are exactly c8 block c)."""
    if isinstance(x, Act16) and all(v % 2 == 0 for v in x.shape[2:]):
        return _resample2x(_S2D, x)
    return _resample2x(_S2D, as_f32(x))


def depth_to_space2(x, out: Optional[OutSlot] = None):
    if isinstance(x, Act16) and x.C % 8 == 0 and (out is None or out.buf16 is not None):
        return _resample2x(_D2S, x, out)
    if out is not None and out.buf16 is not None:
        return pack_act16(_resample2x(_D2S, as_f32(x)), out.buf16.compute, out.act16())
    return _resample2x(_D2S, as_f32(x), out)


def _into_c8_slot(y32, out: Optional[OutSlot], compute):
    """c8 flow: a producer without a c8 epilogue (conv-transpose, trilinear upsampling) computed `y32`
    densely; pack it into its slot of the c8 concat buffer."""
    return pack_act16(y32, compute, out.act16() if out is not None else None)


# ------------------------------------------------------------------- softmax
class _SoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, inner, diag_bias):
        _require(x)
        y = _head_fwd(x, True, inner, diag_bias)
        ctx.inner = inner
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return _head_bwd(y, dy, True, ctx.inner), None, None


class _SigmoidFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _require(x)
        y = _head_fwd(x, False)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return _head_bwd(y, dy, False)


def sigmoid(x):
    """nn.Sigmoid (the hypothesis head where the output convolution has no epilogue for it)"""
    return _SigmoidFn.apply(as_f32(x))


def softmax_channels(x, inner=1, diag_bias=0.0):
    """nn.Softmax(dim=1); inner=C gives StochasticMatrix's reshape+eye-bias+softmax."""
    return _SoftmaxFn.apply(as_f32(x), inner, diag_bias)


# ----------------------------------------------------------------------- loss
# The four criteria share one shape (csrc/loss_common.hpp): a forward that leaves the scalars and the per-row sums on the
# device, and a closed-form backward from the saved sums.
def _loss_operands(named_tensors, named_weights):
    """The checked operands of a criterion.  named_tensors: (name, tensor) of the prediction and of its companion (the
    target, or phi); named_weights: (name, tensor or None) of the per-channel weights.
    -> (prediction, companion, [weights], N, C, S), the tensors contiguous.
    (the argument errors come before the device check: they are the same on a host without a GPU)"""
    (_, x), (other_name, t) = named_tensors
    for name, v in (*named_tensors, *named_weights):
        if v is not None and v.dtype != torch.float32:
            raise _lib.M355Error(f"{name}: expected torch.float32, got {v.dtype}")
    if x.dim() < 2 or x.shape != t.shape:
        raise _lib.M355Error(f"prediction {tuple(x.shape)} and {other_name} {tuple(t.shape)}: expected one shape [N, C, ...]")
    N, Cc = x.shape[0], x.shape[1]
    for name, w in named_weights:
        if w is not None and (w.dim() != 1 or w.numel() != Cc):
            raise _lib.M355Error(f"{name} of shape {tuple(w.shape)} for {Cc} channels")
    weights = [w for _, w in named_weights]
    _require(x, t, *weights)
    return (x.contiguous(), t.contiguous(), [None if w is None else w.contiguous() for w in weights], N, Cc,
            x.numel() // (N * Cc))


def _three_scalars(out3):
    """out3 [3] -> three independent 0-dim tensors for autograd's sake: not views of `out3` (a Function must not return
    views of one base) and not clones either (three 4-byte device copies of ~10 us each per step) -- fresh tensor objects
    over the same storage, as ops._alloc_out makes them for concat slots"""
    st = out3.untyped_storage()
    return tuple(torch.empty((), dtype=torch.float32, device=out3.device).set_(st, i, ()) for i in range(3))


def _dloss32(dloss):
    return dloss.contiguous().to(torch.float32)


class _HybridLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t, dice_weight, class_weights, square_dice):
        L = _lib.lib()
        _require(p, t, class_weights)
        if p.shape != t.shape:
            raise _lib.M355Error(f"prediction {tuple(p.shape)} and target {tuple(t.shape)} differ in shape")
        p, t = p.contiguous(), t.contiguous()
        N, Cc = p.shape[0], p.shape[1]
        S = p.numel() // (N * Cc)
        out3 = torch.empty(3, dtype=torch.float32, device=p.device)
        sums = torch.empty(N * Cc * 4, dtype=torch.float32, device=p.device)
        ws = _workspace(L.m355_hybrid_loss_workspace(N, Cc, S), p.device)
        check(L.m355_hybrid_loss_fwd(_p(p), _p(t), N, Cc, S, float(dice_weight), _p(class_weights),
                                     1 if square_dice else 0, _p(out3), _p(sums), _p(ws), ws.numel(),
                                     _stream()), "hybrid_loss_fwd")
        ctx.args = (N, Cc, S, float(dice_weight), 1 if square_dice else 0)
        ctx.save_for_backward(p, t, sums, class_weights)
        loss, dice, logistic = _three_scalars(out3)
        ctx.mark_non_differentiable(dice, logistic)
        return loss, dice, logistic

    @staticmethod
    def backward(ctx, dloss, _d1, _d2):
        L = _lib.lib()
        p, t, sums, cw = ctx.saved_tensors
        N, Cc, S, dwt, sq = ctx.args
        dp = torch.empty_like(p)
        check(L.m355_hybrid_loss_bwd(_p(p), _p(t), _p(sums), _p(_dloss32(dloss)), N, Cc, S, dwt, _p(cw), sq, _p(dp),
                                     _stream()), "hybrid_loss_bwd")
        return dp, None, None, None, None


def hybrid_logistic_dice_loss(prediction, target, dice_weight=0.5, class_weights=None, square_dice=True):
    """HybridLogisticDiceLoss.forward -> (loss, dice_loss, logistic_loss); the gradient
    flows through `loss` (the only entry the trainer back-propagates, segmentation_trainer.py:177)."""
    return _HybridLossFn.apply(prediction, target, dice_weight, class_weights, square_dice)


class _BinaryLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, dice_weight, class_weights, pos_weight, square_dice, from_logits):
        L = _lib.lib()
        x, t, (cw, pw), N, Cc, S = _loss_operands(
            (("prediction", x), ("target", t)), (("class_weights", class_weights), ("pos_weight", pos_weight)))
        out3 = torch.empty(3, dtype=torch.float32, device=x.device)
        sums = torch.empty(N * Cc * 5, dtype=torch.float32, device=x.device)
        ws = _workspace(L.m355_binary_loss_workspace(N, Cc, S), x.device)
        sq, fl = (1 if square_dice else 0), (1 if from_logits else 0)
        check(L.m355_binary_loss_fwd(_p(x), _p(t), N, Cc, S, float(dice_weight), _p(cw), _p(pw), sq, fl,
                                     _p(out3), _p(sums), _p(ws), ws.numel(), _stream()), "binary_loss_fwd")
        ctx.args = (N, Cc, S, float(dice_weight), sq, fl)
        ctx.save_for_backward(x, t, sums, cw, pw)
        loss, dice, logistic = _three_scalars(out3)
        ctx.mark_non_differentiable(dice, logistic)
        return loss, dice, logistic

    @staticmethod
    def backward(ctx, dloss, _d1, _d2):
        L = _lib.lib()
        x, t, sums, cw, pw = ctx.saved_tensors
        N, Cc, S, dwt, sq, fl = ctx.args
        dx = torch.empty_like(x)
        check(L.m355_binary_loss_bwd(_p(x), _p(t), _p(sums), _p(_dloss32(dloss)), N, Cc, S, dwt, _p(cw), _p(pw), sq, fl,
                                     _p(dx), _stream()), "binary_loss_bwd")
        return dx, None, None, None, None, None, None


def binary_logistic_dice_loss(x, target, dice_weight=0.5, class_weights=None, pos_weight=None, square_dice=True,
                              from_logits=False):
    """HybridBinaryLogisticDiceLoss.forward -> (loss, dice_loss, logistic_loss): binary cross-entropy + Dice per channel
    of `x` [N, C, ...] fp32 -- probabilities, or logits with from_logits -- against `target` in [0, 1].
    class_weights / pos_weight: fp32 device tensors [C] or None.  The gradient flows through `loss`."""
    return _BinaryLossFn.apply(x, target, dice_weight, class_weights, pos_weight, square_dice, from_logits)


class _FocalTverskyLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, tversky_weight, alpha, beta, tversky_power, focal_gamma, focal_class_weights,
                tversky_class_weights, from_logits):
        L = _lib.lib()
        x, t, (fw, tw), N, Cc, S = _loss_operands(
            (("prediction", x), ("target", t)),
            (("focal_class_weights", focal_class_weights), ("tversky_class_weights", tversky_class_weights)))
        out3 = torch.empty(3, dtype=torch.float32, device=x.device)
        sums = torch.empty(N * Cc * 4, dtype=torch.float32, device=x.device)
        ws = _workspace(L.m355_focal_tversky_workspace(N, Cc, S), x.device)
        par = (float(tversky_weight), float(alpha), float(beta), float(tversky_power), float(focal_gamma))
        fl = 1 if from_logits else 0
        check(L.m355_focal_tversky_fwd(_p(x), _p(t), N, Cc, S, *par, _p(fw), _p(tw), fl, _p(out3), _p(sums), _p(ws),
                                       ws.numel(), _stream()), "focal_tversky_fwd")
        ctx.args = (N, Cc, S, par, fl)
        ctx.save_for_backward(x, t, sums, fw, tw)
        loss, tversky, focal = _three_scalars(out3)
        ctx.mark_non_differentiable(tversky, focal)
        return loss, tversky, focal

    @staticmethod
    def backward(ctx, dloss, _d1, _d2):
        L = _lib.lib()
        x, t, sums, fw, tw = ctx.saved_tensors
        N, Cc, S, par, fl = ctx.args
        dx = torch.empty_like(x)
        check(L.m355_focal_tversky_bwd(_p(x), _p(t), _p(sums), _p(_dloss32(dloss)), N, Cc, S, *par, _p(fw), _p(tw), fl,
                                       _p(dx), _stream()), "focal_tversky_bwd")
        return (dx,) + (None,) * 9


def focal_tversky_loss(x, target, tversky_weight=0.5, alpha=0.5, beta=0.5, tversky_power=1.0, focal_gamma=0.0,
                       focal_class_weights=None, tversky_class_weights=None, from_logits=False):
    """HybridFocalTverskyLoss.forward -> (loss, tversky_loss, focal_loss) of `x` [N, C, ...] fp32 -- probabilities, or
    with from_logits the logits of an nn.Identity head, whose log-softmax over C is taken inside -- against `target` in
    [0, 1].  The class weights: fp32 device tensors [C] or None.  The gradient flows through `loss`."""
    return _FocalTverskyLossFn.apply(x, target, tversky_weight, alpha, beta, tversky_power, focal_gamma,
                                     focal_class_weights, tversky_class_weights, from_logits)


def topk_count(N, S, top_k):
    """k = max(1, floor(N * S * top_k)) for a fraction 0 < top_k <= 1 of the N * S voxels of a batch: the one place the
    floor is taken (the criterion's schedule and the tests' reference call it too)"""
    top_k = float(top_k)
    if not (math.isfinite(top_k) and 0.0 < top_k <= 1.0):
        raise ValueError(f"top_k = {top_k}: expected a fraction in (0, 1]")
    M = int(N) * int(S)
    if M < 1:
        raise ValueError(f"N * S = {M}: expected at least one voxel")
    return max(1, min(M, math.floor(M * top_k)))


class _TopKLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, top_k, dice_weight, class_weights, square_dice, from_logits):
        L = _lib.lib()
        x, t, (cw,), N, Cc, S = _loss_operands((("prediction", x), ("target", t)), (("class_weights", class_weights),))
        if torch.is_tensor(top_k):
            # k itself on the device: read by the kernels, never here
            if top_k.dim() != 0 or top_k.dtype != torch.int64:
                raise _lib.M355Error(f"top_k: expected a fraction or a 0-dim torch.int64 tensor holding k, got "
                                     f"{tuple(top_k.shape)} {top_k.dtype}")
            _require(top_k, dtype=torch.int64)
            k, k_dev = 0, top_k
        else:
            k, k_dev = topk_count(N, S, top_k), None
        out3 = torch.empty(3, dtype=torch.float32, device=x.device)
        sums = torch.empty(N * Cc * 3, dtype=torch.float32, device=x.device)
        e = torch.empty(N * S, dtype=torch.float32, device=x.device)     # saved: not the workspace, which the next op reuses
        state = torch.empty(4, dtype=torch.float32, device=x.device)    # {tau, r, k as int64}
        ws = _workspace(L.m355_topk_loss_workspace(N, Cc, S), x.device)
        sq, fl = (1 if square_dice else 0), (1 if from_logits else 0)
        check(L.m355_topk_loss_fwd(_p(x), _p(t), N, Cc, S, k, _p(k_dev), float(dice_weight), _p(cw), sq, fl, _p(out3),
                                   _p(sums), _p(e), _p(state), _p(ws), ws.numel(), _stream()), "topk_loss_fwd")
        ctx.args = (N, Cc, S, float(dice_weight), sq, fl)
        ctx.save_for_backward(x, t, e, sums, state, cw)
        loss, dice, logistic = _three_scalars(out3)
        threshold = torch.empty((), dtype=torch.float32, device=x.device).set_(state.untyped_storage(), 0, ())
        ctx.mark_non_differentiable(dice, logistic, threshold)
        return loss, dice, logistic, threshold

    @staticmethod
    def backward(ctx, dloss, _d1, _d2, _d3):
        L = _lib.lib()
        x, t, e, sums, state, cw = ctx.saved_tensors
        N, Cc, S, dwt, sq, fl = ctx.args
        dx = torch.empty_like(x)
        check(L.m355_topk_loss_bwd(_p(x), _p(t), _p(e), _p(sums), _p(state), _p(_dloss32(dloss)), N, Cc, S, dwt, _p(cw),
                                   sq, fl, _p(dx), _stream()), "topk_loss_bwd")
        return (dx,) + (None,) * 6


def topk_logistic_dice_loss(x, target, top_k, dice_weight=0.5, class_weights=None, square_dice=True, from_logits=False):
    """HybridTopKDiceLoss.forward -> (loss, dice_loss, logistic_loss, threshold) of `x` [N, C, ...] fp32 -- probabilities,
    or with from_logits the logits of an nn.Identity head -- against `target` in [0, 1]: the Dice term of
    hybrid_logistic_dice_loss plus the cross-entropy averaged over the k hardest voxels of the whole batch.
    top_k: the fraction of the voxels in (0, 1] (k = topk_count(N, S, top_k)), or a 0-dim int64 device tensor holding k
    itself, which the kernels read -- a captured step follows it.  threshold: the k-th largest per-voxel cross-entropy.
    class_weights: an fp32 device tensor [C] or None.  The gradient flows through `loss`."""
    return _TopKLossFn.apply(x, target, top_k, dice_weight, class_weights, square_dice, from_logits)


# ------------------------------------- segmented sort and the Lovasz-softmax loss (csrc/lovasz_loss.hip)
def segmented_sort(keys):
    """The rows of `keys` (int32 [R, M] on the device, values >= 0) sorted ascending, each row by itself: a stable LSD
    radix sort over the 31 value bits (csrc/segmented_sort.hip).  Returns a new tensor; nothing is read on the host, a
    call repeats bit for bit and can be captured in a graph.  A negative value keeps its sign bit but is ordered by its
    low 31 bits."""
    if not isinstance(keys, torch.Tensor) or keys.dtype != torch.int32:
        got = keys.dtype if isinstance(keys, torch.Tensor) else type(keys).__name__
        raise _lib.M355Error(f"segmented_sort: keys: element type {got} (expected torch.int32)")
    if keys.dim() != 2 or keys.numel() == 0:
        raise _lib.M355Error(f"segmented_sort: keys of shape {tuple(keys.shape)}: expected a non-empty [R, M]")
    _require(keys, dtype=torch.int32)
    L = _lib.lib()
    keys = keys.contiguous()
    R, M = keys.shape
    out = torch.empty_like(keys)
    with torch.cuda.device(keys.device):
        ws = _workspace(L.m355_segmented_sort_workspace(R, M), keys.device)
        check(L.m355_segmented_sort_u32(_p(keys), _p(out), R, M, 31, _p(ws), ws.numel(), _stream()), "segmented_sort_u32")
    return out


LOVASZ_CLASSES = ("present", "all")


class _LovaszLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t, classes, per_image, class_weights):
        L = _lib.lib()
        p, t, (cw,), N, Cc, S = _loss_operands((("prediction", p), ("target", t)), (("class_weights", class_weights),))
        pi = 1 if per_image else 0
        R, M = (N * Cc, S) if pi else (Cc, N * S)
        out2 = torch.empty(2, dtype=torch.float32, device=p.device)
        # saved: not the workspace, which the next op reuses -- 8 bytes per (class, voxel)
        skeys = torch.empty(R * M, dtype=torch.int32, device=p.device)
        F = torch.empty(R * M, dtype=torch.int32, device=p.device)
        state = torch.empty(2 * R, dtype=torch.int32, device=p.device)   # {G, coefficient} per segment
        ws = _workspace(L.m355_lovasz_loss_workspace(N, Cc, S, pi), p.device)
        check(L.m355_lovasz_loss_fwd(_p(p), _p(t), N, Cc, S, pi, 1 if classes == "all" else 0, _p(cw), _p(out2), _p(skeys),
                                     _p(F), _p(state), _p(ws), ws.numel(), _stream()), "lovasz_loss_fwd")
        ctx.args = (N, Cc, S, pi)
        ctx.save_for_backward(p, t, skeys, F, state)
        return torch.empty((), dtype=torch.float32, device=p.device).set_(out2.untyped_storage(), 0, ())

    @staticmethod
    def backward(ctx, dloss):
        L = _lib.lib()
        p, t, skeys, F, state = ctx.saved_tensors
        N, Cc, S, pi = ctx.args
        dx = torch.empty_like(p)
        check(L.m355_lovasz_loss_bwd(_p(p), _p(t), _p(skeys), _p(F), _p(state), _p(_dloss32(dloss)), N, Cc, S, pi, _p(dx),
                                     _stream()), "lovasz_loss_bwd")
        return dx, None, None, None, None


def lovasz_loss(prediction, target, classes='present', per_image=False, class_weights=None):
    """The Lovasz-softmax loss of Berman et al., a 0-dim tensor: the convex surrogate of the Jaccard index
    of the fp32 probabilities `prediction` [N, C, ...] against `target` (a voxel is foreground of channel c where
    target >= 0.5), one binary problem per channel -- so it serves a softmax and a sigmoid head alike.
    per_image=False: one Jaccard surrogate per channel over the whole batch; True: per (n, c), averaged per image first.
    classes: 'present' averages the channels that have a foreground voxel, 'all' every channel; class_weights: an fp32
    device tensor [C] of values >= 0 or None; nothing to average gives 0.  Elements with equal errors share the mean of
    their subgradients, so loss and gradient repeat bit for bit.  A NaN or a prediction outside [0, 1] gives a NaN loss and
    gradient.  Nothing is read on the host.  The gradient flows to the prediction only."""
    if classes not in LOVASZ_CLASSES:
        raise ValueError(f"lovasz_loss: classes = {classes!r}: expected 'present' or 'all'")
    return _LovaszLossFn.apply(prediction, target, classes, bool(per_image), class_weights)


class _BoundaryLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, phi, class_weights):
        L = _lib.lib()
        p, phi, (cw,), N, Cc, S = _loss_operands((("prediction", p), ("phi", phi)), (("class_weights", class_weights),))
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        ws = _workspace(L.m355_boundary_loss_workspace(N, Cc, S), p.device)
        check(L.m355_boundary_loss_fwd(_p(p), _p(phi), _p(cw), N, Cc, S, _p(loss), _p(ws), ws.numel(), _stream()),
              "boundary_loss_fwd")
        ctx.args = (N, Cc, S)
        ctx.save_for_backward(phi, cw)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        L = _lib.lib()
        phi, cw = ctx.saved_tensors
        N, Cc, S = ctx.args
        dp = torch.empty_like(phi)
        check(L.m355_boundary_loss_bwd(_p(phi), _p(_dloss32(dloss)), _p(cw), N, Cc, S, _p(dp), _stream()), "boundary_loss_bwd")
        return dp, None, None


def boundary_loss(p, phi, class_weights=None):
    """The boundary loss of Kervadec et al.: sum_c w_c sum p phi / (N S sum_c w_c), a 0-dim tensor, of the
    fp32 probabilities `p` [N, C, ...] and the signed distance map `phi` of the target (ops.signed_distance).
    class_weights: an fp32 device tensor [C] of values >= 0 with a positive sum, or None for all ones; a channel with
    weight 0 is not read and gets a zero gradient.  The gradient flows to `p` only."""
    return _BoundaryLossFn.apply(p, phi, class_weights)


# ------------------------------------------------------- blob (lesion-wise) Dice loss (csrc/blob_loss.hip)
def _blob_planes(planes, n_planes, what):
    """planes: None for all, or N * C flags ([N][C] order) -> (host byte array or None, tuple of flags)"""
    if planes is None:
        return None, (True,) * n_planes
    flags = tuple(bool(v) for v in (planes.flatten().tolist() if isinstance(planes, torch.Tensor) else planes))
    if len(flags) != n_planes:
        raise _lib.M355Error(f"{what}: {len(flags)} plane flags for N * C = {n_planes} planes")
    if not any(flags):
        raise _lib.M355Error(f"{what}: no plane is on")
    return (C.c_uint8 * n_planes)(*flags), flags


def _blob_target(target, what):
    if not isinstance(target, torch.Tensor) or target.dtype != torch.float32:
        got = target.dtype if isinstance(target, torch.Tensor) else type(target).__name__
        raise _lib.M355Error(f"{what}: target: element type {got} (expected torch.float32)")
    if target.dim() != 5:
        raise _lib.M355Error(f"{what}: target: expected [N, C, D, H, W], got shape {tuple(target.shape)}")


def _blob_connectivity(connectivity, what):
    if connectivity not in (1, 2, 3):
        raise _lib.M355Error(f"{what}: connectivity {connectivity!r} not in (1, 2, 3): 6, 18 or 26 neighbours")
    return int(connectivity)


def _blob_label(target, on, n_on, connectivity):
    L = _lib.lib()
    n_planes, (D, H, W) = target.shape[0] * target.shape[1], target.shape[2:]
    labels = torch.empty((n_on, D, H, W), dtype=torch.int32, device=target.device)
    ranges = torch.empty((n_on, 2), dtype=torch.int32, device=target.device)
    count = torch.empty((), dtype=torch.int32, device=target.device)
    ws = _workspace(L.m355_blob_label_workspace(n_planes, on, D, H, W), target.device)
    check(L.m355_blob_label(_p(target), n_planes, on, D, H, W, connectivity, _p(labels), _p(ranges), _p(count), _p(ws),
                            ws.numel(), _stream()), "blob_label")
    return labels, ranges, count


def blob_labels(target, planes=None, connectivity=3):
    """The connected components of every on plane of `target` (float32 [N, C, D, H, W], contiguous, on the device; a voxel
    is a member when target > 0.5, a NaN is none) in one labelling, without a synchronisation.
    planes: None for all, or N * C host flags ([N][C] order); the P_on planes that are on take the slots 0 .. P_on - 1 in
    plane order.  connectivity 1 | 2 | 3: 6, 18, 26 neighbours.
    -> (labels int32 [P_on, D, H, W]: 0 outside, else the component's number; ranges int32 [P_on, 2]: the components of
    slot s are the numbers ranges[s, 0] .. ranges[s, 1] (last = first - 1: none), numbered in raster order of their first
    voxel like scipy.ndimage.label's, shifted by first - 1; count: a 0-dim int32 device tensor, the number of components of
    all planes, or -1 when the labelling hit a loop bound)."""
    _blob_target(target, "blob_labels")
    connectivity = _blob_connectivity(connectivity, "blob_labels")
    on, flags = _blob_planes(planes, target.shape[0] * target.shape[1], "blob_labels")
    _dist_arg(target, (torch.float32,), "blob_labels: target")
    with torch.cuda.device(target.device):
        return _blob_label(target, on, sum(flags), connectivity)


class _BlobDiceLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t, class_weights, flags, square_dice, connectivity):
        L = _lib.lib()
        p, t, (cw,), N, Cc, _ = _loss_operands((("prediction", p), ("target", t)), (("class_weights", class_weights),))
        D, H, W = p.shape[2:]
        on = None if all(flags) else (C.c_uint8 * (N * Cc))(*flags)
        sq = 1 if square_dice else 0
        with torch.cuda.device(p.device):
            labels, ranges, count = _blob_label(t, on, sum(flags), connectivity)
            loss = torch.empty((), dtype=torch.float32, device=p.device)
            total = torch.empty((), dtype=torch.int32, device=p.device)
            tables = torch.empty(int(L.m355_blob_dice_tables(N * Cc, on, D, H, W, connectivity)), dtype=torch.uint8,
                                 device=p.device)             # saved: not the workspace, which the next op reuses
            ws = _workspace(L.m355_blob_dice_workspace(N * Cc, on, D, H, W, connectivity), p.device)
            check(L.m355_blob_dice_fwd(_p(p), _p(labels), _p(ranges), _p(count), _p(cw), N, Cc, on, D, H, W, connectivity,
                                       sq, _p(loss), _p(total), _p(tables), tables.numel(), _p(ws), ws.numel(), _stream()),
                  "blob_dice_fwd")
        ctx.args = (N, Cc, D, H, W, on, connectivity, sq)
        ctx.save_for_backward(p if sq else None, labels, tables)
        ctx.mark_non_differentiable(total)
        return loss, total

    @staticmethod
    def backward(ctx, dloss, _dtotal):
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        p, labels, tables = ctx.saved_tensors
        N, Cc, D, H, W, on, connectivity, sq = ctx.args
        dp = torch.empty((N, Cc, D, H, W), dtype=torch.float32, device=labels.device)
        with torch.cuda.device(labels.device):
            check(_lib.lib().m355_blob_dice_bwd(_p(p), _p(labels), _p(tables), _p(_dloss32(dloss)), N, Cc, on, D, H, W,
                                                connectivity, sq, _p(dp), _stream()), "blob_dice_bwd")
        return (dp,) + (None,) * 5


def blob_default_class_weights(channels):
    """0 for channel 0 (the background) when there is more than one channel, 1 otherwise: BoundaryLoss's convention"""
    return (0.0,) + (1.0,) * (channels - 1) if channels > 1 else (1.0,)


def blob_dice_loss(prediction, target, class_weights=None, square_dice=True, connectivity=3, planes=None):
    """The lesion-wise (blob) Dice of Kofler et al. -> (loss, count): the Dice term of
    hybrid_logistic_dice_loss once per connected component of the target (target > 0.5; `connectivity` 1 | 2 | 3) with the
    other components of its (n, c) plane masked out of prediction and target, averaged over the components of a plane and
    over the planes by their channel weights; 0 when no plane has a component.  count: a 0-dim int32 device tensor, the
    number of components (-1, with a NaN loss, when the labelling hit a loop bound).  prediction, target: fp32
    [N, C, D, H, W] on the device; the prediction must hold probabilities: a value that is not finite or outside [0, 1] in
    a plane that is on gives a NaN loss and gradient, nothing raises.
    class_weights: None (0 for channel 0 when C > 1, else 1), a sequence of C host numbers >= 0 -- channels of weight 0 are
    off: not labelled, not read, zero gradient --, or an fp32 device tensor [C], which is not read on the host: then
    `planes` (N * C host flags, [N][C] order; None: all) says which planes are on.  The gradient flows to the prediction
    only; nothing is read on the host."""
    what = "blob_dice_loss"
    _blob_target(target, what)
    connectivity = _blob_connectivity(connectivity, what)
    N, Cc = target.shape[0], target.shape[1]
    if not isinstance(class_weights, torch.Tensor):
        values = blob_default_class_weights(Cc) if class_weights is None else tuple(float(v) for v in class_weights)
        if len(values) != Cc:
            raise _lib.M355Error(f"{what}: class_weights of {len(values)} values for {Cc} channels")
        if any(not (math.isfinite(v) and v >= 0) for v in values) or not sum(values) > 0:
            raise _lib.M355Error(f"{what}: class_weights = {values}: expected finite values >= 0 with a positive sum")
        if planes is not None:
            raise _lib.M355Error(f"{what}: planes goes with a device tensor of class weights; host weights say which "
                                 f"planes are on themselves")
        flags = tuple(v > 0 for v in values) * N
        _require(prediction, target)
        class_weights = torch.tensor(values, dtype=torch.float32, device=prediction.device)
    else:
        _, flags = _blob_planes(planes, N * Cc, what)
    return _BlobDiceLossFn.apply(prediction, target, class_weights, flags, bool(square_dice), connectivity)


# ------------------------------------------------------------- target pyramid
PYRAMID_MODES = {"area": 0, "nearest": 1}   # M355_PYRAMID_AREA, M355_PYRAMID_NEAREST
PYRAMID_MAX_LEVELS = 4


def target_pyramid(y, levels, mode='area'):
    """The targets of `levels` auxiliary heads (criterions.DeepSupervisionLoss): [level 1, ..., level `levels`]
    of the fp32 target `y` [N, C, D, H, W], level j of spatial size (D, H, W) / 2^j -- mode 'area' the mean of the 2^j cube
    (F.avg_pool3d(y, 2**j)), 'nearest' the voxel at (z, y, x) * 2^j (F.interpolate(..., mode='nearest')).  One launch reads
    `y` once and writes every level; the levels are views of one allocation and carry no autograd history."""
    if mode not in PYRAMID_MODES:
        raise ValueError(f"target_pyramid: mode {mode!r} is neither 'area' nor 'nearest'")
    if y.dtype != torch.float32:
        raise _lib.M355Error(f"target: expected torch.float32, got {y.dtype}")
    if y.dim() != 5:
        raise _lib.M355Error(f"target {tuple(y.shape)}: expected [N, C, D, H, W]")
    levels = int(levels)
    N, Cc, D, H, W = y.shape
    if 1 <= levels <= PYRAMID_MAX_LEVELS:
        for name, size in (("D", D), ("H", H), ("W", W)):
            if size % (1 << levels):
                raise _lib.M355Error(f"target_pyramid: {name} = {size} is not divisible by {1 << levels} (2^levels)")
    _require(y)
    L = _lib.lib()
    y = y.detach().contiguous()
    out = torch.empty(max(int(L.m355_target_pyramid_elems(N, Cc, D, H, W, levels)), 1), dtype=torch.float32, device=y.device)
    check(L.m355_target_pyramid(_p(y), N, Cc, D, H, W, levels, PYRAMID_MODES[mode], _p(out), _stream()), "target_pyramid")
    views, off = [], 0
    for j in range(1, levels + 1):
        shape = (N, Cc, D >> j, H >> j, W >> j)
        n = N * Cc * shape[2] * shape[3] * shape[4]
        views.append(out[off:off + n].view(shape))
        off += n
    return views


# ---------------------------------------------------------------- elementwise
class _ChannelScaleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        L = _lib.lib()
        _require(x, scale)
        x = x.contiguous()
        N, Cc = x.shape[0], x.shape[1]
        S = x.numel() // (N * Cc)
        y = torch.empty_like(x)
        check(L.m355_channel_scale(_p(x), _p(scale), _p(y), N, Cc, S, _stream()), "channel_scale")
        ctx.save_for_backward(scale)
        ctx.dims = (N, Cc, S)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        (scale,) = ctx.saved_tensors
        N, Cc, S = ctx.dims
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        check(L.m355_channel_scale(_p(dy), _p(scale), _p(dx), N, Cc, S, _stream()), "channel_scale")
        return dx, None


def _channel_scale_c8(src_ptr, sbs, scale, dst_ptr, dbs, N, Cc, S, compute):
    check(_lib.lib().m355_act16_channel_scale(src_ptr, _p(scale), dst_ptr, N, Cc, S, sbs, dbs, compute, _stream()),
          "act16_channel_scale")


class _ChannelScaleC8Fn(torch.autograd.Function):
    """Dropout3d with a pre-drawn mask on a c8 activation (into its concat slot); backward: the same kernel on the c8
    gradient"""

    @staticmethod
    def forward(ctx, x_t, scale, x: Act16, y16: Act16):
        N, Cc = x.shape[:2]
        _channel_scale_c8(x.ptr(), x.batch_stride(), scale, y16.ptr(), y16.batch_stride(), N, Cc, x.S, x.compute)
        ctx.info = (N, Cc, x.S, x.compute)
        ctx.save_for_backward(scale)
        return y16.alias()

    @staticmethod
    def backward(ctx, dy16):
        (scale,) = ctx.saved_tensors
        N, Cc, S, compute = ctx.info
        dy16, dybs = _c8t(dy16)
        dx16 = _c8_grad(N, Cc, S, compute, dy16.device)
        _channel_scale_c8(_p(dy16), dybs, scale, _p(dx16), 0, N, Cc, S, compute)
        return dx16, None, None, None


def channel_scale(x, scale, out: Optional[OutSlot] = None):
    """y[n,c,...] = x[n,c,...] * scale[n,c]  (Dropout3d with a pre-drawn mask); `out`: written into this concat slot.
    A c8 activation stays c8."""
    scale = scale.contiguous().view(-1)
    if isinstance(x, Act16):
        _require(scale)
        y16 = _c8_out_slot(x, out, x.spatial)
        if _act16_tracks(x):
            return y16.with_t(_ChannelScaleC8Fn.apply(x.t, scale, x, y16))
        _channel_scale_c8(x.ptr(), x.batch_stride(), scale, y16.ptr(), y16.batch_stride(), x.shape[0], x.C, x.S, x.compute)
        return y16
    y = _ChannelScaleFn.apply(x, scale)
    return y if out is None else copy_into(y, out)


class _AddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        L = _lib.lib()
        _require(a, b)
        a, b = a.contiguous(), b.contiguous()
        y = torch.empty_like(a)
        check(L.m355_add(_p(a), _p(b), _p(y), a.numel(), _stream()), "add")
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


def add(a, b):
    return _AddFn.apply(as_f32(a), as_f32(b))


class _CopyIntoFn(torch.autograd.Function):
    """Copy a tensor into a concat slot (the generic torch.cat path for producers
    that cannot write into the buffer themselves)."""

    @staticmethod
    def forward(ctx, x, out):
        L = _lib.lib()
        _require(x)
        x, xbs = _dense_channels(x)
        N, Cc = x.shape[0], x.shape[1]
        S = x.shape[2] * x.shape[3] * x.shape[4]
        y = _alloc_out(out, x.shape, x)
        y, ybs = _dense_channels(y)
        check(L.m355_copy_channels(_p(x), _p(y), N, Cc, S, xbs, ybs, _stream()), "copy_channels")
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, None


def copy_into(x, out: OutSlot):
    if out.buf16 is not None:   # c8 flow: the slot lives in the c8 twin of the concat buffer
        return pack_act16(as_f32(x), out.buf16.compute, out.act16())
    return _CopyIntoFn.apply(as_f32(x), out)


class _BlurWeightFn(torch.autograd.Function):
    """Blur-convolution weight transform (reference models/components.py:112-119, 145-152) ->
    sparse 3x3x3 filter of the space-to-depth formulation; see m355_blur_weight_fwd."""

    @staticmethod
    def forward(ctx, w, scale, standardize, transposed):
        L = _lib.lib()
        _require(w, scale)
        w, scale = w.contiguous(), scale.contiguous()
        A, B = w.shape[0], w.shape[1]
        shape = (8 * B, A, 3, 3, 3) if transposed else (A, 8 * B, 3, 3, 3)
        wexp = torch.empty(shape, dtype=w.dtype, device=w.device)
        ms = torch.empty((A, 2), dtype=torch.float32, device=w.device) if standardize else None
        check(L.m355_blur_weight_fwd(_p(w), _p(scale), _p(wexp), _p(ms), A, B, int(standardize), int(transposed),
                                     _stream()), "blur_weight_fwd")
        ctx.flags = (A, B, int(standardize), int(transposed))
        ctx.save_for_backward(w, scale, ms)
        return wexp

    @staticmethod
    def backward(ctx, dwexp):
        L = _lib.lib()
        w, scale, ms = ctx.saved_tensors
        A, B, standardize, transposed = ctx.flags
        dw = torch.empty_like(w)
        check(L.m355_blur_weight_bwd(_p(dwexp.contiguous()), _p(w), _p(scale), _p(ms), _p(dw), A, B, standardize,
                                     transposed, _stream()), "blur_weight_bwd")
        return dw, None, None, None


def blur_weight(w, scale, standardize=False, transposed=False):
    """[A, B, 3, 3, 3] module weight -> conv3d weight of the space-to-depth form of the Blur convs:
    [A, 8B, 3, 3, 3] (strided conv) or [8B, A, 3, 3, 3] (transposed conv).  `scale`: [B] values of the
    module's `kernel` buffer."""
    if tuple(w.shape[2:]) != (3, 3, 3) or scale.numel() != w.shape[1]:
        raise _lib.M355Error(f"blur_weight: needs a 3x3x3 filter and one scale per dim-1 channel, got {tuple(w.shape)}")
    return _BlurWeightFn.apply(w, scale, bool(standardize), bool(transposed))


class _WeightStandardizeFn(torch.autograd.Function):
    """WSConv3d's (w - mean) / (std + 1e-5) per output filter (reference models/components.py:81-88)."""

    @staticmethod
    def forward(ctx, w):
        L = _lib.lib()
        _require(w)
        w = w.contiguous()
        A, n = w.shape[0], w[0].numel()
        wn = torch.empty_like(w)
        ms = torch.empty((A, 2), dtype=torch.float32, device=w.device)
        check(L.m355_weight_standardize_fwd(_p(w), _p(wn), _p(ms), A, n, _stream()), "weight_standardize_fwd")
        ctx.save_for_backward(w, ms)
        return wn

    @staticmethod
    def backward(ctx, dwn):
        L = _lib.lib()
        w, ms = ctx.saved_tensors
        dw = torch.empty_like(w)
        check(L.m355_weight_standardize_bwd(_p(dwn.contiguous()), _p(w), _p(ms), _p(dw), w.shape[0], w[0].numel(),
                                            _stream()), "weight_standardize_bwd")
        return dw


def weight_standardize(w):
    return _WeightStandardizeFn.apply(w)


# --------------------------------------------------- sliding window / evaluation
def patch_gather(volume, locations, patch_size):
    """volume [C,V0,V1,V2], locations int32 [P,3] (i0,j0,k0) -> patches [P,C,*patch_size]"""
    L = _lib.lib()
    _require(volume)
    _require(locations, dtype=torch.int32)
    volume, locations = volume.contiguous(), locations.contiguous()
    Cc, V0, V1, V2 = volume.shape
    P = locations.shape[0]
    ps0, ps1, ps2 = patch_size
    patches = torch.empty((P, Cc, ps0, ps1, ps2), dtype=volume.dtype, device=volume.device)
    check(L.m355_patch_gather(_p(volume), _p(locations), _p(patches), P, Cc, V0, V1, V2, ps0, ps1, ps2,
                              _stream()), "patch_gather")
    return patches


def sampler_build(prob_map, patch_size):
    """cumulative table of a [V0, V1, V2] probability map for `sampler_draw` (float64, (V / 1024 + 1) entries, the last
    one the total weight of the centres whose patch fits)"""
    L = _lib.lib()
    _require(prob_map)
    prob_map = prob_map.contiguous()
    V0, V1, V2 = prob_map.shape
    table = torch.empty(int(L.m355_sampler_table_bytes(V0, V1, V2)) // 8, dtype=torch.float64, device=prob_map.device)
    check(L.m355_sampler_build(_p(prob_map), V0, V1, V2, *[int(p) for p in patch_size], _p(table), _stream()), "sampler_build")
    return table


def sampler_draw(prob_map, table, patch_size, u):
    """u: float64 [P] uniform in [0, 1) on the device -> int32 [P, 3] patch corners (tio.WeightedSampler semantics)"""
    L = _lib.lib()
    _require(prob_map)
    _require(table, u, dtype=torch.float64)
    V0, V1, V2 = prob_map.shape
    P = u.numel()
    loc = torch.empty((P, 3), dtype=torch.int32, device=prob_map.device)
    check(L.m355_sampler_draw(_p(prob_map), _p(table), V0, V1, V2, *[int(p) for p in patch_size], _p(u.contiguous()), P,
                              _p(loc), _stream()), "sampler_draw")
    return loc


PAD_MODES = {"constant": 0, "edge": 1, "reflect": 2, "symmetric": 3, "wrap": 4}


def patch_gather_padded(volume, locations, patch_size, border, mode, value=0.0):
    """As patch_gather on the volume padded by `border` voxels per side (numpy.pad mode `mode`, or 'constant' with
    `value`) -- locations in PADDED coordinates; the padded volume is never materialised."""
    L = _lib.lib()
    _require(volume)
    _require(locations, dtype=torch.int32)
    volume, locations = volume.contiguous(), locations.contiguous()
    Cc, V0, V1, V2 = volume.shape
    P = locations.shape[0]
    ps0, ps1, ps2 = patch_size
    patches = torch.empty((P, Cc, ps0, ps1, ps2), dtype=volume.dtype, device=volume.device)
    check(L.m355_patch_gather_padded(_p(volume), _p(locations), _p(patches), P, Cc, V0, V1, V2, ps0, ps1, ps2,
                                     border[0], border[1], border[2], PAD_MODES[mode], float(value), _stream()),
          "patch_gather_padded")
    return patches


def patch_finalize_crop(accum, count, border):
    """accum [C, P0, P1, P2] / count with `border` voxels cropped off every side."""
    L = _lib.lib()
    _require(accum, count)
    Cc, P0, P1, P2 = accum.shape
    out = torch.empty((Cc, P0 - 2 * border[0], P1 - 2 * border[1], P2 - 2 * border[2]), dtype=accum.dtype,
                      device=accum.device)
    check(L.m355_patch_finalize_crop(_p(accum), _p(count), _p(out), Cc, P0, P1, P2, border[0], border[1], border[2],
                                     _stream()), "patch_finalize_crop")
    return out


def patch_accumulate(patches, locations, accum, count):
    """accum[C,V] += patches (in patch order), count[V] += 1 over each patch footprint"""
    L = _lib.lib()
    _require(patches, accum, count)
    _require(locations, dtype=torch.int32)
    patches, locations = patches.contiguous(), locations.contiguous()
    P, Cc, ps0, ps1, ps2 = patches.shape
    _, V0, V1, V2 = accum.shape
    check(L.m355_patch_accumulate(_p(patches), _p(locations), _p(accum), _p(count), P, Cc, V0, V1, V2,
                                  ps0, ps1, ps2, _stream()), "patch_accumulate")


def patch_aggregate_grid(tiles, axes, volume_shape, border=(0, 0, 0), window=None):
    """tiles [n0*n1*n2, C, *patch] in GridSampler order over the per-axis start lists `axes` (padded coordinates) ->
    the averaged volume [C, *volume_shape] (the padded volume's interior when `border` > 0); one pass.
    window: None (plain average), or three 1-D fp32 tensors, one per axis and as long as the patch: the covering tiles
    are blended with the weight (w0[d0] * w1[d1]) * w2[d2] (prediction.hann_window_axes for overlap_mode='hann')."""
    L = _lib.lib()
    _require(tiles)
    tiles = tiles.contiguous()
    P, Cc, ps0, ps1, ps2 = tiles.shape
    n0, n1, n2 = (len(a) for a in axes)
    if P != n0 * n1 * n2:
        raise _lib.M355Error(f"patch_aggregate_grid: {P} tiles for a {n0} x {n1} x {n2} grid")
    if window is not None:
        window = list(window)
        if len(window) != 3 or any(not torch.is_tensor(w) or w.dim() != 1 or w.dtype != torch.float32 for w in window):
            raise _lib.M355Error("patch_aggregate_grid: window must be three 1-D float32 tensors")
        if tuple(w.numel() for w in window) != (ps0, ps1, ps2):
            raise _lib.M355Error(f"patch_aggregate_grid: window lengths {tuple(w.numel() for w in window)} for "
                                 f"{ps0} x {ps1} x {ps2} tiles")
        window = torch.cat(window).to(tiles.device)         # w0 | w1 | w2: one copy when the window lives on the host
    starts = torch.tensor([int(v) for a in axes for v in a], dtype=torch.int32, device=tiles.device)
    out = torch.empty((Cc,) + tuple(volume_shape), dtype=torch.float32, device=tiles.device)
    if window is None:
        check(L.m355_patch_aggregate_grid(_p(tiles), _p(starts), n0, n1, n2, _p(out), Cc, *[int(v) for v in volume_shape], ps0,
                                          ps1, ps2, *[int(b) for b in border], _stream()), "patch_aggregate_grid")
    else:
        check(L.m355_patch_aggregate_grid_weighted(_p(tiles), _p(starts), n0, n1, n2, _p(window), _p(out), Cc,
                                                   *[int(v) for v in volume_shape], ps0, ps1, ps2, *[int(b) for b in border],
                                                   _stream()), "patch_aggregate_grid_weighted")
    return out


def patch_finalize(accum, count):
    L = _lib.lib()
    _require(accum, count)
    Cc = accum.shape[0]
    V = count.numel()
    out = torch.empty_like(accum)
    check(L.m355_patch_finalize(_p(accum), _p(count), _p(out), Cc, V, _stream()), "patch_finalize")
    return out


def argmax_confusion(prob, target):
    """prob [N,C,...] float, target [N,...] int32 -> (argmax int32 [N,...], counts int64 [N,C,4] = TP,FP,FN,TN)"""
    L = _lib.lib()
    _require(prob)
    _require(target, dtype=torch.int32)
    prob, target = prob.contiguous(), target.contiguous()
    N, Cc = prob.shape[0], prob.shape[1]
    S = prob.numel() // (N * Cc)
    am = torch.empty(target.shape, dtype=torch.int32, device=prob.device)
    counts = torch.empty((N, Cc, 4), dtype=torch.int64, device=prob.device)
    check(L.m355_argmax_confusion(_p(prob), _p(target), _p(am), _p(counts), N, Cc, S, _stream()),
          "argmax_confusion")
    return am, counts


# ----------------------------------------------------------------- evaluation counts (csrc/evaluate.hip)
_EV_MAP_DTYPE = {torch.bool: _lib.EV_BOOL, torch.uint8: _lib.EV_U8, torch.int8: _lib.EV_I8, torch.int16: _lib.EV_I16,
                 torch.int32: _lib.EV_I32, torch.int64: _lib.EV_I64, torch.float32: _lib.EV_F32}
_EV_SCORE_DTYPE = {torch.float32: _lib.EV_F32, torch.bfloat16: _lib.EV_BF16, torch.float16: _lib.EV_F16}
_EV_LABEL_LIMIT = 2 ** 31 - 128   # float32(v) of a label must stay inside int32


def _ev_code(t, table, what):
    if t.dtype not in table:
        raise _lib.M355Error(f"{what}: element type {t.dtype} (one of {', '.join(str(d) for d in table)})")
    if not t.is_cuda:
        raise _lib.M355Error(f"{what}: expected a device tensor")
    return table[t.dtype]


def _ev_labels(labels):
    """-> (int32 ctypes array, L, nokey).  nokey: an int32 that no label takes in any element type's cast"""
    labels = [int(v) for v in labels]
    if not 1 <= len(labels) <= _lib.EV_MAX_LABELS:
        raise _lib.M355Error(f"{len(labels)} label values (1 .. {_lib.EV_MAX_LABELS})")
    if len(set(labels)) != len(labels):
        raise _lib.M355Error(f"label values {labels} are not distinct")
    if any(abs(v) >= _EV_LABEL_LIMIT for v in labels):
        raise _lib.M355Error(f"label values {labels}: |value| must be below {_EV_LABEL_LIMIT}")
    keys = set()
    for v in labels:
        keys.update((v, v & 0xFF, (v + 128) % 256 - 128, (v + 32768) % 65536 - 32768, int(np.float32(v))))
    nokey = -2 ** 31
    while nokey in keys:
        nokey += 1
    return (C.c_int32 * len(labels))(*labels), len(labels), nokey


def eval_confusion(preds, targets, labels):
    """counts int64 [n, L, 3] = (TP, FP, FN) of label maps preds[i] against targets[i] (None: no target; TP + FP is
    the volume) for the distinct int label values `labels`, every subject in one launch.  Maps: device tensors of
    bool / (u)int8 / int16 / int32 / int64 / float32 holding integers, any shape, a target as many voxels as its
    prediction.  `data == value` semantics of torch (the value cast to the map's type first)."""
    if len(preds) != len(targets) or not preds:
        raise _lib.M355Error("eval_confusion: one target (or None) per prediction, at least one subject")
    arr, L, nokey = _ev_labels(labels)
    n = len(preds)
    descs = (_lib.EvalMapDesc * n)()
    keep = []
    dev = preds[0].device
    for i, (p, t) in enumerate(zip(preds, targets)):
        p = p.contiguous()
        keep.append(p)
        descs[i].pred, descs[i].S = p.data_ptr(), p.numel()
        descs[i].pred_dtype = _ev_code(p, _EV_MAP_DTYPE, f"subject {i}: prediction")
        if p.device != dev:
            raise _lib.M355Error(f"subject {i} is on {p.device}, subject 0 on {dev}")
        if t is not None:
            t = t.contiguous()
            keep.append(t)
            if t.numel() != p.numel() or t.device != dev:
                raise _lib.M355Error(f"subject {i}: target of {t.numel()} voxels on {t.device}, prediction of "
                                     f"{p.numel()} on {dev}")
            descs[i].target, descs[i].target_dtype = t.data_ptr(), _ev_code(t, _EV_MAP_DTYPE, f"subject {i}: target")
    with torch.cuda.device(dev):
        dev_descs = torch.empty(C.sizeof(descs), dtype=torch.uint8, device=dev)
        counts = torch.empty((n, L, 3), dtype=torch.int64, device=dev)
        check(_lib.lib().m355_eval_confusion(descs, n, _p(dev_descs), arr, L, nokey, _p(counts), _stream()),
              "eval_confusion")
    return counts


def eval_scores(scores, table, labels, targets=None, masks=None, half=None, write_pred=False, write_target=False,
                one_hot_targets=True):
    """Counts straight from model scores.  scores: list of device tensors [C, *spatial] (float32 / bfloat16 /
    float16, one type and one C for all).  Per voxel: c = torch.argmax over the channels (first maximum, NaN wins),
    label = table[1][c] inside the mask, table[0][c] outside (table: two lists of C ints; without a mask only table[0]
    is used).  Mask: `half` = (axis, upper) for a half-space of the spatial axes, or `masks` = one label map per
    subject (its nonzero voxels).  targets[i]: None, a one-hot [C, *spatial] map (its argmax goes through the same
    table; one_hot_targets=True) or a label map [1, *spatial] (one_hot_targets=False).
    -> (counts int64 [n, L, 3], predicted label maps int64 [1, *spatial] or None, target label maps or None)."""
    n = len(scores)
    if n == 0:
        raise _lib.M355Error("eval_scores: no subject")
    targets = [None] * n if targets is None else list(targets)
    Cc = scores[0].shape[0]
    sd = _ev_code(scores[0], _EV_SCORE_DTYPE, "eval_scores: scores")
    if not 1 <= Cc <= _lib.EV_MAX_CHANNELS:
        raise _lib.M355Error(f"eval_scores: {Cc} channels (1 .. {_lib.EV_MAX_CHANNELS})")
    outside = [int(v) for v in table[0]]
    inside = [int(v) for v in table[1]] if (half is not None or masks is not None) else outside
    if len(outside) != Cc or len(inside) != Cc:
        raise _lib.M355Error(f"eval_scores: label table of {len(outside)} / {len(inside)} entries for {Cc} channels")
    if half is not None and masks is not None:
        raise _lib.M355Error("eval_scores: a half-space or mask maps, not both")
    arr, L, nokey = _ev_labels(labels)
    tab = (C.c_int32 * (2 * Cc))(*(outside + inside))
    mask_kind, axis, upper = _lib.EV_MASK_NONE, 0, 0
    if half is not None:
        mask_kind, axis, upper = _lib.EV_MASK_HALF, int(half[0]), int(bool(half[1]))
    elif masks is not None:
        mask_kind = _lib.EV_MASK_MAP
    descs = (_lib.EvalScoresDesc * n)()
    keep, pred_outs, target_outs = [], [], []
    dev = scores[0].device
    for i, s in enumerate(scores):
        if s.dim() != 4 or s.shape[0] != Cc or s.dtype != scores[0].dtype or s.device != dev:
            raise _lib.M355Error(f"eval_scores: subject {i}: scores {tuple(s.shape)} {s.dtype} on {s.device}; expected "
                                 f"[{Cc}, D, H, W] {scores[0].dtype} on {dev}")
        s = s.contiguous()
        sp = tuple(s.shape[1:])
        keep.append(s)
        d = descs[i]
        d.scores = s.data_ptr()
        d.size3[:] = sp
        t = targets[i]
        if t is not None:
            t = t.contiguous()
            keep.append(t)
            if t.device != dev or tuple(t.shape[-3:]) != sp or t.dim() not in (3, 4):
                raise _lib.M355Error(f"eval_scores: subject {i}: target {tuple(t.shape)} on {t.device} for scores "
                                     f"{tuple(s.shape)}")
            one_hot = bool(one_hot_targets)
            if t.numel() != (Cc if one_hot else 1) * s[0].numel():
                raise _lib.M355Error(f"eval_scores: subject {i}: {'one-hot' if one_hot else 'label map'} target "
                                     f"{tuple(t.shape)} for scores {tuple(s.shape)}")
            d.target, d.target_dtype = t.data_ptr(), _ev_code(t, _EV_MAP_DTYPE, f"subject {i}: target")
            d.target_kind = _lib.EV_TARGET_ONEHOT if one_hot else _lib.EV_TARGET_MAP
        if mask_kind == _lib.EV_MASK_MAP:
            m = masks[i].contiguous()
            keep.append(m)
            if m.numel() != s[0].numel() or m.device != dev:
                raise _lib.M355Error(f"eval_scores: subject {i}: mask {tuple(m.shape)} for scores {tuple(s.shape)}")
            d.mask, d.mask_dtype = m.data_ptr(), _ev_code(m, _EV_MAP_DTYPE, f"subject {i}: mask")
        po = torch.empty((1,) + sp, dtype=torch.int64, device=dev) if write_pred else None
        to = None
        if write_target and t is not None and d.target_kind == _lib.EV_TARGET_ONEHOT:
            to = torch.empty((1,) + sp, dtype=torch.int64, device=dev)
        d.pred_out, d.target_out = (po.data_ptr() if po is not None else None), (to.data_ptr() if to is not None else None)
        pred_outs.append(po)
        target_outs.append(to)
    with torch.cuda.device(dev):
        dev_descs = torch.empty(C.sizeof(descs), dtype=torch.uint8, device=dev)
        counts = torch.empty((n, L, 3), dtype=torch.int64, device=dev)
        check(_lib.lib().m355_eval_scores(descs, n, _p(dev_descs), sd, Cc, tab, mask_kind, axis, upper, arr, L, nokey,
                                          _p(counts), _stream()), "eval_scores")
    return counts, (pred_outs if write_pred else None), (target_outs if write_target else None)


_EV_TARGET_DTYPE = {**_EV_MAP_DTYPE, torch.bfloat16: _lib.EV_BF16, torch.float16: _lib.EV_F16}


def eval_multilabel(scores, targets, thresholds=0.5):
    """Thresholded counts of sigmoid scores: int64 [n, C, 3] = (TP, FP, FN) per subject and channel of
    `scores[i][c] > thresholds[c]` against `targets[i][c] != 0`, the channels independent, every subject of whatever
    size in one launch.  scores[i]: device tensors [C, *spatial] (float32 / bfloat16 / float16, one type and one C for
    all); targets[i]: the same shape, any evaluation element type or a 16-bit float.  thresholds: a float or C floats
    (+-inf allowed).  torch's comparison rules: a NaN score is not predicted, a NaN target is positive."""
    n = len(scores)
    if n == 0 or len(targets) != n:
        raise _lib.M355Error(f"eval_multilabel: {n} score maps and {len(targets)} targets; one target per subject, at "
                             "least one subject")
    Cc = scores[0].shape[0] if scores[0].dim() >= 1 else 0
    if not 1 <= Cc <= _lib.EV_MAX_CHANNELS:
        raise _lib.M355Error(f"eval_multilabel: {Cc} channels (1 .. {_lib.EV_MAX_CHANNELS})")
    thr = [float(thresholds)] * Cc if isinstance(thresholds, (int, float)) else [float(v) for v in thresholds]
    if len(thr) != Cc:
        raise _lib.M355Error(f"eval_multilabel: {len(thr)} thresholds for {Cc} channels")
    sd = _ev_code(scores[0], _EV_SCORE_DTYPE, "eval_multilabel: scores")
    descs = (_lib.EvalMultilabelDesc * n)()
    keep = []
    dev = scores[0].device
    for i, (s, t) in enumerate(zip(scores, targets)):
        if s.dim() < 2 or s.shape[0] != Cc or s.dtype != scores[0].dtype or s.device != dev:
            raise _lib.M355Error(f"eval_multilabel: subject {i}: scores {tuple(s.shape)} {s.dtype} on {s.device}; expected "
                                 f"[{Cc}, ...] {scores[0].dtype} on {dev}")
        if t is None or tuple(t.shape) != tuple(s.shape) or t.device != dev:
            raise _lib.M355Error(f"eval_multilabel: subject {i}: target "
                                 f"{None if t is None else (tuple(t.shape), t.device)} for scores {tuple(s.shape)} on {dev}")
        s, t = s.contiguous(), t.contiguous()
        keep += [s, t]
        d = descs[i]
        d.scores, d.target, d.S = s.data_ptr(), t.data_ptr(), s[0].numel()
        d.target_dtype = _ev_code(t, _EV_TARGET_DTYPE, f"eval_multilabel: subject {i}: target")
    with torch.cuda.device(dev):
        dev_descs = torch.empty(C.sizeof(descs), dtype=torch.uint8, device=dev)
        counts = torch.empty((n, Cc, 3), dtype=torch.int64, device=dev)
        check(_lib.lib().m355_eval_multilabel(descs, n, _p(dev_descs), sd, Cc, (C.c_float * Cc)(*thr), _p(counts),
                                              _stream()), "eval_multilabel")
    return counts


# ----------------------------------------------------------------- calibration (csrc/calibration.hip)
_EV_INDEX_DTYPE = {k: v for k, v in _EV_MAP_DTYPE.items() if k != torch.float32}
_CAL_KINDS = {'categorical': _lib.CAL_CATEGORICAL, 'binary': _lib.CAL_BINARY}


class CalibrationCounts(NamedTuple):
    """ops.eval_calibration's result, device tensors that are views of one buffer (`packed`, int64 words): top
    [n, B, 3] and classwise [n, C, B, 3] int64 entries (count, hits, conf_sum in 2^-32 fixed point); invalid int64 [n]
    (categorical: voxels) or [n, C] (binary: per channel); brier, nll float64 [n] (sums, not means); voxels int64 [n]."""
    top: torch.Tensor
    classwise: torch.Tensor
    invalid: torch.Tensor
    brier: torch.Tensor
    nll: torch.Tensor
    voxels: torch.Tensor
    packed: torch.Tensor

    @staticmethod
    def unpack(packed, n, channels, bins, kind):
        """the views of a packed buffer (on whatever device it lies: the evaluator copies `packed` back once)"""
        sizes = (n * bins * 3, n * channels * bins * 3, n * channels, n * 2, n)
        top, cls, inv, sums, vox = torch.split(packed, sizes)
        sums = sums.view(torch.float64).view(n, 2)
        inv = inv.view(n, channels)
        return CalibrationCounts(top.view(n, bins, 3), cls.view(n, channels, bins, 3),
                                 inv if kind == 'binary' else inv[:, 0], sums[:, 0], sums[:, 1], vox, packed)


def eval_calibration(scores, targets, bins=15, kind='categorical'):
    """Reliability tables, Brier and NLL sums of probabilities against targets, every subject of whatever size in one
    pass (include/m355seg.h states the definitions).  scores[i]: device tensors [C, *spatial] of PROBABILITIES (float32 /
    bfloat16 / float16, one type and one C for all).  targets[i]: all of one form -- the shape of scores[i] (a one-hot or
    soft map of any evaluation element type or a 16-bit float: channel c is positive where `!= 0`, the class is the first
    maximum), or one value per voxel ([*spatial] or [1, *spatial], an integer type: the channel index; outside [0, C) the
    voxel is invalid).  kind 'categorical' (softmax: top-label and classwise tables) or 'binary' (sigmoid: classwise
    only, every channel a problem of its own).  -> CalibrationCounts; nothing synchronises."""
    n = len(scores)
    if n == 0 or len(targets) != n:
        raise _lib.M355Error(f"eval_calibration: {n} score maps and {len(targets)} targets; one target per subject, at "
                             "least one subject")
    if kind not in _CAL_KINDS:
        raise _lib.M355Error(f"eval_calibration: kind {kind!r} (one of {tuple(_CAL_KINDS)})")
    bins = int(bins)
    if not 1 <= bins <= _lib.CAL_MAX_BINS:
        raise _lib.M355Error(f"eval_calibration: {bins} bins (1 .. {_lib.CAL_MAX_BINS})")
    Cc = scores[0].shape[0] if scores[0].dim() >= 1 else 0
    if not 1 <= Cc <= _lib.EV_MAX_CHANNELS:
        raise _lib.M355Error(f"eval_calibration: {Cc} channels (1 .. {_lib.EV_MAX_CHANNELS})")
    sd = _ev_code(scores[0], _EV_SCORE_DTYPE, "eval_calibration: scores")
    descs = (_lib.EvalCalibrationDesc * n)()
    keep = []
    dev = scores[0].device
    one_hot = None
    for i, (s, t) in enumerate(zip(scores, targets)):
        if s.dim() < 2 or s.shape[0] != Cc or s.dtype != scores[0].dtype or s.device != dev:
            raise _lib.M355Error(f"eval_calibration: subject {i}: scores {tuple(s.shape)} {s.dtype} on {s.device}; expected "
                                 f"[{Cc}, ...] {scores[0].dtype} on {dev}")
        sp = tuple(s.shape[1:])
        form = None
        if t is not None and t.device == dev:
            if tuple(t.shape) == tuple(s.shape):   # (with one channel [1, *spatial] is a map: pass an index as [*spatial])
                form = True
            elif tuple(t.shape) in (sp, (1,) + sp):
                form = False
        if form is None or (one_hot is not None and form != one_hot):
            raise _lib.M355Error(f"eval_calibration: subject {i}: target "
                                 f"{None if t is None else (tuple(t.shape), t.device)} for scores {tuple(s.shape)} on {dev}"
                                 "; all targets one-hot maps or all index maps")
        one_hot = form
        s, t = s.contiguous(), t.contiguous()
        keep += [s, t]
        d = descs[i]
        d.scores, d.target, d.S = s.data_ptr(), t.data_ptr(), s[0].numel()
        d.target_dtype = _ev_code(t, _EV_TARGET_DTYPE if one_hot else _EV_INDEX_DTYPE,
                                  f"eval_calibration: subject {i}: {'target' if one_hot else 'index map'}")
    with torch.cuda.device(dev):
        L = _lib.lib()
        dev_descs = torch.empty(C.sizeof(descs), dtype=torch.uint8, device=dev)
        packed = torch.empty(n * (bins * 3 * (1 + Cc) + Cc + 3), dtype=torch.int64, device=dev)
        out = CalibrationCounts.unpack(packed, n, Cc, bins, kind)
        nbytes = L.m355_eval_calibration_workspace(n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        base = packed.data_ptr()
        off = [0, n * bins * 3, n * bins * 3 * (1 + Cc), n * bins * 3 * (1 + Cc) + n * Cc, n * bins * 3 * (1 + Cc) + n * Cc + 2 * n]
        ptr = [C.c_void_p(base + 8 * o) for o in off]
        check(L.m355_eval_calibration(descs, n, _p(dev_descs), sd, _lib.EV_TARGET_ONEHOT if one_hot else _lib.EV_TARGET_MAP,
                                      Cc, bins, _CAL_KINDS[kind], ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], _p(ws), nbytes,
                                      _stream()), "eval_calibration")
    return out


# ----------------------------------------------------------------- uncertainty maps (csrc/uncertainty.hip)
_UQ_KINDS = {'categorical': _lib.UQ_CATEGORICAL, 'binary': _lib.UQ_BINARY}


def _uq_kind(kind, what):
    if kind not in _UQ_KINDS:
        raise _lib.M355Error(f"{what}: kind {kind!r} (one of {tuple(_UQ_KINDS)})")
    return _UQ_KINDS[kind]


def predictive_entropy(probs, kind='categorical', confidence=False):
    """Entropy map of probabilities [N, C, D, H, W] (float32 / bfloat16 / float16, on the device), natural logarithm,
    float32: 'categorical' -sum_c p_c log p_c -> [N, 1, D, H, W]; 'binary' -p log p - (1 - p) log(1 - p) of every
    channel -> [N, C, D, H, W].  0 log 0 is 0; a NaN makes its voxel NaN and no other.  confidence=True: -> (entropy,
    the maximum channel value [N, 1, D, H, W]).  One pass.  The same expression the ensembles' uncertainty maps use, so
    `predictive_entropy(mean)` has the bits of their 'entropy'.  On a blended PatchPredict volume this is the tool for an
    uncertainty map: the member-wise terms (expected entropy, mutual information) are not aggregated over tiles."""
    k = _uq_kind(kind, "predictive_entropy")
    if probs.dim() < 3:
        raise _lib.M355Error(f"predictive_entropy: probabilities {tuple(probs.shape)}; expected [N, C, *spatial]")
    sd = _ev_code(probs, _EV_SCORE_DTYPE, "predictive_entropy")
    probs = probs.contiguous()
    N, Cc = probs.shape[:2]
    sp = tuple(probs.shape[2:])
    S = math.prod(sp)
    with torch.cuda.device(probs.device):
        ent = torch.empty((N, Cc if kind == 'binary' else 1) + sp, dtype=torch.float32, device=probs.device)
        conf = torch.empty((N, 1) + sp, dtype=torch.float32, device=probs.device) if confidence else None
        check(_lib.lib().m355_predictive_entropy(_p(probs), sd, _p(ent), _p(conf), N, Cc, S, k, _stream()),
              "predictive_entropy")
    return (ent, conf) if confidence else ent


# ----------------------------------------------------------------- contour images (csrc/contour.hip)
PLANES = ("Saggital", "Coronal", "Axial")   # by the axis of [W, H, D] a plane fixes; the reference's spelling
_SLICE_DTYPE = {**_EV_MAP_DTYPE, **_EV_SCORE_DTYPE}


def slice_counts(volumes, one_hot=None):
    """Foreground voxels per slice.  volumes[i]: a device label map [W, H, D] (any evaluation element type,
    foreground = `!= 0`), or where one_hot[i] a one-hot / score map [C, W, H, D] (float32 / bfloat16 / float16,
    foreground = argmax over C != 0).  -> (int32 device tensor, [(offset, (W, H, D))]): subject i's table at
    [offset, offset + W + H + D) holds its sagittal, coronal and axial counts.  One launch, no synchronisation."""
    n = len(volumes)
    if n == 0:
        raise _lib.M355Error("slice_counts: no volume")
    one_hot = [False] * n if one_hot is None else [bool(o) for o in one_hot]
    descs = (_lib.SliceCountsDesc * n)()
    keep, layout, total = [], [], 0
    dev = volumes[0].device
    for i, (v, oh) in enumerate(zip(volumes, one_hot)):
        if v.dim() != (4 if oh else 3) or v.device != dev:
            raise _lib.M355Error(f"slice_counts: subject {i}: {'one-hot' if oh else 'label'} map {tuple(v.shape)} on "
                                 f"{v.device}; expected {'[C, W, H, D]' if oh else '[W, H, D]'} on {dev}")
        v = v.contiguous()
        keep.append(v)
        d = descs[i]
        d.data, d.counts_offset = v.data_ptr(), total
        d.size3[:] = tuple(v.shape[-3:])
        d.dtype = _ev_code(v, _EV_SCORE_DTYPE if oh else _EV_MAP_DTYPE, f"slice_counts: subject {i}")
        d.channels = v.shape[0] if oh else 0
        layout.append((total, tuple(v.shape[-3:])))
        total += sum(v.shape[-3:])
    with torch.cuda.device(dev):
        dev_descs = torch.empty(C.sizeof(descs), dtype=torch.uint8, device=dev)
        counts = torch.empty(total, dtype=torch.int32, device=dev)
        check(_lib.lib().m355_slice_counts(descs, n, _p(dev_descs), _p(counts), _stream()), "slice_counts")
    return counts, layout


def slice_rank(counts, segments):
    """For every segment (offset, length) of the int32 device table `counts`: the slices with a non-zero count by count
    descending, ties by ascending slice id.  -> (ids, ranked counts, nums): int32 device tensors, ids / ranked laid out
    as `counts` (the first nums[s] entries of a segment are valid, the rest id -1 / count 0), nums one per segment.
    One launch, no synchronisation."""
    _require(counts, dtype=torch.int32)
    nseg = len(segments)
    if nseg == 0:
        raise _lib.M355Error("slice_rank: no segment")
    segs = (_lib.SliceSeg * nseg)()
    for s, (off, ln) in enumerate(segments):
        if off < 0 or ln < 1 or off + ln > counts.numel():
            raise _lib.M355Error(f"slice_rank: segment {s} [{off}, {off} + {ln}) of a table of {counts.numel()}")
        segs[s].offset, segs[s].len = off, ln
    counts = counts.contiguous()
    with torch.cuda.device(counts.device):
        dev_descs = torch.empty(C.sizeof(segs), dtype=torch.uint8, device=counts.device)
        ids = torch.full_like(counts, -1)
        ranked = torch.zeros_like(counts)
        nums = torch.empty(nseg, dtype=torch.int32, device=counts.device)
        check(_lib.lib().m355_slice_rank(_p(counts), segs, nseg, _p(dev_descs), _p(ids), _p(ranked), _p(nums), _stream()),
              "slice_rank")
    return ids, ranked, nums


def slice_shape(size3, plane):
    """shape of slice_volume(x, 0, plane, k) for x [1, W, H, D] (utils/utils.py:64-72, reference): Axial x[:, :, k],
    Coronal rot90(x[:, k, :]), Saggital rot90(x[k, :, :])"""
    if plane not in PLANES:
        raise ValueError(f'plane must be one of "Axial", "Coronal", or "Saggital" not {plane}')
    W, H, D = size3
    return {"Axial": (W, H), "Coronal": (D, W), "Saggital": (D, H)}[plane]


def grid_geometry(n, h, w, ncol):
    """torchvision.utils.make_grid(n tiles of h x w, nrow=ncol, padding=1): -> (rows, cols, [(row0, col0) per tile]).
    A single tile is returned bare."""
    if n < 1 or ncol < 1:
        raise ValueError(f"a grid of {n} tiles in rows of {ncol}")
    if n == 1:
        return h, w, [(0, 0)]
    xmaps = min(ncol, n)
    ymaps = -(-n // xmaps)
    return (ymaps * (h + 1) + 1, xmaps * (w + 1) + 1,
            [((k // xmaps) * (h + 1) + 1, (k % xmaps) * (w + 1) + 1) for k in range(n)])


def slice_mosaic(mosaics):
    """Up to three make_grid mosaics in one launch.  mosaics: [(tiles, ncol, pad_value, tile_shape)], tiles a list of
    (volume [W, H, D] device tensor or None, plane name, slice index); None is a tile of zeros of `tile_shape` (h, w)
    (None: the shape of the other tiles).  A mosaic has the element type of its tiles (bfloat16 / float16 tiles give a
    float32 mosaic; all tiles None: float32).  Tiles of differing shape or element type in one mosaic: ValueError,
    before anything is launched.  -> (2-D device tensors, the uint8 device buffer they are views of): one copy of the
    buffer brings every mosaic to the host.  No synchronisation."""
    if not 1 <= len(mosaics) <= 3:
        raise _lib.M355Error(f"slice_mosaic: {len(mosaics)} mosaics (1 .. 3)")
    plans, ntiles, nbytes = [], 0, 0
    for q, (tiles, ncol, pad, tile_shape) in enumerate(mosaics):
        shape = tuple(tile_shape) if tile_shape is not None else None
        dtype = None
        for k, (vol, plane, _) in enumerate(tiles):
            if vol is None:
                continue
            if vol.dim() != 3:
                raise ValueError(f"mosaic {q}, tile {k}: a volume of shape {tuple(vol.shape)}; expected [W, H, D]")
            got = slice_shape(vol.shape, plane)
            if shape is not None and got != shape:
                raise ValueError(f"mosaic {q}, tile {k}: a slice of {got[0]} x {got[1]} among tiles of {shape[0]} x {shape[1]}")
            if dtype is not None and vol.dtype != dtype:
                raise ValueError(f"mosaic {q}, tile {k}: element type {vol.dtype} among tiles of {dtype}")
            shape, dtype = got, vol.dtype
        if shape is None:
            raise ValueError(f"mosaic {q}: no tile has a source and no tile shape is given")
        out_dtype = torch.float32 if dtype in (None, torch.bfloat16, torch.float16) else dtype
        if out_dtype not in _SLICE_DTYPE:
            raise ValueError(f"mosaic {q}: element type {out_dtype}")
        rows, cols, at = grid_geometry(len(tiles), shape[0], shape[1], int(ncol))
        nbytes = -(-nbytes // 16) * 16
        plans.append((tiles, int(ncol), float(pad), shape, out_dtype, rows, cols, at, ntiles, nbytes))
        ntiles += len(tiles)
        nbytes += rows * cols * torch.empty((), dtype=out_dtype).element_size()
    sources = [vol for tiles, *_ in plans for vol, _, _ in tiles if vol is not None]
    if not sources:
        raise _lib.M355Error("slice_mosaic: no tile has a source (nothing says which device)")
    dev = sources[0].device
    if dev.type != "cuda":
        raise _lib.M355Error(f"slice_mosaic: expected device tensors, the first source is on {dev}")
    md = (_lib.SliceMosaicDesc * len(plans))()
    td = (_lib.SliceTileDesc * ntiles)()
    keep, outs = [], []
    with torch.cuda.device(dev):
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        for q, (tiles, ncol, pad, shape, out_dtype, rows, cols, at, first, byte0) in enumerate(plans):
            out = buf[byte0:byte0 + rows * cols * torch.empty((), dtype=out_dtype).element_size()].view(out_dtype).view(rows, cols)
            outs.append(out)
            m = md[q]
            m.out, m.dtype, m.rows, m.cols = out.data_ptr(), _SLICE_DTYPE[out_dtype], rows, cols
            m.tile_h, m.tile_w, m.ncol, m.ntiles, m.first_tile, m.pad = shape[0], shape[1], ncol, len(tiles), first, pad
            for k, (vol, plane, slice_id) in enumerate(tiles):
                t = td[first + k]
                t.row0, t.col0 = at[k]
                if vol is None:
                    continue
                if vol.device != dev:
                    raise _lib.M355Error(f"slice_mosaic: mosaic {q}, tile {k} is on {vol.device}, the first source on {dev}")
                vol = vol.contiguous()
                keep.append(vol)
                t.src, t.dtype = vol.data_ptr(), _ev_code(vol, _SLICE_DTYPE, f"slice_mosaic: mosaic {q}, tile {k}")
                t.size3[:] = tuple(vol.shape)
                t.plane, t.slice = PLANES.index(plane), int(slice_id)
        dev_descs = torch.empty(C.sizeof(td), dtype=torch.uint8, device=dev)
        check(_lib.lib().m355_slice_mosaic(md, len(plans), td, ntiles, _p(dev_descs), _stream()), "slice_mosaic")
    return outs, buf


# ----------------------------------------------------------------- distance transform, surface distances (csrc/distance.hip)
def _dist_arg(t, dtypes, what, shape=None):
    """a tensor argument of the distance family: element type, contiguity, device, shape -- in that order"""
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
        got = t.dtype if isinstance(t, torch.Tensor) else type(t).__name__
        raise _lib.M355Error(f"{what}: element type {got} (expected {' or '.join(str(d) for d in dtypes)})")
    if not t.is_contiguous():
        raise _lib.M355Error(f"{what}: expected a contiguous tensor, got strides {tuple(t.stride())} for shape {tuple(t.shape)}")
    if not t.is_cuda:
        raise _lib.M355Error(f"{what}: expected a device tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise _lib.M355Error(f"{what}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _size3(t, what):
    if t.dim() != 3:
        raise _lib.M355Error(f"{what}: expected one volume [W, H, D], got shape {tuple(t.shape)}")
    return (C.c_int32 * 3)(*t.shape)


def _spacing3(spacing):
    s = [float(spacing)] * 3 if isinstance(spacing, (int, float)) else [float(v) for v in spacing]
    if len(s) != 3:
        raise _lib.M355Error(f"spacing {spacing!r}: a number or three numbers (W, H, D)")
    return tuple(s)


def edt_sq(sites, spacing=(1., 1., 1.), out=None, workspace=None):
    """Squared Euclidean distance of every voxel to the nearest voxel with sites != 0, float32 [W, H, D]; +inf
    everywhere without a site.  sites: a contiguous uint8 or bool device volume [W, H, D] (every axis at most
    _lib.EDT_MAX_DIM); spacing: a number or three (W, H, D), used in fp32.  Exact for unit spacing.  `out` (float32,
    the volume's shape) and `workspace` (uint8, at least m355_edt_workspace bytes) may be handed in to reuse scratch from
    call to call.  Three launches, no synchronisation."""
    _dist_arg(sites, (torch.uint8, torch.bool), "edt_sq: sites")
    size3 = _size3(sites, "edt_sq: sites")
    sp = (C.c_float * 3)(*_spacing3(spacing))
    L = _lib.lib()
    with torch.cuda.device(sites.device):
        nbytes = int(L.m355_edt_workspace(size3))
        if workspace is None:
            workspace = _workspace(nbytes, sites.device)
        elif _dist_arg(workspace, (torch.uint8,), "edt_sq: workspace").numel() < nbytes:
            raise _lib.M355Error(f"edt_sq: workspace of {workspace.numel()} bytes, {nbytes} needed")
        if out is None:
            out = torch.empty(sites.shape, dtype=torch.float32, device=sites.device)
        else:
            _dist_arg(out, (torch.float32,), "edt_sq: out", sites.shape)
        check(L.m355_edt_sq(_p(sites), size3, sp, _p(out), _p(workspace), _stream()), "edt_sq")
    return out


def edt_sqrt(d2, out=None):
    """The correctly rounded float32 square root of every element of d2 (float32, contiguous, on the device); out may be
    d2.  One launch."""
    _dist_arg(d2, (torch.float32,), "edt_sqrt: d2")
    if out is None:
        out = torch.empty_like(d2)
    else:
        _dist_arg(out, (torch.float32,), "edt_sqrt: out", d2.shape)
    with torch.cuda.device(d2.device):
        check(_lib.lib().m355_edt_sqrt(_p(d2), _p(out), d2.numel(), _stream()), "edt_sqrt")
    return out


def signed_distance(target, spacing=(1., 1., 1.), planes=None):
    """The signed distance map of every (n, c) plane of `target` (float32 [N, C, D, H, W], contiguous, on the device;
    a voxel is inside when target > 0.5), float32 of the same shape: +distance to the nearest inside voxel
    outside, -(distance to the nearest outside voxel - 1) inside, 0 everywhere in a plane without a boundary.  spacing: a
    number or three (D, H, W), used in fp32; exact (the fp32 rounding of the true value) for unit spacing.  planes: None
    for all, or N * C host flags ([N][C] order) -- a plane that is off is written as zeros and costs no transform.  One
    transform per plane, three launches for up to 1024 planes, no synchronisation.  Every axis at most _lib.EDT_MAX_DIM."""
    if not isinstance(target, torch.Tensor) or target.dtype != torch.float32:
        got = target.dtype if isinstance(target, torch.Tensor) else type(target).__name__
        raise _lib.M355Error(f"signed_distance: target: element type {got} (expected torch.float32)")
    if target.dim() != 5:
        raise _lib.M355Error(f"signed_distance: target: expected [N, C, D, H, W], got shape {tuple(target.shape)}")
    sp = (C.c_float * 3)(*_spacing3(spacing))
    n_planes = target.shape[0] * target.shape[1]
    on = None
    if planes is not None:
        flags = [bool(v) for v in (planes.flatten().tolist() if isinstance(planes, torch.Tensor) else planes)]
        if len(flags) != n_planes:
            raise _lib.M355Error(f"signed_distance: {len(flags)} plane flags for N * C = {n_planes} planes")
        on = (C.c_uint8 * n_planes)(*flags)
    _dist_arg(target, (torch.float32,), "signed_distance: target")
    size3 = (C.c_int32 * 3)(*target.shape[2:])
    L = _lib.lib()
    with torch.cuda.device(target.device):
        ws = _workspace(L.m355_signed_distance_workspace(n_planes, size3), target.device)
        phi = torch.empty_like(target)
        check(L.m355_signed_distance(_p(target), n_planes, size3, sp, on, _p(phi), _p(ws), ws.numel(), _stream()),
              "signed_distance")
    return phi


def surface_mask(x_i32, value, border=None, count=None):
    """-> (border, count).  border (uint8, x's shape): 1 where x == value and the voxel lies on a face of the volume or
    one of its six face neighbours differs from value, else 0.  count (int32 device tensor of one element): grows by the
    number of border voxels; a fresh zero unless one is handed in (the caller zeroes that one).  x_i32: a contiguous
    int32 device volume [W, H, D].  One launch, no synchronisation."""
    _dist_arg(x_i32, (torch.int32,), "surface_mask: x")
    size3 = _size3(x_i32, "surface_mask: x")
    with torch.cuda.device(x_i32.device):
        if border is None:
            border = torch.empty(x_i32.shape, dtype=torch.uint8, device=x_i32.device)
        else:
            _dist_arg(border, (torch.uint8,), "surface_mask: border", x_i32.shape)
        if count is None:
            count = torch.zeros(1, dtype=torch.int32, device=x_i32.device)
        elif _dist_arg(count, (torch.int32,), "surface_mask: count").numel() != 1:
            raise _lib.M355Error(f"surface_mask: count of {count.numel()} elements (one)")
        check(_lib.lib().m355_surface_mask(_p(x_i32), int(value), size3, _p(border), _p(count), _stream()), "surface_mask")
    return border, count


def surface_gather(border, d2, out, cursor):
    """out[k] = sqrt(d2[v]) (correctly rounded) for every voxel with border[v] != 0, k from cursor (int32 device tensor of
    one element, advanced by the number of border voxels even past out.numel(): a short buffer shows); the order is
    unspecified.  border uint8, d2 float32 of the same shape, out float32 1-D, all contiguous on one device.  One launch,
    no synchronisation.  Returns out."""
    _dist_arg(border, (torch.uint8,), "surface_gather: border")
    _dist_arg(d2, (torch.float32,), "surface_gather: d2", border.shape)
    _dist_arg(out, (torch.float32,), "surface_gather: out")
    if _dist_arg(cursor, (torch.int32,), "surface_gather: cursor").numel() != 1:
        raise _lib.M355Error(f"surface_gather: cursor of {cursor.numel()} elements (one)")
    if border.numel() == 0 or out.numel() >= 1 << 31:
        raise _lib.M355Error(f"surface_gather: {border.numel()} voxels into {out.numel()} slots")
    with torch.cuda.device(border.device):
        check(_lib.lib().m355_surface_gather(_p(border), _p(d2), border.numel(), _p(out), _p(cursor), out.numel(),
                                             _stream()), "surface_gather")
    return out


# ----------------------------------------------------------------- statistics per label region (csrc/region_stats.hip)
REGION_STATS = ('mean', 'std', 'median', 'min', 'max')   # the last axis of RegionStats.stats
_RS_IMAGE_DTYPE = {torch.float32: _lib.EV_F32, torch.float16: _lib.EV_F16, torch.bfloat16: _lib.EV_BF16,
                   torch.uint8: _lib.EV_U8, torch.int16: _lib.EV_I16}


class RegionStats(NamedTuple):
    """count int64 [R], bounds int32 [R, 6] (min, max index along W, H, D; an empty region: axis size, -1), stats
    float32 [R, K, 5] in the order of REGION_STATS.  R = L + 2: the listed values, then 'all' (label != 0) and 'whole'
    (every voxel).  The list form of region_stats stacks the subjects in front: [n, R], [n, R, 6], [n, R, K, 5]."""
    count: torch.Tensor
    bounds: torch.Tensor
    stats: torch.Tensor


def region_stats_plan():
    """(blocks of a pass at most, threads of a block, voxels per thread and trip of the grid-stride loops, regions per
    block of a select pass) of the region statistics kernels"""
    plan = (C.c_int32 * 4)()
    check(_lib.lib().m355_region_stats_plan(plan), "region_stats_plan")
    return tuple(plan)


def _rs_chunks(values):
    values = [int(v) for v in values]
    uniq = list(dict.fromkeys(values))
    chunks = [uniq[i:i + _lib.EV_MAX_LABELS] for i in range(0, len(uniq), _lib.EV_MAX_LABELS)] or [[]]
    return values, uniq, chunks


def _rs_record(L, K):
    """byte offsets of count, bounds and stats in the record of one launch set, and the record's size"""
    R = L + 2
    bounds = 8 * R
    stats = bounds + (24 * R + 7) // 8 * 8
    return 0, bounds, stats, stats + (20 * R * K + 7) // 8 * 8


def region_stats_bytes(n_values, K, median=True):
    """(result bytes of one subject, workspace bytes) of a region_stats call with that many distinct label values and
    K images: what region_stats(..., result=, workspace=) expects at least"""
    chunks = [min(_lib.EV_MAX_LABELS, n_values - i) for i in range(0, n_values, _lib.EV_MAX_LABELS)] or [0]
    ws = max(int(_lib.lib().m355_region_stats_workspace(Lc, K, int(bool(median)))) for Lc in chunks) if K else 0
    return sum(_rs_record(Lc, K)[3] for Lc in chunks), ws


def _rs_subject(labels, images, i):
    what = f"region_stats: subject {i}"
    if not torch.is_tensor(labels) or labels.dim() not in (3, 4) or (labels.dim() == 4 and labels.shape[0] != 1):
        raise _lib.M355Error(f"{what}: a label volume [W, H, D] or [1, W, H, D], got "
                             f"{tuple(labels.shape) if torch.is_tensor(labels) else type(labels).__name__}")
    code = _ev_code(labels, _EV_MAP_DTYPE, f"{what}: label map")
    size = tuple(labels.shape[-3:])
    if min(size) < 1:
        raise _lib.M355Error(f"{what}: empty label volume {size}")
    labels = labels.contiguous()
    out = []
    for k, img in enumerate(images):
        if not torch.is_tensor(img) or img.dim() not in (3, 4) or tuple(img.shape[-3:]) != size:
            raise _lib.M355Error(f"{what}: image {k}: expected [C, {size[0]}, {size[1]}, {size[2]}], got "
                                 f"{tuple(img.shape) if torch.is_tensor(img) else type(img).__name__}")
        dt = _ev_code(img, _RS_IMAGE_DTYPE, f"{what}: image {k}")
        if img.device != labels.device:
            raise _lib.M355Error(f"{what}: image {k} is on {img.device}, the label map on {labels.device}")
        channels = img.shape[0] if img.dim() == 4 else 1
        if channels < 1:
            raise _lib.M355Error(f"{what}: image {k} has no channel")
        out.append((img.contiguous(), dt, channels))
    return labels, code, size, out


def _rs_enqueue(subjects, plans, median, result=None, workspace=None):
    """launches for every (subject, chunk of its label values); plans[i] = _rs_chunks of subject i.
    -> (result buffer, record offsets [subject][chunk])"""
    L = _lib.lib()
    dev = subjects[0][0].device
    need, ws_bytes = 0, 0
    for (_, _, _, images), (_, _, chunks) in zip(subjects, plans):
        K = len(images)
        need += sum(_rs_record(len(c), K)[3] for c in chunks)
        if K:
            ws_bytes = max([ws_bytes] + [int(L.m355_region_stats_workspace(len(c), K, int(median))) for c in chunks])
    with torch.cuda.device(dev):
        if result is None:
            result = torch.empty(need, dtype=torch.uint8, device=dev)
        elif (result.dtype != torch.uint8 or not result.is_contiguous() or result.device != dev or result.data_ptr() % 8
              or result.numel() < need):
            raise _lib.M355Error(f"region_stats: result must be a contiguous uint8 tensor of at least {need} bytes on "
                                 f"{dev}, 8-byte aligned")
        if workspace is None:
            workspace = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        elif (workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.device != dev
              or workspace.data_ptr() % 8 or workspace.numel() < ws_bytes):
            raise _lib.M355Error(f"region_stats: workspace must be a contiguous uint8 tensor of at least {ws_bytes} "
                                 f"bytes on {dev}, 8-byte aligned")
        base = result.data_ptr()
        records = []
        at = 0
        for (labels, code, size, images), (_, _, chunks) in zip(subjects, plans):
            if labels.device != dev:
                raise _lib.M355Error(f"region_stats: subjects on {labels.device} and {dev}")
            K = len(images)
            descs = (_lib.RegionImage * max(K, 1))()
            for k, (img, dt, channels) in enumerate(images):
                descs[k].data, descs[k].dtype, descs[k].channels = img.data_ptr(), dt, channels
            size3 = (C.c_int32 * 3)(*size)
            row = []
            for chunk in chunks:
                o_count, o_bounds, o_stats, nbytes = _rs_record(len(chunk), K)
                vals = (C.c_int32 * max(len(chunk), 1))(*chunk)
                check(L.m355_region_stats(_p(labels), code, size3, descs if K else None, K, vals if chunk else None,
                                          len(chunk), int(median), C.c_void_p(base + at + o_count),
                                          C.c_void_p(base + at + o_bounds), C.c_void_p(base + at + o_stats) if K else None,
                                          _p(workspace) if K else None, workspace.numel() if K else 0, _stream()),
                      "region_stats")
                row.append(at)
                at += nbytes
            records.append(row)
    return result, records


def _rs_unpack(buf, row, plan, K):
    """RegionStats of one subject from the (device or host) byte buffer: rows in the order of its values, then all,
    whole"""
    values, uniq, chunks = plan
    pos = {v: i for i, v in enumerate(uniq)}
    rows = [pos[v] for v in values]
    counts, bounds, stats = [], [], []
    for j, (chunk, at) in enumerate(zip(chunks, row)):
        R = len(chunk) + 2
        o_count, o_bounds, o_stats, _ = _rs_record(len(chunk), K)
        c = buf[at + o_count:at + o_count + 8 * R].view(torch.int64)
        b = buf[at + o_bounds:at + o_bounds + 24 * R].view(torch.int32).view(R, 6)
        s = buf[at + o_stats:at + o_stats + 20 * R * K].view(torch.float32).view(R, K, 5)
        counts.append(c[:-2])
        bounds.append(b[:-2])
        stats.append(s[:-2])
        if j == 0:
            tail = (c[-2:], b[-2:], s[-2:])
    if len(chunks) == 1 and rows == list(range(len(uniq))):
        return RegionStats(c, b, s)
    idx = torch.tensor(rows, dtype=torch.int64, device=buf.device)
    return RegionStats(*(torch.cat([torch.cat(part)[idx], t]) for part, t in zip((counts, bounds, stats), tail)))


def region_stats(labels, images, values, median=True, result=None, workspace=None):
    """Statistics of image values grouped by the label of the voxel.  labels: a device label volume [W, H, D] or
    [1, W, H, D] (bool / (u)int8 / int16 / int32 / int64 / float32 holding integers); images: K >= 0 device tensors
    [C, W, H, D] (or [W, H, D]) on the same grid, float32 / float16 / bfloat16 / uint8 / int16, the channels of an image
    pooled; values: the int label values of the listed regions, any number (more than 64 distinct ones run as several
    launch sets).  -> RegionStats of device tensors; nothing is copied or synchronised.

    List form: labels a list of n label volumes, images a list of n lists of K images (shapes may differ between
    subjects) -> RegionStats of HOST tensors with the subjects stacked in front, from one device-to-host copy.  With
    `values` a list of n lists (each subject its own values; the number of images may then differ too) the result is a
    list of n host RegionStats instead, still from one copy.

    median=False skips the select passes; that column is NaN.  `result` / `workspace`: uint8 device tensors to use
    instead of fresh ones (sizes: region_stats_bytes, added up over the subjects for `result`)."""
    single = torch.is_tensor(labels)
    label_list = [labels] if single else list(labels)
    image_lists = [list(images)] if single else [list(im) for im in images]
    if not label_list or len(label_list) != len(image_lists):
        raise _lib.M355Error("region_stats: one list of images per label volume, at least one subject")
    values = list(values)
    own_values = not single and len(values) > 0 and isinstance(values[0], (list, tuple))
    if own_values and len(values) != len(label_list):
        raise _lib.M355Error(f"region_stats: {len(values)} lists of values for {len(label_list)} subjects")
    if not own_values and any(len(im) != len(image_lists[0]) for im in image_lists):
        raise _lib.M355Error("region_stats: every subject needs the same number of images")
    plans = [_rs_chunks(v) for v in values] if own_values else [_rs_chunks(values)] * len(label_list)
    subjects = [_rs_subject(lab, im, i) for i, (lab, im) in enumerate(zip(label_list, image_lists))]
    buf, records = _rs_enqueue(subjects, plans, bool(median), result, workspace)
    if single:
        return _rs_unpack(buf, records[0], plans[0], len(image_lists[0]))
    host = buf.cpu()
    per = [_rs_unpack(host, row, plan, len(im)) for row, plan, im in zip(records, plans, image_lists)]
    return per if own_values else RegionStats(*(torch.stack(field) for field in zip(*per)))
