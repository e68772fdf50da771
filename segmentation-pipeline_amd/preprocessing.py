"""Preprocessing on the device: the deterministic transforms that wrap the augmentations of the reference's production
configs (research/dmri_hippo/configs/main_config.py:78-120, research/msseg2/msseg2.py:36-80), with the reference's
names and constructor arguments (torchio 0.18.45 for `Crop`, `Pad` and `CropOrPad`).

They are `augmentation.Transform`s with the same call, so one `augmentation.Compose` holds preprocessing and augmentation
transforms together and runs the reference's chains in the reference's order on the device:

    t(subject, label_maps=(), spacing=(1., 1., 1.), generator=None, label_values=None) -> subject

`label_values` maps a label map's name to its {label name: id} (the reference's per-map `label_values`); after every call
`t.last_meta` holds the resulting spacing, label maps, label_values and one-hot maps, and `t.last_history` the concrete
bounds, shapes and spacings chosen.  The caller's tensors are never written.  NaN replacement, crop / pad, label remap
and cast of one tensor are deferred and run as one pass (csrc/preprocess.hip, pre_gather_kernel).  Nothing synchronises
with the host except `CropToMask`, whose output shape depends on the data: it reads the six bounds once.
Semantics and every torchio assumption: DESIGN §4.11.
"""
import ctypes as C
import numbers
import warnings

import numpy as np
import torch

from . import _lib
from ._lib import M355Error, check
from .augmentation import Transform, _i3, _resample, _INTERP
from .ops import _p, _stream

__all__ = ["ReplaceNan", "SetDataType", "EnforceConsistentAffine", "TargetResample", "Crop", "Pad", "CropOrPad",
           "CropToMask", "MinSizePad", "CustomRemapLabels", "CustomOneHot", "ConcatenateImages", "RenameProperty",
           "ImageFromLabels", "target_spacing", "resample_shape", "six_bounds", "min_size_padding"]

_DTYPE = {torch.uint8: _lib.PRE_U8, torch.bool: _lib.PRE_BOOL, torch.int32: _lib.PRE_I32, torch.int64: _lib.PRE_I64,
          torch.float32: _lib.PRE_F32}
_ANATOMICAL = {"Right": (0, 1), "Left": (0, 0), "Anterior": (1, 1), "Posterior": (1, 0), "Superior": (2, 1),
               "Inferior": (2, 0)}   # torchio's get_mask_from_anatomical_label: (axis, upper half)


def _code(t, what):
    if t.dtype not in _DTYPE:
        raise M355Error(f"{what}: element type {t.dtype} (uint8, bool, int32, int64, float32)")
    return _DTYPE[t.dtype]


# ---------------------------------------------------------------------------------------------- host-side semantics
def six_bounds(v):
    """torchio's bounds: n -> (n,) * 6, (a, b, c) -> (a, a, b, b, c, c), six numbers stay"""
    if isinstance(v, numbers.Number):
        v = (v,) * 6
    v = tuple(int(a) for a in v)
    if len(v) == 3:
        v = (v[0], v[0], v[1], v[1], v[2], v[2])
    if len(v) != 6 or min(v) < 0:
        raise ValueError(f"bounds must be one, three or six non-negative integers, got {v}")
    return v


def _three(v, what):
    v = (v,) * 3 if isinstance(v, numbers.Number) else tuple(v)
    if len(v) != 3:
        raise ValueError(f"{what}: one or three values, got {v}")
    return v


def target_spacing(current, target, tolerance):
    """TargetResample's spacing (segmentation_pipeline/transforms/target_resample.py): None when every axis is within
    its tolerance, else the iteratively rounded spacing.  Python's round: half to even."""
    current = tuple(float(c) for c in current)
    if all(abs(c - t) < tol for c, t, tol in zip(current, target, tolerance)):
        return None
    out = []
    for cur, tar, tol in zip(current, target, tolerance):
        step, spacing = 1, cur
        while abs(spacing - tar) > tol:
            if cur < tar:
                scale = round(tar / cur * step) / step
            else:
                scale = 1 / (round(cur / tar * step) / step)
            spacing = cur * scale
            step += 1
        out.append(spacing)
    return tuple(out)


def resample_shape(shape, old, new):
    """torchio Resample's output size: ceil(V old / new), singleton axes stay 1"""
    n = np.ceil(np.asarray(shape, dtype=np.float64) * np.asarray(old, dtype=np.float64) / np.asarray(new, dtype=np.float64))
    return tuple(1 if v == 1 else int(m) for v, m in zip(shape, n))


def min_size_padding(shape, min_size):
    """MinSizePad's six bounds: (d // 2, d // 2 + d % 2) on every axis smaller than min_size"""
    out = []
    for v, m in zip(shape, min_size):
        d = m - v if v < m else 0
        out += [d // 2, d // 2 + d % 2]
    return tuple(out)


def _pad_mode(mode):
    if isinstance(mode, numbers.Number) and not isinstance(mode, bool):
        return float(mode)
    if mode == "minimum":
        return "minimum"
    raise NotImplementedError(f"padding_mode {mode!r}: a number or 'minimum'")


# ---------------------------------------------------------------------------------------------- the deferred pass
class _Pass:
    """one tensor's pending pre_gather: NaN replacement -> window (crop / pad) -> simultaneous remap -> cast.  Its
    output is allocated at once (state.data[name], with its final shape and dtype); the launch waits for the flush."""

    def __init__(self, name, x):
        self._name = name
        self.x = x.contiguous()
        self.src = tuple(x.shape[1:])
        self.base = (0, 0, 0)         # a host crop folded in: the box base .. base + box of x
        self.box = self.src
        self.off = (0, 0, 0)          # host ints, or a device int32 [3]
        self.out = self.src
        self.pad = 0.0
        self.window = False
        self.nan = None
        self.remap = None             # (olds, news, mask kind, axis, upper, mask tensor)
        self.dtype = x.dtype

    def host_inside(self):
        """a host window that pads nothing"""
        return self.window and not isinstance(self.off, torch.Tensor) and all(
            0 <= o and o + n <= b for o, n, b in zip(self.off, self.out, self.box))

    def alloc(self, state, name):
        y = torch.empty((self.x.shape[0],) + tuple(self.out), dtype=self.dtype, device=self.x.device)
        state.set(name, y)

    def run(self, state):
        L = _lib.lib()
        x = self.x
        y = state.data[self._name]
        d = _lib.PreGatherDesc()
        d.x, d.y = x.data_ptr(), y.data_ptr()
        d.in_dtype, d.out_dtype, d.C = _code(x, self._name), _code(y, self._name), x.shape[0]
        d.src3[:], d.base3[:], d.in3[:], d.out3[:] = self.src, self.base, self.box, self.out
        if isinstance(self.off, torch.Tensor):
            d.off_dev = self.off.data_ptr()
            state.keep.append(self.off)
        else:
            d.off3[:] = self.off
        if self.nan is not None:
            d.replace_nan, d.nan_value = 1, float(self.nan)
        if self.pad == "minimum" and not self.host_inside():
            nbytes = int(L.m355_pre_min_tables_bytes(x.shape[0], _i3(self.src)))
            tables = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            state.keep.append(tables)
            check(L.m355_pre_min_tables(_p(x), d.in_dtype, x.shape[0], _i3(self.src), d.replace_nan, d.nan_value,
                                        _p(tables), nbytes, _stream()), "pre_min_tables")
            d.pad_mode, d.tables = 1, tables.data_ptr()
        else:
            d.pad_value = 0.0 if self.pad == "minimum" else float(self.pad)
        if self.remap is not None:
            olds, news, kind, axis, upper, mask = self.remap
            d.nremap = len(olds)
            d.remap_old[:len(olds)], d.remap_new[:len(news)] = olds, news
            d.mask_kind, d.mask_axis, d.mask_upper = kind, axis, upper
            if mask is not None:
                d.mask_map, d.mask_dtype, d.mask_C = mask.data_ptr(), _code(mask, "mask"), mask.shape[0]
                state.keep.append(mask)
        state.keep.append(x)
        check(L.m355_pre_gather(C.byref(d), _stream()), "pre_gather")


def _pass(state, name, accept):
    """the deferred pass of `name` when `accept(pass)` takes the next stage, else a new pass over the flushed tensor"""
    p = state.deferred.get(name)
    if p is not None and name not in state.pending and name not in state.blur and accept(p):
        return p
    state.flush(name)
    p = _Pass(name, state.data[name])
    state.deferred[name] = p
    return p


def _window(state, name, off, out, pad):
    """crop / pad `name`: output voxel p reads the current tensor at p + off (host ints or a device int32 [3])"""
    host = not isinstance(off, torch.Tensor)

    def accept(p):
        if p.remap is not None or p.dtype != p.x.dtype:
            return False
        if not p.window:
            return True
        # a host crop folds into the box; a later 'minimum' pad needs the tables of the whole box, so it does not
        return p.host_inside() and (pad != "minimum" or (host and all(
            0 <= o and o + n <= v for o, n, v in zip(off, out, p.out))))

    p = _pass(state, name, accept)
    if p.window:
        p.base = tuple(b + o for b, o in zip(p.base, p.off))
        p.box = p.out
    p.window, p.off, p.out = True, off if not host else tuple(int(o) for o in off), tuple(int(v) for v in out)
    p.pad = pad
    p.alloc(state, name)


def _spatial_shape(state, names):
    shapes = {tuple(state.data[k].shape[1:]) for k in names}
    if len(shapes) > 1:
        raise M355Error(f"images of different spatial shapes: {sorted(shapes)}")
    return shapes.pop() if shapes else None


class _Pre(Transform):
    """a deterministic transform: `_apply` only"""


# ---------------------------------------------------------------------------------------------- per-voxel
class ReplaceNan(_Pre):
    def __init__(self, replace_val=0, **kw):
        super().__init__(**kw)
        self.replace_val = float(replace_val)

    def _apply(self, state):
        self.last_history = {"replace_val": self.replace_val}
        for name in state.images(self, intensity=True):
            if state.data[name].dtype != torch.float32:
                continue   # only floating tensors hold NaN
            p = _pass(state, name, lambda p: p.nan is None and not p.window and p.remap is None and p.dtype == p.x.dtype)
            p.nan = self.replace_val
            p.alloc(state, name)


class SetDataType(_Pre):
    def __init__(self, dtype, intensity_only=True, **kw):
        super().__init__(**kw)
        if dtype not in _DTYPE:
            raise M355Error(f"SetDataType: {dtype} (uint8, bool, int32, int64, float32)")
        self.dtype = dtype
        self.intensity_only = intensity_only

    def _apply(self, state):
        self.last_history = {"dtype": self.dtype}
        for name in state.images(self, intensity=self.intensity_only):
            if state.data[name].dtype == self.dtype:
                continue
            p = _pass(state, name, lambda p: p.dtype == p.x.dtype)
            p.dtype = self.dtype
            p.alloc(state, name)


class EnforceConsistentAffine(_Pre):
    """subjects here carry one `spacing` for all their tensors: every affine is already the same"""

    def __init__(self, source_image_name=None, **kw):
        super().__init__(**kw)
        self.source_image_name = source_image_name

    def _apply(self, state):
        self.last_history = {"source_image_name": self.source_image_name}


# ---------------------------------------------------------------------------------------------- spatial
class Crop(_Pre):
    def __init__(self, cropping, **kw):
        super().__init__(**kw)
        self.cropping = six_bounds(cropping)

    def _apply(self, state):
        names = state.images(self, intensity=False)
        shape = _spatial_shape(state, names)
        c = self.cropping
        out = tuple(shape[a] - c[2 * a] - c[2 * a + 1] for a in range(3)) if shape else None
        self.last_history = {"cropping": c, "shape": out}
        if shape is None or not any(c):
            return
        if min(out) <= 0:
            raise M355Error(f"Crop {c} of {shape} leaves nothing")
        for name in names:
            _window(state, name, (c[0], c[2], c[4]), out, 0.0)


class Pad(_Pre):
    def __init__(self, padding, padding_mode=0, **kw):
        super().__init__(**kw)
        self.padding = six_bounds(padding)
        self.padding_mode = _pad_mode(padding_mode)

    def _apply(self, state):
        names = state.images(self, intensity=False)
        shape = _spatial_shape(state, names)
        q = self.padding
        out = tuple(shape[a] + q[2 * a] + q[2 * a + 1] for a in range(3)) if shape else None
        self.last_history = {"padding": q, "padding_mode": self.padding_mode, "shape": out}
        if shape is None or not any(q):
            return
        for name in names:
            _window(state, name, (-q[0], -q[2], -q[4]), out, self.padding_mode)


def _centred_offsets(shape, target):
    """torchio's centred crop or pad: ceil(n / 2) of the n voxels cropped or padded go in front"""
    return tuple((v - t + 1) // 2 if v >= t else -((t - v + 1) // 2) for v, t in zip(shape, target))


class CropOrPad(_Pre):
    """torchio 0.18.45: centred on the bounding box of the nonzero voxels of `mask_name`'s channel 0 (offsets computed
    on the device), or on the volume when there is no mask or it is empty"""

    def __init__(self, target_shape, padding_mode=0, mask_name=None, **kw):
        super().__init__(**kw)
        self.target_shape = tuple(int(v) for v in _three(target_shape, "CropOrPad target_shape"))
        self.padding_mode = _pad_mode(padding_mode)
        self.mask_name = mask_name

    def _apply(self, state):
        names = state.images(self, intensity=False)
        shape = _spatial_shape(state, names)
        if shape is None:
            return
        T = self.target_shape
        if self.mask_name is not None and self.mask_name in state.data:
            state.flush(self.mask_name)
            m = state.data[self.mask_name]
            L = _lib.lib()
            bb = torch.empty(8, dtype=torch.int32, device=m.device)
            off = torch.empty(3, dtype=torch.int32, device=m.device)
            check(L.m355_pre_bbox(_p(m), _code(m, self.mask_name), m.shape[0], _i3(shape), 0, 0, 0.0, _p(bb), _stream()),
                  "pre_bbox")
            check(L.m355_pre_crop_or_pad_offsets(_p(bb), _i3(shape), _i3(T), _p(off), _stream()), "pre_offsets")
            state.keep += [m, bb]
            self.last_history = {"target_shape": T, "offsets": off, "bbox": bb}
        else:
            if self.mask_name is not None:
                warnings.warn(f'Mask name "{self.mask_name}" not found in subject. Using volume center instead',
                              RuntimeWarning)
            off = _centred_offsets(shape, T)
            self.last_history = {"target_shape": T, "offsets": off}
            if shape == T:
                return
        for name in names:
            _window(state, name, off, T, self.padding_mode)


class CropToMask(_Pre):
    """crops to [min, max) of `map[label_channel] == label_id` on every axis (the reference drops the last mask slice);
    reads the six bounds to the host: the one synchronisation of this module"""

    def __init__(self, label_map_name, label_id=1, label_channel=0, **kw):
        super().__init__(**kw)
        self.label_map_name = label_map_name
        self.label_id = label_id
        self.label_channel = int(label_channel)

    def _apply(self, state):
        if self.label_map_name not in state.data:
            return
        state.flush(self.label_map_name)
        m = state.data[self.label_map_name]
        shape = tuple(m.shape[1:])
        bb = torch.empty(8, dtype=torch.int32, device=m.device)
        check(_lib.lib().m355_pre_bbox(_p(m), _code(m, self.label_map_name), m.shape[0], _i3(shape), self.label_channel,
                                       1, float(self.label_id), _p(bb), _stream()), "pre_bbox")
        b = bb.cpu().tolist()
        if b[6] == 0:
            raise M355Error(f"CropToMask: no voxel of {self.label_map_name} channel {self.label_channel} is "
                            f"{self.label_id}")
        lo = [shape[a] - b[a] for a in range(3)]
        hi = [b[3 + a] - 1 for a in range(3)]     # the last mask index, itself cropped away
        cropping = (lo[0], shape[0] - hi[0], lo[1], shape[1] - hi[1], lo[2], shape[2] - hi[2])
        if any(h <= l for l, h in zip(lo, hi)):
            raise M355Error(f"CropToMask: the mask spans one slice on some axis ({lo} .. {hi}): nothing is left")
        t = Crop(cropping, include=self.include, exclude=self.exclude)
        t._apply(state)
        self.last_history = {"cropping": cropping, "shape": t.last_history["shape"]}


class MinSizePad(_Pre):
    def __init__(self, min_size, **kw):
        super().__init__(**kw)
        if isinstance(min_size, int):
            self.min_size = (min_size,) * 3
        elif isinstance(min_size, tuple):
            self.min_size = min_size
        else:
            raise KeyError("min_size must be an int or tuple")

    def _apply(self, state):
        names = state.images(self, intensity=False)
        if not names:
            return
        shape = tuple(state.data[next(iter(state.data))].shape[1:])   # the reference reads the first image
        padding = min_size_padding(shape, self.min_size)
        self.last_history = {"padding": padding}
        if any(padding):
            t = Pad(padding, 0, include=self.include, exclude=self.exclude)
            t._apply(state)
            self.last_history["shape"] = t.last_history["shape"]


class TargetResample(_Pre):
    """the reference's iterative spacing (target_spacing) and torchio's Resample onto it: images `image_interpolation`,
    label maps nearest, zero outside, through m355_aug_resample"""

    _MODES = {"mean": lambda s: float(np.mean(s)), "median": lambda s: float(np.median(s)), "min": min, "max": max}

    def __init__(self, target_spacing, tolerance, image_interpolation="linear", pre_affine_name=None,
                 scalars_only=False, **kw):
        super().__init__(**kw)
        if pre_affine_name is not None or scalars_only:
            raise NotImplementedError("TargetResample: pre_affine_name and scalars_only")
        if isinstance(target_spacing, str):
            if target_spacing not in self._MODES:
                raise ValueError(f"Spacing mode must be one of: {tuple(self._MODES)}")
            self.target = target_spacing
        else:
            self.target = tuple(float(v) for v in _three(target_spacing, "target_spacing"))
        self.tolerance = tuple(float(v) for v in _three(tolerance, "tolerance"))
        if image_interpolation not in _INTERP:
            raise ValueError(f"image_interpolation {image_interpolation!r}: one of {tuple(_INTERP)}")
        self.image_interpolation = image_interpolation

    def _apply(self, state):
        cur = state.spacing
        tgt = (self._MODES[self.target](cur),) * 3 if isinstance(self.target, str) else self.target
        new = target_spacing(cur, tgt, self.tolerance)
        self.last_history = {"spacing": new}
        if new is None:
            return
        s = np.asarray(new) / np.asarray(cur)
        mat = np.concatenate([np.diag(s), (0.5 * s - 0.5)[:, None]], axis=1)
        for name in state.images(self, intensity=False):
            out = resample_shape(state.data[name].shape[1:], cur, new)
            _resample(state, name, mat, out, _INTERP[self.image_interpolation])
            self.last_history["shape"] = out
        state.spacing = tuple(new)


# ---------------------------------------------------------------------------------------------- labels
def _parse_remapping(remapping):
    if isinstance(remapping, dict):
        if not all(isinstance(k, int) and isinstance(v, int) for k, v in remapping.items()):
            raise ValueError(f"Label remapping must be a Dict[int, int] or a Sequence[Tuple[str, int, int]], not {remapping}")
        return dict(remapping), None
    try:
        seq = [tuple(r) for r in remapping]
    except TypeError:
        seq = None
    if seq is None or any(len(r) != 3 or not isinstance(r[0], str) or not isinstance(r[1], int)
                          or not isinstance(r[2], int) for r in seq):
        raise ValueError(f"Label remapping must be a Dict[int, int] or a Sequence[Tuple[str, int, int]], not {remapping}")
    return {old: new for _, old, new in seq}, seq


class CustomRemapLabels(_Pre):
    """every pair tests the data before this remap (simultaneous); `masking_method`: None, a label map (its nonzero
    voxels) or one of torchio's anatomical half-spaces"""

    def __init__(self, remapping, masking_method=None, invertible=True, **kw):
        super().__init__(**kw)
        self.mapping, self.named = _parse_remapping(remapping)
        if len(self.mapping) > _lib.PRE_MAX_REMAP:
            raise M355Error(f"CustomRemapLabels: {len(self.mapping)} pairs > {_lib.PRE_MAX_REMAP}")
        self.masking_method = masking_method
        self.invertible = invertible

    def _apply(self, state):
        self.last_history = {"remapping": dict(self.mapping), "masking_method": self.masking_method}
        mm = self.masking_method
        for name in state.images(self, intensity=False):
            if name not in state.labels:
                continue
            if self.named is not None and name in state.label_values:
                for label, _, new in self.named:
                    state.label_values[name][label] = new
            kind, axis, upper, mask = _lib.PRE_MASK_NONE, 0, 0, None
            if mm is None:
                pass
            elif isinstance(mm, str) and mm in state.data:
                state.flush(mm)
                mask = state.data[mm]
                state.owned.discard(mm)   # read by a deferred pass: no later stage may write it in place
                if tuple(mask.shape[1:]) != tuple(state.data[name].shape[1:]) or mask.shape[0] not in (
                        1, state.data[name].shape[0]):
                    raise M355Error(f"CustomRemapLabels: mask {mm} {tuple(mask.shape)} vs {name} "
                                    f"{tuple(state.data[name].shape)}")
                kind = _lib.PRE_MASK_MAP
            elif isinstance(mm, str) and mm.title() in _ANATOMICAL:
                kind = _lib.PRE_MASK_HALF
                axis, upper = _ANATOMICAL[mm.title()]
            else:
                raise NotImplementedError(f"masking_method {mm!r}: None, a name in the subject or an anatomical label")
            p = _pass(state, name, lambda p: p.remap is None and p.dtype == p.x.dtype)
            p.remap = (list(self.mapping), list(self.mapping.values()), kind, axis, upper, mask)
            p.alloc(state, name)


class CustomOneHot(_Pre):
    """K = num_classes, or max(label_values) + 1 when -1; output in the input's element type.  A label outside [0, K)
    gives an all-zero voxel and is counted in last_history['out_of_range'] (a device int32 [1]; no host read)"""

    def __init__(self, num_classes=-1, **kw):
        super().__init__(**kw)
        self.num_classes = int(num_classes)

    def _apply(self, state):
        hist = {}
        for name in state.images(self, intensity=False):
            if name not in state.labels:
                continue
            state.flush(name)
            x = state.data[name]
            if x.shape[0] != 1:
                raise M355Error(f"CustomOneHot: {name} has {x.shape[0]} channels, expected 1")
            K = self.num_classes
            if K == -1:
                if name not in state.label_values:
                    raise M355Error(f"CustomOneHot: {name}: num_classes=-1 needs its label_values (counting the "
                                    "classes in the data would read the device)")
                K = max(state.label_values[name].values()) + 1
            y = torch.empty((K,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
            bad = torch.empty(1, dtype=torch.int32, device=x.device)
            check(_lib.lib().m355_pre_one_hot(_p(x), _code(x, name), _i3(x.shape[1:]), K, _p(y), _p(bad), _stream()),
                  "pre_one_hot")
            state.keep.append(x)
            state.set(name, y)
            state.one_hot.add(name)
            hist[name] = {"num_classes": K, "out_of_range": bad}
        self.last_history = hist


class ConcatenateImages(_Pre):
    """the new image takes the first image's label status, label_values and one-hot flag (the reference deep-copies it)"""

    def __init__(self, image_names, image_channels, new_image_name, **kw):
        super().__init__(**kw)
        assert len(image_names) == len(image_channels), "The number of image names and number of " \
                                                        "channels specified must be the same."
        self.image_names = list(image_names)
        self.image_channels = list(image_channels)
        self.new_image_name = new_image_name

    def _apply(self, state):
        if any(n not in state.data for n in self.image_names):
            return
        for n in self.image_names:
            state.flush(n)
        xs = [state.data[n].contiguous() for n in self.image_names]
        _spatial_shape(state, self.image_names)
        dtype = xs[0].dtype
        for x in xs[1:]:
            dtype = torch.promote_types(dtype, x.dtype)
        shape = tuple(xs[0].shape[1:])
        y = torch.empty((sum(x.shape[0] for x in xs),) + shape, dtype=dtype, device=xs[0].device)
        c0 = 0
        for n, x in zip(self.image_names, xs):
            d = _lib.PreGatherDesc()
            d.x, d.y = x.data_ptr(), y[c0:c0 + x.shape[0]].data_ptr()
            d.in_dtype, d.out_dtype, d.C = _code(x, n), _code(y, self.new_image_name), x.shape[0]
            d.src3[:], d.in3[:], d.out3[:] = shape, shape, shape
            check(_lib.lib().m355_pre_gather(C.byref(d), _stream()), "pre_gather")
            state.keep.append(x)
            c0 += x.shape[0]
        first, new = self.image_names[0], self.new_image_name
        for d in (state.deferred, state.pending, state.blur):
            d.pop(new, None)
        state.set(new, y)
        (state.labels.add if first in state.labels else state.labels.discard)(new)
        (state.one_hot.add if first in state.one_hot else state.one_hot.discard)(new)
        if first in state.label_values:
            state.label_values[new] = dict(state.label_values[first])
        else:
            state.label_values.pop(new, None)
        self.last_history = {"shape": tuple(y.shape), "dtype": dtype}


class RenameProperty(_Pre):
    """label-map status, label_values, the one-hot flag and anything deferred follow the rename"""

    def __init__(self, old_name, new_name, **kw):
        super().__init__(**kw)
        self.old_name, self.new_name = old_name, new_name

    def _apply(self, state):
        old, new = self.old_name, self.new_name
        self.last_history = {"old_name": old, "new_name": new}
        if old not in state.data or old == new:
            return
        state.data[new] = state.data.pop(old)
        for d in (state.deferred, state.pending, state.blur, state.label_values):
            d.pop(new, None)
            if old in d:
                d[new] = d.pop(old)
        if new in state.deferred:
            state.deferred[new]._name = new
        for s in (state.owned, state.labels, state.one_hot):
            s.discard(new)
            if old in s:
                s.discard(old)
                s.add(new)


class ImageFromLabels(_Pre):
    """float32 [1, ...]: entries (map, label id or name, weight) in order, 'overwrite' or 'additive'; a one-hot map is
    read through its argmax over channels; maps missing from the subject are skipped"""

    _MODES = {"overwrite": 0, "additive": 1}

    def __init__(self, new_image_name, label_weights, mode="overwrite", **kw):
        super().__init__(**kw)
        if mode not in self._MODES:
            raise ValueError(f"ImageFromLabels: mode {mode!r} ('overwrite' or 'additive')")
        self.new_image_name = new_image_name
        self.label_weights = [tuple(w) for w in label_weights]
        self.mode = mode

    def _apply(self, state):
        shape = _spatial_shape(state, list(state.data))
        entries, used = [], []
        for name, ident, weight in self.label_weights:
            if name not in state.data:
                continue
            if isinstance(ident, str):
                if name not in state.label_values or ident not in state.label_values[name]:
                    raise M355Error(f'ImageFromLabels: {name} has no label_values entry "{ident}"')
                ident = state.label_values[name][ident]
            state.flush(name)
            m = state.data[name]
            entries.append((m, name, float(ident), float(weight)))
            used.append((name, ident, weight))
        if len(entries) > _lib.PRE_MAX_ENTRIES:
            raise M355Error(f"ImageFromLabels: {len(entries)} entries > {_lib.PRE_MAX_ENTRIES}")
        arr = (_lib.PreLabelEntry * max(1, len(entries)))()
        for j, (m, name, ident, weight) in enumerate(entries):
            arr[j].map, arr[j].dtype, arr[j].C = m.data_ptr(), _code(m, name), m.shape[0]
            arr[j].one_hot, arr[j].weight, arr[j].id = int(name in state.one_hot), weight, ident
            state.keep.append(m)
        dev = next(iter(state.data.values())).device
        y = torch.empty((1,) + tuple(shape), dtype=torch.float32, device=dev)
        check(_lib.lib().m355_pre_image_from_labels(arr, len(entries), _i3(shape), self._MODES[self.mode], _p(y),
                                                    _stream()), "pre_image_from_labels")
        new = self.new_image_name
        for d in (state.deferred, state.pending, state.blur, state.label_values):
            d.pop(new, None)
        state.labels.discard(new)
        state.one_hot.discard(new)
        state.set(new, y)
        self.last_history = {"entries": used, "mode": self.mode}
