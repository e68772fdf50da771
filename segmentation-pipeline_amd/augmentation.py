"""Training augmentation on the device: the torchio 0.18.45 transforms of the reference's production configs
(research/dmri_hippo/configs/main_config.py:86-100, research/msseg2/msseg2.py:44-57), with torchio's names.

Each random transform draws its parameters on the host from a CPU `torch.Generator` and hands them to a deterministic
counterpart (`Flip`, `PermuteDimensions`, `ElasticDeformation`, `Affine`, `BiasField`, `Gamma`, `Blur`, `Noise`); every
per-voxel step runs in libm355seg.so (csrc/augment.hip).  A call never synchronises with the host: statistics
(percentile cutoffs, min / max, the Otsu pad value) stay in device memory and parameters go up from pinned memory.

    t(subject, label_maps=(), spacing=(1., 1., 1.), generator=None) -> subject

`subject` is a dict of device tensors [C, V0, V1, V2] (what `sampling.VolumeFeeder` yields); images are float32, names in
`label_maps` may also be uint8 / bool, int32, int64 or float32 and follow the spatial transforms with nearest
interpolation (intensity transforms skip them).  The input tensors are never modified.  Consecutive intensity
transforms of one tensor are fused into one streaming pass (plus the statistics passes a rescale needs).
`t.last_history` records the concrete parameters of the last call.  Semantics and every torchio assumption: DESIGN §4.10.

`ReconstructMeanDWI` / `ReconstructMeanDWIClassic` (the reference's own transforms) replace `mean_dwi` with the mean of
drawn channels of `full_dwi` (csrc/dwi.hip, through `MeanDWI`); they read full_dwi's gradient table from the call's
`attributes={"full_dwi": {"grad": [N, 4] host table}}`.
"""
import ctypes as C
import math
import numbers

import numpy as np
import torch

from . import _lib
from ._lib import M355Error, check
from .ops import _p, _stream

__all__ = ["Compose", "OneOf", "RandomFlip", "RandomPermuteDimensions", "RandomElasticDeformation", "RandomAffine",
           "RandomBiasField", "RescaleIntensity", "RandomGamma", "RandomBlur", "RandomNoise", "Flip", "PermuteDimensions",
           "ElasticDeformation", "Affine", "BiasField", "Gamma", "Blur", "Noise", "ReconstructMeanDWI",
           "ReconstructMeanDWIClassic", "MeanDWI"]

NEAREST, LINEAR, BSPLINE = 0, 1, 2
_INTERP = {"nearest": NEAREST, "linear": LINEAR, "bspline": BSPLINE}
_LABEL_DTYPES = {torch.uint8: 1, torch.bool: 1, torch.int32: 4, torch.float32: 4, torch.int64: 8}


def _i3(v):
    return (C.c_int32 * 3)(*[int(a) for a in v])


def _upload(values, dtype, device):
    """host values -> device tensor through pinned memory, without blocking the host"""
    t = torch.tensor(values, dtype=dtype)
    if device.type == "cuda":
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


def _percentile_rank(n, q):
    """np.percentile(method='linear') of n sorted values: (rank k, fraction t) with value lerp(v[k], v[k+1], t)"""
    vi = (n - 1) * (np.float64(q) / 100.0)
    k = int(np.floor(vi))
    t = float(vi - k)
    if k >= n - 1:
        return n - 1, 0.0
    return k, t


class _State:
    """A subject during one call: materialised tensors and, per name, the intensity stages not yet applied."""

    def __init__(self, subject, label_maps, spacing, generator, label_values=None, attributes=None):
        self.data = dict(subject)
        self.owned = set()
        self.labels = set(label_maps)
        self.spacing = tuple(float(s) for s in spacing)
        self.gen = generator
        self.pending = {}
        self.blur = {}        # name -> sigmas in voxels of a blur not yet applied (it runs before pending[name])
        self.keep = []        # device parameter tensors of launches already enqueued
        # metadata of the preprocessing transforms (preprocessing.py)
        self.label_values = {k: dict(v) for k, v in (label_values or {}).items()}
        self.one_hot = set()
        # name -> preprocessing pass not yet launched into data[name] (already allocated with its final shape and dtype);
        # it runs before blur[name] and pending[name]
        self.deferred = {}
        # per-image host attributes ({image name: {key: value}}, the reference's TensorLoader(belongs_to=...)), e.g.
        # full_dwi's gradient table; None when the caller gave none
        self.attributes = None if attributes is None else {k: dict(v) for k, v in attributes.items()}

    def images(self, t, intensity):
        names = [k for k in self.data if (t.include is None or k in t.include) and k not in t.exclude]
        return [k for k in names if k not in self.labels] if intensity else names

    def set(self, name, tensor):
        self.data[name] = tensor
        self.owned.add(name)

    def flush(self, name):
        """apply the deferred blur and the pending intensity stages of `name`.  The caller's tensors are never written:
        a name is `owned` only once it holds a tensor this call allocated."""
        pre = self.deferred.pop(name, None)
        if pre is not None:
            pre.run(self)
        stages = self.pending.pop(name, None) or []
        sig = self.blur.pop(name, None)
        if sig is not None:
            # the stages up to the first rescale need no statistics of the blurred image: they run as the epilogue of
            # the last blurred axis
            k = next((i for i, st in enumerate(stages) if st[0] == "rescale"), len(stages))
            self.set(name, _run_blur(self.data[name], sig, stages[:k], self))
            stages = stages[k:]
        if stages:
            x = self.data[name]
            y = x if name in self.owned else torch.empty_like(x)
            _run_program(x, y, stages, self)
            self.set(name, y)

    def flush_all(self):
        for name in list(self.deferred) + list(self.pending) + list(self.blur):
            self.flush(name)

    def meta(self):
        m = {"spacing": self.spacing, "label_maps": sorted(k for k in self.labels if k in self.data),
             "label_values": {k: dict(v) for k, v in self.label_values.items() if k in self.data},
             "one_hot": sorted(k for k in self.one_hot if k in self.data)}
        if self.attributes is not None:
            m["attributes"] = {k: dict(v) for k, v in self.attributes.items() if k in self.data}
        return m


# ---------------------------------------------------------------------------------------------- native calls
def _program(x, stages, state):
    """stage descriptors -> ctypes array; rescale statistics are computed here, each over the stages before it"""
    L = _lib.lib()
    dev = x.device
    arr = (_lib.AugStage * max(1, len(stages)))()
    C_, size3 = x.shape[0], _i3(x.shape[1:])
    n = x.numel()
    for j, st in enumerate(stages):
        kind = st[0]
        s = arr[j]
        if kind == "bias":
            coef = _upload(st[2], torch.float32, dev)
            state.keep.append(coef)
            s.op, s.order, s.vec = _lib.AUG_BIAS, st[1], coef.data_ptr()
        elif kind == "gamma":
            g = _upload(st[1], torch.float32, dev)
            state.keep.append(g)
            s.op, s.vec = _lib.AUG_GAMMA, g.data_ptr()
        elif kind == "noise":
            s.op, s.a, s.b, s.seed = _lib.AUG_NOISE, st[1], st[2], st[3]
        elif kind == "rescale":
            (omin, omax), (plo, phi) = st[1], st[2]
            stats = torch.empty(2, dtype=torch.float64, device=dev)
            state.keep.append(stats)
            ranks = [_percentile_rank(n, plo), _percentile_rank(n, phi)]
            ws = torch.empty(int(L.m355_aug_workspace()), dtype=torch.uint8, device=dev)
            state.keep.append(ws)
            ks = (C.c_int64 * 2)(*[r[0] for r in ranks])
            fr = (C.c_double * 2)(*[r[1] for r in ranks])
            check(L.m355_aug_order_stats(_p(x), C_, size3, arr, j, 2, ks, fr, _p(stats), _p(ws), ws.numel(), _stream()),
                  "aug_order_stats")
            s.op, s.a, s.b, s.stats = _lib.AUG_RESCALE, float(omin), float(omax), stats.data_ptr()
        else:
            raise M355Error(f"unknown intensity stage {kind}")
    return arr


def _run_blur(x, sigmas, epilogue, state):
    """separable Gaussian over the axes with sigma > 0 (at least one), `epilogue` stages fused into the last axis"""
    L = _lib.lib()
    axes = [a for a in range(3) if sigmas[a] > 0]
    for a in axes:
        y = torch.empty_like(x)
        last = a == axes[-1]
        arr = _program(x, epilogue, state) if last else None
        check(L.m355_aug_blur(_p(x), _p(y), x.shape[0], _i3(x.shape[1:]), a, float(sigmas[a]), arr,
                              len(epilogue) if last else 0, _stream()), "aug_blur")
        state.keep.append(x)
        x = y
    return x


def _run_program(x, y, stages, state):
    arr = _program(x, stages, state)
    check(_lib.lib().m355_aug_intensity(_p(x), _p(y), x.shape[0], _i3(x.shape[1:]), arr, len(stages), _stream()),
          "aug_intensity")


def _pad_values(x, pad, state):
    """(device double per channel or None, constant) for a float image"""
    L = _lib.lib()
    C_ = x.shape[0]
    if isinstance(pad, numbers.Number):
        return None, float(pad)
    out = torch.empty(C_, dtype=torch.float64, device=x.device)
    state.keep.append(out)
    if pad == "otsu":
        check(L.m355_aug_otsu_pad(_p(x), C_, _i3(x.shape[1:]), _p(out), _stream()), "aug_otsu_pad")
    elif pad == "minimum":
        ws = torch.empty(8 * C_, dtype=torch.uint8, device=x.device)
        state.keep.append(ws)
        check(L.m355_aug_channel_minmax(_p(x), C_, _i3(x.shape[1:]), 0, _p(out), _p(ws), ws.numel(), _stream()),
              "aug_channel_minmax")
    else:
        raise M355Error(f"pad value {pad!r}: a number, 'minimum' or 'otsu'")
    return out, 0.0


def _resample(state, name, mat, out_shape, interp, grid=None, pad=0.0, exact=False):
    """state.data[name] <- resampled: q = mat[:, :3] p + mat[:, 3] + d(p) (index space)"""
    state.flush(name)
    x = state.data[name]
    is_label = name in state.labels
    if x.dim() != 4 or not x.is_cuda:
        raise M355Error(f"{name}: expected a device tensor [C, V0, V1, V2], got {tuple(x.shape)} on {x.device}")
    if is_label:
        if x.dtype not in _LABEL_DTYPES:
            raise M355Error(f"{name}: label dtype {x.dtype} (uint8, bool, int32, int64, float32)")
        elem = _LABEL_DTYPES[x.dtype]
    elif x.dtype != torch.float32:
        raise M355Error(f"{name}: images must be float32, got {x.dtype}")
    else:
        elem = 4
    mode = NEAREST if (is_label or exact) else interp
    x = x.contiguous()
    src = x
    if mode == BSPLINE:
        src = x.clone()
        check(_lib.lib().m355_aug_prefilter(_p(src), x.shape[0], _i3(x.shape[1:]), _stream()), "aug_prefilter")
        state.keep.append(src)
    pad_dev, pad_c = (None, 0.0) if (is_label or exact) else _pad_values(x, pad, state)
    y = torch.empty((x.shape[0],) + tuple(out_shape), dtype=x.dtype, device=x.device)
    m = (C.c_double * 12)(*np.asarray(mat, dtype=np.float64).reshape(12).tolist())
    gptr, g3 = None, None
    if grid is not None:
        g = _upload(np.ascontiguousarray(grid, dtype=np.float32).reshape(-1).tolist(), torch.float32, x.device)
        state.keep.append(g)
        gptr, g3 = _p(g), _i3(grid.shape[:3])
    check(_lib.lib().m355_aug_resample(_p(src), _p(y), x.shape[0], _i3(x.shape[1:]), _i3(out_shape), elem, mode, m, None,
                                       gptr, g3, _p(pad_dev), pad_c, _stream()), "aug_resample")
    state.set(name, y)


# ---------------------------------------------------------------------------------------------- base classes
class Transform:
    """include / exclude / p as torchio's; __call__ runs the transform on a subject dict"""

    def __init__(self, p=1.0, include=None, exclude=None):
        self.probability = float(p)
        self.include = None if include is None else ([include] if isinstance(include, str) else list(include))
        self.exclude = [] if exclude is None else ([exclude] if isinstance(exclude, str) else list(exclude))
        self.last_history = None
        self.last_meta = None

    def __call__(self, subject, label_maps=(), spacing=(1.0, 1.0, 1.0), generator=None, label_values=None,
                 attributes=None):
        """label_values: {label map name: {label name: id}} (the reference's per-map `label_values`); the resulting
        metadata (spacing, label maps, label_values, one-hot maps) is published as `last_meta`.  attributes: host
        values attached to an image, {image name: {key: value}} (the reference's TensorLoader(belongs_to=...)), e.g.
        {"full_dwi": {"grad": [N, 4] table}} for ReconstructMeanDWI; published in `last_meta` only when given"""
        for k, v in subject.items():
            if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dim() != 4:
                raise M355Error(f"{k}: expected a device tensor [C, V0, V1, V2]")
        state = _State(subject, label_maps, spacing, generator, label_values, attributes)
        self._run(state)
        state.flush_all()
        self.last_meta = state.meta()
        return dict(state.data)

    def _rand(self, state, *shape):
        return torch.rand(*shape, generator=state.gen, dtype=torch.float64)

    def _uniform(self, state, lo, hi, *shape):
        return lo + (hi - lo) * self._rand(state, *shape)

    def _run(self, state):
        self.last_history = None
        if float(self._rand(state, 1)[0]) > self.probability:   # torchio draws the gate on every call
            return
        self._apply(state)

    def _apply(self, state):
        raise NotImplementedError


def _range(v, around=None):
    """torchio's parameter ranges: a number x -> (-x, x) (or (around - x, around + x)), a pair stays"""
    if isinstance(v, numbers.Number):
        return (around - v, around + v) if around is not None else (-v, v)
    return tuple(float(a) for a in v)


class Compose(Transform):
    def __init__(self, transforms, p=1.0, include=None, exclude=None):
        super().__init__(p, include, exclude)
        self.transforms = list(transforms)

    def _apply(self, state):
        hist = []
        inc, exc = self.include, self.exclude
        for t in self.transforms:
            # a Compose's include / exclude narrows every child's
            saved = (t.include, t.exclude)
            if inc is not None:
                t.include = inc if t.include is None else [k for k in t.include if k in inc]
            t.exclude = list(t.exclude) + list(exc)
            try:
                t._run(state)
            finally:
                t.include, t.exclude = saved
            hist.append((type(t).__name__, t.last_history))
        self.last_history = hist


class OneOf(Compose):
    """one child, drawn with the given weights (a list: equal weights; a dict: transform -> weight)"""

    def __init__(self, transforms, p=1.0, include=None, exclude=None):
        if isinstance(transforms, dict):
            items, w = list(transforms.keys()), [float(v) for v in transforms.values()]
        else:
            items, w = list(transforms), [1.0] * len(transforms)
        super().__init__(items, p, include, exclude)
        self.weights = torch.tensor(w, dtype=torch.float64)

    def _apply(self, state):
        i = int(torch.multinomial(self.weights / self.weights.sum(), 1, generator=state.gen)[0])
        chosen = self.transforms
        self.transforms = [chosen[i]]
        try:
            Compose._apply(self, state)
        finally:
            self.transforms = chosen
        self.last_history = {"chosen": i, "history": self.last_history[0]}


# ---------------------------------------------------------------------------------------------- spatial
def _signed_permutation(perm, flip, shape):
    """index-space matrix of y = x.permute(perm).flip(flipped axes): output axis j reads input axis perm[j]"""
    M = np.zeros((3, 4))
    out = [shape[perm[j]] for j in range(3)]
    for j in range(3):
        if flip[j]:
            M[perm[j], j], M[perm[j], 3] = -1.0, out[j] - 1
        else:
            M[perm[j], j] = 1.0
    return M, out


class Flip(Transform):
    def __init__(self, axes, **kw):
        super().__init__(**kw)
        self.axes = tuple(int(a) for a in axes)

    def _apply(self, state):
        flip = [a in self.axes for a in range(3)]
        self.last_history = {"flip": tuple(flip)}
        if not any(flip):
            return   # the identity: no pass over the subject
        for name in state.images(self, intensity=False):
            M, out = _signed_permutation((0, 1, 2), flip, state.data[name].shape[1:])
            _resample(state, name, M, out, NEAREST, exact=True)


class RandomFlip(Transform):
    def __init__(self, axes=0, flip_probability=0.5, p=1.0, include=None, exclude=None):
        super().__init__(p, include, exclude)
        self.axes = (axes,) if isinstance(axes, int) else tuple(axes)
        self.flip_probability = flip_probability

    def _apply(self, state):
        r = self._rand(state, 3)
        axes = tuple(a for a in range(3) if a in self.axes and float(r[a]) < self.flip_probability)
        t = Flip(axes, include=self.include, exclude=self.exclude)
        t._apply(state)
        self.last_history = t.last_history


class PermuteDimensions(Transform):
    def __init__(self, permutation, **kw):
        super().__init__(**kw)
        self.permutation = tuple(int(a) for a in permutation)

    def _apply(self, state):
        self.last_history = {"permutation": self.permutation}
        if self.permutation == (0, 1, 2):
            return   # the identity: no pass over the subject
        for name in state.images(self, intensity=False):
            M, out = _signed_permutation(self.permutation, (False,) * 3, state.data[name].shape[1:])
            _resample(state, name, M, out, NEAREST, exact=True)


class RandomPermuteDimensions(Transform):
    """the reference's own transform (segmentation_pipeline/transforms/permute_dimensions.py:47-57): a uniformly random
    permutation of the three spatial axes; the spacing is not permuted (the reference leaves the affine alone)"""

    def _apply(self, state):
        perm = tuple(int(a) for a in torch.randperm(3, generator=state.gen))
        t = PermuteDimensions(perm, include=self.include, exclude=self.exclude)
        t._apply(state)
        self.last_history = t.last_history


class ElasticDeformation(Transform):
    """control_grid: [K0, K1, K2, 3] displacements in mm; spans the volume; images pad with their minimum"""

    def __init__(self, control_grid, image_interpolation="linear", **kw):
        super().__init__(**kw)
        self.control_grid = np.asarray(control_grid, dtype=np.float64)
        self.interp = _INTERP[image_interpolation]

    def _apply(self, state):
        grid = self.control_grid / np.asarray(state.spacing)     # mm -> voxels
        M = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
        for name in state.images(self, intensity=False):
            _resample(state, name, M, state.data[name].shape[1:], self.interp, grid=grid, pad="minimum")
        self.last_history = {"control_grid": self.control_grid.copy()}


class RandomElasticDeformation(Transform):
    def __init__(self, num_control_points=7, max_displacement=7.5, locked_borders=2, image_interpolation="linear",
                 label_interpolation="nearest", p=1.0, include=None, exclude=None):
        super().__init__(p, include, exclude)
        self.ncp = (num_control_points,) * 3 if isinstance(num_control_points, int) else tuple(num_control_points)
        self.max_disp = (float(max_displacement),) * 3 if isinstance(max_displacement, numbers.Number) \
            else tuple(float(a) for a in max_displacement)
        if locked_borders not in (0, 1, 2):
            raise ValueError("locked_borders must be 0, 1 or 2")
        if min(self.ncp) < 4:
            raise ValueError("num_control_points must be >= 4 on every axis")
        self.locked_borders = locked_borders
        self.image_interpolation = image_interpolation

    def _apply(self, state):
        f = (self._rand(state, *self.ncp, 3) - 0.5).numpy()
        f *= 2.0 * np.asarray(self.max_disp)
        for b in range(self.locked_borders):
            f[b, :, :] = 0
            f[-1 - b, :, :] = 0
            f[:, b, :] = 0
            f[:, -1 - b, :] = 0
            f[:, :, b] = 0
            f[:, :, -1 - b] = 0
        t = ElasticDeformation(f, self.image_interpolation, include=self.include, exclude=self.exclude)
        t._apply(state)
        self.last_history = t.last_history


def _rotation(deg):
    a, b, c = (math.radians(d) for d in deg)
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def affine_index_matrix(scales, degrees, translation, shape, spacing):
    """3x4 index-space matrix of q = R S (p - c) + c + t about the volume centre c, built in mm with `spacing`"""
    sp = np.asarray(spacing, dtype=np.float64)
    A = np.diag(1.0 / sp) @ _rotation(degrees) @ np.diag(np.asarray(scales, dtype=np.float64)) @ np.diag(sp)
    c = (np.asarray(shape, dtype=np.float64) - 1) / 2
    t = c + np.asarray(translation, dtype=np.float64) / sp - A @ c
    return np.concatenate([A, t[:, None]], axis=1)


class Affine(Transform):
    def __init__(self, matrix, image_interpolation="linear", default_pad_value="minimum", **kw):
        super().__init__(**kw)
        self.matrix = np.asarray(matrix, dtype=np.float64).reshape(3, 4)
        self.interp = _INTERP[image_interpolation]
        self.pad = default_pad_value

    def _apply(self, state):
        for name in state.images(self, intensity=False):
            _resample(state, name, self.matrix, state.data[name].shape[1:], self.interp, pad=self.pad)
        self.last_history = {"matrix": self.matrix.copy(), "pad": self.pad}


class RandomAffine(Transform):
    def __init__(self, scales=0.1, degrees=10, translation=0, isotropic=False, center="image",
                 default_pad_value="minimum", image_interpolation="linear", p=1.0, include=None, exclude=None):
        super().__init__(p, include, exclude)
        self.scales = _range(scales, 1.0)
        self.degrees = _range(degrees)
        self.translation = _range(translation)
        self.isotropic = isotropic
        if center != "image":
            raise M355Error("RandomAffine: only center='image' is supported")
        self.pad = default_pad_value
        self.image_interpolation = image_interpolation

    def _apply(self, state):
        s = self._uniform(state, *self.scales, 3).numpy()
        if self.isotropic:
            s[:] = s[0]
        d = self._uniform(state, *self.degrees, 3).numpy()
        tr = self._uniform(state, *self.translation, 3).numpy()
        names = state.images(self, intensity=False)
        if not names:
            return
        shape = state.data[names[0]].shape[1:]
        M = affine_index_matrix(s, d, tr, shape, state.spacing)
        t = Affine(M, self.image_interpolation, self.pad, include=self.include, exclude=self.exclude)
        t._apply(state)
        self.last_history = dict(t.last_history, scales=s, degrees=d, translation=tr)


# ---------------------------------------------------------------------------------------------- intensity
class _Intensity(Transform):
    def _stage(self, name, state):
        raise NotImplementedError

    def _apply(self, state):
        for name in state.images(self, intensity=True):
            x = state.data[name]
            if x.dtype != torch.float32:
                raise M355Error(f"{name}: images must be float32, got {x.dtype}")
            st = self._stage(name, state)
            pend = state.pending.setdefault(name, [])
            if len(pend) >= _lib.AUG_MAX_STAGES:
                state.flush(name)
                pend = state.pending.setdefault(name, [])
            pend.append(st)


class BiasField(_Intensity):
    def __init__(self, coefficients, order=3, **kw):
        super().__init__(**kw)
        self.coefficients = [float(c) for c in coefficients]
        self.order = int(order)
        if len(self.coefficients) != (order + 1) * (order + 2) * (order + 3) // 6:
            raise ValueError("BiasField: wrong number of coefficients for the order")

    def _stage(self, name, state):
        self.last_history = {"coefficients": list(self.coefficients), "order": self.order}
        return ("bias", self.order, self.coefficients)


class RandomBiasField(_Intensity):
    def __init__(self, coefficients=0.5, order=3, p=1.0, include=None, exclude=None):
        super().__init__(p, include, exclude)
        self.coefficients = _range(coefficients)
        self.order = order

    def _apply(self, state):
        """one coefficient set per image, drawn in subject order"""
        n = (self.order + 1) * (self.order + 2) * (self.order + 3) // 6
        hist = {}
        for name in state.images(self, intensity=True):
            c = self._uniform(state, *self.coefficients, n).tolist()
            BiasField(c, self.order, include=[name])._apply(state)
            hist[name] = c
        self.last_history = {"coefficients": hist, "order": self.order}


class RescaleIntensity(_Intensity):
    def __init__(self, out_min_max=(0, 1), percentiles=(0, 100), p=1.0, include=None, exclude=None):
        super().__init__(p, include, exclude)
        self.out_min_max = _range(out_min_max)
        self.percentiles = (float(percentiles), 100.0 - float(percentiles)) if isinstance(percentiles, numbers.Number) \
            else tuple(float(a) for a in percentiles)

    def _stage(self, name, state):
        self.last_history = {"out_min_max": self.out_min_max, "percentiles": self.percentiles}
        return ("rescale", self.out_min_max, self.percentiles)


class Gamma(_Intensity):
    def __init__(self, gammas, **kw):
        super().__init__(**kw)
        self.gammas = [float(g) for g in np.atleast_1d(gammas)]

    def _stage(self, name, state):
        C_ = state.data[name].shape[0]
        g = self.gammas * C_ if len(self.gammas) == 1 else self.gammas
        if len(g) != C_:
            raise M355Error(f"Gamma: {len(g)} exponents for {C_} channels")
        self.last_history = {"gammas": list(g)}
        return ("gamma", g)


class RandomGamma(_Intensity):
    def __init__(self, log_gamma=0.3, p=1.0, include=None, exclude=None):
        super().__init__(p, include, exclude)
        self.log_gamma = _range(log_gamma)

    def _apply(self, state):
        hist = {}
        for name in state.images(self, intensity=True):
            g = torch.exp(self._uniform(state, *self.log_gamma, state.data[name].shape[0])).tolist()
            t = Gamma(g, include=[name])
            t._apply(state)
            hist[name] = t.last_history["gammas"]
        self.last_history = {"gammas": hist}


class Noise(_Intensity):
    def __init__(self, mean, std, seed, **kw):
        super().__init__(**kw)
        self.mean, self.std, self.seed = float(mean), float(std), int(seed) & ((1 << 64) - 1)

    def _stage(self, name, state):
        self.last_history = {"mean": self.mean, "std": self.std, "seed": self.seed}
        return ("noise", self.mean, self.std, self.seed)


class RandomNoise(_Intensity):
    def __init__(self, mean=0, std=(0, 0.25), p=1.0, include=None, exclude=None):
        super().__init__(p, include, exclude)
        self.mean = _range(mean)
        self.std = (0.0, float(std)) if isinstance(std, numbers.Number) else tuple(float(a) for a in std)

    def _apply(self, state):
        """one (mean, std, seed) per call, as torchio: images of one shape get the same noise field"""
        mean = float(self._uniform(state, *self.mean, 1)[0])
        std = float(self._uniform(state, *self.std, 1)[0])
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=state.gen)[0])
        t = Noise(mean, std, seed, include=self.include, exclude=self.exclude)
        t._apply(state)
        self.last_history = t.last_history


class Blur(Transform):
    """scipy gaussian_filter(mode='reflect', truncate=4) per channel; sigmas in mm, converted with the spacing"""

    def __init__(self, sigmas, **kw):
        super().__init__(**kw)
        self.sigmas = tuple(float(s) for s in sigmas)

    def _apply(self, state):
        """the blur is deferred: the bias / gamma / noise stages queued after it run as the epilogue of its last axis
        (_State.flush).  sigma = 0 on every axis is the identity and touches nothing."""
        sv = tuple(self.sigmas[a] / state.spacing[a] for a in range(3))
        self.last_history = {"sigmas": self.sigmas}
        if not any(s > 0 for s in sv):
            return
        for name in state.images(self, intensity=True):
            if state.data[name].dtype != torch.float32:
                raise M355Error(f"{name}: images must be float32, got {state.data[name].dtype}")
            state.flush(name)
            state.blur[name] = sv


class RandomBlur(Transform):
    def __init__(self, std=(0, 2), p=1.0, include=None, exclude=None):
        super().__init__(p, include, exclude)
        self.std = _range(std) if not isinstance(std, numbers.Number) else (0.0, float(std))

    def _apply(self, state):
        """three sigmas per image, drawn in subject order (torchio draws the blur per image)"""
        hist = {}
        for name in state.images(self, intensity=True):
            s = tuple(self._uniform(state, *self.std, 3).tolist())
            Blur(s, include=[name])._apply(state)
            hist[name] = s
        self.last_history = {"sigmas": hist}


# ---------------------------------------------------------------------------------------------- diffusion
def _grad_table(grad, num_channels=None):
    """a host gradient table -> float64 [N, 4] (bvec x, y, z, bval); N must be the channel count of full_dwi"""
    if isinstance(grad, torch.Tensor):
        if grad.device.type != "cpu":
            raise M355Error("the gradient table must be a host tensor or array (reading a device one would synchronise)")
        grad = grad.numpy()
    g = np.asarray(grad, dtype=np.float64)
    if g.ndim != 2 or g.shape[1] != 4:
        raise M355Error(f"gradient table of shape {g.shape}: expected [N, 4] (bvec, bval)")
    if num_channels is not None and g.shape[0] != num_channels:
        raise M355Error(f"gradient table of {g.shape[0]} rows for a full_dwi of {num_channels} channels")
    return g


def _eligible(g, bval_range):
    """row indices whose bval lies strictly inside bval_range"""
    lo, hi = bval_range
    idx = np.nonzero((g[:, 3] > lo) & (g[:, 3] < hi))[0]
    if idx.size == 0:
        raise M355Error(f"no gradient with a bval strictly inside {tuple(bval_range)}")
    return idx


def _pair(v):
    return isinstance(v, (tuple, list)) and len(v) == 2


def _dwi_grad(state, full, key):
    attrs = (state.attributes or {}).get(full, {})
    if key not in attrs:
        raise M355Error(f"{full}: no '{key}' gradient table: pass attributes={{'{full}': {{'{key}': [N, 4] table}}}}")
    return _grad_table(attrs[key], state.data[full].shape[0])


class MeanDWI(Transform):
    """mean_dwi <- the mean of the channels `channels` (indices into full_dwi, in pick order, duplicates allowed) of
    full_dwi: one launch of m355_dwi_mean.  full_dwi's deferred and pending work runs first; an existing mean_dwi is
    replaced and its own deferred / pending work dropped (it belonged to the old data); a missing full_dwi is a no-op.
    include / exclude are not consulted: the images are addressed by name."""

    def __init__(self, channels, full_dwi_image_name="full_dwi", mean_dwi_image_name="mean_dwi", **kw):
        super().__init__(**kw)
        self.channels = [int(c) for c in np.atleast_1d(np.asarray(channels))]
        if not self.channels or min(self.channels) < 0:
            raise M355Error(f"MeanDWI: channels {self.channels}: at least one, none negative")
        self.full_dwi_image_name = full_dwi_image_name
        self.mean_dwi_image_name = mean_dwi_image_name

    def _apply(self, state):
        full, mean = self.full_dwi_image_name, self.mean_dwi_image_name
        self.last_history = {"channels": list(self.channels)}
        if full not in state.data:
            return
        state.flush(full)
        x = state.data[full]
        if x.dtype != torch.float32:
            raise M355Error(f"{full}: images must be float32, got {x.dtype}")
        N = x.shape[0]
        if max(self.channels) >= N:
            raise M355Error(f"MeanDWI: channel {max(self.channels)} of a {full} with {N} channels")
        x = x.contiguous()
        for pend in (state.deferred, state.blur, state.pending):
            pend.pop(mean, None)
        created = mean not in state.data
        idx = _upload(self.channels, torch.int32, x.device)
        y = torch.empty((1,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
        check(_lib.lib().m355_dwi_mean(_p(x), N, _i3(x.shape[1:]), _p(idx), len(self.channels), _p(y), _stream()),
              "dwi_mean")
        state.keep += [x, idx]
        state.set(mean, y)
        if created and state.attributes is not None and full in state.attributes:
            state.attributes[mean] = dict(state.attributes[full])   # the reference deep-copies full_dwi's image


class ReconstructMeanDWI(Transform):
    """the reference's ReconstructMeanDWI (segmentation_pipeline/transforms/reconstruct_mean_dwi.py): mean_dwi <- the
    mean of num_dwis channels of full_dwi, drawn with replacement with probability proportional to
    max_j |b_i . d_j|^directionality over m random unit directions d_j; only gradients whose bval lies strictly inside
    bval_range are eligible.  The gradient table comes from the call's attributes[full_dwi_image_name][bvec_name].
    Draw order and laws: `draw`; DESIGN §4.10."""

    def __init__(self, full_dwi_image_name="full_dwi", mean_dwi_image_name="mean_dwi", bvec_name="grad", num_dwis=15,
                 num_directions=1, directionality=4, bval_range=(1e-5, 501.0), p=1.0):
        super().__init__(p)
        self.full_dwi_image_name = full_dwi_image_name
        self.mean_dwi_image_name = mean_dwi_image_name
        self.bvec_name = bvec_name
        for what, v in (("num_dwis", num_dwis), ("num_directions", num_directions)):
            ok = (_pair(v) and all(isinstance(a, numbers.Integral) for a in v) and v[0] <= v[1]) or \
                isinstance(v, numbers.Integral)
            if not ok:
                raise M355Error(f"ReconstructMeanDWI: {what} {v!r}: an int or a pair of ints (lo <= hi)")
        if (min(num_dwis) if _pair(num_dwis) else num_dwis) < 1:
            raise M355Error(f"ReconstructMeanDWI: num_dwis {num_dwis!r} can draw fewer than one image")
        if _pair(num_directions) and num_directions[0] < 1:
            raise M355Error(f"ReconstructMeanDWI: num_directions {num_directions!r} can draw no direction")
        if isinstance(num_directions, numbers.Integral) and _pair(num_dwis):
            # the reference returns num_dwis for an int num_directions: randn(3, (lo, hi)) raises there
            raise M355Error("ReconstructMeanDWI: an int num_directions with a range of num_dwis (the reference fails)")
        if not (isinstance(directionality, numbers.Number) or
                (_pair(directionality) and all(isinstance(a, numbers.Number) for a in directionality))):
            raise M355Error(f"ReconstructMeanDWI: directionality {directionality!r}: a number or a pair")
        self.num_dwis = tuple(num_dwis) if _pair(num_dwis) else int(num_dwis)
        self.num_directions = tuple(num_directions) if _pair(num_directions) else int(num_directions)
        self.directionality = tuple(float(a) for a in directionality) if _pair(directionality) else float(directionality)
        self.bval_range = tuple(float(a) for a in bval_range)

    def draw(self, grad, generator=None, num_channels=None):
        """the draws after the gate, on the host, from `generator`: num_dwis (int, or int(u^2 (hi - lo + 1) + lo) with
        u ~ U[0, 1)), num_directions (uniform on the inclusive range; an int gives num_dwis, the reference's quirk),
        directionality (U(a, b) for a pair), randn(3, m) directions with unit columns, then num_dwis picks with
        replacement (torch.multinomial).  -> history; `channels` index full_dwi"""
        g = _grad_table(grad, num_channels)
        elig = _eligible(g, self.bval_range)
        gen = generator

        def rand():
            return float(torch.rand(1, generator=gen, dtype=torch.float64)[0])

        if isinstance(self.num_dwis, int):
            n = self.num_dwis
        else:
            lo, hi = self.num_dwis
            n = int(rand() ** 2 * (hi - lo + 1) + lo)
        if isinstance(self.num_directions, int):
            m = n                                   # the reference's quirk (num_dwis is an int here)
        else:
            m = int(torch.randint(self.num_directions[0], self.num_directions[1] + 1, (1,), generator=gen)[0])
        if isinstance(self.directionality, float):
            a = self.directionality
        else:
            a = self.directionality[0] + (self.directionality[1] - self.directionality[0]) * rand()
        d = torch.randn(3, m, generator=gen, dtype=torch.float64).numpy()
        d = d / np.linalg.norm(d, axis=0, keepdims=True)
        prob = np.max(np.abs(g[elig, :3] @ d) ** a, axis=1)
        if not np.isfinite(prob).all() or not prob.sum() > 0:
            raise M355Error("ReconstructMeanDWI: every eligible gradient has probability zero (or a non-finite one)")
        picks = torch.multinomial(torch.from_numpy(prob), n, replacement=True, generator=gen).numpy()
        return {"num_dwis": n, "num_directions": m, "directionality": a, "directions": d,
                "channels": [int(c) for c in elig[picks]]}

    def _apply(self, state):
        if self.full_dwi_image_name not in state.data:
            return   # as the reference: nothing drawn, nothing changed
        hist = self.draw(_dwi_grad(state, self.full_dwi_image_name, self.bvec_name), state.gen)
        MeanDWI(hist["channels"], self.full_dwi_image_name, self.mean_dwi_image_name)._apply(state)
        self.last_history = hist


class ReconstructMeanDWIClassic(Transform):
    """the reference's ReconstructMeanDWIClassic: a random eligible gradient, its subset_size nearest eligible gradients
    (squared distance of the bvecs), and the mean of randint(1, subset_size) of them (a random permutation's first).
    Draw order: `draw`; DESIGN §4.10."""

    def __init__(self, full_dwi_image_name="full_dwi", mean_dwi_image_name="mean_dwi", bvec_name="grad", subset_size=15,
                 bval_range=(1e-5, 501.0), p=1.0):
        super().__init__(p)
        if not isinstance(subset_size, numbers.Integral) or subset_size < 2:
            raise M355Error(f"ReconstructMeanDWIClassic: subset_size {subset_size!r} < 2 (randint(1, subset_size))")
        self.full_dwi_image_name = full_dwi_image_name
        self.mean_dwi_image_name = mean_dwi_image_name
        self.bvec_name = bvec_name
        self.subset_size = int(subset_size)
        self.bval_range = tuple(float(a) for a in bval_range)

    def draw(self, grad, generator=None, num_channels=None):
        """reference gradient (uniform over the eligible ones), the stable float64 squared-distance ranking (the
        reference's argsort is unstable: ties may order differently there), number of selections randint(1,
        subset_size) (upper bound excluded), then randperm of the candidates, whose first selections are taken"""
        g = _grad_table(grad, num_channels)
        elig = _eligible(g, self.bval_range)
        gen = generator
        r = int(torch.randint(0, elig.size, (1,), generator=gen)[0])
        b = g[elig, :3]
        dist = np.sum((b - b[r]) ** 2, axis=1)
        cand = np.argsort(dist, kind="stable")[:self.subset_size]
        nsel = int(torch.randint(1, self.subset_size, (1,), generator=gen)[0])
        perm = torch.randperm(cand.size, generator=gen).numpy()[:nsel]
        return {"reference": int(elig[r]), "subset": [int(c) for c in elig[cand]], "num_selections": nsel,
                "channels": [int(c) for c in elig[cand[perm]]]}

    def _apply(self, state):
        if self.full_dwi_image_name not in state.data:
            return
        hist = self.draw(_dwi_grad(state, self.full_dwi_image_name, self.bvec_name), state.gen)
        MeanDWI(hist["channels"], self.full_dwi_image_name, self.mean_dwi_image_name)._apply(state)
        self.last_history = hist
