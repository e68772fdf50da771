"""Post-processing of label maps on the device: connected components, hole filling, small-component removal and
keep-the-largest-components, with the names, signatures and results of the reference's
segmentation_pipeline/post_processing.py (skimage 0.18 semantics; see DESIGN.md "Post-processing").

Every per-voxel step runs in libm355seg.so (csrc/components.hip): labelling, histograms, the masked 6-neighbour grey
dilation and the dtype casts at the boundary.  Torch only handles arrays with one entry per component or per class
value, and each iteration of the fill loops reads a few scalars back to the host to decide whether to go on.

Inputs: a 3-D numpy array (computed on the current GPU, returned as numpy), a CUDA tensor (stays on its device) or a
CPU tensor (computed on the current GPU, returned on the CPU); dtypes bool, uint8, int8, int16, int32 and int64 (values
must fit int32).  Results have the input's dtype; the input is never modified.

`distance_transform_edt` (scipy.ndimage's, next to `label`) is the exact Euclidean distance transform of
csrc/distance.hip; it also takes float32 volumes and returns float32 distances.

Ties: the reference ranks sizes with numpy's default (unstable) argsort.  Here equal sizes keep numpy's STABLE order --
ascending value for ascending sorts, and the reverse of the stable ascending order for the descending component sort.
"""
import ctypes as C
import operator

import numpy as np
import torch

from . import _lib, ops
from ._lib import M355Error, check
from .ops import _p, _stream

__all__ = ["label", "remove_holes", "keep_components", "remove_small_components", "distance_transform_edt"]

_DTYPE_CODE = {torch.bool: 0, torch.uint8: 0, torch.int8: 1, torch.int16: 2, torch.int32: 3, torch.int64: 4}
_OP_COPY, _OP_IS_ZERO, _OP_POSITIVE = 0, 1, 2
_MODE_VALUES, _MODE_NONPOSITIVE = 0, 1    # m355_ccl_label modes
_MAX_CLASS_RANGE = 1 << 24                # keep_components: max - min + 1 of the class values (documented there)


def _device_volume(img, also=()):
    """(contiguous 3-D tensor on a GPU, function mapping a result tensor back to the caller's kind); `also`: element
    types taken besides the integer ones."""
    if isinstance(img, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(img)).to(torch.device("cuda", torch.cuda.current_device()))
        back = lambda r: r.cpu().numpy()   # noqa: E731
    elif isinstance(img, torch.Tensor):
        if img.is_cuda:
            t, back = img.contiguous(), (lambda r: r)
        else:
            t = img.contiguous().to(torch.device("cuda", torch.cuda.current_device()))
            back = lambda r: r.cpu()   # noqa: E731
    else:
        raise TypeError(f"expected a numpy array or a torch tensor, got {type(img).__name__}")
    if t.dim() != 3:
        raise M355Error(f"expected one 3-D volume [D, H, W], got shape {tuple(t.shape)}")
    if t.dtype not in _DTYPE_CODE and t.dtype not in also:
        raise M355Error(f"unsupported dtype {t.dtype} (bool, uint8, int8, int16, int32, int64)")
    if t.numel() == 0 or t.numel() >= 1 << 31:
        raise M355Error(f"volume of {t.numel()} voxels: need 1 .. 2^31 - 1")
    return t, back


def _to_i32(t, op=_OP_COPY):
    out = torch.empty(t.shape, dtype=torch.int32, device=t.device)
    status = torch.empty(1, dtype=torch.int32, device=t.device)
    check(_lib.lib().m355_label_convert_in(_p(t), _DTYPE_CODE[t.dtype], op, _p(out), t.numel(), _p(status), _stream()),
          "label_convert_in")
    if op == _OP_COPY and t.dtype == torch.int64 and int(status.item()):
        raise M355Error("label values must fit int32")
    return out


def _from_i32(x, dtype, zero_where=None, orig=None):
    out = torch.empty(x.shape if x is not None else orig.shape, dtype=dtype,
                      device=x.device if x is not None else orig.device)
    check(_lib.lib().m355_label_convert_out(_p(x), _p(zero_where), _p(orig), _p(out), _DTYPE_CODE[dtype], out.numel(),
                                            _stream()), "label_convert_out")
    return out


def _ccl(x, connectivity, mode=_MODE_VALUES):
    """(int32 labels 0..n, n) of an int32 device volume; n is read back to the host."""
    L = _lib.lib()
    D, H, W = x.shape
    ws_bytes = int(L.m355_ccl_workspace(D, H, W))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    labels = torch.empty_like(x)
    n = torch.empty(1, dtype=torch.int32, device=x.device)
    check(L.m355_ccl_label(_p(x), _p(labels), _p(n), D, H, W, connectivity, mode, _p(ws), ws_bytes, _stream()), "ccl_label")
    n = int(n.item())
    if n < 0:
        raise M355Error("ccl_label: a bounded find / union loop reached its bound (labels are not valid)")
    return labels, n


def _histogram(a, lo, nbins, b=None, bstride=0, minmax=False):
    """int64 counts [nbins] of the keys a (or a * bstride + b) in [lo, lo + nbins); with minmax also (min, max) of a."""
    counts = torch.empty(nbins, dtype=torch.int64, device=a.device)
    mm = torch.empty(2, dtype=torch.int32, device=a.device) if minmax else None
    check(_lib.lib().m355_label_histogram(_p(a), _p(b), a.numel(), bstride, lo, nbins, _p(counts), _p(mm), _stream()),
          "label_histogram")
    if minmax:
        lo_hi = mm.tolist()
        return counts, (lo_hi[0], lo_hi[1])
    return counts


def _dilate(src, dst, labels, flag, class_rank=None, rank_class=None, lo=0):
    """One masked 6-neighbour dilation step src -> dst; returns the number of voxels that changed."""
    changed = torch.empty(1, dtype=torch.int64, device=src.device)
    D, H, W = src.shape
    check(_lib.lib().m355_masked_dilate6(_p(src), _p(dst), D, H, W, _p(labels), _p(flag), _p(class_rank),
                                         _p(rank_class), int(lo), _p(changed), _stream()), "masked_dilate6")
    return int(changed.item())


def _connectivity(connectivity):
    if connectivity is None:
        return 3   # skimage: None = full connectivity (ndim)
    if connectivity not in (1, 2, 3):
        raise ValueError(f"connectivity {connectivity!r} not in (1, 2, 3) for a 3-D volume")
    return int(connectivity)


def label(img, connectivity=None, return_num=False):
    """skimage.measure.label(img, connectivity=connectivity, return_num=return_num) with background 0: voxels that hold
    the same non-zero value and are neighbours (6 / 18 / 26 for connectivity 1 / 2 / 3 or None) form one component;
    components are numbered 1..n in raster order of their first voxel.  The labels are int64."""
    conn = _connectivity(connectivity)
    t, back = _device_volume(img)
    labels, n = _ccl(_to_i32(t), conn)
    out = back(_from_i32(labels, torch.int64))
    return (out, n) if return_num else out


def distance_transform_edt(img, sampling=None):
    """scipy.ndimage.distance_transform_edt(img, sampling=sampling) for one volume: the Euclidean distance from every
    nonzero voxel to the nearest zero voxel, 0 on the zero voxels.  sampling: the voxel spacing, a number or one per
    axis (None: 1).  Takes the element types of `label` and float32; a numpy array comes back as numpy, a device tensor
    stays on its device, a CPU tensor returns to the CPU.

    The result is float32 (scipy returns float64): exact squared distances for unit sampling -- with a correctly
    rounded square root -- and fp32 rounding of each term otherwise.  A volume without a zero voxel gives +inf
    everywhere (scipy's result is undefined there).  Every axis at most _lib.EDT_MAX_DIM.  Three launches of
    ops.edt_sq and one square-root pass (csrc/distance.hip)."""
    t, back = _device_volume(img, also=(torch.float32,))
    with torch.cuda.device(t.device):
        d2 = ops.edt_sq(t == 0, (1., 1., 1.) if sampling is None else sampling)
        return back(ops.edt_sqrt(d2, out=d2))


def _fill_holes(w, hole_size, max_dilations):
    """remove_holes on an int32 device volume: (filled volume, hole voxels of the first iteration).

    A hole is a 6-connected component of (w <= 0) with fewer than hole_size voxels, wherever it lies (border included).
    Its voxels take the maximum of w over themselves and their 6 neighbours, one Jacobi step per iteration."""
    buf = torch.empty_like(w)
    total = 0
    for it in range(max_dilations):
        labels, n = _ccl(w, 1, _MODE_NONPOSITIVE)
        sizes = _histogram(labels, 0, n + 1)
        hole = sizes < hole_size
        hole[0] = False
        num_holes = int(sizes[hole].sum().item())
        if it == 0:
            total = num_holes
        if num_holes == 0:
            break
        changed = _dilate(w, buf, labels, hole.to(torch.int32))
        w, buf = buf, w
        if changed == 0:
            break   # a fixed point: every further iteration would repeat this one
    return w, total


def remove_holes(img, hole_size, max_dilations=100):
    """Fill the holes of (img > 0) -- 6-connected components of img <= 0 with fewer than hole_size voxels, touching the
    border or not -- from the 6-neighbour grey dilation of the class values, until none is left or max_dilations
    iterations ran.  Returns (filled image, hole voxels found in the first iteration)."""
    t, back = _device_volume(img)
    w, total = _fill_holes(_to_i32(t), hole_size, max_dilations)
    return back(_from_i32(w, t.dtype)), total


def remove_small_components(img, component_size, max_dilations=100):
    """The reference's process: fill the holes of (img == 0) with remove_holes(component_size) -- the holes being the
    6-connected foreground components (any class) with fewer than component_size voxels -- and zero what was filled.
    Returns (image, voxels of those components)."""
    t, back = _device_volume(img)
    w, count = _fill_holes(_to_i32(t, _OP_IS_ZERO), component_size, max_dilations)
    return back(_from_i32(None, t.dtype, zero_where=w, orig=t)), count


def _stable_descending_ranks(counts):
    """rank of every entry when counts are sorted descending (0 = largest); ties: reversed stable ascending order."""
    order = torch.sort(counts, stable=True).indices.flip(0)
    ranks = torch.empty_like(order)
    ranks[order] = torch.arange(order.numel(), device=order.device)
    return ranks


def _as_int(v, what):
    """A Python int from an int, a numpy integer or an integral 0-d tensor / float (any device)."""
    if isinstance(v, torch.Tensor):
        v = v.item()
    if isinstance(v, (bool, np.bool_)):
        raise TypeError(f"{what} must be an integer, got {v!r}")
    if isinstance(v, (float, np.floating)):
        if not float(v).is_integer():
            raise TypeError(f"{what} must be an integer, got {v!r}")
        return int(v)
    return operator.index(v)


def keep_components(img, num, max_dilations=100):
    """Keep the num largest 26-connected components (background voxels together rank as one more entry); the voxels of
    every other component take, one dilation step per iteration, the class of the neighbour whose class has the
    highest count rank (class ranks ascending by voxel count; the rarest class and removed voxels contribute nothing).
    Labels and ranks are recomputed every iteration.  Returns (image, num_components_removed, num_elements_removed),
    both Python ints counted in the first iteration; num_components_removed = entries - 1 - num can be negative.

    num may be any integer, numpy scalar or 0-d tensor -- `img.max()`, as the reference's callers pass it, included:
    the counts are computed with Python integers, never in the dtype of num.  Unlike the reference, class values
    whose max - min + 1 exceeds 2^24 are refused (the class-rank table has one entry per value in that range)."""
    num = _as_int(num, "num")
    t, back = _device_volume(img)
    w = _to_i32(t)
    buf = torch.empty_like(w)
    dev = w.device
    _, (lo, hi) = _histogram(w, 0, 1, minmax=True)   # dilation only copies existing values: the range never grows
    if hi - lo + 1 > _MAX_CLASS_RANGE:
        raise M355Error(f"keep_components: class values span {hi - lo + 1} > {_MAX_CLASS_RANGE}")
    components_removed = elements_removed = 0
    for it in range(max_dilations):
        labels, n = _ccl(w, 3)
        sizes = _histogram(labels, 0, n + 1)
        present = torch.nonzero(sizes > 0).flatten()          # label values in ascending order, as np.unique
        comp_rank = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        comp_rank[present] = _stable_descending_ranks(sizes[present])
        removed = comp_rank > num
        n_removed = int(sizes[removed].sum().item())
        if it == 0:
            elements_removed = n_removed
            components_removed = present.numel() - 1 - num
        if n_removed == 0:
            break
        ccount = _histogram(w, lo, hi - lo + 1)
        classes = torch.nonzero(ccount > 0).flatten()
        order = torch.sort(ccount[classes], stable=True).indices   # ascending count rank
        rank_class = (classes[order] + lo).to(torch.int32)
        class_rank = torch.zeros(hi - lo + 1, dtype=torch.int32, device=dev)
        class_rank[classes[order]] = torch.arange(classes.numel(), dtype=torch.int32, device=dev)
        changed = _dilate(w, buf, labels, removed.to(torch.int32), class_rank, rank_class, lo)
        w, buf = buf, w
        if changed == 0:
            break   # a fixed point: every further iteration would repeat this one
    return back(_from_i32(w, t.dtype)), components_removed, elements_removed
