"""float64 numpy restatement of the preprocessing transforms, written from the reference and torchio
0.18.45 independently of segmentation_pipeline_amd.preprocessing.  Arrays are [C, V0, V1, V2]; padding calls np.pad."""
import math

import numpy as np

import augment_ref as AR


def replace_nan(x, v=0.0):
    x = np.array(x, copy=True)
    if np.issubdtype(x.dtype, np.floating):
        x[np.isnan(x)] = v
    return x


def crop(x, c):
    """c = (ini0, fin0, ini1, fin1, ini2, fin2)"""
    V = x.shape[1:]
    return x[:, c[0]:V[0] - c[1], c[2]:V[1] - c[3], c[4]:V[2] - c[5]].copy()


def pad(x, p, mode=0):
    widths = ((0, 0), (p[0], p[1]), (p[2], p[3]), (p[4], p[5]))
    if mode == "minimum":
        return np.pad(x, widths, mode="minimum")
    return np.pad(x, widths, mode="constant", constant_values=mode)


def bbox(mask3):
    """torchio _bbox_mask: (bb_min, bb_max + 1) of the nonzero voxels"""
    idx = np.nonzero(mask3)
    return np.array([i.min() for i in idx]), np.array([i.max() for i in idx]) + 1


def crop_or_pad_bounds(shape, target, mask3=None):
    """torchio 0.18.45 CropOrPad: (padding, cropping) six-tuples, mask-centred or (no / empty mask) centred"""
    shape, target = np.asarray(shape), np.asarray(target)
    if mask3 is None or not np.any(mask3):
        diff = target - shape
        c, p = -np.minimum(diff, 0), np.maximum(diff, 0)
        six = lambda v: tuple(x for n in v for x in (int(math.ceil(n / 2)), int(math.floor(n / 2))))
        return six(p), six(c)
    bb_min, bb_max = bbox(mask3)
    centre = np.mean((bb_min, bb_max), axis=0)
    padding, cropping = [], []
    for d in range(3):
        T, c, V = target[d], centre[d], shape[d]
        if (not (T % 2)) ^ (not (c % 1)):
            c -= 0.5
        begin, end = c - T / 2, c + T / 2
        cropping += [begin if begin >= 0 else 0, V - end if end <= V else 0]
        padding += [0 if begin >= 0 else -begin, 0 if end <= V else end - V]
    return tuple(np.asarray(padding, dtype=int).tolist()), tuple(np.asarray(cropping, dtype=int).tolist())


def crop_or_pad(x, padding, cropping, mode=0):
    return crop(pad(x, padding, mode), cropping)


def crop_to_mask_bounds(m, label_id=1, channel=0):
    """the reference's cropping: (min, V - max) per axis, max the last mask index (so it is cropped away)"""
    w = np.where(m[channel] == label_id)
    V = m.shape[1:]
    return tuple(v for a in range(3) for v in (int(w[a].min()), int(V[a] - w[a].max())))


def min_size_padding(shape, min_size):
    out = []
    for v, m in zip(shape, min_size):
        d = m - v
        out += list((d // 2, d // 2) if d % 2 == 0 else (d // 2, d // 2 + 1)) if v < m else [0, 0]
    return tuple(out)


def anatomical_mask(label, shape):
    W, H, D = shape[1:]
    m = np.zeros(shape, bool)
    if label == "Right":
        m[:, W // 2:] = True
    elif label == "Left":
        m[:, :W // 2] = True
    elif label == "Anterior":
        m[:, :, H // 2:] = True
    elif label == "Posterior":
        m[:, :, :H // 2] = True
    elif label == "Superior":
        m[:, :, :, D // 2:] = True
    elif label == "Inferior":
        m[:, :, :, :D // 2] = True
    return m


def remap(x, mapping, mask=None):
    out = x.copy()
    mask = np.ones(x.shape, bool) if mask is None else np.broadcast_to(mask, x.shape)
    for old, new in mapping.items():
        out[mask & (x == old)] = new
    return out


def one_hot(x, K):
    lab = x[0].astype(np.int64)
    return np.stack([(lab == k) for k in range(K)]).astype(x.dtype)


def image_from_labels(entries, shape, mode="overwrite", one_hot_maps=()):
    """entries: (label array, id, weight, is_one_hot)"""
    out = np.zeros((1,) + tuple(shape), np.float32)
    for data, ident, w, oh in entries:
        lab = np.argmax(data, axis=0)[None] if oh else data[0:1]
        m = lab == ident
        if mode == "additive":
            out += m.astype(np.float32) * np.float32(w)
        else:
            out[m] = w
    return out


def target_spacing(current, target, tolerance):
    if all(abs(c - t) < tol for c, t, tol in zip(current, target, tolerance)):
        return None
    new = []
    for cur, tar, tol in zip(current, target, tolerance):
        step, spacing = 1, cur
        while abs(spacing - tar) > tol:
            scale = round(tar / cur * step) / step if cur < tar else 1 / (round(cur / tar * step) / step)
            spacing = cur * scale
            step += 1
        new.append(spacing)
    return tuple(new)


def resample(x, old, new, mode):
    """torchio Resample: size ceil(V old / new) (singletons stay 1), q = (p + 0.5) s - 0.5, s = new / old, 0 outside"""
    shape = x.shape[1:]
    size = np.ceil(np.asarray(shape) * np.asarray(old, float) / np.asarray(new, float)).astype(int)
    size = tuple(1 if v == 1 else int(n) for v, n in zip(shape, size))
    s = np.asarray(new, float) / np.asarray(old, float)
    mat = np.concatenate([np.diag(s), (0.5 * s - 0.5)[:, None]], axis=1)
    q = AR.coordinates(mat, size)
    y = AR.sample(x.astype(np.float64) if mode != "nearest" else x, q, mode, pad=0.0)
    return np.where(AR.inside(q, shape)[None], y, 0).astype(np.float64 if mode != "nearest" else x.dtype), q
