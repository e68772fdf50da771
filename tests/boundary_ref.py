"""Brute-force restatement of what m355_signed_distance and the boundary-loss kernels compute: the signed
distance map of Kervadec et al.'s `one_hot2dist` in numpy fp64 with tests/distance_ref.edt_sq's arithmetic (a minimum over ALL
voxels of the other membership, no scipy; tested equal to two whole-volume edt_sq calls), its fp32 value for unit spacing, and the loss with its gradient in fp64 torch.  Small
volumes only (distance_ref's O(voxels x sites))."""
import numpy as np
import torch

import distance_ref as DR


def membership(target):
    """bool, target's shape: t > 0.5; a NaN is outside"""
    return np.asarray(target) > 0.5


def _min_d2(voxels, sites, spacing):
    """fp64 [len(voxels)]: distance_ref.edt_sq's minimum over `sites` (its arithmetic, term by term), for the index
    coordinates `voxels` only -- a voxel needs the other membership alone, which is |in| x |out| pairs, not voxels^2"""
    sp = np.asarray(spacing, dtype=np.float64)
    v, s = voxels.astype(np.float64), sites.astype(np.float64)
    out = np.empty(v.shape[0])
    step = max(1, DR._CHUNK_ENTRIES // s.shape[0])
    for at in range(0, v.shape[0], step):
        d = (v[at:at + step, None, :] - s[None, :, :]) * sp
        out[at:at + step] = (d * d).sum(axis=2).min(axis=1)
    return out


def plane_d2_full(m, spacing=(1.0, 1.0, 1.0)):
    """_plane_d2 through two whole-volume distance_ref.edt_sq calls (what _plane_d2 must equal bit for bit)"""
    if m.all() or not m.any():
        return None
    return np.where(m, DR.edt_sq(~m, spacing), DR.edt_sq(m, spacing))


def _plane_d2(m, spacing):
    """fp64 squared distance of every voxel of one plane to the nearest voxel of the OTHER membership, or None for a
    plane with one membership only"""
    if m.all() or not m.any():
        return None
    inside, outside = np.argwhere(m), np.argwhere(~m)
    out = np.empty(m.shape)
    out[m] = _min_d2(inside, outside, spacing)        # (boolean indexing and argwhere share the C order)
    out[~m] = _min_d2(outside, inside, spacing)
    return out


def signed_distance(target, spacing=(1.0, 1.0, 1.0), planes=None):
    """fp64 [N, C, D, H, W]: +d(nearest inside voxel) outside, -(d(nearest outside voxel) - 1) inside, 0 everywhere in a
    plane without a boundary and in the planes switched off by `planes` (N * C flags)"""
    m = membership(target)
    N, C = m.shape[:2]
    out = np.zeros(m.shape, dtype=np.float64)
    for i in range(N * C):
        if planes is not None and not planes[i]:
            continue
        mm = m[i // C, i % C]
        d2 = _plane_d2(mm, spacing)
        if d2 is not None:
            d = np.sqrt(d2)
            out[i // C, i % C] = np.where(mm, -(d - 1.0), d)
    return out


def signed_distance_f32(target, planes=None):
    """the fp32 value for unit spacing, which the kernel must give bit for bit: d2 is an exact integer, float32(sqrt(d2))
    the correctly rounded root, and 1 - root exact in fp32 (root >= 1 is a multiple of its own ulp, and so is root - 1)"""
    m = membership(target)
    N, C = m.shape[:2]
    out = np.zeros(m.shape, dtype=np.float32)
    for i in range(N * C):
        if planes is not None and not planes[i]:
            continue
        mm = m[i // C, i % C]
        d2 = _plane_d2(mm, (1.0, 1.0, 1.0))
        if d2 is not None:
            root = np.sqrt(d2).astype(np.float32)
            out[i // C, i % C] = np.where(mm, np.float32(1) - root, root)
    return out


def scipy_signed_distance(target, spacing=(1.0, 1.0, 1.0)):
    """the published two-transform formula on scipy: distance(negmask) * negmask - (distance(posmask) - 1) * posmask"""
    from scipy.ndimage import distance_transform_edt
    m = membership(target)
    out = np.zeros(m.shape, dtype=np.float64)
    for n in range(m.shape[0]):
        for c in range(m.shape[1]):
            pos = m[n, c]
            if pos.any() and not pos.all():
                neg = ~pos
                out[n, c] = distance_transform_edt(neg, sampling=spacing) * neg - \
                    (distance_transform_edt(pos, sampling=spacing) - 1) * pos
    return out


def loss(p, phi, weights):
    """fp64 0-dim: sum_n sum_c w_c sum_v p phi / (N S sum_c w_c); p, phi [N, C, ...], weights C values"""
    p, phi = p.double(), phi.double()
    w = torch.as_tensor(weights, dtype=torch.float64)
    N, C = p.shape[:2]
    S = p[0, 0].numel()
    rows = (p * phi).reshape(N, C, -1).sum(dim=2)
    return (rows * w).sum() / (N * S * w.sum())


def abs_mass(p, phi, weights):
    """sum_c w_c sum |p phi| / (N S sum_c w_c): the scale of the loss's rounding bound"""
    return loss(p.double().abs(), phi.double().abs(), weights)


def grad(phi, weights, dloss=1.0):
    """fp64 dloss * w_c / (N S sum_c w_c) * phi"""
    phi = phi.double()
    w = torch.as_tensor(weights, dtype=torch.float64)
    N, C = phi.shape[:2]
    S = phi[0, 0].numel()
    return float(dloss) * (w / (N * S * w.sum())).reshape((1, C) + (1,) * (phi.dim() - 2)) * phi
