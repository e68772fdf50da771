"""Reference of the blob (lesion-wise) Dice loss in fp64 torch + scipy.ndimage.label.

`blob_dice_literal` is the definition of Kofler et al.: for every connected component of the binarised target
(target > 0.5, a NaN is no member) of every on plane, the mask of the OTHER components is multiplied into prediction and
target and the Dice expression of the reference HybridLogisticDiceLoss (oracle.torch_ref.hybrid_logistic_dice_loss, eps =
1e-8) is applied to the masked tensors; gradients come from autograd through it.  `blob_dice_closed_form` restates value
and gradient from the sums S, Q, A, B -- the formula the kernels implement; tests/test_blob_loss_cpu.py asserts that the
two agree."""
import numpy as np
import torch
from scipy import ndimage

EPS = 1e-8


def membership(target):
    """bool numpy array of target's shape: t > 0.5; a NaN is no member"""
    t = target.detach().cpu().numpy() if torch.is_tensor(target) else np.asarray(target)
    with np.errstate(invalid="ignore"):
        return t > 0.5


def default_weights(channels):
    return (0.0,) + (1.0,) * (channels - 1) if channels > 1 else (1.0,)


def _is_on(w, planes, n, c):
    """a plane is on when its channel weight is > 0 (and its flag in `planes`, [N][C] order, when those are given)"""
    return w[c] > 0 and (planes is None or bool(planes[n * len(w) + c]))


def plane_labels(member, connectivity=3):
    """scipy's labels of one plane [D, H, W] (numbered in raster order of the first voxel) and their count"""
    lab, n = ndimage.label(member, structure=ndimage.generate_binary_structure(3, connectivity))
    return lab.astype(np.int32), int(n)


def stacked_labels(target, planes=None, connectivity=3):
    """what ops.blob_labels returns, from scipy: (labels int32 [P_on, D, H, W], ranges int32 [P_on, 2], count)"""
    m = membership(target)
    N, C = m.shape[:2]
    flags = [True] * (N * C) if planes is None else [bool(v) for v in planes]
    labels, ranges, run = [], [], 0
    for i, on in enumerate(flags):
        if not on:
            continue
        lab, n = plane_labels(m[i // C, i % C], connectivity)
        labels.append(np.where(lab > 0, lab + run, 0).astype(np.int32))
        ranges.append((run + 1, run + n))
        run += n
    return np.stack(labels), np.asarray(ranges, dtype=np.int32).reshape(-1, 2), run


def _dice(prediction, target, square_dice):
    """the Dice coefficient of oracle.torch_ref.hybrid_logistic_dice_loss for one plane"""
    overlap = (prediction * target).sum()
    if square_dice:
        total = (target * target).sum() + (prediction * prediction).sum()
    else:
        total = target.sum() + prediction.sum()
    return 2 * overlap / (total + EPS)


def blob_dice_literal(prediction, target, class_weights=None, square_dice=True, connectivity=3, planes=None):
    """-> (loss, number of components); prediction: an fp64 tensor [N, C, D, H, W] (autograd flows through it)"""
    m = membership(target)
    N, C = m.shape[:2]
    w = default_weights(C) if class_weights is None else tuple(float(v) for v in class_weights)
    num, wsum, count = prediction.new_zeros(()), 0.0, 0
    for n in range(N):
        for c in range(C):
            if not _is_on(w, planes, n, c):
                continue
            lab, K = plane_labels(m[n, c], connectivity)
            if K == 0:
                continue
            count += K
            y = torch.from_numpy(m[n, c].astype(np.float64))
            plane = prediction.new_zeros(())
            for k in range(1, K + 1):
                others = torch.from_numpy(((lab == 0) | (lab == k)).astype(np.float64))   # 0 on the other components
                plane = plane + (1 - _dice(prediction[n, c] * others, y * others, square_dice))
            num = num + w[c] * plane / K
            wsum += w[c]
    return (num / wsum if wsum > 0 else num), count


def blob_dice_closed_form(prediction, target, class_weights=None, square_dice=True, connectivity=3, planes=None):
    """-> (loss, gradient) as fp64 tensors, from the sums S, Q, A, B of every component and plane"""
    m = membership(target)
    p = prediction.detach().double()
    N, C = m.shape[:2]
    w = default_weights(C) if class_weights is None else tuple(float(v) for v in class_weights)
    per_plane = {}
    for n in range(N):
        for c in range(C):
            if _is_on(w, planes, n, c):
                lab, K = plane_labels(m[n, c], connectivity)
                if K:
                    per_plane[n, c] = (torch.from_numpy(lab.astype(np.int64)), K)
    wsum = sum(w[c] for _, c in per_plane)
    loss, grad = torch.zeros((), dtype=torch.float64), torch.zeros_like(p)
    for (n, c), (lab, K) in per_plane.items():
        q = p[n, c]
        f = w[c] / (K * wsum)
        non = lab == 0
        B = ((q * q) if square_dice else q)[non].sum()
        g_nc = 0.0
        for k in range(1, K + 1):
            sel = lab == k
            S, Q, A = q[sel].sum(), (q[sel] * q[sel]).sum(), float(sel.sum())
            den = A + (Q if square_dice else S) + B + EPS
            loss = loss + f * (1 - 2 * S / den)
            dB = 2 * S / (den * den)
            g_nc = g_nc + dB
            if square_dice:
                grad[n, c][sel] = f * (-2 / den + 2 * dB * q[sel])
            else:
                grad[n, c][sel] = f * (-2 * (A + B + EPS) / (den * den))
        grad[n, c][non] = f * g_nc * (2 * q[non] if square_dice else 1.0)
    return loss, grad


def literal_with_grad(prediction, target, class_weights=None, square_dice=True, connectivity=3, planes=None):
    """-> (loss, gradient, count) of the literal definition through autograd, fp64"""
    p = prediction.detach().double().requires_grad_()
    loss, count = blob_dice_literal(p, target, class_weights, square_dice, connectivity, planes)
    if loss.requires_grad:
        loss.backward()
    return loss.detach(), (p.grad if p.grad is not None else torch.zeros_like(p)), count


# ------------------------------------------------------------------------------------------------------------- cases
def _rand(shape, density, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < density).float()


def _snake():
    """(1, 1, 17, 10, 130): one 6-connected line through every other slice, 22100 voxels in six 4096-voxel chunks"""
    t = torch.zeros(1, 1, 17, 10, 130)
    for i, z in enumerate(range(0, 17, 2)):
        y = 9 if i % 2 else 0
        t[0, 0, z, y, :] = 1.0
        if z + 2 < 17:
            t[0, 0, z + 1, y, 129 if i % 2 == 0 else 0] = 1.0              # up to the next slice at the line's end ..
            t[0, 0, z + 2, :, 129 if i % 2 == 0 else 0] = 1.0              # .. and across it to the next line's row
    return t


def cases():
    """name -> (target fp32 [N, C, D, H, W], class weights (host) or None for the default, planes or None, connectivity).
    With `planes` the weights go to the device as a tensor and the flags say which planes are on."""
    out = {"one_member": (torch.ones(1, 1, 1, 1, 1), None, None, 3),
           "one_non_member": (torch.zeros(1, 1, 1, 1, 1), None, None, 3),
           "rows_1x2x1x1x7": (torch.tensor([[0., 1, 1, 0, 0, 1, 0], [1, 1, 0, 1, 1, 1, 1]]).reshape(1, 2, 1, 1, 7),
                              (1.0, 2.0), None, 3)}
    for density in (0.02, 0.6):     # rows that are no multiple of 4 or 64, off planes, N > 1
        out[f"random_2x3x3x5x70_d{density}"] = (_rand((2, 3, 3, 5, 70), density, 11), (1.0, 1.0, 1.0), [1, 0, 1, 1, 1, 0], 3)
    out["random_6conn_2x3x3x5x70"] = (_rand((2, 3, 3, 5, 70), 0.3, 12), (0.5, 0.0, 2.0), None, 1)
    out["random_18conn_1x2x4x5x9"] = (_rand((1, 2, 4, 5, 9), 0.3, 13), None, None, 2)
    # one component across the faces of the 8 x 8 x 64 labelling tiles on all three axes, a second one elsewhere
    tile = torch.zeros(1, 2, 9, 9, 65)
    tile[0, 1, 7, 7, 60:64] = 1.0
    tile[0, 1, 8, 8, 64] = 1.0          # a corner neighbour of (7, 7, 63) in the next tile along z, y and x
    tile[0, 1, 1, 2, 3:6] = 1.0
    tile[0, 0] = 1.0 - tile[0, 1]
    out["tile_faces_1x2x9x9x65"] = (tile, None, None, 3)
    # the last slice of plane s and the first slice of plane s + 1 are all members: they touch in the stacked volume
    stack = torch.zeros(1, 3, 4, 6, 8)
    stack[0, :, 0] = 1.0
    stack[0, :, 3] = 1.0
    out["stacked_slices_1x3x4x6x8"] = (stack, (1.0, 1.0, 1.0), None, 3)
    z, y, x = torch.meshgrid(torch.arange(6), torch.arange(6), torch.arange(66), indexing="ij")
    checker = ((z + y + x) % 2 == 0).float().reshape(1, 1, 6, 6, 66)
    out["checkerboard_6conn"] = (checker, None, None, 1)      # 1188 single-voxel components: more than an LDS hash holds
    out["checkerboard_26conn"] = (checker, None, None, 3)     # one component
    out["snake_1x1x17x10x130"] = (_snake(), None, None, 1)
    out["all_members"] = (torch.ones(1, 1, 3, 5, 7), None, None, 3)
    empty = torch.zeros(1, 3, 2, 3, 9)
    empty[0, 1, 0, 1, 2:5] = 1.0
    empty[0, 0] = 1.0 - empty[0, 1]
    out["on_plane_without_member"] = (empty, None, None, 3)
    nothing = torch.zeros(1, 2, 2, 3, 9)
    nothing[0, 0] = 1.0
    out["no_member_at_all"] = (nothing, None, None, 3)
    soft = torch.rand((1, 2, 3, 5, 70), generator=torch.Generator().manual_seed(50))
    soft[0, 0, 1, 2, 3:9] = torch.tensor([float("nan"), 0.5, 0.50001, float("inf"), -float("inf"), 0.49999])
    out["soft_1x2x3x5x70"] = (soft, (1.0, 1.0), None, 3)
    return out


PREDICTIONS = ("uniform", "saturated", "tiny")


def prediction(kind, shape, seed=7):
    """fp32 probabilities: uniform in [0, 1); exact zeros and ones (both inside and outside the components); 1e-7"""
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        return torch.rand(shape, generator=g)
    if kind == "saturated":
        return (torch.rand(shape, generator=g) < 0.5).float()
    return torch.full(shape, 1e-7)
