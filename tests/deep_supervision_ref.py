"""Torch restatements for the deep-supervision tests: the target pyramid, the multi-level forward of
models.DeepSupervisionUNet -- oracle.torch_ref.unet_forward's decoder loop repeated with the auxiliary heads -- and the
weighted loss of criterions.DeepSupervisionLoss.  Test infrastructure, not product code."""
import torch
import torch.nn.functional as F

from oracle import torch_ref as R


def pyramid(y, levels, mode="area"):
    """[level 1, ..., level `levels`] of y [N, C, D, H, W]: the mean of the 2^j cube, or the voxel at its origin"""
    if mode == "area":
        return [F.avg_pool3d(y, 2 ** j) for j in range(1, levels + 1)]
    if mode == "nearest":
        return [y[..., ::2 ** j, ::2 ** j, ::2 ** j].contiguous() for j in range(1, levels + 1)]
    raise ValueError(mode)


def one_hot_target(shape, seed):
    """a seeded one-hot fp32 target [N, C, D, H, W]"""
    N, C = shape[:2]
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, C, (N,) + tuple(shape[2:]), generator=g)
    return F.one_hot(lab, C).permute(0, 4, 1, 2, 3).float().contiguous()


def _head(sd, prefix, x, spec):
    """the tail of R.unet_forward on the convolution `prefix` (softmax or no hypothesis)"""
    x = F.conv3d(x, R._r(sd[prefix + ".weight"], spec), sd[prefix + ".bias"], padding=1)
    if spec.hypothesis == "softmax":
        return torch.softmax(x, dim=1)
    if spec.hypothesis == "none":
        return x
    raise NotImplementedError(spec.hypothesis)


def unet_forward_levels(sd, spec, x, aux_levels, training=True):
    """(y_pred, aux_1, ..., aux_k) of DeepSupervisionUNet in training mode: R.unet_forward (oracle/torch_ref.py) with
    `aux_convs.{i-1}` applied to the output of up_blocks.{i}; the same operations in the same order for level 0"""
    skips = []
    x = R._r(x, spec)
    for i in range(spec.depth):
        x = R.block3d(sd, f"down_blocks.{i}", x, spec, training)
        if i != spec.depth - 1:
            skips.append(x)
            assert spec.down == "avgpool"
            x = R._r(F.avg_pool3d(x, 2, 2, count_include_pad=False), spec)
    aux = [None] * aux_levels
    for i in reversed(range(spec.depth - 1)):
        if spec.up == "trilinear":
            x = R._r(F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=True), spec)
        else:
            assert spec.up == "convT"
            w = sd[f"upsampling.{i}.weight"]
            if x[0, 0].numel() >= 16384 and w.shape[0] <= 128:
                w = R._r(w, spec)
            x = R._r(F.conv_transpose3d(x, w, sd.get(f"upsampling.{i}.bias"), stride=spec.up_stride,
                                        padding=spec.up_padding), spec)
        x = R.block3d(sd, f"up_blocks.{i}", torch.cat([x, skips[i]], dim=1), spec, training)
        if 1 <= i <= aux_levels:
            aux[i - 1] = _head(sd, f"aux_convs.{i - 1}", x, spec)
    return (_head(sd, "out_conv", x, spec), *aux)


def default_weights(n):
    total = sum(2.0 ** -i for i in range(n))
    return [2.0 ** -j / total for j in range(n)]


def weighted_loss(criterion, predictions, target, weights=None, mode="area"):
    """(total, [loss of level j]) -- w_0 l_0 + w_1 l_1 + ... left to right; `criterion` maps (p, t) to a dict with 'loss'"""
    k = len(predictions) - 1
    targets = [target] + pyramid(target, k, mode)
    weights = default_weights(k + 1) if weights is None else weights
    losses = [criterion(p, t)["loss"] for p, t in zip(predictions, targets)]
    total = None
    for w, l in zip(weights, losses):
        if w == 0.0:
            continue
        total = w * l if total is None else total + w * l
    return total, losses
