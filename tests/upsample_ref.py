"""TEST HELPER -- CPU formulations of nn.Upsample(scale_factor=2) in the three conventions ModularUNet executes
(stock F.interpolate, fp32 and fp64), the error scales the kernel tests bound against, and a CPU restatement of
ModularUNet.forward that takes the upsampling mode, composed from oracle.torch_ref.block3d the way
tests/maxpool_ref.py composes its max-pool forward."""
import torch
import torch.nn.functional as F

from oracle import torch_ref as R

# mode name (ops / _lib.UPSAMPLE2X_MODES) -> F.interpolate keywords
INTERPOLATE = {
    "nearest": dict(mode="nearest"),
    "trilinear_hp": dict(mode="trilinear", align_corners=False),
    "trilinear": dict(mode="trilinear", align_corners=True),
}


def upsample(x, mode):
    """stock torch on the CPU in x's own precision"""
    return F.interpolate(x, scale_factor=2, **INTERPOLATE[mode])


def upsample_grad(dy, mode, in_shape):
    """torch autograd's gradient of upsample() in dy's precision"""
    x = torch.zeros(in_shape, dtype=dy.dtype, requires_grad=True)
    return torch.autograd.grad(upsample(x, mode), x, dy)[0]


def neighbourhood_max(x):
    """per OUTPUT voxel of the 2x tensor: max |x| over the clamped 3x3x3 neighbourhood of its input voxel"""
    a = x.abs()
    a = F.max_pool3d(F.pad(a, (1, 1, 1, 1, 1, 1), mode="replicate"), 3, 1)
    return F.interpolate(a, scale_factor=2, mode="nearest")


def ill_conditioned(shape, seed, dtype=torch.float32):
    """randn * exp(3 * randn): magnitudes over several decades, both signs"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64)
            * torch.exp(3 * torch.randn(shape, generator=g, dtype=torch.float64))).to(dtype)


def unet_forward_upsample(sd, spec: R.UNetSpec, x, mode: str, training: bool = True):
    """models/modular_unet.py:86-102 with the default average pool and nn.Upsample(scale_factor=2, **INTERPOLATE[mode])
    between the decoder blocks; `spec` describes the blocks (its `down` / `up` fields are not read)."""
    skips = []
    for i in range(spec.depth):
        x = R.block3d(sd, f"down_blocks.{i}", x, spec, training)
        if i != spec.depth - 1:
            skips.append(x)
            x = F.avg_pool3d(x, 2, 2)
    for i in reversed(range(spec.depth - 1)):
        x = upsample(x, mode)
        x = R.block3d(sd, f"up_blocks.{i}", torch.cat([x, skips[i]], dim=1), spec, training)
    x = F.conv3d(x, sd["out_conv.weight"], sd["out_conv.bias"], padding=1)
    return torch.softmax(x, dim=1)
