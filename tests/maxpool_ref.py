"""TEST HELPER -- CPU restatement of ModularUNet.forward with downsample_class=nn.MaxPool3d(2, 2), composed from
oracle.torch_ref.block3d and stock torch functions (oracle/torch_ref.unet_forward knows the average pool and the blur
convolution only), plus the route arithmetic the kernel tests share."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_ref as R


def unet_forward_maxpool(sd, spec: R.UNetSpec, x, training: bool = True):
    """models/modular_unet.py:86-102 with nn.MaxPool3d(kernel_size=2, stride=2) between the encoder blocks and the
    default trilinear upsampling; `spec` describes the blocks (its `down` / `up` fields are not read)."""
    skips = []
    for i in range(spec.depth):
        x = R.block3d(sd, f"down_blocks.{i}", x, spec, training)
        if i != spec.depth - 1:
            skips.append(x)
            x = F.max_pool3d(x, 2, 2)
    for i in reversed(range(spec.depth - 1)):
        x = F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=True)
        x = R.block3d(sd, f"up_blocks.{i}", torch.cat([x, skips[i]], dim=1), spec, training)
    x = F.conv3d(x, sd["out_conv.weight"], sd["out_conv.bias"], padding=1)
    return torch.softmax(x, dim=1)


def window_position(indices, H, W):
    """torch's return_indices (flat offsets into D*H*W of each (n, c) volume) reduced to the position inside the
    2x2x2 window, 0..7 = (dd * 2 + dh) * 2 + dw -- the route byte of m355_maxpool3d_2x_fwd"""
    iz, iy, ix = indices // (H * W), (indices // W) % H, indices % W
    return (((iz & 1) * 2 + (iy & 1)) * 2 + (ix & 1)).to(torch.uint8)


NAN, INF = float("nan"), float("inf")
# 2x2x2 windows in scan order (d, h, w) with the route torch takes
PLANTED = [
    ([1.0, NAN, 0.0, 2.0, NAN, -1.0, 0.0, 1.0], 4),          # two NaNs: the LAST one
    ([NAN, 1.0, 2.0, 2.0, 0.0, 1.0, 2.0, -2.0], 0),          # NaN first, larger values behind it: still the NaN
    ([-INF] * 8, 0),                                         # all -inf: element 0
    ([-0.0, 0.0, -0.0, 0.0, -1.0, -2.0, -0.0, 0.0], 0),      # -0.0 first: -0.0 comes out
    ([0.0, -0.0, 0.0, -0.0, -1.0, -0.0, -2.0, 0.0], 0),      # +0.0 first: +0.0 comes out
]


def tie_heavy_input(shape, seed):
    """integers in [-2, 2] as float32 (about two thirds of the windows hold a tie for the maximum) with the PLANTED
    windows written into it, spread over the pooled grid; -> (x, [(n, c, oz, oy, ox, route)])"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, shape, generator=g).float()
    N, C, D, H, W = shape
    grid = (N, C, D // 2, H // 2, W // 2)
    nwin = N * C * (D // 2) * (H // 2) * (W // 2)
    step = max(1, nwin // len(PLANTED))
    planted = {}
    for i, (vals, route) in enumerate(PLANTED):
        wid = (i * step + i) % nwin
        n, c, oz, oy, ox = [int(v) for v in np.unravel_index(wid, grid)]
        x[n, c, 2 * oz:2 * oz + 2, 2 * oy:2 * oy + 2, 2 * ox:2 * ox + 2] = torch.tensor(vals).view(2, 2, 2)
        planted[(n, c, oz, oy, ox)] = route       # (a later window may overwrite an earlier one in the tiniest shape)
    return x, [k + (r,) for k, r in planted.items()]
