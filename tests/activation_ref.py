"""TEST HELPER -- the smooth activations Block3d executes through the fused normalisation passes (csrc/activation.hpp:
nn.ELU, nn.GELU in both approximations, nn.SiLU), as stock torch on the CPU: the nn module itself under autograd, in fp64 for
the kernel tests (the C oracle does not know these codes) and in the model's own fp32 for a CPU restatement of
ModularUNet.forward with the activation as a module, composed the way tests/upsample_ref.py composes its forward."""
import torch
import torch.nn.functional as F
from torch import nn

from oracle import torch_ref as R

# name -> (M355_ACT_* code, activation_class, activation_params, the parameter the descriptor carries in act_slope)
ACTS = {
    "elu": (3, nn.ELU, {'alpha': 0.7}, 0.7),          # (alpha != 1: a dropped parameter shows)
    "gelu": (4, nn.GELU, {}, 0.0),
    "gelu_tanh": (5, nn.GELU, {'approximate': 'tanh'}, 0.0),
    "silu": (6, nn.SiLU, {}, 0.0),
}
# pre-activation values planted in the activation-only descriptor: both ends of every libm call
PLANTED = [0.0, 1e-6, -1e-6, 1e-3, -1e-3, 0.5, -0.5, 3.0, -3.0, 9.0, -9.0, 20.0, -20.0, 90.0, -90.0, -104.0]


def module(name):
    _, cls, params, _ = ACTS[name]
    return cls(**params)


def statistics(x, groups, eps):
    """(mean, rstd) of the descriptor's statistics in x's precision: per channel over (N, voxels) for groups == 0, else per
    (n, group); biased variance"""
    N, Cc = x.shape[:2]
    v = x.transpose(0, 1).reshape(Cc, -1) if groups == 0 else x.reshape(N * groups, -1)
    return v.mean(dim=1), (v.var(dim=1, unbiased=False) + eps).rsqrt()


def _per_element(stat, x, groups):
    N, Cc = x.shape[:2]
    if groups == 0:
        return stat.view(1, Cc, 1, 1, 1)
    return stat.view(N, groups, 1).expand(N, groups, Cc // groups).reshape(N, Cc, 1, 1, 1)


def norm_act(x, mean, rstd, gamma, beta, groups, act, add=None):
    """y = act((x - mean) * rstd * gamma + beta) (+ add): `act` an nn module, mean / rstd as statistics() returns them --
    inside the autograd graph for a training-mode backward, detached for an eval-mode one"""
    y = (x - _per_element(mean, x, groups)) * _per_element(rstd, x, groups)
    if gamma is not None:
        y = y * gamma.view(1, -1, 1, 1, 1) + beta.view(1, -1, 1, 1, 1)
    y = act(y)
    return y if add is None else y + add


def _stat_mean(v, groups):
    """mean of v over each statistic's elements, per element"""
    N, Cc = v.shape[:2]
    m = (v.transpose(0, 1).reshape(Cc, -1) if groups == 0 else v.reshape(N * groups, -1)).mean(dim=1)
    return _per_element(m, v, groups)


def norm_bwd_as_defined(x, dy, mean, rstd, gamma, beta, groups, act):
    """the training-mode backward as include/m355seg.h defines it for statistics handed in as numbers (they need not be
    those of x): g = dy f'(pre) -- f' from the module's autograd --, dx = rstd (g gamma - mean_s(g gamma) - xhat
    mean_s(g gamma xhat)), dgamma = sum g xhat, dbeta = sum g.  With the true statistics this is autograd's result."""
    xh = (x - _per_element(mean, x, groups)) * _per_element(rstd, x, groups)
    ga = torch.ones(x.shape[1], dtype=x.dtype) if gamma is None else gamma
    be = torch.zeros(x.shape[1], dtype=x.dtype) if beta is None else beta
    pre = (xh * ga.view(1, -1, 1, 1, 1) + be.view(1, -1, 1, 1, 1)).detach().requires_grad_(True)
    g = torch.autograd.grad(act(pre), pre, dy)[0]
    gg = g * ga.view(1, -1, 1, 1, 1)
    dx = _per_element(rstd, x, groups) * (gg - _stat_mean(gg, groups) - xh * _stat_mean(gg * xh, groups))
    return dx, (g * xh).sum(dim=(0, 2, 3, 4)), g.sum(dim=(0, 2, 3, 4))


def norm_act_fwd_bwd(x, dy, gamma, beta, groups, eps, act, training=True, add=None, given_stats=None, dtype=torch.float64):
    """forward and backward of one fused pass in `dtype` on the CPU -> dict(mean, rstd, y, dx, dgamma, dbeta); the inputs are
    taken as they are (already rounded where the kernel under test reads 16-bit values).  The backward is the nn module
    under autograd: through the statistics of x in training mode, with the statistics as constants in eval mode.
    given_stats = (mean, rstd): numbers handed to the kernel in place of x's statistics (the activation-only descriptor:
    mean 0, rstd 1); a training-mode backward on them is norm_bwd_as_defined."""
    x = x.to(dtype).clone().requires_grad_(True)
    dy = dy.to(dtype)
    g = None if gamma is None else gamma.to(dtype).clone().requires_grad_(True)
    b = None if beta is None else beta.to(dtype).clone().requires_grad_(True)
    mean, rstd = statistics(x, groups, eps) if given_stats is None else (t.to(dtype) for t in given_stats)
    if not training or given_stats is not None:
        mean, rstd = mean.detach(), rstd.detach()
    y = norm_act(x, mean, rstd, g, b, groups, act, None if add is None else add.to(dtype))
    if training and given_stats is not None:
        dx, dg, db = norm_bwd_as_defined(x.detach(), dy, mean, rstd, gamma if g is None else g.detach(),
                                         beta if b is None else b.detach(), groups, act)
        if g is None:
            dg = db = None
    else:
        grads = torch.autograd.grad(y, [x] + ([g, b] if g is not None else []), dy)
        dx, dg, db = grads[0], (grads[1] if g is not None else None), (grads[2] if g is not None else None)
    return dict(mean=mean.detach(), rstd=rstd.detach(), y=y.detach(), dx=dx, dgamma=dg, dbeta=db)


def block3d(sd, prefix, x, spec: R.UNetSpec, act, training):
    """oracle.torch_ref.block3d (fp32 arithmetic) with the activation as an nn module; BatchNorm updates the running
    statistics in `sd` in place, as the module does"""
    x_in = x
    for j in range(spec.num_convs):
        x = F.conv3d(x, sd[f"{prefix}.layers.conv{j}.weight"], sd.get(f"{prefix}.layers.conv{j}.bias"), padding=1)
        key = f"{prefix}.layers.norm{j}"
        if spec.norm == "batch":
            x = F.batch_norm(x, sd[key + ".running_mean"], sd[key + ".running_var"], sd[key + ".weight"], sd[key + ".bias"],
                             training, spec.momentum, spec.eps)
        elif spec.norm == "group":
            x = F.group_norm(x, spec.groups, sd[key + ".weight"], sd[key + ".bias"], spec.eps)
        x = act(x)
    if spec.residual:
        x = F.conv3d(x_in, sd[f"{prefix}.res_conv.weight"], sd[f"{prefix}.res_conv.bias"], padding=1) + x
    return x


def unet_forward_act(sd, spec: R.UNetSpec, x, act, training=True):
    """models/modular_unet.py:86-102 with the default average pool and align_corners=True trilinear upsampling and
    `act` (an nn module) inside every block; `spec` describes the blocks (its `act` field is not read)."""
    skips = []
    for i in range(spec.depth):
        x = block3d(sd, f"down_blocks.{i}", x, spec, act, training)
        if i != spec.depth - 1:
            skips.append(x)
            x = F.avg_pool3d(x, 2, 2)
    for i in reversed(range(spec.depth - 1)):
        x = F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=True)
        x = block3d(sd, f"up_blocks.{i}", torch.cat([x, skips[i]], dim=1), spec, act, training)
    x = F.conv3d(x, sd["out_conv.weight"], sd["out_conv.bias"], padding=1)
    return torch.softmax(x, dim=1)
