"""HybridFocalTverskyLoss in torch: the expected values of the focal Tversky tests.  The formulas run in the
dtype of their inputs -- fp64 for the expected values, fp32 for the "torch fp32 on the CPU" figures the tests print -- and
the gradients come from autograd; `closed_form_bwd` is the backward the kernels implement, written out.  Also the raw
C-ABI wrappers of the three entry points."""
import torch

from loss_ref_common import _chk, _dev, _per_channel, _stream
from raw_ops import _p
from segmentation_pipeline_amd import _lib

EPS = 1e-8
TINY = 1e-300


def _pow(base, exponent):
    """base ** exponent for base >= 0 with the conventions of the kernels: exponent 0 -> exactly 1, exponent 1 -> base"""
    if exponent == 0:
        return torch.ones_like(base)
    if exponent == 1:
        return base
    return base.pow(exponent)


def _probabilities(xs, from_logits):
    """(p, q, lp) of x [N, C, S]"""
    if from_logits:
        lp = torch.log_softmax(xs, dim=1)
        return torch.exp(lp), -torch.expm1(lp), lp
    return xs, 1 - xs, torch.log((xs + EPS) / (1 + EPS))


def focal_tversky(x, t, tversky_weight=0.5, alpha=0.5, beta=0.5, tversky_power=1.0, focal_gamma=0.0,
                  focal_class_weights=None, tversky_class_weights=None, from_logits=False):
    """-> {'loss', 'tversky_loss', 'focal_loss', 'sums' [N, C, 4], 'p'} for x, t of shape [N, C, *spatial]"""
    N, C_ = x.shape[:2]
    xs, ts = x.reshape(N, C_, -1), t.reshape(N, C_, -1)
    S = xs.shape[2]
    p, q, lp = _probabilities(xs, from_logits)
    w, v = _per_channel(focal_class_weights, C_, xs), _per_channel(tversky_class_weights, C_, xs)
    TP, FP, FN = (p * ts).sum(2), (p * (1 - ts)).sum(2), (q * ts).sum(2)
    F = (ts * _pow(q, focal_gamma) * lp).sum(2)
    TI = TP / (TP + alpha * FP + beta * FN + EPS / 2)
    u = (1 - TI).clamp_min(0)
    # u ** e with the gradient defined as 0 where u == 0 (e < 1: u ** (e - 1) is infinite there)
    term = torch.where(u > 0, _pow(u.clamp_min(TINY), tversky_power), torch.zeros_like(u))
    tversky_loss = (v[None] * term).mean()
    focal_loss = (-(w[None] * F / S)).mean()
    return {'loss': (1 - tversky_weight) * focal_loss + tversky_weight * tversky_loss, 'tversky_loss': tversky_loss,
            'focal_loss': focal_loss, 'sums': torch.stack([TP, FP, FN, F], dim=2), 'p': p}


def _run(x, t, dloss, dtype, cfg):
    xd = x.detach().to(dtype).requires_grad_(True)
    r = focal_tversky(xd, t.detach().to(dtype), **cfg)
    (r['loss'] * dloss).backward()
    out3 = torch.stack([r['loss'], r['tversky_loss'], r['focal_loss']]).detach()
    return out3, r['sums'].detach().flatten(), xd.grad


def expected(x, t, dloss, **cfg):
    """fp64: (out3 [3], sums [N*C*4], dx like x for the upstream gradient `dloss` of 'loss')"""
    return _run(x, t, dloss, torch.float64, cfg)


def torch32(x, t, dloss, **cfg):
    """the same in fp32 on the CPU"""
    return _run(x, t, dloss, torch.float32, cfg)


def closed_form_bwd(x, t, dloss, tversky_weight=0.5, alpha=0.5, beta=0.5, tversky_power=1.0, focal_gamma=0.0,
                    focal_class_weights=None, tversky_class_weights=None, from_logits=False):
    """dx from the four saved sums, as the backward kernels form it (in the dtype of x)"""
    N, C_ = x.shape[:2]
    xs, ts = x.reshape(N, C_, -1), t.reshape(N, C_, -1)
    S = xs.shape[2]
    lam, e, gam = tversky_weight, tversky_power, focal_gamma
    p, q, lp = _probabilities(xs, from_logits)
    w, v = _per_channel(focal_class_weights, C_, xs)[None, :, None], _per_channel(tversky_class_weights, C_, xs)[None, :, None]
    TP, FP, FN = ((p * ts).sum(2, keepdim=True), (p * (1 - ts)).sum(2, keepdim=True), (q * ts).sum(2, keepdim=True))
    D = TP + alpha * FP + beta * FN + EPS / 2
    u = (1 - TP / D).clamp_min(0)
    du = torch.where(u > 0, e * _pow(u.clamp_min(TINY), e - 1) if e != 1 else torch.ones_like(u), torch.zeros_like(u))
    dTI = (ts * D - TP * (ts + alpha * (1 - ts) - beta * ts)) / D ** 2
    h = -lam / (N * C_) * v * du * dTI
    qg = _pow(q, gam)
    gq = gam * _pow(q, gam - 1) if gam != 0 else torch.zeros_like(q)
    kf = -(1 - lam) / (N * C_ * S) * w * ts
    if from_logits:
        g = kf * (qg - gq * p * lp)
        dx = g - p * g.sum(1, keepdim=True) + p * (h - (p * h).sum(1, keepdim=True))
    else:
        dx = h + kf * (qg / (p + EPS) - gq * lp)
    return (dloss * dx).reshape(x.shape)


# ---------------------------------------------------------------------------------------------- raw entry points
def raw_fwd(x, t, tversky_weight=0.5, alpha=0.5, beta=0.5, tversky_power=1.0, focal_gamma=0.0, focal_class_weights=None,
            tversky_class_weights=None, from_logits=False):
    """m355_focal_tversky_fwd on device tensors (x, t: any views whose rows are dense) -> (out3, sums)"""
    L = _lib.lib()
    N, C_ = x.shape[:2]
    S = x.numel() // (N * C_)
    fw, tw = _dev(focal_class_weights), _dev(tversky_class_weights)
    out3 = torch.empty(3, device="cuda")
    sums = torch.empty(N * C_ * 4, device="cuda")
    ws = torch.empty(max(int(L.m355_focal_tversky_workspace(N, C_, S)), 16), dtype=torch.uint8, device="cuda")
    _chk(L.m355_focal_tversky_fwd(_p(x), _p(t), N, C_, S, tversky_weight, alpha, beta, tversky_power, focal_gamma, _p(fw),
                                  _p(tw), int(from_logits), _p(out3), _p(sums), _p(ws), ws.numel(), _stream()),
         "focal_tversky_fwd")
    return out3, sums


def raw_bwd(x, t, sums, dloss, tversky_weight=0.5, alpha=0.5, beta=0.5, tversky_power=1.0, focal_gamma=0.0,
            focal_class_weights=None, tversky_class_weights=None, from_logits=False, out=None):
    L = _lib.lib()
    N, C_ = x.shape[:2]
    S = x.numel() // (N * C_)
    fw, tw = _dev(focal_class_weights), _dev(tversky_class_weights)
    g = torch.tensor([dloss], dtype=torch.float32, device="cuda")
    dx = torch.empty(x.shape, device="cuda") if out is None else out
    _chk(L.m355_focal_tversky_bwd(_p(x), _p(t), _p(sums), _p(g), N, C_, S, tversky_weight, alpha, beta, tversky_power,
                                  focal_gamma, _p(fw), _p(tw), int(from_logits), _p(dx), _stream()), "focal_tversky_bwd")
    return dx
