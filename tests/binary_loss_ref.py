"""HybridBinaryLogisticDiceLoss in torch: the expected values of the binary-loss tests.  The formulas run in
the dtype of their inputs -- fp64 for the expected values, fp32 for the "torch fp32 on the CPU" figures the tests print --
and the gradients come from autograd.  Also the raw C-ABI wrappers of the three entry points."""
import torch

from loss_ref_common import _chk, _dev, _per_channel, _stream
from raw_ops import _p
from segmentation_pipeline_amd import _lib

EPS = 1e-8


def binary_loss(x, t, dice_weight=0.5, class_weights=None, pos_weight=None, square_dice=True, from_logits=False):
    """-> {'loss', 'dice_loss', 'logistic_loss', 'sums' [N, C, 5], 'p'} for x, t of shape [N, C, *spatial]"""
    N, C_ = x.shape[:2]
    xs, ts = x.reshape(N, C_, -1), t.reshape(N, C_, -1)
    S = xs.shape[2]
    if from_logits:
        p = torch.sigmoid(xs)
        # softplus(v) = max(v, 0) + log1p(exp(-|v|)).  torch's own op, for its derivative sigmoid(v) at v == 0 (autograd
        # through max and abs gives 0 there); it evaluates log1p(exp(v)) up to `threshold` and v beyond, where the two
        # differ by less than exp(-threshold): exact to fp64 at 700 / 1.4e-9 relative in fp32 at torch's default 20
        thr = 700.0 if xs.dtype == torch.float64 else 20.0
        lp = -torch.nn.functional.softplus(-xs, threshold=thr)
        lq = -torch.nn.functional.softplus(xs, threshold=thr)
    else:
        p = xs
        q = 1 - p
        lp = torch.log((p + EPS) / (1 + EPS))
        lq = torch.log((q + EPS) / (1 + EPS))
    cw, pw = _per_channel(class_weights, C_, xs), _per_channel(pos_weight, C_, xs)
    overlap = (p * ts).sum(2)
    sp, st = ((p * p).sum(2), (ts * ts).sum(2)) if square_dice else (p.sum(2), ts.sum(2))
    tlp, tlq = (ts * lp).sum(2), ((1 - ts) * lq).sum(2)
    dice = 2 * overlap / (sp + st + EPS)
    logistic = cw[None] * (pw[None] * tlp + tlq) / S
    logistic_loss, dice_loss = (-logistic).mean(), (1 - dice).mean()
    return {'loss': (1 - dice_weight) * logistic_loss + dice_weight * dice_loss, 'dice_loss': dice_loss,
            'logistic_loss': logistic_loss, 'sums': torch.stack([overlap, sp, st, tlp, tlq], dim=2), 'p': p}


def expected(x, t, dloss, **cfg):
    """fp64: (out3 [3], sums [N*C*5], dx like x for the upstream gradient `dloss` of 'loss')"""
    xd = x.detach().double().requires_grad_(True)
    r = binary_loss(xd, t.detach().double(), **cfg)
    (r['loss'] * dloss).backward()
    out3 = torch.stack([r['loss'], r['dice_loss'], r['logistic_loss']]).detach()
    return out3, r['sums'].detach().flatten(), xd.grad


def torch32(x, t, dloss, **cfg):
    """the same in fp32 on the CPU"""
    xf = x.detach().float().requires_grad_(True)
    r = binary_loss(xf, t.detach().float(), **cfg)
    (r['loss'] * dloss).backward()
    return torch.stack([r['loss'], r['dice_loss'], r['logistic_loss']]).detach(), r['sums'].detach().flatten(), xf.grad


# ---------------------------------------------------------------------------------------------- raw entry points
def raw_fwd(x, t, dice_weight=0.5, class_weights=None, pos_weight=None, square_dice=True, from_logits=False):
    """m355_binary_loss_fwd on device tensors (x, t: any views whose rows are dense) -> (out3, sums)"""
    L = _lib.lib()
    N, C_ = x.shape[:2]
    S = x.numel() // (N * C_)
    cw, pw = _dev(class_weights), _dev(pos_weight)
    out3 = torch.empty(3, device="cuda")
    sums = torch.empty(N * C_ * 5, device="cuda")
    ws = torch.empty(max(int(L.m355_binary_loss_workspace(N, C_, S)), 16), dtype=torch.uint8, device="cuda")
    _chk(L.m355_binary_loss_fwd(_p(x), _p(t), N, C_, S, dice_weight, _p(cw), _p(pw), int(square_dice), int(from_logits),
                                _p(out3), _p(sums), _p(ws), ws.numel(), _stream()), "binary_loss_fwd")
    return out3, sums


def raw_bwd(x, t, sums, dloss, dice_weight=0.5, class_weights=None, pos_weight=None, square_dice=True, from_logits=False,
            out=None):
    L = _lib.lib()
    N, C_ = x.shape[:2]
    S = x.numel() // (N * C_)
    cw, pw = _dev(class_weights), _dev(pos_weight)
    g = torch.tensor([dloss], dtype=torch.float32, device="cuda")
    dx = torch.empty(x.shape, device="cuda") if out is None else out
    _chk(L.m355_binary_loss_bwd(_p(x), _p(t), _p(sums), _p(g), N, C_, S, dice_weight, _p(cw), _p(pw), int(square_dice),
                                int(from_logits), _p(dx), _stream()), "binary_loss_bwd")
    return dx
