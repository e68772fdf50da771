"""HybridTopKDiceLoss in torch: the expected values of the top-k tests.  The formulas run in the dtype of
their inputs -- fp64 for the expected values, fp32 for the "torch fp32 on the CPU" figures the tests print -- and the
gradients come from autograd; `closed_form_bwd` is the backward the kernels implement, written out.  Ties at the
threshold are shared: a voxel's selection weight is 1 above the k-th largest value tau, (k - n_gt) / n_eq on it, 0 below.
Also the inputs with a guaranteed margin between the k-th and the (k + 1)-th largest value, without which a comparison
of gradients would compare different selections, and the raw C-ABI wrappers of the entry points."""
import torch

from loss_ref_common import _chk, _dev, _per_channel, _stream
from raw_ops import _p
from segmentation_pipeline_amd import _lib, ops

EPS = 1e-8
MARGIN = 1e-4

# name -> shape.  small: S = 990, a multiple of neither 4 nor 256, less than one chunk, N = 2 (the batch-wide selection
# crosses samples); large: S = 17391, odd (every second row misaligned), a ragged last chunk; c17: one channel more than
# the register variants hold
CASES = {"small": (2, 3, 9, 10, 11), "large": (1, 2, 17, 33, 31), "c17": (1, 17, 5, 6, 7)}


def probabilities(xs, from_logits):
    """(p, lp) of x [N, C, S]"""
    if from_logits:
        lp = torch.log_softmax(xs, dim=1)
        return torch.exp(lp), lp
    return xs, torch.log((xs + EPS) / (1 + EPS))


def voxel_ce(x, t, class_weights=None, from_logits=False):
    """e [N, S] = -sum_c w_c t lp, and p [N, C, S]"""
    N, C_ = x.shape[:2]
    xs, ts = x.reshape(N, C_, -1), t.reshape(N, C_, -1)
    p, lp = probabilities(xs, from_logits)
    w = _per_channel(class_weights, C_, xs)
    return -(w[None, :, None] * ts * lp).sum(1), p


def select(e, k):
    """(tau, n_gt, n_eq, sel like e) of the k largest entries of e with shared ties; sum(sel) == k"""
    flat = e.detach().flatten()
    tau = torch.topk(flat, k).values[-1]
    gt, eq = e.detach() > tau, e.detach() == tau
    n_gt, n_eq = int(gt.sum()), int(eq.sum())
    r = (k - n_gt) / n_eq
    return tau, n_gt, n_eq, gt.to(e.dtype) + r * eq.to(e.dtype)


def topk_dice(x, t, top_k=None, k=None, dice_weight=0.5, class_weights=None, square_dice=True, from_logits=False):
    """-> {'loss', 'dice_loss', 'logistic_loss', 'sums' [N, C, 3], 'e' [N, S], 'threshold', 'sel' [N, S], 'k'} for x, t of
    shape [N, C, *spatial]; top_k: the fraction, or k: the count itself"""
    N, C_ = x.shape[:2]
    ts = t.reshape(N, C_, -1)
    S = ts.shape[2]
    if k is None:
        k = ops.topk_count(N, S, top_k)
    e, p = voxel_ce(x, t, class_weights, from_logits)
    tau, _, _, sel = select(e, k)
    logistic_loss = torch.where(sel > 0, sel * e, torch.zeros_like(e)).sum() / (C_ * k)
    overlap = (p * ts).sum(2)
    sp, st = ((p * p).sum(2), (ts * ts).sum(2)) if square_dice else (p.sum(2), ts.sum(2))
    dice_loss = (1 - 2 * overlap / (sp + st + EPS)).mean()
    return {'loss': (1 - dice_weight) * logistic_loss + dice_weight * dice_loss, 'dice_loss': dice_loss,
            'logistic_loss': logistic_loss, 'sums': torch.stack([overlap, sp, st], dim=2), 'e': e, 'threshold': tau,
            'sel': sel, 'k': k}


def margin(e, k):
    """the gap between the k-th and the (k + 1)-th largest entry of e (inf for k == numel)"""
    flat = e.detach().flatten()
    if k >= flat.numel():
        return float("inf")
    top = torch.topk(flat, k + 1).values
    return (top[k - 1] - top[k]).item()


def _run(x, t, dloss, dtype, cfg):
    xd = x.detach().to(dtype).requires_grad_(True)
    r = topk_dice(xd, t.detach().to(dtype), **cfg)
    (r['loss'] * dloss).backward()
    out3 = torch.stack([r['loss'], r['dice_loss'], r['logistic_loss']]).detach()
    return {'out3': out3, 'sums': r['sums'].detach().flatten(), 'dx': xd.grad, 'e': r['e'].detach(), 'sel': r['sel'],
            'threshold': r['threshold'], 'k': r['k']}


def expected(x, t, dloss, **cfg):
    """fp64: out3 [3], sums [N*C*3], dx like x for the upstream gradient `dloss` of 'loss', e, sel, threshold, k.  The gap
    below the k-th largest e must be at least MARGIN, in fp64 and in torch's fp32: otherwise fp32 and fp64 need not select
    the same voxels and their gradients are not comparable."""
    r = _run(x, t, dloss, torch.float64, cfg)
    e32, _ = voxel_ce(x.float(), t.float(), cfg.get('class_weights'), cfg.get('from_logits', False))
    for what, e in (("fp64", r['e']), ("fp32", e32)):
        gap = margin(e, r['k'])
        assert gap >= MARGIN, f"the gap below the k-th largest value is {gap:.3e} in {what}: no margin for a comparison"
    r['threshold32'] = torch.topk(e32.flatten(), r['k']).values[-1]
    return r


def torch32(x, t, dloss, **cfg):
    """the same in fp32 on the CPU (no margin check: the figures are printed, not asserted)"""
    return _run(x, t, dloss, torch.float32, cfg)


def closed_form_bwd(x, t, dloss, top_k=None, k=None, dice_weight=0.5, class_weights=None, square_dice=True,
                    from_logits=False):
    """dx as the backward kernels form it (in the dtype of x): from the Dice sums, tau, r and k"""
    N, C_ = x.shape[:2]
    xs, ts = x.reshape(N, C_, -1), t.reshape(N, C_, -1)
    S = xs.shape[2]
    if k is None:
        k = ops.topk_count(N, S, top_k)
    e, p = voxel_ce(x, t, class_weights, from_logits)
    _, _, _, sel = select(e, k)
    w = _per_channel(class_weights, C_, xs)[None, :, None]
    O = (p * ts).sum(2, keepdim=True)
    T = ((p * p).sum(2, keepdim=True) + (ts * ts).sum(2, keepdim=True) if square_dice
         else p.sum(2, keepdim=True) + ts.sum(2, keepdim=True)) + EPS
    dT = 2 * p if square_dice else torch.ones_like(p)
    h = -dice_weight / (N * C_) * (2 * ts / T - 2 * O * dT / T ** 2)
    kl = (1 - dice_weight) * sel[:, None, :] / (C_ * k)
    if from_logits:
        dx = p * (h - (p * h).sum(1, keepdim=True) + kl * (w * ts).sum(1, keepdim=True)) - kl * w * ts
    else:
        dx = h - kl * w * ts / (xs + EPS)
    return (dloss * dx).reshape(x.shape)


# ------------------------------------------------------------------------------------------------ inputs with a margin
def margin_inputs(case):
    """(z, p, t) on the host, fp32: the per-voxel cross-entropies are linspace(0.05, 6, N * S) in a seeded order, so two
    neighbours in the sorted order differ by at least 5.95 / (N * S) whatever k is.  Hard random labels, p_true =
    exp(-e), the rest of the mass spread over the other channels in proportion to rand + 0.1; z = log p."""
    shape = CASES[case]
    N, C_ = shape[:2]
    S = 1
    for d in shape[2:]:
        S *= d
    g = torch.Generator().manual_seed(sorted(CASES).index(case) + 11)
    M = N * S
    e = torch.linspace(0.05, 6, M, dtype=torch.float64)[torch.randperm(M, generator=g)].reshape(N, 1, S)
    lab = torch.randint(0, C_, (N, 1, S), generator=g)
    t = torch.zeros(N, C_, S, dtype=torch.float64).scatter_(1, lab, 1.0)
    p_true = torch.exp(-e)
    rest = (torch.rand((N, C_, S), generator=g, dtype=torch.float64) + 0.1) * (1 - t)
    p = t * p_true + rest / rest.sum(1, keepdim=True) * (1 - p_true)
    return torch.log(p).float().reshape(shape), p.float().reshape(shape), t.float().reshape(shape)


# ---------------------------------------------------------------------------------------------- raw entry points
def raw_fwd(x, t, top_k=None, k=None, k_device=None, dice_weight=0.5, class_weights=None, square_dice=True,
            from_logits=False, e=None, ws=None):
    """m355_topk_loss_fwd on device tensors (x, t: any views whose rows are dense) -> (out3, sums, e, state [4 words]);
    e and ws: buffers of the caller's (the canary tests)"""
    L = _lib.lib()
    N, C_ = x.shape[:2]
    S = x.numel() // (N * C_)
    if k is None and k_device is None:
        k = ops.topk_count(N, S, top_k)
    cw = _dev(class_weights)
    out3 = torch.empty(3, device="cuda")
    sums = torch.empty(N * C_ * 3, device="cuda")
    state = torch.empty(4, device="cuda")
    if e is None:
        e = torch.empty(N * S, device="cuda")
    if ws is None:
        ws = torch.empty(max(int(L.m355_topk_loss_workspace(N, C_, S)), 16), dtype=torch.uint8, device="cuda")
    _chk(L.m355_topk_loss_fwd(_p(x), _p(t), N, C_, S, 0 if k is None else int(k), _p(k_device), dice_weight, _p(cw),
                              int(square_dice), int(from_logits), _p(out3), _p(sums), _p(e), _p(state), _p(ws), ws.numel(),
                              _stream()), "topk_loss_fwd")
    return out3, sums, e, state


def raw_bwd(x, t, e, sums, state, dloss, dice_weight=0.5, class_weights=None, square_dice=True, from_logits=False,
            out=None, **_):
    L = _lib.lib()
    N, C_ = x.shape[:2]
    S = x.numel() // (N * C_)
    cw = _dev(class_weights)
    g = torch.tensor([dloss], dtype=torch.float32, device="cuda")
    dx = torch.empty(x.shape, device="cuda") if out is None else out
    _chk(L.m355_topk_loss_bwd(_p(x), _p(t), _p(e), _p(sums), _p(state), _p(g), N, C_, S, dice_weight, _p(cw),
                              int(square_dice), int(from_logits), _p(dx), _stream()), "topk_loss_bwd")
    return dx


def state_fields(state):
    """(tau, r, k) of the saved state"""
    words = state.cpu().view(torch.int32)
    return state[0].item(), state[1].item(), (int(words[3]) << 32) | (int(words[2]) & 0xffffffff)
