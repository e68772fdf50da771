"""The Lovasz-softmax loss in torch: the expected values of the Lovasz tests.

`berman` is the formula of Berman et al. (CVPR 2018) -- sort the errors, dot them with the increments of the Jaccard loss
-- in the dtype of its inputs, with autograd: fp64 for the checks of the definition, fp32 for the "torch fp32 on the CPU"
figures the tests print.  `closed_form` is what the kernels implement: e = |fg - p| taken in fp32 exactly as the device
takes it, grouped by that fp32 value, and everything after that in int64 / fp64: a group [lo, hi) of equal errors
contributes e (J(hi) - J(lo)) to its segment's loss and gives each member dL/de = (J(hi) - J(lo)) / (hi - lo).  `reduce`
is the presence / weight / per-image reduction both share.  Also the input builders and the raw C-ABI wrappers of the
entry points; the wrappers allocate through a tests/raw_ops.py RawOps, so they run under its scratch() modes."""
import torch

from loss_ref_common import _chk, _dev, _stream
from raw_ops import _p
from segmentation_pipeline_amd import _lib

CLASSES = ("present", "all")


def sort_tile():
    return int(_lib.lib().m355_segmented_sort_tile())


def loss_tile():
    return int(_lib.lib().m355_lovasz_loss_tile())


# ------------------------------------------------------------------------------------------------------------ segments
def segments(x, per_image):
    """x [N, C, *spatial] -> [R, M]: per_image: (n, c) rows of S; else channel rows of N * S, sample after sample"""
    N, C_ = x.shape[:2]
    xs = x.reshape(N, C_, -1)
    return xs.reshape(N * C_, -1) if per_image else xs.transpose(0, 1).reshape(C_, -1)


def unsegment(v, shape, per_image):
    """the inverse of `segments` for a [R, M] tensor"""
    N, C_ = shape[:2]
    if per_image:
        return v.reshape(shape)
    return v.reshape(C_, N, -1).transpose(0, 1).reshape(shape)


def reduce(L, G, classes, per_image, class_weights, N, C_):
    """-> (loss, coef [R], segments averaged): loss = sum_r coef_r L_r.  L [R] (any float dtype, may carry autograd), G [R]
    the foreground counts.  Per image (the whole batch is one image without per_image) the weighted mean of the segments
    that take part, 0 for an image without one; then the mean over the images."""
    images = N if per_image else 1
    w = torch.ones(C_, dtype=L.dtype) if class_weights is None else torch.as_tensor(class_weights, dtype=L.dtype)
    part = torch.ones(images, C_, dtype=L.dtype) if classes == "all" else (G.reshape(images, C_) > 0).to(L.dtype)
    wp = part * w[None, :]
    den = wp.sum(1, keepdim=True)
    coef = torch.where(den > 0, wp / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(wp)) / images
    coef = coef.reshape(-1)
    return (coef * L).sum(), coef, int((wp != 0).sum())


# -------------------------------------------------------------------------------------------------------------- Berman
def lovasz_grad(fg_sorted):
    """the increments of the Jaccard loss along the sorted order (Berman's Alg. 1)"""
    gts = fg_sorted.sum()
    intersection = gts - fg_sorted.cumsum(0)
    union = gts + (1 - fg_sorted).cumsum(0)
    jaccard = 1 - intersection / union
    return torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])


def berman(p, t, classes='present', per_image=False, class_weights=None):
    """the loss, with autograd through p, in p's dtype"""
    N, C_ = p.shape[:2]
    ps, fgs = segments(p, per_image), (segments(t, per_image) >= 0.5).to(p.dtype)
    losses = []
    for r in range(ps.shape[0]):
        errors = (fgs[r] - ps[r]).abs()
        order = torch.sort(errors.detach(), descending=True, stable=True).indices
        losses.append(torch.dot(errors[order], lovasz_grad(fgs[r][order])))
    return reduce(torch.stack(losses), fgs.sum(1), classes, per_image, class_weights, N, C_)[0]


def berman_run(p, t, dloss, dtype, **cfg):
    """(loss, dx) of `berman` in `dtype` for the upstream gradient dloss"""
    pd = p.detach().to(dtype).requires_grad_(True)
    loss = berman(pd, t.detach().to(dtype), **cfg)
    (loss * dloss).backward()
    return loss.detach(), pd.grad


_berman32_cache = {}


def torch32(p, t, dloss, classes='present', per_image=False, class_weights=None, key=None):
    """Berman's formula in fp32 on the CPU -> (loss, dx): the figures the tests print beside the device's error, never
    asserted.  The segments are disjoint, so one backward of sum_r L_r gives every dL_r/dp; key: as in closed_form"""
    N, C_ = p.shape[:2]
    ck = None if key is None else (key, bool(per_image))
    if ck is None or ck not in _berman32_cache:
        pd = p.detach().float().requires_grad_(True)
        ps, fgs = segments(pd, per_image), (segments(t, per_image) >= 0.5).float()
        losses = []
        for r in range(ps.shape[0]):
            errors = (fgs[r] - ps[r]).abs()
            order = torch.sort(errors.detach(), descending=True, stable=True).indices
            losses.append(torch.dot(errors[order], lovasz_grad(fgs[r][order])))
        L = torch.stack(losses)
        L.sum().backward()
        seg = (L.detach(), segments(pd.grad, per_image), fgs.sum(1))
        if ck is not None:
            _berman32_cache[ck] = seg
    else:
        seg = _berman32_cache[ck]
    L, dp, G = seg
    loss, coef, _ = reduce(L, G, classes, per_image, class_weights, N, C_)
    return loss, unsegment(dp * (coef * dloss)[:, None], p.shape, per_image)


# ---------------------------------------------------------------------------------------------------------- closed form
def closed_form_segments(p, t, per_image):
    """-> (L [R] fp64, dL/dp [R, M] fp64, G [R] int64) of fp32 p, t [N, C, ...]: the definition the kernels implement"""
    assert p.dtype == torch.float32 and t.dtype == torch.float32
    ps, ts = segments(p, per_image), segments(t, per_image)
    fg = ts >= 0.5
    e = (fg.float() - ps).abs()                      # one fp32 subtraction
    R, M = e.shape
    L = torch.zeros(R, dtype=torch.float64)
    dp = torch.zeros(R, M, dtype=torch.float64)
    G = fg.sum(1)
    for r in range(R):
        values, inverse, counts = torch.unique(e[r], return_inverse=True, return_counts=True)   # ascending
        fg_counts = torch.zeros_like(counts).scatter_add_(0, inverse, fg[r].long())
        values, counts, fg_counts = values.flip(0), counts.flip(0), fg_counts.flip(0)           # descending errors
        hi, f_hi = counts.cumsum(0), fg_counts.cumsum(0)
        lo, f_lo = hi - counts, f_hi - fg_counts
        g = int(G[r])
        i_lo, u_lo, i_hi, u_hi = g - f_lo, g + lo - f_lo, g - f_hi, g + hi - f_hi
        first = lo == 0
        num = torch.where(first, u_hi - i_hi, i_lo * u_hi - i_hi * u_lo)
        den = torch.where(first, u_hi, u_lo * u_hi)
        dj = num.double() / den.double()
        L[r] = (values.double() * dj).sum()
        per_member = (dj / counts.double()).flip(0)[inverse]
        dp[r] = torch.where(fg[r], -per_member, per_member)
    return L, dp, G


_segments_cache = {}


def closed_form(p, t, dloss, classes='present', per_image=False, class_weights=None, key=None):
    """-> {'loss', 'dx' like p, 'count', 'L', 'G'} in fp64; key: a hashable name of (p, t) under which the per-segment
    part -- the expensive one -- is computed once for all reductions"""
    N, C_ = p.shape[:2]
    ck = None if key is None else (key, bool(per_image))
    if ck is None or ck not in _segments_cache:
        seg = closed_form_segments(p, t, per_image)
        if ck is not None:
            _segments_cache[ck] = seg
    else:
        seg = _segments_cache[ck]
    L, dp, G = seg
    loss, coef, count = reduce(L, G, classes, per_image, class_weights, N, C_)
    return {'loss': loss, 'dx': unsegment(dp * (coef * dloss)[:, None], p.shape, per_image), 'count': count, 'L': L, 'G': G}


# --------------------------------------------------------------------------------------------------------------- inputs
# name -> shape: the shapes of the forward / backward comparison.  "scan": S = 103 * 101 * 103 = 1071509 with N = 1 is 262
# tiles of 4096 per segment -- more than the 256 tile counts the scan kernel takes at a time (its carry), more than the 64
# a wave of the sort's scan takes at a time, and a ragged last tile
CASES = {"tiny": (2, 3, 7, 5, 3), "ragged": (1, 3, 17, 19, 23), "blocks": (2, 5, 24, 20, 12), "scan": (1, 2, 103, 101, 103)}


def softmax_inputs(shape, seed):
    """(p, t) fp32 on the host: p a softmax over C of 2 randn, t the one-hot of random labels"""
    g = torch.Generator().manual_seed(seed)
    N, C_ = shape[:2]
    p = torch.softmax(2 * torch.randn(shape, generator=g), dim=1)
    lab = torch.randint(0, C_, (N, 1) + tuple(shape[2:]), generator=g)
    return p.contiguous(), torch.zeros(shape).scatter_(1, lab, 1.0)


def untied_inputs(shape, seed):
    """(p, t) fp32: within every channel of the batch the errors are the distinct values k / 4096, k = 1 .. N * S < 4096,
    in a seeded order, exact in fp32 as is 1 - e; no e = 0.  (p is no softmax: the loss takes every channel by itself.)"""
    g = torch.Generator().manual_seed(seed)
    N, C_ = shape[:2]
    S = 1
    for d in shape[2:]:
        S *= d
    assert N * S < 4096
    e = torch.stack([(torch.randperm(N * S, generator=g) + 1).float() / 4096 for _ in range(C_)])   # [C, N * S]
    e = e.reshape(C_, N, S).transpose(0, 1)
    fg = torch.rand((N, C_, S), generator=g) < 0.3
    return torch.where(fg, 1 - e, e).reshape(shape).contiguous(), fg.float().reshape(shape)


def tied_inputs(shape, seed, levels=8):
    """(p, t) fp32: probabilities on a grid of `levels` + 1 values, 0 and 1 included, so most errors are tied"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(0, levels + 1, shape, generator=g).float() / levels
    return p, (torch.rand(shape, generator=g) < 0.4).float()


# ----------------------------------------------------------------------------------------------------- raw entry points
def raw_sort(hip, keys, end_bit=32, out=None, ws=None):
    """m355_segmented_sort_u32 on an int32 device tensor [R, M] (its bits are the uint32 keys) -> the sorted copy"""
    L = _lib.lib()
    R, M = keys.shape
    if out is None:
        out = hip.empty(R, M, dtype=torch.int32)
    if ws is None:
        ws = hip._workspace(L.m355_segmented_sort_workspace(R, M))
    _chk(L.m355_segmented_sort_u32(_p(keys), _p(out), R, M, end_bit, _p(ws), ws.numel(), _stream()), "segmented_sort_u32")
    return out


def raw_fwd(hip, p, t, classes='present', per_image=False, class_weights=None, skeys=None, F=None, ws=None):
    """m355_lovasz_loss_fwd on device tensors (any views whose rows are dense) -> (out2, sorted keys, F, state)"""
    L = _lib.lib()
    N, C_ = p.shape[:2]
    S = p.numel() // (N * C_)
    R, M = (N * C_, S) if per_image else (C_, N * S)
    cw = _dev(class_weights)
    out2 = hip.empty(2)
    state = hip.empty(2 * R, dtype=torch.int32)
    if skeys is None:
        skeys = hip.empty(R * M, dtype=torch.int32)
    if F is None:
        F = hip.empty(R * M, dtype=torch.int32)
    if ws is None:
        ws = hip._workspace(L.m355_lovasz_loss_workspace(N, C_, S, int(per_image)))
    _chk(L.m355_lovasz_loss_fwd(_p(p), _p(t), N, C_, S, int(per_image), int(classes == "all"), _p(cw), _p(out2), _p(skeys),
                                _p(F), _p(state), _p(ws), ws.numel(), _stream()), "lovasz_loss_fwd")
    return out2, skeys, F, state


def raw_bwd(hip, p, t, skeys, F, state, dloss, per_image=False, out=None, **_):
    L = _lib.lib()
    N, C_ = p.shape[:2]
    S = p.numel() // (N * C_)
    g = torch.tensor([dloss], dtype=torch.float32, device="cuda")
    dx = hip.empty(*p.shape) if out is None else out
    _chk(L.m355_lovasz_loss_bwd(_p(p), _p(t), _p(skeys), _p(F), _p(state), _p(g), N, C_, S, int(per_image), _p(dx),
                                _stream()), "lovasz_loss_bwd")
    return dx


def state_fields(state):
    """(G [R] int64, coefficient [R] fp32) of the saved state, on the host"""
    words = state.cpu().reshape(-1, 2)
    return words[:, 0].long(), words[:, 1].contiguous().view(torch.float32)
