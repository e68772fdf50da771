"""HybridTopKDiceLoss on the device: m355_topk_loss_fwd / _bwd in both modes against the fp64 formulas of
tests/topk_loss_ref.py on inputs with a guaranteed margin below the k-th largest value, the equivalence with the hybrid
and the focal Tversky losses at top_k = 1, shared ties, non-finite values, determinism and memory safety, the models
with the Softmax and the Identity head in the three activation flows, the wrappers, and the captured train step that
follows set_top_k.
The lines starting with `topk_loss_accuracy` are what profiles/topk_loss_accuracy.txt records."""
import copy
from functools import partial

import pytest
import torch
from torch import nn

import topk_loss_ref as T
from segmentation_pipeline_amd import _lib, ops
from segmentation_pipeline_amd.criterions import BoundaryLoss, DeepSupervisionLoss, HybridTopKDiceLoss
from segmentation_pipeline_amd.criterions.deep_supervision_loss import default_weights
from segmentation_pipeline_amd.models import DeepSupervisionUNet, ModularUNet

pytestmark = pytest.mark.gpu

MODES = [False, True]
FRACTIONS = [0.1, 0.5, 1.0, 1e-6]     # the last one: k = 1
DLOSS = 0.7


def close(got, ref, rtol, atol, what, torch32=None):
    """tests/test_kernels_gpu.py's close(): max |got - ref| <= atol + rtol * max |ref|; prints the figure first"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, bound = (got - ref).abs().max().item(), atol + rtol * ref.abs().max().item()
    t32 = "" if torch32 is None else f"  torch fp32 on the CPU {(torch32.double() - ref).abs().max().item():.3e}"
    print(f"topk_loss_accuracy {what}: max err {err:.3e}  bound {bound:.3e}{t32}")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def ulps(a, b):
    """the distance of two fp32 values of one sign in units of the last place"""
    ia, ib = (torch.tensor(float(v), dtype=torch.float32).view(torch.int32).item() for v in (a, b))
    return abs(ia - ib)


def _weights(channels):
    return [float(c + 1) for c in range(channels)]


_inputs, _expected = {}, {}


def inputs(case):
    if case not in _inputs:
        _inputs[case] = T.margin_inputs(case)
    return _inputs[case]


def expected(case, from_logits, weighted, square_dice, top_k, dice_weight=0.5):
    """the fp64 values and the fp32 torch figures of one combination, computed once"""
    key = (case, from_logits, weighted, square_dice, top_k, dice_weight)
    if key not in _expected:
        z, p, t = inputs(case)
        x = z if from_logits else p
        kw = dict(top_k=top_k, dice_weight=dice_weight, class_weights=_weights(x.shape[1]) if weighted else None,
                  square_dice=square_dice, from_logits=from_logits)
        _expected[key] = (x, t, kw, T.expected(x, t, DLOSS, **kw), T.torch32(x, t, DLOSS, **kw))
    return _expected[key]


def _tag(case, from_logits, weighted, square_dice, top_k):
    return (f"{case} {'logits' if from_logits else 'prob'} {'weights' if weighted else 'ones'} "
            f"{'square' if square_dice else 'plain'} top_k {top_k:g}")


# ------------------------------------------------------------------------------------------------ kernels against fp64
FWD_BWD = [pytest.param(case, fl, w, sq, id=f"{case}-{'logits' if fl else 'prob'}-{'w' if w else 'ones'}-{'sq' if sq else 'plain'}")
           for case in T.CASES for fl in MODES for w in (False, True) for sq in (True, False)]


@pytest.mark.parametrize("case,from_logits,weighted,square_dice", FWD_BWD)
def test_fwd_bwd_against_fp64(case, from_logits, weighted, square_dice):
    """at top_k 0.1, 0.5, 1.0 and k = 1: out3 within close(2e-6, 1e-7), the Dice sums within close(2e-6, 1e-6), the
    gradient for dloss = 0.7 within close(1e-5, 1e-9) -- the bounds of test_hybrid_loss_fwd_bwd -- and the threshold
    within 2 ulp of the k-th largest of torch's fp32 e"""
    for top_k in FRACTIONS:
        x, t, kw, ref, t32 = expected(case, from_logits, weighted, square_dice, top_k)
        tag = _tag(case, from_logits, weighted, square_dice, top_k)
        xd, td = x.cuda(), t.cuda()
        out3, sums, e, state = T.raw_fwd(xd, td, **kw)
        dx = T.raw_bwd(xd, td, e, sums, state, DLOSS, **kw)
        tau, r, k = T.state_fields(state)
        d_ulp = ulps(tau, ref['threshold32'].item())
        print(f"topk_loss_accuracy {tag} threshold: {tau:.9g} vs torch fp32 {ref['threshold32'].item():.9g} "
              f"({d_ulp} ulp), fp64 {ref['threshold'].item():.9g}; k {k}, r {r:g}")
        close(out3, ref['out3'], 2e-6, 1e-7, f"{tag} out3", t32['out3'])
        close(sums, ref['sums'], 2e-6, 1e-6, f"{tag} sums", t32['sums'])
        close(dx, ref['dx'], 1e-5, 1e-9, f"{tag} dx", t32['dx'])
        assert k == ref['k'] and r == 1.0
        assert d_ulp <= 2, f"{tag}: threshold {tau!r} is {d_ulp} ulp from {ref['threshold32'].item()!r}"
        assert bool(torch.isfinite(out3).all()) and bool(torch.isfinite(dx).all())


@pytest.mark.parametrize("from_logits", MODES, ids=["prob", "logits"])
@pytest.mark.parametrize("case", list(T.CASES))
def test_unselected_voxels_have_no_gradient(case, from_logits):
    """dice_weight = 0: dx is exactly 0 in every channel of every voxel the reference does not select, and the selected
    voxels are those with a gradient at their true class"""
    for top_k in (0.1, 0.5):
        x, t, kw, ref, _ = expected(case, from_logits, True, True, top_k, dice_weight=0.0)
        xd, td = x.cuda(), t.cuda()
        out3, sums, e, state = T.raw_fwd(xd, td, **kw)
        N, C_ = x.shape[:2]
        dx = T.raw_bwd(xd, td, e, sums, state, DLOSS, **kw).cpu().reshape(N, C_, -1)
        unselected = (ref['sel'] == 0)[:, None, :].expand(N, C_, -1)
        at_true = (dx * t.reshape(N, C_, -1)).sum(1)
        print(f"topk_loss_accuracy {_tag(case, from_logits, True, True, top_k)} dice_weight 0: {int((ref['sel'] == 0).sum())} "
              f"voxels unselected, max |dx| there {dx[unselected].abs().max().item():.3e}, "
              f"{int((at_true != 0).sum())} voxels with a gradient (k {ref['k']})")
        assert bool((dx[unselected] == 0).all())
        assert torch.equal(at_true != 0, ref['sel'] > 0) and int((at_true != 0).sum()) == ref['k']
        assert torch.equal(e.cpu().reshape(N, -1) >= T.state_fields(state)[0], ref['sel'] == 1)


@pytest.mark.parametrize("from_logits", MODES, ids=["prob", "logits"])
def test_autograd_function_matches_the_entry_points(from_logits):
    """the criterion through ops.topk_logistic_dice_loss: the bits of the raw calls whether k is a fraction on the host or a
    count on the device, four 0-dim fp32 tensors, the gradient through 'loss' only"""
    x, t, kw, ref, _ = expected("small", from_logits, True, True, 0.1, dice_weight=0.3)
    crit = HybridTopKDiceLoss(0.1, 0.3, kw['class_weights'], True, from_logits)
    xd = x.cuda().requires_grad_(True)
    ld = crit(xd, t.cuda())
    assert list(ld) == ['loss', 'dice_loss', 'logistic_loss', 'topk_threshold']
    assert all(v.shape == () and v.dtype == torch.float32 and v.is_cuda for v in ld.values())
    assert ld['loss'].requires_grad and not any(ld[k].requires_grad for k in ('dice_loss', 'logistic_loss', 'topk_threshold'))
    (ld['loss'] * DLOSS).backward()
    out3, sums, e, state = T.raw_fwd(x.cuda(), t.cuda(), **kw)
    assert torch.equal(torch.stack([ld[k].detach() for k in ('loss', 'dice_loss', 'logistic_loss')]), out3)
    assert torch.equal(ld['topk_threshold'], state[0])
    assert torch.equal(xd.grad, T.raw_bwd(x.cuda(), t.cuda(), e, sums, state, DLOSS, **kw))
    # the host's k and the device's
    by_fraction = ops.topk_logistic_dice_loss(x.cuda(), t.cuda(), 0.1, 0.3, torch.tensor(kw['class_weights'], device="cuda"),
                                              True, from_logits)
    assert torch.equal(torch.stack(by_fraction[:3]), out3) and torch.equal(by_fraction[3], state[0])
    (count,) = crit._counts.values()
    assert count.item() == ref['k'] == T.state_fields(state)[2]
    assert set(crit._uploaded) == {"logistic_class_weights"}
    # a count outside [1, M] on the device is clamped there
    big = torch.tensor(10 ** 12, dtype=torch.int64, device="cuda")
    full = T.raw_fwd(x.cuda(), t.cuda(), **dict(kw, top_k=1.0))
    clamped = T.raw_fwd(x.cuda(), t.cuda(), k_device=big, **{k: v for k, v in kw.items() if k != 'top_k'})
    assert all(torch.equal(a, b) for a, b in zip(full, clamped))


# ------------------------------------------------------------------------------------------- top_k = 1 is the old losses
@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
@pytest.mark.parametrize("case", list(T.CASES))
def test_top_k_one_is_the_hybrid_and_the_focal_tversky_loss(case, weighted):
    """on the device, within twice the bounds each side is held to against fp64: prob mode against
    ops.hybrid_logistic_dice_loss with and without square_dice; logits mode with square_dice=False against
    ops.focal_tversky_loss(alpha = beta = .5, power 1, gamma 0, from_logits=True)"""
    z, p, t = inputs(case)
    C_ = p.shape[1]
    cw = torch.tensor(_weights(C_), device="cuda") if weighted else None
    td = t.cuda()

    def run(fn, x):
        xd = x.cuda().requires_grad_(True)
        out = fn(xd)
        (out[0] * DLOSS).backward()
        return torch.stack([v.detach() for v in out[:3]]), xd.grad

    for what, x, mine, theirs in (
            ("prob square vs hybrid", p, lambda x: ops.topk_logistic_dice_loss(x, td, 1.0, 0.3, cw, True, False),
             lambda x: ops.hybrid_logistic_dice_loss(x, td, 0.3, cw, True)),
            ("prob plain vs hybrid", p, lambda x: ops.topk_logistic_dice_loss(x, td, 1.0, 0.3, cw, False, False),
             lambda x: ops.hybrid_logistic_dice_loss(x, td, 0.3, cw, False)),
            ("logits plain vs focal Tversky", z, lambda x: ops.topk_logistic_dice_loss(x, td, 1.0, 0.3, cw, False, True),
             lambda x: ops.focal_tversky_loss(x, td, 0.3, .5, .5, 1.0, 0.0, cw, None, True))):
        out3_a, dx_a = run(mine, x)
        out3_b, dx_b = run(theirs, x)
        close(out3_a, out3_b, 4e-6, 2e-7, f"{case} {'weights' if weighted else 'ones'} top_k 1 {what} out3")
        close(dx_a, dx_b, 2e-5, 2e-9, f"{case} {'weights' if weighted else 'ones'} top_k 1 {what} dx")


# ------------------------------------------------------------------------------------------------ ties
def _hard_target(shape, seed):
    N, C_, S = shape
    lab = torch.randint(0, C_, (N, 1, S), generator=torch.Generator().manual_seed(seed))
    return torch.zeros(shape).scatter_(1, lab, 1.0)


@pytest.mark.parametrize("from_logits", MODES, ids=["prob", "logits"])
def test_a_constant_prediction_ties_every_voxel(from_logits):
    """every e is equal: tau is that value, n_gt = 0, r = k / M; logistic_loss = tau / C whatever k is; with dice_weight
    0 the gradient is the same at every voxel and sums to the shared-tie closed form's"""
    shape = (2, 3, 1155)     # M = 2310: odd rows, less than one chunk
    t = _hard_target(shape, 3)
    x = torch.full(shape, 0.0 if from_logits else 0.25)
    e32 = T.voxel_ce(x, t, None, from_logits)[0]
    assert bool((e32 == e32[0, 0]).all())
    M = shape[0] * shape[2]
    for top_k in (1e-6, 0.1, 0.5, 1.0):
        k = ops.topk_count(shape[0], shape[2], top_k)
        kw = dict(k=k, dice_weight=0.0, from_logits=from_logits)
        out3, sums, e, state = T.raw_fwd(x.cuda(), t.cuda(), **kw)
        tau, r, k_dev = T.state_fields(state)
        ref = T.topk_dice(x.double(), t.double(), **kw)
        assert k_dev == k and ulps(tau, e32[0, 0].item()) <= 2 and bool((e == tau).all())
        assert r == torch.tensor(k / M, dtype=torch.float32).item()
        assert out3[2].item() == torch.tensor(tau / 3, dtype=torch.float32).item()          # (k tau) / (C k), exactly
        close(out3[2], ref['logistic_loss'], 2e-6, 1e-7, f"all tied {'logits' if from_logits else 'prob'} k {k} logistic_loss")
        dx = T.raw_bwd(x.cuda(), t.cuda(), e, sums, state, DLOSS, **kw).cpu()
        closed = T.closed_form_bwd(x.double(), t.double(), DLOSS, **kw)
        on, off = dx[t == 1], dx[t == 0]
        assert bool((on == on[0]).all()) and bool((off == off[0]).all()) and on[0].item() < 0
        assert from_logits or off[0].item() == 0.0
        for part, mask in (("true class", t == 1), ("other classes", t == 0)):
            got, want = dx[mask].double().sum().item(), closed[mask].sum().item()
            print(f"topk_loss_accuracy all tied {'logits' if from_logits else 'prob'} k {k}: gradient summed over the {part} "
                  f"{got:.9e} vs closed form {want:.9e}")
            assert abs(got - want) <= 1e-5 * abs(want) + 1e-12


def test_a_saturated_block_larger_than_k_shares_k():
    """prob mode, 1000 voxels with x = 0 on the true class and k = 600: tau = -log(1e-8 / (1 + 1e-8)) in fp32, n_gt = 0,
    the selection weights -- r = k / n_eq on the block, recovered from the gradient too -- sum to k within 1e-6 k"""
    shape, n_sat, k = (1, 2, 3001), 1000, 600
    g = torch.Generator().manual_seed(9)
    t = _hard_target(shape, 4)
    p0 = torch.rand((1, 1, shape[2]), generator=g) * 0.8 + 0.1
    x = torch.cat([p0, 1 - p0], dim=1)
    sat = torch.randperm(shape[2], generator=g)[:n_sat]
    x[:, :, sat] = 1 - t[:, :, sat]                     # all the mass on the wrong class
    tau32 = -torch.log((torch.zeros((), dtype=torch.float32) + 1e-8) / (1 + 1e-8))
    kw = dict(k=k, dice_weight=0.0)
    out3, sums, e, state = T.raw_fwd(x.cuda(), t.cuda(), **kw)
    tau, r, k_dev = T.state_fields(state)
    n_gt, n_eq = int((e > tau).sum()), int((e == tau).sum())
    dx = T.raw_bwd(x.cuda(), t.cuda(), e, sums, state, 1.0, **kw).cpu().double()
    # dx = -sel / (C k) / (x + eps) at the true class (fp32: eps is 1e-8f there)
    sel = -(dx * t).sum(1) * (2 * k) * ((x * t).sum(1).double() + float(torch.tensor(1e-8, dtype=torch.float32)))
    print(f"topk_loss_accuracy saturated block: tau {tau:.9g} (fp32 {tau32.item():.9g}), n_gt {n_gt}, n_eq {n_eq}, r {r:.9g}, "
          f"r n_eq - k {r * n_eq - k:.3e}, sum of the selection weights from dx - k {sel.sum().item() - k:.3e}")
    assert ulps(tau, tau32.item()) <= 2 and (n_gt, n_eq, k_dev) == (0, n_sat, k)
    assert abs(r * n_eq + n_gt - k) <= 1e-6 * k
    assert abs(sel.sum().item() - k) <= 1e-6 * k
    assert int((sel != 0).sum()) == n_sat
    ref = T.topk_dice(x.double(), t.double(), **kw)
    close(out3, torch.stack([ref['loss'], ref['dice_loss'], ref['logistic_loss']]), 2e-6, 1e-7, "saturated block out3")


# ------------------------------------------------------------------------------------------------ non-finite values
def test_a_nan_logit_gives_a_nan_loss():
    z, _, t = inputs("small")
    z = z.clone()
    z[1, 2, 3, 4, 5] = float("nan")
    kw = dict(top_k=0.1, from_logits=True)
    out3, sums, e, state = T.raw_fwd(z.cuda(), t.cuda(), **kw)
    dx = T.raw_bwd(z.cuda(), t.cuda(), e, sums, state, DLOSS, **kw)
    torch.cuda.synchronize()
    tau, r, k = T.state_fields(state)
    assert bool(torch.isnan(out3[0])) and bool(torch.isnan(out3[2]))
    assert int(torch.isnan(e).sum()) == 1 and tau == tau and k == 198     # one NaN voxel, selected above a finite threshold
    assert int((e > tau).sum()) == 196                                    # ... which a comparison of floats does not count
    assert bool(torch.isfinite(dx[0]).all()) and bool(torch.isnan(dx[1]).any())   # the other sample's rows stay finite
    out3_1, _, _, state_1 = T.raw_fwd(z.cuda(), t.cuda(), **dict(kw, top_k=1e-6))
    assert bool(torch.isnan(out3_1[2])) and bool(torch.isnan(state_1[0]))      # k = 1: the NaN is the threshold itself


def test_an_infinite_cross_entropy_is_selected_first():
    """prob mode, x = 0 at the one voxel of class 1, whose weight is 3e38: e = +inf there.  k = 1: the threshold and the
    log term are +inf; k = 5: the threshold is the 4th largest finite e and the log term still +inf"""
    S = 500
    g = torch.Generator().manual_seed(2)
    t = torch.zeros(1, 2, S)
    t[0, 0] = 1.0
    t[0, :, 7] = torch.tensor([0.0, 1.0])
    p0 = torch.rand(S, generator=g) * 0.8 + 0.1
    x = torch.stack([p0, 1 - p0])[None].contiguous()
    x[0, :, 7] = torch.tensor([1.0, 0.0])
    cw = [1.0, 3e38]
    e32 = T.voxel_ce(x, t, cw, False)[0].flatten()
    assert e32[7].item() == float("inf") and int(torch.isinf(e32).sum()) == 1
    out3, _, e, state = T.raw_fwd(x.cuda(), t.cuda(), k=1, class_weights=cw)
    assert T.state_fields(state)[0] == float("inf") and out3[2].item() == float("inf") and e[7].item() == float("inf")
    out3, sums, e, state = T.raw_fwd(x.cuda(), t.cuda(), k=5, class_weights=cw)
    tau, r, k = T.state_fields(state)
    assert ulps(tau, torch.topk(e32, 5).values[-1].item()) <= 2 and out3[2].item() == float("inf")
    assert int((e > tau).sum()) == 4 and r == 1.0
    dx = T.raw_bwd(x.cuda(), t.cuda(), e, sums, state, DLOSS, dice_weight=0.0, class_weights=cw).cpu()
    assert int((dx[0, 0] != 0).sum()) == 4 and dx[0, 1, 7].item() != 0      # the four finite ones and the infinite one


# ------------------------------------------------------------------------------------------------ determinism, memory
@pytest.mark.parametrize("from_logits", MODES, ids=["prob", "logits"])
@pytest.mark.parametrize("case", list(T.CASES))
def test_determinism_canaries_and_misaligned_views(case, from_logits):
    """two calls give the same bits; the workspace past its declared size, the floats around e and around dx keep their
    0x5A canaries; views offset by one element (not 16-byte aligned) give the bits of their aligned clones"""
    x, t, kw, _, _ = expected(case, from_logits, True, True, 0.1)
    n = x.numel()
    N, C_ = x.shape[:2]
    M = n // C_
    xd, td = x.cuda(), t.cuda()
    first = T.raw_fwd(xd, td, **kw)
    nbytes = int(_lib.lib().m355_topk_loss_workspace(N, C_, M // N))
    ws = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    ebuf = torch.full(((M + 8) * 4,), 0x5A, dtype=torch.uint8, device="cuda")
    canary = ebuf[:4].view(torch.float32).clone()
    second = T.raw_fwd(xd, td, e=ebuf.view(torch.float32)[4:4 + M], ws=ws[:nbytes], **kw)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert bool((ws[nbytes:] == 0x5A).all()), "the workspace's declared size"
    assert bool((ebuf[:16] == 0x5A).all()) and bool((ebuf[(4 + M) * 4:] == 0x5A).all()), "the floats around e"
    out3, sums, e, state = first
    guard = 64
    buf = torch.full((n + 2 * guard,), canary.item(), device="cuda")
    dx = T.raw_bwd(xd, td, e, sums, state, DLOSS, out=buf[guard:guard + n].view(x.shape), **kw)
    assert torch.equal(buf[:guard].view(torch.int32), canary.view(torch.int32).expand(guard))
    assert torch.equal(buf[guard + n:].view(torch.int32), canary.view(torch.int32).expand(guard))
    assert torch.equal(dx, T.raw_bwd(xd, td, e, sums, state, DLOSS, **kw))
    # offset by one element
    xb, tb, eb = torch.zeros(n + 8, device="cuda"), torch.zeros(n + 8, device="cuda"), torch.zeros(M + 8, device="cuda")
    xb[1:1 + n], tb[1:1 + n] = xd.flatten(), td.flatten()
    xo, to = xb[1:1 + n].view(x.shape), tb[1:1 + n].view(x.shape)
    assert xo.data_ptr() % 16 != 0 and to.data_ptr() % 16 != 0 and xd.data_ptr() % 16 == 0
    out3_o, sums_o, e_o, state_o = T.raw_fwd(xo, to, e=eb[1:1 + M], **kw)
    assert e_o.data_ptr() % 16 != 0
    assert torch.equal(out3_o, out3) and torch.equal(sums_o, sums) and torch.equal(e_o, e) and torch.equal(state_o, state)
    assert eb[0].item() == 0 and not eb[1 + M:].any()
    buf_o = torch.full((n + 2 * guard + 1,), 7.0, device="cuda")
    dx_o = T.raw_bwd(xo, to, e_o, sums, state, DLOSS, out=buf_o[guard + 1:guard + 1 + n].view(x.shape), **kw)
    assert dx_o.data_ptr() % 16 != 0
    assert torch.equal(dx_o, dx)
    assert bool((buf_o[:guard + 1] == 7.0).all()) and bool((buf_o[guard + 1 + n:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ models
FILTERS = [8, 16]
HEADS = {False: (nn.Softmax, {"dim": 1}), True: (nn.Identity, {})}
GN4 = {'normalization_class': partial(nn.GroupNorm, 4)}


def _unet(from_logits):
    torch.manual_seed(0)
    head, params = HEADS[from_logits]
    return ModularUNet(2, 3, FILTERS, 2, block_params=dict(GN4), hypothesis_class=head, hypothesis_params=params)


def _batch(cin, cout, seed=1234, size=(16, 16, 16)):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, cin, *size), generator=g)
    lab = torch.randint(0, cout, (1, *size), generator=g)
    return x, torch.nn.functional.one_hot(lab, cout).permute(0, 4, 1, 2, 3).float().contiguous()


def _step(model, loss_fn, x, y):
    model.zero_grad(set_to_none=True)
    out = model(x)
    ld = loss_fn(out, y)
    ld["loss"].backward()
    return {k: v.detach().clone() for k, v in ld.items()}, {k: v.grad.detach().clone() for k, v in model.named_parameters()}


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("from_logits", MODES, ids=["softmax_head_prob", "identity_head_logits"])
def test_model_step_equals_the_raw_op_path(from_logits, prec):
    """one training step of the ModularUNet (the sizes of test_focal_tversky_gpu.py's model test) in each activation flow:
    loss and every parameter gradient finite and, bit for bit, those of the same step with the loss taken through
    ops.topk_logistic_dice_loss and a fraction on the host"""
    import segmentation_pipeline_amd as sp
    model = _unet(from_logits).cuda().train()
    x, y = _batch(2, 3)
    x, y = x.cuda(), y.cuda()
    crit = HybridTopKDiceLoss(0.25, 0.4, [1, 2, 3], True, from_logits)
    cw = torch.tensor([1.0, 2.0, 3.0], device="cuda")

    def raw(out, target):
        loss, dice, logistic, thr = ops.topk_logistic_dice_loss(out, target, 0.25, 0.4, cw, True, from_logits)
        return {'loss': loss, 'dice_loss': dice, 'logistic_loss': logistic, 'topk_threshold': thr}
    with sp.precision(prec):
        ops.fp16_overflow()
        ld, grads = _step(model, crit, x, y)
        ld_raw, grads_raw = _step(model, raw, x, y)
    print(f"topk_loss_accuracy unet {prec} {'identity head, logits' if from_logits else 'softmax head, prob'}: loss "
          f"{ld['loss'].item():.6f} dice {ld['dice_loss'].item():.6f} logistic {ld['logistic_loss'].item():.6f} threshold "
          f"{ld['topk_threshold'].item():.6f}")
    assert all(bool(torch.isfinite(v)) for v in ld.values()) and len(grads) > 10
    assert ld['logistic_loss'].item() > 0 and ld['topk_threshold'].item() > 0
    for k in ld:
        assert torch.equal(ld[k], ld_raw[k]), k
    for k, g in grads.items():
        assert bool(torch.isfinite(g).all()) and torch.equal(g, grads_raw[k]), k
    assert any(g.abs().max().item() > 0 for g in grads.values())


def test_inside_deep_supervision_and_boundary_loss():
    """DeepSupervisionLoss(BoundaryLoss(HybridTopKDiceLoss)): every level selects its own k of its own voxels; the total
    is the weighted sum of the levels taken by hand and the gradients are finite"""
    torch.manual_seed(5)
    model = DeepSupervisionUNet(2, 3, [8, 16, 24], 3, aux_levels=1, block_params=dict(GN4),
                                upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2}).cuda().train()
    x, y = _batch(2, 3, seed=200, size=(8, 16, 16))
    x, y = x.cuda(), y.cuda()
    inner = HybridTopKDiceLoss(0.2, logistic_class_weights=[1, 2, 3])
    crit = DeepSupervisionLoss(BoundaryLoss(inner))
    out = model(x)
    assert [tuple(p.shape) for p in out] == [(1, 3, 8, 16, 16), (1, 3, 4, 8, 8)]
    ld = crit(out, y)
    assert {'loss', 'dice_loss', 'logistic_loss', 'topk_threshold', 'boundary_loss', 'loss_level0', 'loss_level1'} <= set(ld)
    assert sorted(c.item() for c in inner._counts.values()) == [ops.topk_count(1, 256, 0.2), ops.topk_count(1, 2048, 0.2)]
    targets = [y] + ops.target_pyramid(y, 1, 'area')
    by_hand = [crit.criterion(p.detach(), t)["loss"] for p, t in zip(out, targets)]
    w = default_weights(2)
    total = w[0] * by_hand[0] + w[1] * by_hand[1]
    print(f"topk_loss_accuracy deep supervision + boundary: total {ld['loss'].item():.7f} levels "
          f"{[round(v.item(), 6) for v in by_hand]} threshold {ld['topk_threshold'].item():.6f}")
    assert torch.equal(ld['loss'].detach(), total) and bool(torch.isfinite(ld['loss']))
    ld["loss"].backward()
    for k, v in model.named_parameters():
        assert v.grad is not None and bool(torch.isfinite(v.grad).all()) and v.grad.abs().max().item() > 0, k


@pytest.mark.parametrize("from_logits", MODES, ids=["prob", "logits"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_graphed_train_step_follows_the_schedule(prec, from_logits):
    """trainer.GraphedTrainStep with the criterion: two eager warm-up steps, then four replayed ones, set_top_k(0.5)
    before the last two.  The loss dicts equal those of six eager steps from the same seed bit for bit, the eager
    logistic_loss after the change is that of a fresh criterion at 0.5 and differs from the one at 0.1, and the step
    was captured once"""
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd.trainer import GraphedTrainStep
    m_e = _unet(from_logits).cuda().train()
    m_g = copy.deepcopy(m_e)
    batches = []
    for i in range(6):
        x, y = _batch(2, 3, seed=100 + i)
        batches.append({"X": x.cuda(), "y": y.cuda()})
    crit = HybridTopKDiceLoss(0.1, 0.3, [1, 2, 3], True, from_logits)
    with sp.precision(prec):
        opt_e = torch.optim.SGD(m_e.parameters(), lr=1e-2, momentum=0.9)
        opt_g = torch.optim.SGD(m_g.parameters(), lr=1e-2, momentum=0.9)
        step = GraphedTrainStep(m_g, crit, opt_g, warmup=2)
        losses_e, losses_g = [], []
        for i, b in enumerate(batches):
            if i == 4:
                crit.set_top_k(0.5)
            opt_e.zero_grad(set_to_none=True)
            out = m_e(b["X"])
            ld = crit(out, b["y"])
            if i >= 4:
                for fraction, same in ((0.5, True), (0.1, False)):
                    fresh = HybridTopKDiceLoss(fraction, 0.3, [1, 2, 3], True, from_logits)(out.detach(), b["y"])
                    assert torch.equal(fresh['logistic_loss'], ld['logistic_loss']) == same, (i, fraction)
            ld["loss"].backward()
            opt_e.step()
            losses_e.append(torch.stack([v.detach().clone() for v in ld.values()]))
            losses_g.append(torch.stack([v.detach().clone() for v in step(b).values()]))
    print(f"topk_loss_accuracy graphed {prec} {'logits' if from_logits else 'prob'}: logistic_loss per step "
          f"{[round(v[2].item(), 6) for v in losses_g]}")
    assert torch.equal(torch.stack(losses_e), torch.stack(losses_g))
    assert len(step._graphs) == 1 and next(iter(step._graphs.values()))["graph"] is not None
    assert len(crit._counts) == 1
