"""HybridFocalTverskyLoss on the device: m355_focal_tversky_fwd / _bwd in both modes against the fp64 formulas of
tests/focal_tversky_ref.py, the recorded fixture of the hybrid loss, saturated probabilities and logits, a perfect
prediction with a power below 1, determinism and memory safety, the models with the Softmax and the Identity head in the
three activation flows, and the captured train step.
The lines starting with `focal_tversky_accuracy` are what profiles/focal_tversky_accuracy.txt records."""
import copy
from functools import partial

import pytest
import torch
from torch import nn

import focal_tversky_ref as F
import sigmoid_ref as S
from oracle import torch_ref as R
from segmentation_pipeline_amd import ops
from segmentation_pipeline_amd.criterions import HybridFocalTverskyLoss
from segmentation_pipeline_amd.models import ModularUNet, NestedResUNet

pytestmark = pytest.mark.gpu

# (tversky_weight, alpha, beta, tversky_power, focal_gamma, focal weights, Tversky weights); a case of fewer than 3
# channels takes the first C weights, the 17-channel case repeats them
CONFIGS = [(0.5, .5, .5, 1.0, 0.0, None, None), (0.3, .3, .7, 0.75, 2.0, [1, 2, 3], [0, 1, 1]),
           (0.5, .7, .3, 1.5, 2.5, [1, 100, 1], None), (0.5, .5, .5, 1.0, 1.0, None, None)]
MODES = [False, True]
# name -> (shape, soft target).  (2, 3, 9, 10, 11): S = 990, a multiple of neither 4 nor 256, less than one chunk;
# (.., 17, 33, 31): S = 17391, odd (every second row misaligned), a ragged last chunk in both modes (8192 per block in
# prob mode, 4096 in logits mode); c1: one channel, prob mode only; c17: one channel more than the logits kernels hold in
# registers (16), so the kernels that read the planes again run
CASES = {"small": ((2, 3, 9, 10, 11), False), "large": ((1, 2, 17, 33, 31), False), "c1": ((1, 1, 17, 33, 31), False),
         "soft": ((1, 2, 17, 33, 31), True), "c17": ((1, 17, 5, 6, 7), False)}
DLOSS = 0.7


def _weights(w, channels):
    return None if w is None else [float(v) for v in (list(w) * ((channels + 2) // 3))[:channels]]


def cfg_kwargs(cfg, channels, from_logits):
    lam, al, be, e, gam, w, v = cfg
    return dict(tversky_weight=lam, alpha=al, beta=be, tversky_power=e, focal_gamma=gam,
                focal_class_weights=_weights(w, channels), tversky_class_weights=_weights(v, channels),
                from_logits=from_logits)


def close(got, ref, rtol, atol, what, torch32=None):
    """tests/test_kernels_gpu.py's close(): max |got - ref| <= atol + rtol * max |ref|; prints the figure first"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, bound = (got - ref).abs().max().item(), atol + rtol * ref.abs().max().item()
    t32 = "" if torch32 is None else f"  torch fp32 on the CPU {(torch32.double() - ref).abs().max().item():.3e}"
    print(f"focal_tversky_accuracy {what}: max err {err:.3e}  bound {bound:.3e}{t32}")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def inputs(case):
    """(z, p, t) on the host: z = randn * 2, p = softmax(z) over the channels (sigmoid for one channel), t one-hot from
    random labels (rand < 0.3 for one channel), or rand for the soft case"""
    shape, soft = CASES[case]
    g = torch.Generator().manual_seed(sorted(CASES).index(case) + 1)
    z = torch.randn(shape, generator=g) * 2
    u = torch.rand(shape, generator=g)
    if shape[1] == 1:
        return z, torch.sigmoid(z), (u < 0.3).float()
    p = torch.softmax(z, dim=1)
    if soft:
        return z, p, u
    return z, p, torch.nn.functional.one_hot(u.argmax(dim=1), shape[1]).permute(0, 4, 1, 2, 3).float().contiguous()


_expected = {}


def expected(case, ci, from_logits):
    """the fp64 values and the fp32 torch figures of one (case, configuration, mode), computed once"""
    key = (case, ci, from_logits)
    if key not in _expected:
        z, p, t = inputs(case)
        x = z if from_logits else p
        kw = cfg_kwargs(CONFIGS[ci], x.shape[1], from_logits)
        _expected[key] = (x, t, kw, F.expected(x, t, DLOSS, **kw), F.torch32(x, t, DLOSS, **kw))
    return _expected[key]


# ------------------------------------------------------------------------------------------------ kernels against fp64
# (one channel: the log-softmax of a single logit is 0; that case is for prob mode)
FWD_BWD = [pytest.param(case, ci, fl, id=f"{case}-cfg{ci}-{'logits' if fl else 'prob'}") for case in CASES
           for ci in range(len(CONFIGS)) for fl in MODES if not (fl and CASES[case][0][1] == 1)]


@pytest.mark.parametrize("case,ci,from_logits", FWD_BWD)
def test_fwd_bwd_against_fp64(case, ci, from_logits):
    """out3 within close(2e-6, 1e-7), sums within close(2e-6, 1e-6), the gradient for dloss = 0.7 (from the device's own
    sums) within close(1e-5, 1e-9): the bounds of test_hybrid_loss_fwd_bwd"""
    x, t, kw, (out3_ref, sums_ref, dx_ref), (out3_32, sums_32, dx_32) = expected(case, ci, from_logits)
    tag = f"{case} cfg{ci} {'logits' if from_logits else 'prob'}"
    xd, td = x.cuda(), t.cuda()
    out3, sums = F.raw_fwd(xd, td, **kw)
    dx = F.raw_bwd(xd, td, sums, DLOSS, **kw)
    close(out3, out3_ref, 2e-6, 1e-7, f"{tag} out3", out3_32)
    close(sums, sums_ref, 2e-6, 1e-6, f"{tag} sums", sums_32)
    close(dx, dx_ref, 1e-5, 1e-9, f"{tag} dx", dx_32)
    assert bool(torch.isfinite(out3).all()) and bool(torch.isfinite(dx).all())


def test_golden_anchor(hip, golden):
    """hybrid_loss.npz case1 (dice_weight 0.3, no square_dice, class weights 1, 2, 3) in prob mode with alpha = beta = 0.5,
    power 1, gamma 0: the recorded out and dp at the bounds test_loss_golden holds the hybrid loss to.  On the random case
    out3 against m355_hybrid_loss_fwd(square_dice=False) on the device within twice the bounds each side is held to
    against fp64."""
    g = golden("hybrid_loss.npz")
    assert g["case1.cfg"].tolist() == [0.3, 0.0, 1.0, 2.0, 3.0]
    p, t = g.t("p").cuda(), g.t("t").cuda()
    kw = dict(tversky_weight=0.3, alpha=.5, beta=.5, tversky_power=1.0, focal_gamma=0.0, focal_class_weights=[1.0, 2.0, 3.0])
    out3, sums = F.raw_fwd(p, t, **kw)
    close(out3, g.t("case1.out"), 2e-6, 1e-7, "golden case1 out3")
    close(F.raw_bwd(p, t, sums, 1.0, **kw), g.t("case1.dp"), 1e-5, 1e-8, "golden case1 dp")
    _, pr, tr = inputs("small")
    out3_r, _ = F.raw_fwd(pr.cuda(), tr.cuda(), **kw)
    out3_h, _ = hip.loss_fwd(pr, tr, 0.3, torch.tensor([1.0, 2.0, 3.0]), False)
    close(out3_r, out3_h, 4e-6, 2e-7, "small, the defaults against m355_hybrid_loss_fwd out3")


@pytest.mark.parametrize("from_logits", MODES, ids=["prob", "logits"])
def test_autograd_function_matches_the_entry_points(from_logits):
    """the criterion through ops.focal_tversky_loss: the bits of the raw calls, three 0-dim fp32 tensors, the gradient
    through 'loss' only"""
    x, t, kw, _, _ = expected("small", 1, from_logits)
    lam, al, be, e, gam, w, v = CONFIGS[1]
    crit = HybridFocalTverskyLoss(lam, al, be, e, gam, w, v, from_logits)
    xd = x.cuda().requires_grad_(True)
    ld = crit(xd, t.cuda())
    assert list(ld) == ['loss', 'tversky_loss', 'focal_loss']
    assert all(v_.shape == () and v_.dtype == torch.float32 and v_.is_cuda for v_ in ld.values())
    assert ld['loss'].requires_grad and not ld['tversky_loss'].requires_grad and not ld['focal_loss'].requires_grad
    (ld['loss'] * DLOSS).backward()
    out3, sums = F.raw_fwd(x.cuda(), t.cuda(), **kw)
    assert torch.equal(torch.stack([v_.detach() for v_ in ld.values()]), out3)
    assert torch.equal(xd.grad, F.raw_bwd(x.cuda(), t.cuda(), sums, DLOSS, **kw))
    assert set(crit._uploaded) == {"logistic_class_weights", "tversky_class_weights"}


# ------------------------------------------------------------------------------------------------ saturation
def _entrywise(dx, dx_ref, g0, what):
    """every entry within 1e-5 |ref| + 1e-6 g0: relative where the gradient lives, absolute (a millionth of the gradient
    of one unweighted log term) where the focal factor drives it to zero"""
    dx, dx_ref = dx.detach().cpu().double(), dx_ref.double()
    excess = (dx - dx_ref).abs() / (1e-5 * dx_ref.abs() + 1e-6 * g0)
    print(f"focal_tversky_accuracy {what}: worst entrywise gradient error / (1e-5 |ref| + 1e-6 g0) = {excess.max().item():.3e}"
          f"  (g0 {g0:.3e}, max |ref| {dx_ref.abs().max().item():.3e}, {int((dx_ref == 0).sum())} entries exactly 0)")
    assert bool(torch.isfinite(dx).all())
    assert excess.max().item() <= 1.0, what


def _g0(kw, x, dloss):
    N, C_ = x.shape[:2]
    w = kw["focal_class_weights"]
    return abs(dloss) * (1.0 if w is None else max(w)) / (N * C_ * (x.numel() // (N * C_)))


def _combos(values):
    """every value against t = 0 and t = 1, as two channels of S = 2 * len(values) in different orders"""
    v = torch.tensor(values, dtype=torch.float32)
    x = torch.cat([v, v])
    t = torch.cat([torch.zeros(len(values)), torch.ones(len(values))])
    return torch.stack([x, x.flip(0)])[None].contiguous(), torch.stack([t, t.roll(3)])[None].contiguous()


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_saturated_probabilities(ci):
    """prob mode at p in {0, 1, 1e-8, 1 - 6e-8, 0.5, 1e-30} against t in {0, 1}: everything finite, the loss at the bounds
    of the fp64 test, every gradient entry within 1e-5 |ref| + 1e-6 g0, g0 = |dloss| max(w) / (N C S)"""
    x, t = _combos([0.0, 1.0, 1e-8, 1.0 - 6e-8, 0.5, 1e-30])
    kw = cfg_kwargs(CONFIGS[ci], 2, False)
    out3_ref, _, dx_ref = F.expected(x, t, DLOSS, **kw)
    out3, sums = F.raw_fwd(x.cuda(), t.cuda(), **kw)
    dx = F.raw_bwd(x.cuda(), t.cuda(), sums, DLOSS, **kw)
    assert bool(torch.isfinite(out3).all()) and bool(torch.isfinite(sums).all())
    _entrywise(dx, dx_ref, _g0(kw, x, DLOSS), f"saturated prob cfg{ci}")
    close(out3, out3_ref, 2e-6, 1e-7, f"saturated prob cfg{ci} out3")


def _one_hot(shape, seed):
    """(N, C, S) one-hot target in which every class occurs"""
    N, C_, S_ = shape
    lab = torch.randint(0, C_, (N, S_), generator=torch.Generator().manual_seed(seed))
    lab[:, :C_] = torch.arange(C_)
    return torch.nn.functional.one_hot(lab, C_).permute(0, 2, 1).float().contiguous()


@pytest.mark.parametrize("gamma", [0.0, 2.0])
@pytest.mark.parametrize("from_logits", MODES, ids=["prob", "logits"])
def test_perfect_prediction_with_a_power_below_one(from_logits, gamma):
    """p = t one-hot (logits +-40) with tversky_power 0.75: u = 1 - TI is exactly 0 in fp32, u^(e-1) would be infinite,
    the Tversky gradient is defined as 0.  Everything is finite, tversky_loss <= 1e-6, the gradient of the Tversky term
    alone (tversky_weight 1) is exactly 0 and that of the mix is exactly the focal term's share."""
    t = _one_hot((2, 3, 1000), 7)
    x = (t * 80 - 40) if from_logits else t.clone()
    kw = dict(alpha=.3, beta=.7, tversky_power=0.75, focal_gamma=gamma, focal_class_weights=[1.0, 2.0, 3.0],
              from_logits=from_logits)
    xd, td = x.cuda(), t.cuda()
    grads = {}
    for lam in (0.0, 0.5, 1.0):
        out3, sums = F.raw_fwd(xd, td, tversky_weight=lam, **kw)
        grads[lam] = F.raw_bwd(xd, td, sums, DLOSS, tversky_weight=lam, **kw)
        assert bool(torch.isfinite(out3).all()) and bool(torch.isfinite(sums).all()) and bool(torch.isfinite(grads[lam]).all())
        assert 0.0 <= out3[1].item() <= 1e-6, out3
    print(f"focal_tversky_accuracy perfect prediction {'logits' if from_logits else 'prob'} gamma {gamma}: tversky_loss "
          f"{out3[1].item():.3e}, max |Tversky-only gradient| {grads[1.0].abs().max().item():.3e}, "
          f"max |focal-only gradient| {grads[0.0].abs().max().item():.3e}")
    assert bool((grads[1.0] == 0).all())
    # (exact halving; an entry below the smallest normal number, p = exp(-80) times a gradient, may round by one step)
    assert (grads[0.5].double() - 0.5 * grads[0.0].double()).abs().max().item() <= 2.0 ** -149


ROWS = [(40.0, -40.0, 0.0), (-100.0, 100.0, 100.0), (88.7, 0.0, 0.0), (0.0, 0.0, 0.0)]


def _saturated_logits():
    """every row of ROWS against every one-hot target: z, t of shape [1, 3, 12], voxel 3 * row + class"""
    z = torch.tensor([r for r in ROWS for _ in range(3)], dtype=torch.float32).t().contiguous()[None]
    t = torch.eye(3).repeat(1, len(ROWS))[None].contiguous()
    return z, t


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_saturated_logits(ci):
    """logits mode on the rows (40, -40, 0), (-100, 100, 100), (88.7, 0, 0), (0, 0, 0), each against every one-hot target:
    everything finite, the loss at the bounds of the fp64 test, every gradient entry within 1e-5 |ref| + 1e-6 g0"""
    z, t = _saturated_logits()
    kw = cfg_kwargs(CONFIGS[ci], 3, True)
    out3_ref, _, dx_ref = F.expected(z, t, DLOSS, **kw)
    out3, sums = F.raw_fwd(z.cuda(), t.cuda(), **kw)
    dx = F.raw_bwd(z.cuda(), t.cuda(), sums, DLOSS, **kw)
    assert bool(torch.isfinite(out3).all()) and bool(torch.isfinite(sums).all())
    _entrywise(dx, dx_ref, _g0(kw, z, DLOSS), f"saturated logits cfg{ci}")
    close(out3, out3_ref, 2e-6, 1e-7, f"saturated logits cfg{ci} out3")


def test_a_voxel_saturated_on_the_wrong_class_keeps_its_gradient():
    """The reason the logits mode exists, with gamma = 0 (configuration 0) and dloss = 1.  Voxel 1: the row (40, -40, 0)
    against class 1, lp = -80; voxel 3: (-100, 100, 100) against class 0, lp = -200.7.  The logits-mode gradient of the true
    class's logit has magnitude >= 0.5 g0 at both.  Through ops.softmax_channels and the prob-mode loss the same gradient
    is the softmax backward's p_k (dp_k - sum p dp): exactly 0 at voxel 3, where p_k = exp(-200.7) is 0 in fp32.  At voxel
    1 p_k = exp(-80) = 1.8e-35 is still an fp32 number and the product is not exactly 0, as the issue had it, but
    p_k / (p_k + 1e-8) = 1.8e-27 of a live gradient; it is held to 1e-20 g0."""
    z, t = _saturated_logits()
    kw = cfg_kwargs(CONFIGS[0], 3, True)
    g0 = _g0(kw, z, 1.0)
    out3, sums = F.raw_fwd(z.cuda(), t.cuda(), **kw)
    dz = F.raw_bwd(z.cuda(), t.cuda(), sums, 1.0, **kw).cpu().double()
    zd = z.cuda().requires_grad_(True)
    loss, _, _ = ops.focal_tversky_loss(ops.softmax_channels(zd), t.cuda(), *CONFIGS[0][:5])
    loss.backward()
    via_p = zd.grad.cpu().double()
    print(f"focal_tversky_accuracy wrong-class voxels, gradient of the true class's logit / g0: logits mode "
          f"{dz[0, 1, 1].item() / g0:.6f} (lp -80), {dz[0, 0, 3].item() / g0:.6f} (lp -200.7); softmax head + prob mode "
          f"{via_p[0, 1, 1].item() / g0:.3e}, {via_p[0, 0, 3].item() / g0:.3e}")
    assert t[0, 1, 1] == 1 and t[0, 0, 3] == 1
    assert abs(dz[0, 1, 1].item()) >= 0.5 * g0 and abs(dz[0, 0, 3].item()) >= 0.5 * g0
    assert dz[0, 1, 1].item() < 0 and dz[0, 0, 3].item() < 0          # descent raises the true class's logit
    assert via_p[0, 0, 3].item() == 0.0
    assert abs(via_p[0, 1, 1].item()) <= 1e-20 * g0


# ------------------------------------------------------------------------------------------------ determinism, memory
@pytest.mark.parametrize("from_logits", MODES, ids=["prob", "logits"])
@pytest.mark.parametrize("case", ["large", "c17"])
def test_determinism_guards_and_misaligned_views(case, from_logits):
    """two calls give the same bits; a dx buffer keeps its guard elements; views offset by one element (not 16-byte
    aligned) give the bits of their aligned clones"""
    x, t, kw, _, _ = expected(case, 1, from_logits)
    n = x.numel()
    xd, td = x.cuda(), t.cuda()
    out3, sums = F.raw_fwd(xd, td, **kw)
    out3_b, sums_b = F.raw_fwd(xd, td, **kw)
    assert torch.equal(out3, out3_b) and torch.equal(sums, sums_b)
    guard = 64
    buf = torch.full((n + 2 * guard,), 7.0, device="cuda")
    dx = F.raw_bwd(xd, td, sums, DLOSS, out=buf[guard:guard + n].view(x.shape), **kw)
    assert bool((buf[:guard] == 7.0).all()) and bool((buf[guard + n:] == 7.0).all())
    assert torch.equal(dx, F.raw_bwd(xd, td, sums, DLOSS, **kw))
    # offset by one element
    xb, tb = torch.zeros(n + 8, device="cuda"), torch.zeros(n + 8, device="cuda")
    xb[1:1 + n], tb[1:1 + n] = xd.flatten(), td.flatten()
    xo, to = xb[1:1 + n].view(x.shape), tb[1:1 + n].view(x.shape)
    assert xo.data_ptr() % 16 != 0 and to.data_ptr() % 16 != 0 and xd.data_ptr() % 16 == 0
    out3_o, sums_o = F.raw_fwd(xo, to, **kw)
    assert torch.equal(out3_o, out3) and torch.equal(sums_o, sums)
    buf_o = torch.full((n + 2 * guard + 1,), 7.0, device="cuda")
    dx_o = F.raw_bwd(xo, to, sums, DLOSS, out=buf_o[guard + 1:guard + 1 + n].view(x.shape), **kw)
    assert dx_o.data_ptr() % 16 != 0
    assert torch.equal(dx_o, dx)
    assert bool((buf_o[:guard + 1] == 7.0).all()) and bool((buf_o[guard + 1 + n:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ models
FILTERS = [8, 16]
SPEC = R.UNetSpec(2, 3, FILTERS, 2, norm="group", groups=4, hypothesis="none")
HEADS = {False: (nn.Softmax, {"dim": 1}), True: (nn.Identity, {})}


def _unet(from_logits):
    torch.manual_seed(0)
    head, params = HEADS[from_logits]
    return ModularUNet(2, 3, FILTERS, 2, block_params={'normalization_class': partial(nn.GroupNorm, 4)},
                       hypothesis_class=head, hypothesis_params=params)


def _nested(from_logits):
    torch.manual_seed(0)
    head, params = HEADS[from_logits]
    return NestedResUNet(3, 2, 8, hypothesis_class=head, hypothesis_params=params)


# name -> (builder, input channels, output channels, logits on the CPU, (focal weights, Tversky weights))
MODELS = {"unet": (_unet, 2, 3, lambda sd, x: S.unet_logits(sd, SPEC, x), ([1, 2, 3], [0, 1, 1])),
          "nested": (_nested, 3, 2, S.nested_logits, ([1, 5], None))}
MODEL_CFG = dict(tversky_weight=0.5, alpha=0.3, beta=0.7, tversky_power=0.75, focal_gamma=2.0)


def _batch(cin, cout, seed=1234):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, cin, 16, 16, 16), generator=g)
    lab = torch.randint(0, cout, (1, 16, 16, 16), generator=g)
    return x, torch.nn.functional.one_hot(lab, cout).permute(0, 4, 1, 2, 3).float().contiguous()


def _train_step(model, crit, x, y):
    model.zero_grad(set_to_none=True)
    out = model(x)
    ld = crit(out, y)
    ld["loss"].backward()
    return out.detach(), ld["loss"].detach(), {k: v.grad.detach().clone() for k, v in model.named_parameters()}


def _criterion(name, from_logits):
    w, v = MODELS[name][4]
    return HybridFocalTverskyLoss(logistic_class_weights=w, tversky_class_weights=v, from_logits=from_logits, **MODEL_CFG)


@pytest.fixture(scope="module")
def fp32_steps():
    """(model name, from_logits) -> (state_dict before, model, x, y, output, loss, gradients) of one fp32-flow step"""
    steps = {}
    for name, (make, cin, cout, _, _) in MODELS.items():
        for from_logits in MODES:
            model = make(from_logits).cuda().train()
            sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
            x, y = _batch(cin, cout)
            steps[name, from_logits] = (sd0, model, x, y) + _train_step(model, _criterion(name, from_logits), x.cuda(), y.cuda())
    return steps


@pytest.mark.parametrize("from_logits", MODES, ids=["softmax_head_prob", "identity_head_logits"])
@pytest.mark.parametrize("name", list(MODELS))
def test_model_fp32_flow_matches_the_cpu(fp32_steps, name, from_logits):
    """one training step against the CPU formulation (the oracle's forward up to the logits, torch.softmax, the formulas of
    focal_tversky_ref) at the bounds of tests/test_binary_loss_gpu.py: probabilities and loss within 1e-4, every parameter
    gradient within 1e-3 * max |g_ref| + 1e-7.  The Identity head's probabilities are the softmax of its logits."""
    sd0, model, x, y, out, loss, grads = fp32_steps[name, from_logits]
    names = {k for k, _ in model.named_parameters()}
    sd = {k: v.clone().requires_grad_(k in names) for k, v in sd0.items()}
    logits_ref = MODELS[name][3](sd, x)
    p_ref = torch.softmax(logits_ref, dim=1)
    w, v = MODELS[name][4]
    loss_ref = F.focal_tversky(logits_ref if from_logits else p_ref, y, focal_class_weights=w, tversky_class_weights=v,
                               from_logits=from_logits, **MODEL_CFG)["loss"]
    loss_ref.backward()
    p = torch.softmax(out.cpu(), dim=1) if from_logits else out.cpu()
    err = (p - p_ref.detach()).abs().max().item()
    gerr = max(((grads[k].cpu() - sd[k].grad).abs().max() / (1e-3 * sd[k].grad.abs().max() + 1e-7)).item() for k in names)
    print(f"focal_tversky_accuracy {name} {'identity head, logits' if from_logits else 'softmax head, prob'} fp32 flow vs CPU: "
          f"max |dp| {err:.3e}, loss {loss.item():.6f} vs {loss_ref.item():.6f}, worst gradient error / bound {gerr:.3f}")
    assert set(grads) == names and len(names) > 10
    assert err <= 1e-4
    assert abs(loss.item() - loss_ref.item()) <= 1e-4
    for k in sorted(names):
        g_ref = sd[k].grad
        assert (grads[k].cpu() - g_ref).abs().max().item() <= 1e-3 * g_ref.abs().max().item() + 1e-7, k


@pytest.mark.parametrize("prec,from_logits", [("bf16", True), ("fp16", False)], ids=["bf16_logits", "fp16_prob"])
def test_unet_16bit_training_step(fp32_steps, prec, from_logits):
    """one c8-flow training step of the ModularUNet at the bounds tests/test_binary_loss_gpu.py holds its own to: every
    parameter gradient finite, worst cosine with the fp32-flow gradient >= 0.95, the fp16 step (on its calibrated loss
    scale) leaves the overflow word clear"""
    import segmentation_pipeline_amd as sp
    _, model, x, y, _, loss32, grads32 = fp32_steps["unet", from_logits]
    m = copy.deepcopy(model).train()
    with sp.precision(prec):
        ops.fp16_overflow()
        _, loss, grads = _train_step(m, _criterion("unet", from_logits), x.cuda(), y.cuda())
        if prec == "fp16":
            assert ops.fp16_overflow() == 0
    worst_cos = (2.0, None)
    for k, g32 in grads32.items():
        a, b = grads[k].double().flatten(), g32.double().flatten()
        assert torch.isfinite(a).all(), k
        worst_cos = min(worst_cos, (float(a @ b / (a.norm() * b.norm() + 1e-300)), k))
    print(f"focal_tversky_accuracy unet {prec} {'logits' if from_logits else 'prob'}: c8 training flow, loss {loss.item():.6f} "
          f"(fp32 flow {loss32.item():.6f}), worst parameter cosine with the fp32 flow {worst_cos[0]:.4f} ({worst_cos[1]})")
    assert bool(torch.isfinite(loss))
    assert worst_cos[0] >= 0.95, worst_cos


@pytest.mark.parametrize("from_logits", MODES, ids=["prob", "logits"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_graphed_train_step_reproduces_the_eager_losses(prec, from_logits):
    """trainer.GraphedTrainStep with the new criterion: two eager warm-up steps, then two replayed ones; the loss dicts
    equal those of four eager steps from the same seed bit for bit -- nothing in the criterion synchronises"""
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd.trainer import GraphedTrainStep
    m_e = _unet(from_logits).cuda().train()
    m_g = copy.deepcopy(m_e)
    batches = []
    for i in range(4):
        x, y = _batch(2, 3, seed=100 + i)
        batches.append({"X": x.cuda(), "y": y.cuda()})
    crit = HybridFocalTverskyLoss(0.3, 0.3, 0.7, 0.75, 2.0, [1, 2, 3], [0, 1, 1], from_logits)
    with sp.precision(prec):
        opt_e = torch.optim.SGD(m_e.parameters(), lr=1e-2, momentum=0.9)
        opt_g = torch.optim.SGD(m_g.parameters(), lr=1e-2, momentum=0.9)
        step = GraphedTrainStep(m_g, crit, opt_g, warmup=2)
        losses_e, losses_g = [], []
        for b in batches:
            opt_e.zero_grad(set_to_none=True)
            ld = crit(m_e(b["X"]), b["y"])
            ld["loss"].backward()
            opt_e.step()
            losses_e.append(torch.stack([v.detach().clone() for v in ld.values()]))
            losses_g.append(torch.stack([v.detach().clone() for v in step(b).values()]))
    assert torch.equal(torch.stack(losses_e), torch.stack(losses_g))
    assert len(step._graphs) == 1 and next(iter(step._graphs.values()))["graph"] is not None
