"""HybridBinaryLogisticDiceLoss on the device: m355_binary_loss_fwd / _bwd in both modes against the fp64 formulas of
tests/binary_loss_ref.py, saturated inputs, determinism and memory safety, the Dice term against m355_hybrid_loss_fwd bit for
bit, the models with the Sigmoid and the Identity head in the three activation flows, and the captured train step.
The lines starting with `binary_loss_accuracy` are what profiles/binary_loss_accuracy.txt records."""
import copy
from functools import partial

import pytest
import torch
from torch import nn

import binary_loss_ref as B
import sigmoid_ref as S
from oracle import torch_ref as R
from segmentation_pipeline_amd import ops
from segmentation_pipeline_amd.criterions import HybridBinaryLogisticDiceLoss
from segmentation_pipeline_amd.models import ModularUNet, NestedResUNet

pytestmark = pytest.mark.gpu

# (dice_weight, logistic_class_weights, pos_weight, square_dice); a case of fewer than 3 channels takes the first C weights
CONFIGS = [(0.5, None, None, True), (0.3, [1, 2, 3], [1, 5, 0.5], False), (0.5, [1, 100, 1], [2, 2, 2], True)]
MODES = [False, True]
# name -> (shape, soft target).  (2, 3, 9, 10, 11): S = 990, a multiple of neither 4 nor 256, less than one chunk;
# (.., 17, 33, 31): S = 17391, odd, two chunks of 16384, the second ragged
CASES = {"small": ((2, 3, 9, 10, 11), False), "large": ((1, 2, 17, 33, 31), False), "c1": ((1, 1, 17, 33, 31), False),
         "soft": ((1, 2, 17, 33, 31), True)}
DLOSS = 0.7


def cfg_kwargs(cfg, channels, from_logits):
    dw, cw, pw, sq = cfg
    return dict(dice_weight=dw, class_weights=None if cw is None else cw[:channels],
                pos_weight=None if pw is None else pw[:channels], square_dice=sq, from_logits=from_logits)


def close(got, ref, rtol, atol, what, torch32=None):
    """tests/test_kernels_gpu.py's close(): max |got - ref| <= atol + rtol * max |ref|; prints the figure first"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, bound = (got - ref).abs().max().item(), atol + rtol * ref.abs().max().item()
    t32 = "" if torch32 is None else f"  torch fp32 on the CPU {(torch32.double() - ref).abs().max().item():.3e}"
    print(f"binary_loss_accuracy {what}: max err {err:.3e}  bound {bound:.3e}{t32}")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def inputs(case):
    """(z, p, t) on the host: z = randn * 2, p = sigmoid(z), t = (rand < 0.3) or rand"""
    shape, soft = CASES[case]
    g = torch.Generator().manual_seed(sorted(CASES).index(case) + 1)
    z = torch.randn(shape, generator=g) * 2
    u = torch.rand(shape, generator=g)
    return z, torch.sigmoid(z), (u if soft else (u < 0.3).float())


_expected = {}


def expected(case, ci, from_logits):
    """the fp64 values and the fp32 torch figures of one (case, configuration, mode), computed once"""
    key = (case, ci, from_logits)
    if key not in _expected:
        z, p, t = inputs(case)
        x = z if from_logits else p
        kw = cfg_kwargs(CONFIGS[ci], x.shape[1], from_logits)
        _expected[key] = (x, t, kw, B.expected(x, t, DLOSS, **kw), B.torch32(x, t, DLOSS, **kw))
    return _expected[key]


# ------------------------------------------------------------------------------------------------ kernels against fp64
@pytest.mark.parametrize("from_logits", MODES, ids=["prob", "logits"])
@pytest.mark.parametrize("ci", range(len(CONFIGS)))
@pytest.mark.parametrize("case", list(CASES))
def test_fwd_bwd_against_fp64(case, ci, from_logits):
    """out3 within close(2e-6, 1e-7), sums within close(2e-6, 1e-6), the gradient for dloss = 0.7 (from the device's own
    sums) within close(1e-5, 1e-9): the bounds of test_hybrid_loss_fwd_bwd"""
    x, t, kw, (out3_ref, sums_ref, dx_ref), (out3_32, sums_32, dx_32) = expected(case, ci, from_logits)
    tag = f"{case} cfg{ci} {'logits' if from_logits else 'prob'}"
    xd, td = x.cuda(), t.cuda()
    out3, sums = B.raw_fwd(xd, td, **kw)
    dx = B.raw_bwd(xd, td, sums, DLOSS, **kw)
    close(out3, out3_ref, 2e-6, 1e-7, f"{tag} out3", out3_32)
    close(sums, sums_ref, 2e-6, 1e-6, f"{tag} sums", sums_32)
    close(dx, dx_ref, 1e-5, 1e-9, f"{tag} dx", dx_32)
    assert bool(torch.isfinite(out3).all()) and bool(torch.isfinite(dx).all())


@pytest.mark.parametrize("from_logits", MODES, ids=["prob", "logits"])
def test_autograd_function_matches_the_entry_points(from_logits):
    """the criterion through ops.binary_logistic_dice_loss: the bits of the raw calls, three 0-dim fp32 tensors, the
    gradient through 'loss' only"""
    x, t, kw, _, _ = expected("small", 1, from_logits)
    dw, cw, pw, sq = CONFIGS[1]
    crit = HybridBinaryLogisticDiceLoss(dw, cw, pw, sq, from_logits)
    xd = x.cuda().requires_grad_(True)
    ld = crit(xd, t.cuda())
    assert list(ld) == ['loss', 'dice_loss', 'logistic_loss']
    assert all(v.shape == () and v.dtype == torch.float32 and v.is_cuda for v in ld.values())
    assert ld['loss'].requires_grad and not ld['dice_loss'].requires_grad and not ld['logistic_loss'].requires_grad
    (ld['loss'] * DLOSS).backward()
    out3, sums = B.raw_fwd(x.cuda(), t.cuda(), **kw)
    assert torch.equal(torch.stack([v.detach() for v in ld.values()]), out3)
    assert torch.equal(xd.grad, B.raw_bwd(x.cuda(), t.cuda(), sums, DLOSS, **kw))
    assert set(crit._uploaded) == {"logistic_class_weights", "pos_weight"}


# ------------------------------------------------------------------------------------------------ saturation
def _combos(values):
    """every value against t = 0 and t = 1, as two channels of S = 2 * len(values) in different orders"""
    v = torch.tensor(values, dtype=torch.float32)
    x = torch.cat([v, v])
    t = torch.cat([torch.zeros(len(values)), torch.ones(len(values))])
    return torch.stack([x, x.flip(0)])[None].contiguous(), torch.stack([t, t.roll(3)])[None].contiguous()


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_saturated_probabilities(ci):
    """prob mode at p in {0, 1, 1e-8, 1 - 6e-8, 0.5, 1e-30} against t in {0, 1}: everything finite, every gradient entry
    within 1e-5 of its own fp64 value"""
    x, t = _combos([0.0, 1.0, 1e-8, 1.0 - 6e-8, 0.5, 1e-30])
    kw = cfg_kwargs(CONFIGS[ci], 2, False)
    out3_ref, _, dx_ref = B.expected(x, t, DLOSS, **kw)
    out3, sums = B.raw_fwd(x.cuda(), t.cuda(), **kw)
    dx = B.raw_bwd(x.cuda(), t.cuda(), sums, DLOSS, **kw).cpu().double()
    assert bool(torch.isfinite(out3).all()) and bool(torch.isfinite(sums).all()) and bool(torch.isfinite(dx).all())
    rel = ((dx - dx_ref).abs() / dx_ref.abs()).max().item()
    loss_rel = abs(out3[0].item() - out3_ref[0].item()) / abs(out3_ref[0].item())
    print(f"binary_loss_accuracy saturated prob cfg{ci}: worst relative gradient error {rel:.3e} (bound 1e-5), "
          f"loss relative error {loss_rel:.3e}")
    assert bool((dx_ref != 0).all())
    assert rel <= 1e-5
    close(out3, out3_ref, 2e-6, 1e-7, f"saturated prob cfg{ci} out3")


LOGITS = [0.0, 20.0, -20.0, 88.0, -88.0, 90.0, -90.0, 104.0, -104.0]


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_saturated_logits(ci):
    """logits mode at z in {0, +-20, +-88, +-90, +-104} against t in {0, 1}: everything finite, the loss within 2e-6
    relative, gradient entries within 1e-5 * max |ref|; a saturated wrong voxel keeps a gradient"""
    x, t = _combos(LOGITS)
    kw = cfg_kwargs(CONFIGS[ci], 2, True)
    out3_ref, _, dx_ref = B.expected(x, t, DLOSS, **kw)
    out3, sums = B.raw_fwd(x.cuda(), t.cuda(), **kw)
    dx = B.raw_bwd(x.cuda(), t.cuda(), sums, DLOSS, **kw)
    assert bool(torch.isfinite(out3).all()) and bool(torch.isfinite(sums).all()) and bool(torch.isfinite(dx).all())
    loss_rel = abs(out3[0].item() - out3_ref[0].item()) / abs(out3_ref[0].item())
    print(f"binary_loss_accuracy saturated logits cfg{ci}: loss relative error {loss_rel:.3e} (bound 2e-6)")
    assert loss_rel <= 2e-6
    close(dx, dx_ref, 1e-5, 0.0, f"saturated logits cfg{ci} dx")
    wrong = (x[0, 0] == 104.0) & (t[0, 0] == 0)          # p == 1 against t == 0: a sigmoid's own backward gives 0 here
    assert bool(wrong.any()) and bool((dx.cpu()[0, 0][wrong] > 0).all())


def test_the_loss_uses_the_librarys_sigmoid():
    """p inside the loss is m355_sigmoid_fwd(z) bit for bit: the saved sum of p of one-voxel rows (square_dice off)"""
    z = torch.tensor(LOGITS + [1.0, -1.0, 1e-6, -3.3, 7.7], dtype=torch.float32).reshape(-1, 1, 1).cuda()
    t = torch.ones_like(z)
    _, sums = B.raw_fwd(z, t, square_dice=False, from_logits=True)
    p = S.SigmoidOps("hip").sigmoid_fwd(z.flatten())
    assert torch.equal(sums.view(-1, 5)[:, 1], p)
    assert torch.equal(sums.view(-1, 5)[:, 0], p)        # sum p t with t == 1


# ------------------------------------------------------------------------------------------------ determinism, memory
@pytest.mark.parametrize("from_logits", MODES, ids=["prob", "logits"])
def test_determinism_guards_and_misaligned_views(from_logits):
    """two calls give the same bits; a dx buffer keeps its guard elements; views offset by one element (not 16-byte
    aligned) give the bits of their aligned clones"""
    x, t, kw, _, _ = expected("large", 1, from_logits)
    n = x.numel()
    xd, td = x.cuda(), t.cuda()
    out3, sums = B.raw_fwd(xd, td, **kw)
    out3_b, sums_b = B.raw_fwd(xd, td, **kw)
    assert torch.equal(out3, out3_b) and torch.equal(sums, sums_b)
    guard = 64
    buf = torch.full((n + 2 * guard,), 7.0, device="cuda")
    dx = B.raw_bwd(xd, td, sums, DLOSS, out=buf[guard:guard + n].view(x.shape), **kw)
    assert bool((buf[:guard] == 7.0).all()) and bool((buf[guard + n:] == 7.0).all())
    assert torch.equal(dx, B.raw_bwd(xd, td, sums, DLOSS, **kw))
    # offset by one element
    xb, tb = torch.zeros(n + 8, device="cuda"), torch.zeros(n + 8, device="cuda")
    xb[1:1 + n], tb[1:1 + n] = xd.flatten(), td.flatten()
    xo, to = xb[1:1 + n].view(x.shape), tb[1:1 + n].view(x.shape)
    assert xo.data_ptr() % 16 != 0 and to.data_ptr() % 16 != 0 and xd.data_ptr() % 16 == 0
    out3_o, sums_o = B.raw_fwd(xo, to, **kw)
    assert torch.equal(out3_o, out3) and torch.equal(sums_o, sums)
    buf_o = torch.full((n + 2 * guard + 1,), 7.0, device="cuda")
    dx_o = B.raw_bwd(xo, to, sums, DLOSS, out=buf_o[guard + 1:guard + 1 + n].view(x.shape), **kw)
    assert dx_o.data_ptr() % 16 != 0
    assert torch.equal(dx_o, dx)
    assert bool((buf_o[:guard + 1] == 7.0).all()) and bool((buf_o[guard + 1 + n:] == 7.0).all())


@pytest.mark.parametrize("square_dice", [True, False])
@pytest.mark.parametrize("shape", [(2, 3, 9, 10, 11), (1, 2, 17, 33, 31)], ids=["small", "large"])
def test_dice_term_is_the_softmax_losss(hip, shape, square_dice):
    """pos_weight=None, from_logits=False, a one-hot target: dice_loss has the bits of m355_hybrid_loss_fwd's, and so
    have the three Dice sums"""
    g = torch.Generator().manual_seed(5)
    p = torch.softmax(torch.randn(shape, generator=g) * 2, dim=1)
    lab = torch.randint(0, shape[1], (shape[0],) + shape[2:], generator=g)
    t = torch.nn.functional.one_hot(lab, shape[1]).permute(0, 4, 1, 2, 3).float().contiguous()
    out3, sums = B.raw_fwd(p.cuda(), t.cuda(), dice_weight=0.5, square_dice=square_dice)
    out3_s, sums_s = hip.loss_fwd(p, t, 0.5, None, square_dice)
    assert torch.equal(out3[1], out3_s[1])
    assert torch.equal(sums.view(-1, 5)[:, :3], sums_s.view(-1, 4)[:, :3])


# ------------------------------------------------------------------------------------------------ models
FILTERS = [8, 16]
SPEC = R.UNetSpec(2, 3, FILTERS, 2, norm="group", groups=4, hypothesis="none")


def _unet(head):
    torch.manual_seed(0)
    return ModularUNet(2, 3, FILTERS, 2, block_params={'normalization_class': partial(nn.GroupNorm, 4)},
                       hypothesis_class=head, hypothesis_params={})


def _nested(head):
    torch.manual_seed(0)
    return NestedResUNet(3, 2, 8, hypothesis_class=head, hypothesis_params={})


MODELS = {"unet": (_unet, 2, 3, lambda sd, x: S.unet_logits(sd, SPEC, x), [1, 5, 0.5]),
          "nested": (_nested, 3, 2, S.nested_logits, [2, 0.5])}


def _batch(cin, cout, seed=1234):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, cin, 16, 16, 16), generator=g)
    y = (torch.rand((1, cout, 16, 16, 16), generator=g) < 0.4).float()
    return x, y


def _train_step(model, crit, x, y):
    model.zero_grad(set_to_none=True)
    out = model(x)
    ld = crit(out, y)
    ld["loss"].backward()
    return out.detach(), ld["loss"].detach(), {k: v.grad.detach().clone() for k, v in model.named_parameters()}


def _criterion(name, from_logits):
    return HybridBinaryLogisticDiceLoss(pos_weight=MODELS[name][4], from_logits=from_logits)


@pytest.fixture(scope="module")
def fp32_steps():
    """(model name, from_logits) -> (state_dict before, model, x, y, output, loss, gradients) of one fp32-flow step"""
    steps = {}
    for name, (make, cin, cout, _, _) in MODELS.items():
        for from_logits in MODES:
            model = make(nn.Identity if from_logits else nn.Sigmoid).cuda().train()
            sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
            x, y = _batch(cin, cout)
            steps[name, from_logits] = (sd0, model, x, y) + _train_step(model, _criterion(name, from_logits), x.cuda(), y.cuda())
    return steps


@pytest.mark.parametrize("from_logits", MODES, ids=["sigmoid_head_prob", "identity_head_logits"])
@pytest.mark.parametrize("name", list(MODELS))
def test_model_fp32_flow_matches_the_cpu(fp32_steps, name, from_logits):
    """one training step against the CPU formulation (the oracle's forward up to the logits, torch.sigmoid, the formulas of
    binary_loss_ref) at the bounds of tests/test_sigmoid_head_gpu.py: probabilities and loss within 1e-4, every parameter
    gradient within 1e-3 * max |g_ref| + 1e-7.  The Identity head's probabilities are the sigmoid of its logits."""
    sd0, model, x, y, out, loss, grads = fp32_steps[name, from_logits]
    names = {k for k, _ in model.named_parameters()}
    sd = {k: v.clone().requires_grad_(k in names) for k, v in sd0.items()}
    logits_ref = MODELS[name][3](sd, x)
    p_ref = torch.sigmoid(logits_ref)
    loss_ref = B.binary_loss(logits_ref if from_logits else p_ref, y, pos_weight=MODELS[name][4],
                             from_logits=from_logits)["loss"]
    loss_ref.backward()
    p = torch.sigmoid(out.cpu()) if from_logits else out.cpu()
    err = (p - p_ref.detach()).abs().max().item()
    gerr = max(((grads[k].cpu() - sd[k].grad).abs().max() / (1e-3 * sd[k].grad.abs().max() + 1e-7)).item() for k in names)
    print(f"binary_loss_accuracy {name} {'identity head, logits' if from_logits else 'sigmoid head, prob'} fp32 flow vs CPU: "
          f"max |dp| {err:.3e}, loss {loss.item():.6f} vs {loss_ref.item():.6f}, worst gradient error / bound {gerr:.3f}")
    assert set(grads) == names and len(names) > 10
    assert err <= 1e-4
    assert abs(loss.item() - loss_ref.item()) <= 1e-4
    for k in sorted(names):
        g_ref = sd[k].grad
        assert (grads[k].cpu() - g_ref).abs().max().item() <= 1e-3 * g_ref.abs().max().item() + 1e-7, k


@pytest.mark.parametrize("from_logits", MODES, ids=["sigmoid_head_prob", "identity_head_logits"])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_unet_16bit_training_step(fp32_steps, prec, from_logits):
    """one c8-flow training step of the ModularUNet at the bounds tests/test_sigmoid_head_gpu.py holds its own to: every
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
    print(f"binary_loss_accuracy unet {prec} {'logits' if from_logits else 'prob'}: c8 training flow, loss {loss.item():.6f} "
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
    m_e = _unet(nn.Identity if from_logits else nn.Sigmoid).cuda().train()
    m_g = copy.deepcopy(m_e)
    batches = []
    for i in range(4):
        x, y = _batch(2, 3, seed=100 + i)
        batches.append({"X": x.cuda(), "y": y.cuda()})
    crit = HybridBinaryLogisticDiceLoss(0.3, [1, 2, 3], [1, 5, 0.5], True, from_logits)
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
