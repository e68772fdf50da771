"""nn.Sigmoid as hypothesis_class on the device: the stand-alone kernels against fp64, the M355_CONV_SIGMOID epilogue of the
three output-convolution kernels bit for bit against convolution + m355_sigmoid_fwd and against the oracle, the unfused route
with its gradients, the models in the three activation flows, the captured train step and sliding-window prediction.
The lines starting with `sigmoid_head_accuracy` are what profiles/sigmoid_head_accuracy.txt records."""
import copy
import ctypes as C
from functools import partial

import pytest
import torch
from torch import nn

import sigmoid_ref as S
from oracle import torch_ref as R
from segmentation_pipeline_amd import _lib, ops
from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss
from segmentation_pipeline_amd.models import ModularUNet, NestedResUNet

pytestmark = pytest.mark.gpu


def rnd(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def close(got, ref, rtol, atol, what, torch32=None):
    """tests/test_kernels_gpu.py's close(): max |got - ref| <= atol + rtol * max |ref|; prints the figure first"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, bound = (got - ref).abs().max().item(), atol + rtol * ref.abs().max().item()
    t32 = "" if torch32 is None else f"  torch fp32 on the CPU {(torch32.double() - ref).abs().max().item():.3e}"
    print(f"sigmoid_head_accuracy {what}: max err {err:.3e}  bound {bound:.3e}{t32}")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


@pytest.fixture(scope="module")
def hip():
    return S.SigmoidOps("hip")


# ------------------------------------------------------------------------------------------------ stand-alone kernels
N_EL = 4099      # 1024 float4 + a tail of 3; more than one block of the float4 grid and of the scalar grid


@pytest.mark.parametrize("layout", ["aligned", "offset_by_one"])
def test_stand_alone_kernels(hip, layout):
    """m355_sigmoid_fwd against torch.sigmoid in fp64, m355_sigmoid_bwd against dy * y * (1 - y) in fp64 from the device's
    own y, both at close(2e-5, 1e-6) -- the bound of the softmax epilogue test; every output finite and in [0, 1].  The view
    offset by one element is not 16-byte aligned: the scalar kernels."""
    x = rnd(N_EL, seed=1) * 4.0
    for k, v in enumerate(S.PLANTED):
        x[(k * 311 + 5) % N_EL] = v
    dy = rnd(N_EL, seed=2)
    off = 1 if layout == "offset_by_one" else 0

    def dev(t):
        buf = torch.full((N_EL + 8,), float("nan"), device="cuda")
        buf[off:off + N_EL] = t.cuda()
        return buf, buf[off:off + N_EL]
    (_, xd), (_, dyd) = dev(x), dev(dy)
    ybuf, dxbuf = torch.full((N_EL + 8,), 7.0, device="cuda"), torch.full((N_EL + 8,), 7.0, device="cuda")
    yd, dxd = ybuf[off:off + N_EL], dxbuf[off:off + N_EL]
    assert (xd.data_ptr() % 16 == 0) == (off == 0) and (yd.data_ptr() % 16 == 0) == (off == 0)
    hip.sigmoid_fwd(xd, out=yd)
    hip.sigmoid_bwd(yd, dyd, out=dxd)
    torch.cuda.synchronize()
    y, dx = yd.cpu(), dxd.cpu()
    # nothing outside the n elements is written
    assert bool((ybuf[:off] == 7.0).all()) and bool((ybuf[off + N_EL:] == 7.0).all())
    assert bool((dxbuf[:off] == 7.0).all()) and bool((dxbuf[off + N_EL:] == 7.0).all())
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    assert y.min().item() >= 0.0 and y.max().item() <= 1.0
    ref = torch.sigmoid(x.double())
    close(y, ref, 2e-5, 1e-6, f"sigmoid_fwd {layout}", torch.sigmoid(x))
    ref_dx = dy.double() * y.double() * (1.0 - y.double())
    close(dx, ref_dx, 2e-5, 1e-6, f"sigmoid_bwd {layout}", dy * y * (1.0 - y))
    planted = {v: y[(k * 311 + 5) % N_EL].item() for k, v in enumerate(S.PLANTED)}
    assert planted[0.0] == 0.5 and planted[-90.0] == 0.0 and planted[-104.0] == 0.0 and planted[90.0] == 1.0
    assert 0.0 <= planted[-88.0] < 1e-37    # 1 / (1 + e^88) = 6e-39 is below the smallest normal fp32


def test_aligned_and_scalar_kernels_agree(hip):
    """the float4 body, its scalar tail and the scalar kernel evaluate one expression: the same bits"""
    x = (rnd(N_EL + 1, seed=3) * 6.0).cuda()
    dy = rnd(N_EL + 1, seed=4).cuda()
    ys = torch.empty(N_EL + 1, device="cuda")
    hip.sigmoid_fwd(x[1:], out=ys[1:])                      # misaligned input and output: the scalar kernel
    assert torch.equal(ys[1:], hip.sigmoid_fwd(x[1:].clone()))     # float4 body + tail of 3
    assert torch.equal(hip.sigmoid_fwd(x[:N_EL].clone()), hip.sigmoid_fwd(x.clone())[:N_EL])   # tail elements == body elements
    dxs = torch.empty(N_EL + 1, device="cuda")
    hip.sigmoid_bwd(ys[1:], dy[1:], out=dxs[1:])
    assert torch.equal(dxs[1:], hip.sigmoid_bwd(ys[1:].clone(), dy[1:].clone()))


# ------------------------------------------------------------------------------------------------ fused epilogues
# (N, Cin, Cout, D, H, W); the last is the binary head, with ragged rows
HEAD_SHAPES = [(1, 32, 3, 8, 16, 64), (2, 8, 2, 9, 10, 36), (1, 16, 4, 8, 8, 32), (2, 40, 1, 5, 7, 64)]


def _operands(shape):
    N, ci, co, D, H, W = shape
    return rnd(N, ci, D, H, W, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * 0.2, rnd(co, seed=3)


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_out_conv_sigmoid_fused_epilogue(hip, oracle, shape):
    """fp32: the head of conv3_valu_smallcout_kernel gives the very bits of m355_conv3d_fwd followed by m355_sigmoid_fwd
    and matches the oracle's convolution -> torch.sigmoid in fp64 at the softmax test's bounds.  The library fuses a head in
    fp32 only from D >= 8 on (small_cout_fwd): the binary case (D = 5) is refused with the flag and takes the pair inside
    ops.conv3d(sigmoid=True) -- the same two checks hold for what that call returns."""
    x, w, b = _operands(shape)
    N, ci, co, D, H, W = shape
    pair = hip.sigmoid_fwd(hip.conv3d_fwd(x, w, b))
    d = hip.conv_desc((N, ci, D, H, W), co, 3, 1, 1)
    fuses = bool(hip.lib.m355_conv3d_fuses_sigmoid(C.byref(d)))
    assert fuses == (D >= 8)
    if fuses:
        fused = hip.conv3d_fwd(x, w, b, sigmoid=True)
        assert torch.equal(fused, pair)
    else:
        with pytest.raises(RuntimeError, match="SIGMOID"):
            _flagged_call(hip, x, w, b)
    with torch.no_grad():
        through_ops = ops.conv3d(x.cuda(), w.cuda(), b.cuda(), sigmoid=True)
    assert torch.equal(through_ops, pair)
    close(through_ops, torch.sigmoid(oracle.conv3d_fwd(x, w, b).double()), 2e-5, 1e-6, f"conv + sigmoid fp32 {shape}")
    assert through_ops.min().item() >= 0.0 and through_ops.max().item() <= 1.0


def _flagged_call(hip, x, w, b):
    """m355_conv3d_fwd with M355_CONV_SIGMOID on a descriptor that does not fuse it (no assertion in front)"""
    hip._head_flag = _lib.CONV_SIGMOID
    try:
        return S.RawOps.conv3d_fwd(hip, x, w, b)
    finally:
        hip._head_flag = 0


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_out_conv_sigmoid_fused_epilogue_16bit(hip, oracle, compute, tuning):
    """conv3_h16_kernel's sigmoid instantiations (queue-driven 4-wave / 8-wave, one-shot): bit equality with the same
    convolution followed by m355_sigmoid_fwd, close(1e-4, 1e-5) against the oracle on equally rounded operands"""
    reached = set()
    for w8, one in ((0, 3), (2, 3), (0, 1)):
        tuning(M355_H16_W8=w8, M355_H16_ONESHOT=one, M355_CONV_KSPLIT=1)
        for shape in HEAD_SHAPES:
            N, ci, co, D, H, W = shape
            x, w, b = _operands(shape)
            x16 = hip.act16_pack(x, compute)
            reached.add(hip.conv_launch_plan(4, (N, ci, D, H, W), co, compute=compute, flags=_lib.CONV_SIGMOID)[0])
            fused = hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute, sigmoid=True)
            assert torch.equal(fused, hip.sigmoid_fwd(hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute))), (w8, one, shape)
            close(fused, torch.sigmoid(oracle.conv3d_fwd(x, w, b, compute=compute).double()), 1e-4, 1e-5,
                  f"conv + sigmoid {('bf16', 'fp16')[compute - 1]} w8={w8} oneshot={one} {shape}")
    assert reached == {6, 7, 8}, reached     # H16Queue, H16Queue8, H16OneShot: each SIGMOID instantiation family ran


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
def test_out_conv_sigmoid_on_the_cout4_kernel_16bit(hip, oracle, compute, tuning):
    """conv3_cout4_h16_kernel at the settings of test_out_conv_tap_rows_on_the_m_side_16bit"""
    for shape in [(1, 32, 3, 8, 16, 64), (2, 40, 1, 5, 7, 64), (1, 24, 4, 9, 10, 32), (1, 8, 2, 4, 4, 96)]:
        N, ci, co, D, H, W = shape
        x, w, b = _operands(shape)
        x16 = hip.act16_pack(x, compute)
        tuning(M355_NO_SMALL=0, M355_CONV_KSPLIT=1, M355_CONV_NTW=4)
        plan = hip.conv_plan((N, ci, D, H, W), co, compute=compute)
        assert plan[1] == 4 and plan[2] == 32, plan
        lp = hip.conv_launch_plan(4, (N, ci, D, H, W), co, compute=compute, flags=_lib.CONV_SIGMOID)
        assert lp[0] == 10, lp                      # H16Cout4
        y = hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute)
        fused = hip.conv3d_fwd_h16(x16, ci, (D, H, W), w, b, compute=compute, sigmoid=True)
        assert torch.equal(fused, hip.sigmoid_fwd(y))
        close(fused, torch.sigmoid(oracle.conv3d_fwd(x, w, b, compute=compute).double()), 1e-4, 1e-5,
              f"conv + sigmoid cout4 {('bf16', 'fp16')[compute - 1]} {shape}")
    tuning(M355_NO_SMALL=0)


# ------------------------------------------------------------------------------------------------ unfused route
def test_unfused_route_and_its_gradients():
    """Cout = 6: no epilogue; ops.conv3d(sigmoid=True) is ops.sigmoid(ops.conv3d(...)) bit for bit, and the gradients of x, w
    and b agree with CPU autograd in fp64 within 2e-5 + 2e-5 * max |ref|"""
    N, ci, co, D, H, W = 1, 8, 6, 4, 6, 10
    x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * 0.2, rnd(co, seed=3)
    g = rnd(N, co, D, H, W, seed=4)
    leaves = [t.cuda().requires_grad_(True) for t in (x, w, b)]
    y = ops.conv3d(*leaves, sigmoid=True)
    with torch.no_grad():
        assert torch.equal(y, ops.sigmoid(ops.conv3d(*[t.detach() for t in leaves])))
    y.backward(g.cuda())
    ref_leaves = [t.double().requires_grad_(True) for t in (x, w, b)]
    y_ref = torch.sigmoid(torch.nn.functional.conv3d(*ref_leaves, padding=1))
    y_ref.backward(g.double())
    close(y, y_ref, 2e-5, 1e-6, "unfused conv + sigmoid")
    for name, t, r in zip("xwb", leaves, ref_leaves):
        close(t.grad, r.grad, 2e-5, 2e-5, f"unfused route d{name}")
    # the stand-alone autograd function alone
    z = (rnd(3, 5, 7, seed=5) * 3).cuda().requires_grad_(True)
    ops.sigmoid(z).backward(torch.ones_like(z))
    zr = z.detach().cpu().double()
    close(z.grad, torch.sigmoid(zr) * (1 - torch.sigmoid(zr)), 2e-5, 1e-6, "ops.sigmoid backward")


# ------------------------------------------------------------------------------------------------ models
FILTERS = [8, 16, 16]


def _unet(out_channels=3, head=nn.Sigmoid, params=None):
    torch.manual_seed(0)        # (a head has no parameters: every hypothesis_class gives the same weights)
    return ModularUNet(2, out_channels, FILTERS, 3, block_params={'normalization_class': partial(nn.GroupNorm, 4)},
                       hypothesis_class=head, hypothesis_params={} if params is None else params)


def _nested(head=nn.Sigmoid, params=None):
    torch.manual_seed(0)
    return NestedResUNet(3, 2, 8, hypothesis_class=head, hypothesis_params={} if params is None else params)


def _batch(in_channels, out_channels, seed=1234):
    """a multi-label target: independent random binary masks per channel, not one-hot"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, in_channels, 16, 16, 16), generator=g)
    y = (torch.rand((1, out_channels, 16, 16, 16), generator=g) < 0.4).float()
    return x, y


def _train_step(model, x, y):
    model.zero_grad(set_to_none=True)
    p = model(x)
    ld = HybridLogisticDiceLoss()(p, y)
    ld["loss"].backward()
    return p.detach(), ld["loss"].detach(), {k: v.grad.detach().clone() for k, v in model.named_parameters()}


MODELS = {
    "unet3": (lambda: _unet(3), 2, 3,
              lambda sd, x: S.unet_logits(sd, R.UNetSpec(2, 3, FILTERS, 3, norm="group", groups=4, hypothesis="none"), x)),
    "unet1": (lambda: _unet(1), 2, 1,
              lambda sd, x: S.unet_logits(sd, R.UNetSpec(2, 1, FILTERS, 3, norm="group", groups=4, hypothesis="none"), x)),
    "nested": (_nested, 3, 2, S.nested_logits),
}


@pytest.fixture(scope="module")
def fp32_steps():
    """per model: (state_dict before, model, x, y, probabilities, loss, gradients) of one fp32-flow training step"""
    steps = {}
    for name, (make, cin, cout, _) in MODELS.items():
        model = make().cuda().train()
        sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        x, y = _batch(cin, cout)
        steps[name] = (sd0, model, x, y) + _train_step(model, x.cuda(), y.cuda())
    return steps


@pytest.mark.parametrize("name", list(MODELS))
def test_model_fp32_flow_matches_the_cpu(fp32_steps, name):
    """one training step with HybridLogisticDiceLoss on a multi-label target against the CPU formulation (the oracle's
    forward up to the logits, torch.sigmoid, the oracle's loss) at smoke()'s bounds: probabilities and loss within 1e-4,
    every parameter gradient within 1e-3 * max |g_ref| + 1e-7.  The channels do not sum to 1: no silent softmax."""
    sd0, model, x, y, p, loss, grads = fp32_steps[name]
    logits_fn = MODELS[name][3]
    names = {k for k, _ in model.named_parameters()}
    sd = {k: v.clone().requires_grad_(k in names) for k, v in sd0.items()}
    p_ref = torch.sigmoid(logits_fn(sd, x))
    loss_ref = R.hybrid_logistic_dice_loss(p_ref, y)["loss"]
    loss_ref.backward()
    err = (p.cpu() - p_ref.detach()).abs().max().item()
    gerr = max(((grads[k].cpu() - sd[k].grad).abs().max() / (1e-3 * sd[k].grad.abs().max() + 1e-7)).item() for k in names)
    print(f"sigmoid_head_accuracy {name} fp32 flow vs CPU: max |dp| {err:.3e}, loss {loss.item():.6f} vs {loss_ref.item():.6f}, "
          f"worst gradient error / bound {gerr:.3f}")
    assert set(grads) == names and len(names) > 10
    assert bool(torch.isfinite(p).all()) and p.min().item() >= 0.0 and p.max().item() <= 1.0
    assert err <= 1e-4
    assert abs(loss.item() - loss_ref.item()) <= 1e-4
    for k in sorted(names):
        g_ref = sd[k].grad
        assert (grads[k].cpu() - g_ref).abs().max().item() <= 1e-3 * g_ref.abs().max().item() + 1e-7, k
    assert (p.sum(1) - 1).abs().max().item() > 1e-3


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["unet3", "nested"])
def test_model_16bit_flows(fp32_steps, name, prec):
    """c8 no-grad flow: finite output in [0, 1], a non-zero distance to the fp32 flow of at most 2x that of the softmax twin
    of the same weights on the same input.  c8 training flow: every parameter gradient finite, worst cosine with the
    fp32-flow gradient >= 0.95; the fp16 step leaves the overflow word clear.
    NestedResUNet takes the no-grad part and the finiteness / overflow checks only: the per-parameter cosine is no property
    of the head there -- with the softmax head the same model's worst BatchNorm scale / shift gradient has a cosine of 0.40
    to 0.90 in bf16 and 0.92 to 0.99 in fp16 (one-hot and multi-label targets, N = 1 and 2), 0.60 to 0.97 and 0.89 to 0.99
    with the sigmoid head."""
    import segmentation_pipeline_amd as sp
    _, model, x, y, _, _, grads32 = fp32_steps[name]
    xd, yd = x.cuda(), y.cuda()
    twin = (_unet(3, nn.Softmax, {"dim": 1}) if name == "unet3" else _nested(nn.Softmax, {"dim": 1})).cuda()
    twin.load_state_dict(model.state_dict())
    dist = {}
    for tag, m in (("sigmoid", copy.deepcopy(model)), ("softmax", twin)):
        m.eval()
        with torch.no_grad():
            p32 = m(xd)
            with sp.precision(prec):
                p16 = m(xd)
        assert torch.isfinite(p16).all() and p16.min().item() >= 0.0 and p16.max().item() <= 1.0
        dist[tag] = (p16 - p32).abs().max().item()
    print(f"sigmoid_head_accuracy {name} {prec}: max |p16 - p32| {dist['sigmoid']:.4e}  softmax twin {dist['softmax']:.4e}  "
          f"ratio {dist['sigmoid'] / max(dist['softmax'], 1e-300):.2f}")
    assert dist["softmax"] > 0 and dist["sigmoid"] > 0, "the 16-bit mode must really run the 16-bit kernels"
    assert dist["sigmoid"] <= 2.0 * dist["softmax"], dist
    m = copy.deepcopy(model).train()
    with sp.precision(prec):
        ops.fp16_overflow()
        _, _, grads = _train_step(m, xd, yd)
        if prec == "fp16":
            assert ops.fp16_overflow() == 0
    worst_cos = (2.0, None)
    for k, g32 in grads32.items():
        a, b = grads[k].double().flatten(), g32.double().flatten()
        assert torch.isfinite(a).all(), k
        cos = float(a @ b / (a.norm() * b.norm() + 1e-300))
        worst_cos = min(worst_cos, (cos, k))
    print(f"sigmoid_head_accuracy {name} {prec}: c8 training flow, worst parameter cosine with the fp32 flow {worst_cos[0]:.4f} "
          f"({worst_cos[1]})")
    assert name == "nested" or worst_cos[0] >= 0.95, worst_cos


def test_fp16_calibration_tells_the_heads_apart():
    """the loss-scale calibration is keyed per head: a sigmoid head does not read the cell a softmax head of the same
    output convolution and shape has calibrated"""
    import segmentation_pipeline_amd as sp
    x, y = _batch(2, 3)
    m = _unet(3).cuda().train()
    with sp.precision("fp16"):
        ops.fp16_overflow()
        _train_step(m, x.cuda(), y.cuda())
    wid, shape = id(m.out_conv.weight), (1, 3, 16, 16, 16)
    assert (wid, shape, "sigmoid") in ops._fp16_calibration and (wid, shape) not in ops._fp16_calibration


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_graphed_train_step_reproduces_the_eager_losses(prec):
    """trainer.GraphedTrainStep on the sigmoid model: three eager warm-up steps, then two replayed ones; the losses equal
    those of five eager steps from the same seed"""
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd.trainer import GraphedTrainStep
    m_e = _unet(3).cuda().train()
    m_g = copy.deepcopy(m_e)
    batches = []
    for i in range(5):
        x, y = _batch(2, 3, seed=100 + i)
        batches.append({"X": x.cuda(), "y": y.cuda()})
    crit = HybridLogisticDiceLoss()
    with sp.precision(prec):
        opt_e = torch.optim.SGD(m_e.parameters(), lr=1e-2, momentum=0.9)
        opt_g = torch.optim.SGD(m_g.parameters(), lr=1e-2, momentum=0.9)
        step = GraphedTrainStep(m_g, crit, opt_g, warmup=3)
        losses_e, losses_g = [], []
        for b in batches:
            opt_e.zero_grad(set_to_none=True)
            ld = crit(m_e(b["X"]), b["y"])
            ld["loss"].backward()
            opt_e.step()
            losses_e.append(ld["loss"].detach().clone())
            losses_g.append(step(b)["loss"].detach().clone())
    assert torch.equal(torch.stack(losses_e), torch.stack(losses_g))
    assert len(step._graphs) == 1 and next(iter(step._graphs.values()))["graph"] is not None


def test_patch_predict_with_the_sigmoid_model():
    """PatchPredict(patch_size=8, patch_overlap=2, overlap_mode='average') over a 12^3 volume equals the manual tile loop
    through the same model (the same tile batches, the oracle's GridAggregator('average')).  Bound: a voxel is the fp32 sum of
    at most 8 values in [0, 1] divided by their count, in either order -- a few ulp of 1: 1e-6, as tests/test_distributed_cpu.py."""
    from segmentation_pipeline_amd.prediction import PatchPredict
    torch.manual_seed(0)
    model = ModularUNet(2, 3, [8, 16], 2, hypothesis_class=nn.Sigmoid, hypothesis_params={}).cuda().eval()
    vol = rnd(2, 12, 12, 12, seed=11).cuda()
    got = PatchPredict(patch_size=8, patch_overlap=2, overlap_mode="average", patch_batch_size=4).predict_volume(model, vol)
    locs = R.grid_locations((12, 12, 12), (8, 8, 8), (2, 2, 2))
    assert len(locs) == 8
    outs = []
    with torch.no_grad():
        for s in range(0, len(locs), 4):
            loc = torch.tensor(locs[s:s + 4], dtype=torch.int32, device="cuda")
            outs.append(model(ops.patch_gather(vol, loc, (8, 8, 8))))
    ref = R.aggregate_average(torch.cat(outs).cpu(), locs, (12, 12, 12))
    assert got.shape == ref.shape == (3, 12, 12, 12)
    err = (got.cpu() - ref).abs().max().item()
    print(f"sigmoid_head_accuracy PatchPredict average vs the manual tile loop: max err {err:.3e}")
    assert err <= 1e-6
    assert (got.sum(0) - 1).abs().max().item() > 1e-3
