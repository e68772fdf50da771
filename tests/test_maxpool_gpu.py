"""nn.MaxPool3d(2, 2) as downsample_class of ModularUNet (csrc/maxpool.hip): the four kernels bit for bit against stock
torch on the CPU (value, route, gradient; ties, NaN, -inf and signed zeros planted), the model in the fp32 flow bit for
bit against the unfused formulation and within smoke()'s bounds of the CPU, the 16-bit flows against the fp32 flow and
the AvgPool twin, and the captured train step against the eager loop."""
import copy
import ctypes as C
from functools import partial

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import maxpool_ref as M
from oracle import torch_ref as R
from segmentation_pipeline_amd import _lib, ops
from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss
from segmentation_pipeline_amd.models import ModularUNet

pytestmark = pytest.mark.gpu

CANARY = -777.25
GUARD = 3                      # guard channels on each side of a slice
COMPUTE = {"bf16": _lib.COMPUTE_BF16, "fp16": _lib.COMPUTE_F16}
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int32)


class Slot:
    """a [N, C, ...] device tensor in one of three layouts, with the memory around it filled with a canary:
    dense    its own allocation
    slice    channels [3 : 3 + C] of a wider buffer (own batch stride; the skip slice of a concat buffer)
    shifted  dense, but starting one element into its allocation (a base that is only 4-byte aligned)"""

    def __init__(self, shape, layout, fill=None):
        N, Cc = shape[:2]
        if layout == "slice":
            self.buf = torch.full((N, Cc + 2 * GUARD) + tuple(shape[2:]), CANARY, device="cuda")
            self.t = self.buf[:, GUARD:GUARD + Cc]
            self.guards = [self.buf[:, :GUARD], self.buf[:, GUARD + Cc:]]
        elif layout == "shifted":
            n = int(torch.Size(shape).numel())
            self.buf = torch.full((n + 2,), CANARY, device="cuda")
            self.t = self.buf[1:n + 1].view(shape)
            self.guards = [self.buf[:1], self.buf[n + 1:]]
        else:
            self.buf = self.t = torch.full(shape, CANARY, device="cuda")
            self.guards = []
        if fill is not None:
            self.t.copy_(fill)
        self.bs = self.t.stride(0)

    def intact(self):
        return all(bool((g == CANARY).all()) for g in self.guards)


FP32_SHAPES = [(1, 3, 2, 2, 2), (2, 5, 4, 6, 10), (1, 2, 2, 4, 6),      # rows of W = 6 / 10 floats: 8-byte aligned only
               (2, 3, 4, 4, 8), (1, 2, 2, 2, 4)]                        # W % 4 == 0: the 16-byte paths


@pytest.fixture(scope="module")
def fp32_refs():
    """per shape: input, torch's value / route on the CPU, gradients and torch autograd's dx -- computed once"""
    refs = {}
    for i, shape in enumerate(FP32_SHAPES):
        x, planted = M.tie_heavy_input(shape, seed=10 + i)
        N, Cc, D, H, W = shape
        y, ind = F.max_pool3d(x, 2, 2, return_indices=True)
        route = M.window_position(ind, H, W)
        for n, c, oz, oy, ox, r in planted:
            assert int(route[n, c, oz, oy, ox]) == r
        g = torch.Generator().manual_seed(50 + i)
        dy, add = torch.randn(y.shape, generator=g), torch.randn(shape, generator=g)
        dx = {}
        for with_add in (False, True):
            xr = x.clone().requires_grad_(True)
            outs, gs = [F.max_pool3d(xr, 2, 2)], [dy]
            if with_add:                      # the skip use of the same tensor: autograd sums the two gradients
                outs, gs = outs + [xr.view_as(xr)], gs + [add]
            dx[with_add] = torch.autograd.grad(outs, xr, gs)[0]
        refs[shape] = dict(x=x, y=y, route=route, dy=dy, add=add, dx=dx)
    return refs


@pytest.mark.parametrize("layout", ["dense", "slice", "shifted"])
@pytest.mark.parametrize("shape", FP32_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_kernels_are_bit_exact(fp32_refs, shape, layout):
    L, ref = _lib.lib(), fp32_refs[shape]
    N, Cc, D, H, W = shape
    oshape = (N, Cc, D // 2, H // 2, W // 2)
    xs, ys = Slot(shape, layout, ref["x"].cuda()), Slot(oshape, layout)
    idx = torch.full(oshape, 255, dtype=torch.uint8, device="cuda")
    assert L.m355_maxpool3d_2x_fwd(_p(xs.t), _p(ys.t), _p(idx), N, Cc, D, H, W, xs.bs, ys.bs, _stream()) == 0, L.m355_last_error()
    y = ys.t.cpu()
    assert torch.equal(y.isnan(), ref["y"].isnan())
    assert torch.equal(bits(y), bits(ref["y"]))            # the selected element's bits: -0.0 / +0.0 / NaN included
    assert torch.equal(idx.cpu(), ref["route"])
    assert xs.intact() and ys.intact()
    # inference form: no route
    y2 = Slot(oshape, layout)
    assert L.m355_maxpool3d_2x_fwd(_p(xs.t), _p(y2.t), None, N, Cc, D, H, W, xs.bs, y2.bs, _stream()) == 0
    assert torch.equal(bits(y2.t.cpu()), bits(ref["y"])) and y2.intact()
    # backward: a gather through the route, with and without the skip gradient
    dys, adds = Slot(oshape, layout, ref["dy"].cuda()), Slot(shape, layout, ref["add"].cuda())
    for with_add in (False, True):
        dxs = Slot(shape, layout)
        rc = L.m355_maxpool3d_2x_bwd(_p(dys.t), _p(idx), _p(adds.t) if with_add else None, _p(dxs.t), N, Cc, D, H, W, dys.bs,
                                     adds.bs if with_add else 0, dxs.bs, _stream())
        assert rc == 0, L.m355_last_error()
        assert torch.equal(dxs.t.cpu(), ref["dx"][with_add]), with_add
        assert dxs.intact() and dys.intact() and adds.intact()


def test_fp32_ops_autograd_and_no_grad(monkeypatch):
    """ops.maxpool3d_2x / _with_skip: torch autograd's gradient bit for bit; under no_grad no route is allocated, also
    for an input that requires grad (the forward launches are watched through ops._resample_launch: the route pointer they
    pass; whether a route was asked for, through ops._tracks, where the public functions take that from)"""
    routes, asked = [], []
    launch, tracks = ops._resample_launch, ops._tracks

    def watched_tracks(x):
        asked.append(tracks(x))
        return asked[-1]

    def watched(row, bwd, c8, pointers, *args):
        launch(row, bwd, c8, pointers, *args)
        if not bwd:
            assert row.fwd == "maxpool3d_2x_fwd" and not c8
            routes.append((bool(asked.pop()), pointers[3] is not None))
            assert not asked
    monkeypatch.setattr(ops, "_tracks", watched_tracks)
    monkeypatch.setattr(ops, "_resample_launch", watched)
    x, _ = M.tie_heavy_input((2, 3, 4, 4, 8), seed=3)
    x = x.nan_to_num(0.0, 2.0, -2.0)
    g = torch.Generator().manual_seed(4)
    dy, dskip = torch.randn((2, 3, 2, 2, 4), generator=g), torch.randn(x.shape, generator=g)
    xr = x.clone().requires_grad_(True)
    ref_pool = torch.autograd.grad(F.max_pool3d(xr, 2, 2), xr, dy)[0]
    xd = x.cuda().requires_grad_(True)
    y = ops.maxpool3d_2x(xd)
    assert torch.equal(y.detach().cpu(), F.max_pool3d(x, 2, 2))
    assert torch.equal(torch.autograd.grad(y, xd, dy.cuda())[0].cpu(), ref_pool)
    skip, pooled = ops.maxpool3d_2x_with_skip(xd)
    assert skip.data_ptr() == xd.data_ptr()
    got = torch.autograd.grad([skip, pooled], xd, [dskip.cuda(), dy.cuda()])[0]
    assert torch.equal(got.cpu(), ref_pool + dskip)
    assert routes == [(True, True), (True, True)]
    with torch.no_grad():
        y = ops.maxpool3d_2x(xd)
        skip, pooled = ops.maxpool3d_2x_with_skip(xd)
    assert y.grad_fn is None and torch.equal(y.cpu(), F.max_pool3d(x, 2, 2)) and torch.equal(pooled, y)
    assert routes[2:] == [(False, False), (False, False)]
    assert ops.maxpool3d_2x(xd.detach()).grad_fn is None and routes[4:] == [(False, False)]
    with pytest.raises(_lib.M355Error, match="no CPU fallback"):
        ops.maxpool3d_2x(x)


# ------------------------------------------------------------------------------------------------ c8 kernels
def _round(t, mode):
    return t.to(DT[mode]).float()


def _unpack(t16, Cc, spatial, mode):
    with torch.no_grad():
        return ops.Act16(t16, Cc, spatial, COMPUTE[mode]).to_f32().cpu()


def _pad_lanes(t16, Cc):
    """the lanes past C of the last channel block of a [N, CB, S, 8] tensor, as raw 16-bit patterns"""
    return t16.view(torch.int16)[:, -1, :, Cc % 8:] if Cc % 8 else t16.view(torch.int16)[:, :0]


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("spatial", [(2, 2, 4), (4, 6, 8)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("Cc", [8, 12, 16])
def test_c8_kernels_are_bit_exact(Cc, spatial, mode):
    import segmentation_pipeline_amd as sp
    N, (D, H, W) = 2, spatial
    x, _ = M.tie_heavy_input((N, Cc, D, H, W), seed=7 + Cc)
    x = _round(x, mode)                                  # (small integers, NaN, -inf and signed zeros are exact)
    y_ref, ind = F.max_pool3d(x, 2, 2, return_indices=True)
    compute = COMPUTE[mode]
    # no-grad flow: pack -> pool -> unpack
    with torch.no_grad(), sp.precision(mode):
        y16 = ops.maxpool3d_2x(ops.pack_act16(x.cuda(), compute))
        assert isinstance(y16, ops.Act16) and y16.t is None
        y = y16.to_f32().cpu()
    assert torch.equal(y.isnan(), y_ref.isnan()) and torch.equal(bits(y), bits(y_ref))
    assert not _pad_lanes(y16.data, Cc).any()
    # training flow: the route is checked through the backward, with and without the skip gradient
    g = torch.Generator().manual_seed(70 + Cc)
    dpool, dskip = _round(torch.randn(y_ref.shape, generator=g), mode), _round(torch.randn(x.shape, generator=g), mode)
    xr = x.clone().requires_grad_(True)
    routed = torch.autograd.grad(F.max_pool3d(xr, 2, 2), xr, dpool)[0]
    with torch.no_grad():
        dpool16, dskip16 = ops.pack_act16(dpool.cuda(), compute).data, ops.pack_act16(dskip.cuda(), compute).data
    with sp.precision(mode):
        a = ops.pack_act16(x.cuda().requires_grad_(True), compute)
        assert a.requires_grad
        pooled = ops.maxpool3d_2x(a)
        dx16 = torch.autograd.grad(pooled.t, a.t, dpool16)[0]
        assert torch.equal(bits(pooled.to_f32().detach().cpu()), bits(y_ref))
        assert torch.equal(_unpack(dx16, Cc, spatial, mode), routed)
        assert not _pad_lanes(dx16, Cc).any()
        skip, pooled = ops.maxpool3d_2x_with_skip(a)
        dx16 = torch.autograd.grad([skip.t, pooled.t], a.t, [dskip16, dpool16])[0]
        assert torch.equal(_unpack(dx16, Cc, spatial, mode), _round(dskip + routed, mode))       # rounded once
        assert not _pad_lanes(dx16, Cc).any()


def test_c8_backward_saturates_into_the_fp16_overflow_word(monkeypatch):
    """dskip = dpool = 60000 in one voxel: the fp16 sum is clamped to 65504 and bit 0 of the overflow word is set, as in
    the avg-pool backward.  The word is read before and after, so the test leaves it clear (and the loss-scale target it
    adapts is put back)."""
    import segmentation_pipeline_amd as sp
    for name in ("_fp16_target", "_fp16_clean_checks"):
        monkeypatch.setattr(ops, name, getattr(ops, name))
    compute, Cc, spatial = COMPUTE["fp16"], 12, (2, 2, 4)
    x = torch.zeros((1, Cc) + spatial)
    x[0, 9, 1, 0, 2] = 5.0                      # the maximum of its window, at position (1, 0, 0) -> route 4
    dpool, dskip = torch.zeros((1, Cc, 1, 1, 2)), torch.zeros(x.shape)
    dpool[0, 9, 0, 0, 1] = dskip[0, 9, 1, 0, 2] = 60000.0
    with torch.no_grad():
        dpool16, dskip16 = ops.pack_act16(dpool.cuda(), compute).data, ops.pack_act16(dskip.cuda(), compute).data
    with sp.precision("fp16"):
        a = ops.pack_act16(x.cuda().requires_grad_(True), compute)
        skip, pooled = ops.maxpool3d_2x_with_skip(a)
        ops.fp16_overflow()                     # whatever earlier tests left
        assert ops.fp16_overflow() == 0
        dx16 = torch.autograd.grad([skip.t, pooled.t], a.t, [dskip16, dpool16])[0]
        word = ops.fp16_overflow()
    dx = _unpack(dx16, Cc, spatial, "fp16")
    assert dx[0, 9, 1, 0, 2] == 65504.0 and int((dx != 0).sum()) == 1
    assert word == 1, word
    assert ops.fp16_overflow() == 0


# ------------------------------------------------------------------------------------------------ model
GN4 = {'normalization_class': partial(nn.GroupNorm, 4)}
MAXPOOL = dict(downsample_class=nn.MaxPool3d, downsample_params={'kernel_size': 2, 'stride': 2})
FILTERS = [8, 16, 16]


def _model(maxpool=True):
    torch.manual_seed(0)
    return ModularUNet(2, 3, FILTERS, 3, block_params=dict(GN4), **(MAXPOOL if maxpool else {}))


def _batch(seed=1234, n=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, 2, 16, 16, 16), generator=g)
    lab = torch.randint(0, 3, (n, 16, 16, 16), generator=g)
    return x, F.one_hot(lab, 3).permute(0, 4, 1, 2, 3).float().contiguous()


def _train_step(model, x, y):
    model.zero_grad(set_to_none=True)
    p = model(x)
    ld = HybridLogisticDiceLoss()(p, y)
    ld["loss"].backward()
    return p.detach(), ld["loss"].detach(), {k: v.grad.detach().clone() for k, v in model.named_parameters()}


@pytest.fixture(scope="module")
def fp32_step():
    """the item-3 model after one fp32-flow training step on the device: (model, x, y, probabilities, loss, gradients)"""
    model = _model().cuda().train()
    x, y = _batch()
    p, loss, grads = _train_step(model, x.cuda(), y.cuda())
    return model, x, y, p, loss, grads


def test_model_fp32_flow_equals_the_unfused_formulation(fp32_step, monkeypatch):
    """the same step with ops.maxpool3d_2x(_with_skip) replaced by torch's own device max_pool3d: both see bit-identical
    pre-pool activations, so probabilities and every parameter gradient are bit-identical too"""
    model, x, y, p, loss, grads = fp32_step
    assert set(grads) == {k for k, _ in model.named_parameters()} and len(grads) > 10
    twin = copy.deepcopy(model)
    monkeypatch.setattr(ops, "maxpool3d_2x", lambda t, out=None: F.max_pool3d(t, 2, 2))
    monkeypatch.setattr(ops, "maxpool3d_2x_with_skip", lambda t, out=None: (t, F.max_pool3d(t, 2, 2)))
    p_t, loss_t, grads_t = _train_step(twin, x.cuda(), y.cuda())
    assert torch.equal(p, p_t) and torch.equal(loss, loss_t)
    for k in grads:
        assert torch.equal(grads[k], grads_t[k]), k


def test_model_fp32_forward_matches_the_cpu(fp32_step):
    """probabilities and loss within smoke()'s bounds of the CPU formulation (tests/maxpool_ref.py).  Parameter gradients
    are not compared with the CPU: a near-tie may route differently after a 1e-7 difference in the activations, which
    moves a whole voxel's gradient; the bit-exact test above pins them instead."""
    model, x, y, p, loss, _ = fp32_step
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    spec = R.UNetSpec(2, 3, FILTERS, 3, norm="group", groups=4)
    with torch.no_grad():
        p_ref = M.unet_forward_maxpool(sd, spec, x, training=True)
        loss_ref = R.hybrid_logistic_dice_loss(p_ref, y)["loss"]
    err = (p.cpu() - p_ref).abs().max().item()
    print(f"maxpool fp32 flow vs CPU: max |dp| {err:.3e}, loss {loss.item():.6f} vs {loss_ref.item():.6f}")
    assert err <= 1e-4
    assert abs(loss.item() - loss_ref.item()) <= 1e-4


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_model_16bit_flows(fp32_step, mode):
    """c8 no-grad flow: finite probabilities that sum to 1, and a distance to the fp32 flow of at most 4x that of the
    AvgPool twin of the same model on the same input (averaging eight rounded values shrinks their rounding noise by up
    to sqrt(8), the maximum does not; the rest is slack).  c8 training flow: every parameter gradient finite, cosine with
    the fp32-flow gradient >= 0.95 (the per-parameter bound tests/test_fullsize_gpu.py uses for the composed flows)."""
    import segmentation_pipeline_amd as sp
    model, x, y, _, _, grads32 = fp32_step
    xd, yd = x.cuda(), y.cuda()
    avg = _model(maxpool=False).cuda()
    avg.load_state_dict(model.state_dict())            # (strict: a pool has no parameters)
    dist = {}
    for name, m in (("max", copy.deepcopy(model)), ("avg", avg)):
        m.eval()
        with torch.no_grad():
            p32 = m(xd)
            with sp.precision(mode):
                p16 = m(xd)
        assert torch.isfinite(p16).all()
        assert (p16.sum(dim=1) - 1).abs().max().item() <= 1e-5
        dist[name] = (p16 - p32).abs().max().item()
    print(f"maxpool_accuracy {mode}: max |p16 - p32| MaxPool3d {dist['max']:.4e}  AvgPool3d twin {dist['avg']:.4e}  "
          f"ratio {dist['max'] / dist['avg']:.2f}")
    assert dist["avg"] > 0 and dist["max"] > 0, "the 16-bit mode must really run the 16-bit kernels"
    assert dist["max"] <= 4.0 * dist["avg"], dist
    m = copy.deepcopy(model).train()
    with sp.precision(mode):
        _, _, grads = _train_step(m, xd, yd)
    worst = (2.0, None)
    for k, g32 in grads32.items():
        a, b = grads[k].double().flatten(), g32.double().flatten()
        assert torch.isfinite(a).all(), k
        cos = float(a @ b / (a.norm() * b.norm() + 1e-300))
        worst = min(worst, (cos, k))
    print(f"maxpool_accuracy {mode}: c8 training flow, worst parameter cosine with the fp32 flow {worst[0]:.4f} ({worst[1]})")
    assert worst[0] >= 0.95, worst


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_graphed_train_step_reproduces_the_eager_losses(mode):
    """trainer.GraphedTrainStep on the max-pool model: three eager warm-up steps, then two replayed ones; the losses
    equal those of five eager steps from the same seed (the route tensor comes from the caching allocator and nothing
    synchronises with the host, so the step can be captured)."""
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd.trainer import GraphedTrainStep
    m_e = _model().cuda().train()
    m_g = copy.deepcopy(m_e)
    batches = []
    for i in range(5):
        x, y = _batch(seed=100 + i)
        batches.append({"X": x.cuda(), "y": y.cuda()})
    crit = HybridLogisticDiceLoss()
    with sp.precision(mode):
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
