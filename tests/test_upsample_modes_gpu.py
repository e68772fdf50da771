"""nn.Upsample(scale_factor=2) in nearest and half-pixel trilinear mode as upsample_class of ModularUNet
(csrc/upsample.hip): the eight kernels against stock torch on the CPU (fp32: bit for bit resp. within rounding-error bounds
of the fp64 result, on dense, sliced and shifted tensors with guard canaries; c8: bit for bit resp. within one ulp of the
fp64 result rounded once), the fp16 saturation of the c8 backward kernels, the model in the fp32 flow against the CPU
formulation (tests/upsample_ref.py), the 16-bit flows against the fp32 flow and the align_corners=True twin, and the
captured train step against the eager loop."""
import copy
import ctypes as C
from functools import partial

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import upsample_ref as U
from oracle import torch_ref as R
from segmentation_pipeline_amd import _lib, ops
from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss
from segmentation_pipeline_amd.models import ModularUNet

pytestmark = pytest.mark.gpu

CANARY = -777.25
CANARY16 = -776.0              # (exact in bf16 and fp16)
GUARD = 3                      # guard channels on each side of a slice
COMPUTE = {"bf16": _lib.COMPUTE_BF16, "fp16": _lib.COMPUTE_F16}
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
MODES = ["nearest", "trilinear_hp"]
FAMILY = {"nearest": "m355_upsample_nearest2x", "trilinear_hp": "m355_upsample_trilinear2x_hp"}
EPS = 2.0 ** -24


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int32)


def up_shape(shape):
    return tuple(shape[:2]) + tuple(2 * s for s in shape[2:])


class Slot:
    """a [N, C, ...] device tensor in one of three layouts, with the memory around it filled with a canary (the layouts of
    tests/test_maxpool_gpu.py):
    dense    its own allocation
    slice    channels [3 : 3 + C] of a wider buffer (own batch stride; a slice of a concat buffer)
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


def call(name, src: Slot, dst: Slot, in_shape):
    L = _lib.lib()
    rc = getattr(L, name)(_p(src.t), _p(dst.t), *in_shape, src.bs, dst.bs, _stream())
    assert rc == 0, L.m355_last_error()
    torch.cuda.synchronize()
    assert src.intact() and dst.intact(), name
    return dst.t.cpu()


# ------------------------------------------------------------------------------------------------ fp32 kernels
FP32_SHAPES = [(1, 3, 1, 1, 1),                        # every clamp at once
               (2, 5, 2, 3, 5), (1, 2, 3, 2, 4),       # odd sizes
               (1, 2, 2, 2, 3),                        # output rows of 6 floats: 8-byte aligned only
               (2, 3, 4, 4, 8)]                        # the 16-byte paths
SPECIALS = [float("nan"), -float("nan"), 0.0, -0.0, float("inf"), -float("inf"), 1e-40, -1e-45, 1.17549435e-38]


def worst(err, scale):
    """max of err / (2^-24 * scale) over the elements; an element with scale 0 must be exact"""
    assert bool((err[scale == 0] == 0).all())
    m = scale > 0
    return float((err[m] / (EPS * scale[m])).max()) if bool(m.any()) else 0.0


@pytest.fixture(scope="module")
def fp32_refs():
    """per shape, computed once on the CPU: inputs of the form randn * exp(3 * randn); torch's results in fp32 and fp64,
    and the per-element scales of the bounds"""
    refs = {}
    for i, shape in enumerate(FP32_SHAPES):
        x = U.ill_conditioned(shape, seed=20 + i)
        dy = U.ill_conditioned(up_shape(shape), seed=40 + i)
        xs = x.clone()                                  # the nearest forward's input: special values planted
        flat = xs.view(-1)
        for k, v in enumerate(SPECIALS[:flat.numel()]):
            flat[(k * 7) % flat.numel()] = v
        if flat.numel() > len(SPECIALS):                # a NaN with a payload
            flat.view(torch.int32)[flat.numel() - 1] = 0x7fc12345
        r = dict(x=x, xs=xs, dy=dy, near_y=U.upsample(xs, "nearest"))
        for mode in MODES:
            r[mode + "_y32"], r[mode + "_y64"] = U.upsample(x, mode), U.upsample(x.double(), mode)
            r[mode + "_dx32"] = U.upsample_grad(dy, mode, shape)
            r[mode + "_dx64"] = U.upsample_grad(dy.double(), mode, shape)
            r[mode + "_dxscale"] = U.upsample_grad(dy.double().abs(), mode, shape)      # sum |w * dy| (nearest: w = 1)
        r["hp_yscale"] = U.neighbourhood_max(x.double())
        refs[shape] = r
    return refs


@pytest.mark.parametrize("layout", ["dense", "slice", "shifted"])
@pytest.mark.parametrize("shape", FP32_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_nearest_kernels(fp32_refs, shape, layout):
    """forward: stock torch's bits, NaN payloads, signed zeros, infinities and denormals included.  backward:
    |dx - dx64| <= 7 * 2^-24 * sum |dy| over the block, the bound of an 8-term fp32 sum in any order; torch's own fp32
    result is held to the same bound."""
    ref = fp32_refs[shape]
    y = call("m355_upsample_nearest2x_fwd", Slot(shape, layout, ref["xs"].cuda()), Slot(up_shape(shape), layout), shape)
    assert torch.equal(bits(y), bits(ref["near_y"]))
    dx = call("m355_upsample_nearest2x_bwd", Slot(up_shape(shape), layout, ref["dy"].cuda()), Slot(shape, layout), shape)
    scale = ref["nearest_dxscale"]
    ours = worst((dx.double() - ref["nearest_dx64"]).abs(), scale)
    torchs = worst((ref["nearest_dx32"].double() - ref["nearest_dx64"]).abs(), scale)
    print(f"nearest bwd {shape} {layout}: worst |dx - dx64| / (2^-24 sum|dy|): kernel {ours:.2f}  torch fp32 {torchs:.2f}")
    assert torchs <= 7.0
    assert ours <= 7.0


@pytest.mark.parametrize("layout", ["dense", "slice", "shifted"])
@pytest.mark.parametrize("shape", FP32_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_half_pixel_kernels(fp32_refs, shape, layout):
    """forward: |y - y64| <= 10 * 2^-24 * max |x| over the clamped 3x3x3 neighbourhood (three weight products and seven
    additions); backward: |dx - dx64| <= 66 * 2^-24 * sum |w * dy| over the contributing outputs (up to 64 terms and
    three weight products).  torch's own fp32 results are held to the same bounds."""
    ref = fp32_refs[shape]
    y = call("m355_upsample_trilinear2x_hp_fwd", Slot(shape, layout, ref["x"].cuda()), Slot(up_shape(shape), layout), shape)
    ours = worst((y.double() - ref["trilinear_hp_y64"]).abs(), ref["hp_yscale"])
    torchs = worst((ref["trilinear_hp_y32"].double() - ref["trilinear_hp_y64"]).abs(), ref["hp_yscale"])
    print(f"half-pixel fwd {shape} {layout}: worst |y - y64| / (2^-24 max|x|): kernel {ours:.2f}  torch fp32 {torchs:.2f}")
    assert torchs <= 10.0
    assert ours <= 10.0
    # y[0] == x[0] along every axis: the corner output is the corner input
    assert torch.equal(y[:, :, 0, 0, 0], ref["x"][:, :, 0, 0, 0]) and torch.equal(y[:, :, -1, -1, -1], ref["x"][:, :, -1, -1, -1])
    dx = call("m355_upsample_trilinear2x_hp_bwd", Slot(up_shape(shape), layout, ref["dy"].cuda()), Slot(shape, layout), shape)
    scale = ref["trilinear_hp_dxscale"]
    ours = worst((dx.double() - ref["trilinear_hp_dx64"]).abs(), scale)
    torchs = worst((ref["trilinear_hp_dx32"].double() - ref["trilinear_hp_dx64"]).abs(), scale)
    print(f"half-pixel bwd {shape} {layout}: worst |dx - dx64| / (2^-24 sum|w dy|): kernel {ours:.2f}  torch fp32 {torchs:.2f}")
    assert torchs <= 66.0
    assert ours <= 66.0


@pytest.mark.parametrize("mode", MODES)
def test_fp32_ops_autograd_slot_and_determinism(mode):
    """ops.upsample_nearest2x / upsample_trilinear2x_hp (and the `mode` argument of upsample_trilinear2x): value and
    gradient as the kernels give them, into an OutSlot of a concat buffer, twice with the same bits; the default of
    upsample_trilinear2x is still align_corners=True"""
    fn = {"nearest": ops.upsample_nearest2x, "trilinear_hp": ops.upsample_trilinear2x_hp}[mode]
    x = U.ill_conditioned((2, 3, 3, 4, 6), seed=5)
    dy = U.ill_conditioned((2, 3, 6, 8, 12), seed=6)
    y64, dx64 = U.upsample(x.double(), mode), U.upsample_grad(dy.double(), mode, x.shape)
    xd = x.cuda().requires_grad_(True)
    buf = torch.full((2, 5, 6, 8, 12), CANARY, device="cuda")
    outs = []
    for y in (fn(xd), fn(xd, out=ops.OutSlot(buf, 0, 3)), ops.upsample_trilinear2x(xd, mode=mode)):
        dx = torch.autograd.grad(y, xd, dy.cuda())[0]
        outs.append((y.detach().cpu(), dx.cpu()))
    assert torch.equal(buf[:, :3].cpu(), outs[0][0]) and bool((buf[:, 3:] == CANARY).all())
    for y, dx in outs[1:]:
        assert torch.equal(bits(y), bits(outs[0][0])) and torch.equal(bits(dx), bits(outs[0][1]))
    y, dx = outs[0]
    assert worst((y.double() - y64).abs(), U.neighbourhood_max(x.double())) <= 10.0
    assert worst((dx.double() - dx64).abs(), U.upsample_grad(dy.double().abs(), mode, x.shape)) <= 66.0
    with torch.no_grad():
        assert fn(xd).grad_fn is None
        y_default = ops.upsample_trilinear2x(xd).cpu()
    assert (y_default - U.upsample(x, "trilinear")).abs().max() <= 1e-5 * x.abs().max() and not torch.equal(y_default, y)


# ------------------------------------------------------------------------------------------------ c8 kernels
def pack_c8(x, dt):
    """[N, C, D, H, W] fp32 (CPU) -> [N, CB, S, 8] in the 16-bit type, lanes past C zero"""
    N, Cc = x.shape[:2]
    S, CB = x[0, 0].numel(), (Cc + 7) // 8
    p = torch.zeros((N, CB * 8, S))
    p[:, :Cc] = x.reshape(N, Cc, S)
    return p.view(N, CB, 8, S).permute(0, 1, 3, 2).contiguous().to(dt)


def unpack_c8(t16, Cc, spatial):
    N, CB, S, _ = t16.shape
    return t16.double().permute(0, 1, 3, 2).reshape(N, CB * 8, S)[:, :Cc].reshape((N, Cc) + tuple(spatial))


def ulp16(v, dt):
    """spacing of the 16-bit type at |v| (the subnormal spacing below the smallest normal)"""
    mant, emin = (7, -126) if dt == torch.bfloat16 else (10, -14)
    e = torch.frexp(v.abs().double())[1] - 1
    return torch.exp2((torch.where(v == 0, torch.full_like(e, emin), e).clamp(min=emin) - mant).double())


class Slot16:
    """a [N, CB, S, 8] c8 tensor on the device: its own allocation, or the blocks [1, 1 + CB) of a wider c8 buffer (a
    slot of a concat buffer) whose other blocks hold a canary"""

    def __init__(self, N, Cc, S, dt, wide, fill=None):
        CB = (Cc + 7) // 8
        self.buf = torch.full((N, CB + (2 if wide else 0), S, 8), CANARY16, dtype=dt, device="cuda")
        self.t = self.buf[:, 1:1 + CB] if wide else self.buf
        self.guards = [self.buf[:, :1], self.buf[:, 1 + CB:]] if wide else []
        if fill is not None:
            self.t.copy_(fill)
        self.bs = self.buf.stride(0)

    def intact(self):
        return all(bool((g == CANARY16).all()) for g in self.guards)


def call16(name, src: Slot16, dst: Slot16, in_shape, mode):
    L = _lib.lib()
    rc = getattr(L, name)(_p(src.t), _p(dst.t), *in_shape, src.bs, dst.bs, COMPUTE[mode], _stream())
    assert rc == 0, L.m355_last_error()
    torch.cuda.synchronize()
    assert src.intact() and dst.intact(), name
    return dst.t.cpu().contiguous()


def _pad_lanes(t16, Cc):
    """the lanes past C of the last channel block of a [N, CB, S, 8] tensor, as raw 16-bit patterns"""
    return t16.view(torch.int16)[:, -1, :, Cc % 8:] if Cc % 8 else t16.view(torch.int16)[:, :0]


@pytest.mark.parametrize("wide", [False, True], ids=["dense", "slot"])
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("spatial", [(1, 1, 1), (2, 3, 5), (2, 2, 4)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("Cc", [8, 12, 16])
def test_c8_kernels(Cc, spatial, mode, wide):
    """nearest forward: the input items, bit for bit.  The other three: within one ulp of the 16-bit type of the fp64
    result from the 16-bit-rounded inputs, rounded once.  Padding lanes (C = 12: a half-filled block) come out zero."""
    N, dt = 2, DT[mode]
    S = spatial[0] * spatial[1] * spatial[2]
    shape = (N, Cc) + spatial
    g = torch.Generator().manual_seed(100 + Cc + S)
    x16, dy16 = pack_c8(torch.randn(shape, generator=g), dt), pack_c8(torch.randn(up_shape(shape), generator=g), dt)
    x64, dy64 = unpack_c8(x16, Cc, spatial), unpack_c8(dy16, Cc, up_shape(shape)[2:])
    xs, dys = Slot16(N, Cc, S, dt, wide, x16.cuda()), Slot16(N, Cc, 8 * S, dt, wide, dy16.cuda())
    for m in MODES:
        y16 = call16(FAMILY[m] + "_fwd_h16", xs, Slot16(N, Cc, 8 * S, dt, wide), shape, mode)
        dx16 = call16(FAMILY[m] + "_bwd_h16", dys, Slot16(N, Cc, S, dt, wide), shape, mode)
        assert not _pad_lanes(y16, Cc).any() and not _pad_lanes(dx16, Cc).any()
        if m == "nearest":
            want = pack_c8(U.upsample(unpack_c8(x16, Cc, spatial).float(), "nearest"), dt)
            assert torch.equal(y16.view(torch.int16), want.view(torch.int16))
        checks = [("bwd", unpack_c8(dx16, Cc, spatial), U.upsample_grad(dy64, m, shape))]
        if m != "nearest":
            checks.append(("fwd", unpack_c8(y16, Cc, up_shape(shape)[2:]), U.upsample(x64, m)))
        for what, got, ref64 in checks:
            ref16 = ref64.to(dt).double()               # rounded once
            off = ((got - ref16).abs() / ulp16(ref16, dt)).max().item()
            assert off <= 1.0, (m, what, off)


@pytest.mark.parametrize("m", MODES)
def test_c8_backward_saturates_into_the_fp16_overflow_word(m, monkeypatch):
    """a block of loss-scaled gradients of 20000 sums past 65504 in the input voxel under it (nearest: 8 x 20000;
    half-pixel: at least 1.5^3 x 20000): it comes out saturated and bit 0 of the overflow word is set.  A block of 8000s in
    the same call stays finite and exact (nearest: 64000), and on its own sets nothing.  The word is read before and
    after, so the test leaves it clear (and the loss-scale target it adapts is put back)."""
    import segmentation_pipeline_amd as sp
    for name in ("_fp16_target", "_fp16_clean_checks"):
        monkeypatch.setattr(ops, name, getattr(ops, name))
    fn = {"nearest": ops.upsample_nearest2x, "trilinear_hp": ops.upsample_trilinear2x_hp}[m]
    compute, Cc, spatial = COMPUTE["fp16"], 12, (2, 2, 4)
    big, fine = torch.zeros((1, Cc, 4, 4, 8)), torch.zeros((1, Cc, 4, 4, 8))
    big[0, 9, 0:2, 0:2, 0:2] = 20000.0             # the block of input voxel (0, 0, 0), channel 9
    fine[0, 3, 2:4, 2:4, 6:8] = 8000.0             # the block of input voxel (1, 1, 3), channel 3
    words, dxs = [], []
    with sp.precision("fp16"):
        a = ops.pack_act16(torch.zeros((1, Cc) + spatial).cuda().requires_grad_(True), compute)
        up = fn(a)
        ops.fp16_overflow()                         # whatever earlier tests left
        assert ops.fp16_overflow() == 0
        for dy in (fine, fine + big):
            dx16 = torch.autograd.grad(up.t, a.t, pack_c8(dy, torch.float16).cuda(), retain_graph=True)[0]
            words.append(ops.fp16_overflow())
            dxs.append(unpack_c8(dx16.cpu(), Cc, spatial))
    want_fine = U.upsample_grad(fine.double(), m, (1, Cc) + spatial)
    assert want_fine.max() < 65504 and torch.equal(dxs[0], want_fine.half().double())
    assert words == [0, 1], words
    want = U.upsample_grad((fine + big).double(), m, (1, Cc) + spatial)
    assert want[0, 9, 0, 0, 0] > 65504 and dxs[1][0, 9, 0, 0, 0] == 65504.0
    assert torch.equal(dxs[1], want.clamp(max=65504.0).half().double())
    assert torch.equal(dxs[1][0, 3], dxs[0][0, 3])      # the finite block of the same call
    assert ops.fp16_overflow() == 0


# ------------------------------------------------------------------------------------------------ model
GN4 = {'normalization_class': partial(nn.GroupNorm, 4)}
FILTERS = [8, 16, 16]
PARAMS = {"nearest": {'scale_factor': 2}, "trilinear_hp": {'scale_factor': 2, 'mode': 'trilinear'}, "trilinear": None}


def _model(mode):
    torch.manual_seed(0)
    params = PARAMS[mode]
    return ModularUNet(2, 3, FILTERS, 3, block_params=dict(GN4), upsample_params=None if params is None else dict(params))


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
def fp32_steps():
    """per new mode: the model after one fp32-flow training step on the device: (model, x, y, probabilities, loss, gradients)"""
    steps = {}
    for mode in MODES:
        model = _model(mode).cuda().train()
        x, y = _batch()
        steps[mode] = (model, x, y) + _train_step(model, x.cuda(), y.cuda())
    return steps


def test_default_nn_upsample_runs_forward_and_backward():
    """upsample_params={'scale_factor': 2} -- nn.Upsample's own default mode -- used to raise NotImplementedError"""
    torch.manual_seed(0)
    model = ModularUNet(2, 3, FILTERS, 3, block_params=dict(GN4), upsample_params={'scale_factor': 2}).cuda().train()
    assert all(u.mode == "nearest" and u.align_corners is None for u in model.upsampling)
    x, y = _batch()
    p, loss, grads = _train_step(model, x.cuda(), y.cuda())
    assert p.shape == (1, 3, 16, 16, 16) and torch.isfinite(p).all() and torch.isfinite(loss)
    assert all(torch.isfinite(g).all() and g.abs().max() > 0 for g in grads.values()) and len(grads) > 10


@pytest.mark.parametrize("mode", MODES)
def test_model_fp32_flow_matches_the_cpu(fp32_steps, mode):
    """probabilities and loss within 1e-4 of the CPU formulation (tests/upsample_ref.py), every parameter gradient within
    1e-3 * max |g_ref| + 1e-7: smoke()'s bounds.  No routing tie here, so the gradients are compared as well."""
    model, x, y, p, loss, grads = fp32_steps[mode]
    names = {k for k, _ in model.named_parameters()}
    sd = {k: v.detach().cpu().clone().requires_grad_(k in names) for k, v in model.state_dict().items()}
    spec = R.UNetSpec(2, 3, FILTERS, 3, norm="group", groups=4)
    p_ref = U.unet_forward_upsample(sd, spec, x, mode, training=True)
    loss_ref = R.hybrid_logistic_dice_loss(p_ref, y)["loss"]
    loss_ref.backward()
    err = (p.cpu() - p_ref.detach()).abs().max().item()
    gerr = max(((grads[k].cpu() - sd[k].grad).abs().max() / (1e-3 * sd[k].grad.abs().max() + 1e-7)).item() for k in names)
    print(f"upsample_accuracy {mode} fp32 flow vs CPU: max |dp| {err:.3e}, loss {loss.item():.6f} vs {loss_ref.item():.6f}, "
          f"worst gradient error / bound {gerr:.3f}")
    assert set(grads) == names and len(names) > 10
    assert err <= 1e-4
    assert abs(loss.item() - loss_ref.item()) <= 1e-4
    for k in sorted(names):
        g_ref = sd[k].grad
        assert (grads[k].cpu() - g_ref).abs().max().item() <= 1e-3 * g_ref.abs().max().item() + 1e-7, k


def test_model_nearest_forward_equals_torch_interpolate_on_the_device(fp32_steps, monkeypatch):
    """the same forward with ops.upsample_nearest2x replaced by torch's device F.interpolate (copied into the concat
    slot): the kernel's forward is a copy, so the probabilities are bit-identical"""
    model, x, _, _, _, _ = fp32_steps["nearest"]
    xd = x.cuda()
    with torch.no_grad():
        p = model(xd)
    calls = []

    def twin(t, out=None):
        y = F.interpolate(t, scale_factor=2, mode="nearest")
        calls.append(tuple(y.shape))
        out.view().copy_(y)
        return out.view()
    monkeypatch.setattr(ops, "upsample_nearest2x", twin)
    with torch.no_grad():
        p_t = model(xd)
    assert calls == [(1, 16, 8, 8, 8), (1, 16, 16, 16, 16)]
    assert torch.equal(p, p_t)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", MODES)
def test_model_16bit_flows(fp32_steps, mode, prec):
    """c8 no-grad flow: finite probabilities that sum to 1 within 1e-5, and a distance to the fp32 flow of at most 2x that
    of the align_corners=True twin of the same weights on the same input (the three modes round the same number of
    values per output; the factor is slack for the different interpolants).  c8 training flow: every parameter gradient
    finite, cosine with the fp32-flow gradient >= 0.95 (tests/test_fullsize_gpu.py's per-parameter bound)."""
    import segmentation_pipeline_amd as sp
    model, x, y, _, _, grads32 = fp32_steps[mode]
    xd, yd = x.cuda(), y.cuda()
    twin = _model("trilinear").cuda()
    twin.load_state_dict(model.state_dict())           # (strict: an upsampler has no parameters)
    dist = {}
    for name, m in (("new", copy.deepcopy(model)), ("twin", twin)):
        m.eval()
        with torch.no_grad():
            p32 = m(xd)
            with sp.precision(prec):
                p16 = m(xd)
        assert torch.isfinite(p16).all()
        assert (p16.sum(dim=1) - 1).abs().max().item() <= 1e-5
        dist[name] = (p16 - p32).abs().max().item()
    print(f"upsample_accuracy {mode} {prec}: max |p16 - p32| {dist['new']:.4e}  align_corners=True twin {dist['twin']:.4e}  "
          f"ratio {dist['new'] / max(dist['twin'], 1e-300):.2f}")
    assert dist["twin"] > 0 and dist["new"] > 0, "the 16-bit mode must really run the 16-bit kernels"
    assert dist["new"] <= 2.0 * dist["twin"], dist
    m = copy.deepcopy(model).train()
    with sp.precision(prec):
        _, _, grads = _train_step(m, xd, yd)
    worst_cos = (2.0, None)
    for k, g32 in grads32.items():
        a, b = grads[k].double().flatten(), g32.double().flatten()
        assert torch.isfinite(a).all(), k
        cos = float(a @ b / (a.norm() * b.norm() + 1e-300))
        worst_cos = min(worst_cos, (cos, k))
    print(f"upsample_accuracy {mode} {prec}: c8 training flow, worst parameter cosine with the fp32 flow {worst_cos[0]:.4f} "
          f"({worst_cos[1]})")
    assert worst_cos[0] >= 0.95, worst_cos


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_graphed_train_step_reproduces_the_eager_losses(prec):
    """trainer.GraphedTrainStep on the nearest model: three eager warm-up steps, then two replayed ones; the losses equal
    those of five eager steps from the same seed (no host synchronisation, nothing outside the caching allocator)."""
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd.trainer import GraphedTrainStep
    m_e = _model("nearest").cuda().train()
    m_g = copy.deepcopy(m_e)
    batches = []
    for i in range(5):
        x, y = _batch(seed=100 + i)
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
