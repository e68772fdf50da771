"""nn.ELU, nn.GELU (erf and tanh) and nn.SiLU as activation_class of Block3d (csrc/activation.hpp, the codes 3..6 of
m355_norm_desc.act): the ten normalisation passes against the nn module under autograd on the CPU in fp64
(tests/activation_ref.py) at the tolerances tests/test_kernels_gpu.py holds ReLU to, the model in the fp32 flow against the
CPU formulation, the 16-bit flows against the fp32 flow and the LeakyReLU twin, and the captured train step against the
eager loop.  The lines starting with `activation_accuracy` are what profiles/activation_accuracy.txt records."""
import copy
from functools import partial

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import activation_ref as A
from oracle import torch_ref as R
from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss
from segmentation_pipeline_amd.models import ModularUNet

pytestmark = pytest.mark.gpu

NAMES = list(A.ACTS)
DT = {1: torch.bfloat16, 2: torch.float16}
ULP = {1: 2.0 ** -8, 2: 2.0 ** -11}
PREC = {1: "bf16", 2: "fp16"}


def rnd(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def check(got, ref, rtol, atol, what, torch32=None):
    """tests/test_kernels_gpu.py's close(): max |got - ref| <= atol + rtol * max |ref|, every value finite; prints the
    figure (and torch's own fp32 CPU result against the same fp64 reference) before asserting"""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, bound = (got - ref).abs().max().item(), atol + rtol * ref.abs().max().item()
    t32 = "" if torch32 is None else f"  torch fp32 on the CPU {(torch32.detach().double() - ref).abs().max().item():.3e}"
    print(f"activation_accuracy {what}: max err {err:.3e}  bound {bound:.3e}{t32}")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def rounded_check(got, ref, compute, atol, what):
    """test_kernels_gpu.py's _rounded_close(): `got` = one rounding to the 16-bit type of (a value within atol of) `ref`"""
    got, ref = got.double(), ref.detach().double()
    excess = (got - ref).abs() - (ULP[compute] * ref.abs() * 1.01 + atol)
    print(f"activation_accuracy {what}: max err {(got - ref).abs().max().item():.3e}  atol {atol:.3e}  "
          f"worst excess over one rounding + atol {excess.max().item():.3e}")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    assert not bool((excess > 0).any()), f"{what}: {int((excess > 0).sum())} elements off"


# ------------------------------------------------------------------------------------------------ fp32 kernels
# (N, C, D, H, W, groups, layout): S = 30 scalar path, three channels per group, N = 2 | BatchNorm, float4 path, pool-able |
# the activation-only descriptor with the planted values | the first on a batch stride of dense + 1 (misaligned: scalar kernels)
FP32 = {"gn_s30": (2, 12, 2, 3, 5, 4, "dense"), "bn_vec": (1, 8, 4, 4, 4, 0, "dense"), "act_only": (1, 8, 4, 4, 4, 0, "dense"),
        "gn_s30_stride": (2, 12, 2, 3, 5, 4, "strided")}


@pytest.fixture(scope="module")
def fp32_refs():
    """per (descriptor, activation), computed once on the CPU: inputs, the fp64 results for each mode the kernels are run in,
    and torch's own fp32 results"""
    refs = {}
    for dname, (N, Cc, D, H, W, groups, _) in FP32.items():
        only = dname == "act_only"
        x = rnd(N, Cc, D, H, W, seed=1) * 1.7 + 0.3
        if only:
            flat = x.view(-1)
            for k, v in enumerate(A.PLANTED):
                flat[(k * 37) % flat.numel()] = v
        dy, add = rnd(N, Cc, D, H, W, seed=7), rnd(N, Cc, D, H, W, seed=4)
        gamma, beta = (None, None) if only else (rnd(Cc, seed=2), rnd(Cc, seed=3))
        given = (torch.zeros(Cc), torch.ones(Cc)) if only else None
        eps = 0.0 if only else 1e-5
        for name in NAMES:
            act = A.module(name)
            r = dict(x=x, dy=dy, add=add, gamma=gamma, beta=beta, eps=eps)
            for training in ((1,) if groups else (1, 0)):
                for dt in (torch.float64, torch.float32):
                    r[training, dt] = A.norm_act_fwd_bwd(x, dy, gamma, beta, groups, eps, act, bool(training), None, given, dt)
            r["y_add"] = A.norm_act_fwd_bwd(x, dy, gamma, beta, groups, eps, act, True, add, given)["y"]
            refs[dname, name] = r
    return refs


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dname", list(FP32))
def test_fp32_passes(hip, fp32_refs, dname, name):
    """forward with and without `add`, the pooled-output forward, backward in training (and, BatchNorm, eval) mode, the
    reduce / apply pair bit for bit against the one-call backward.  fwd and dx: close(2e-5, 2e-5); dgamma / dbeta: rtol 2e-5,
    atol 1e-4.  Every output is finite -- the planted pre-activations 0 ... +-90, -104 included."""
    N, Cc, D, H, W, groups, layout = FP32[dname]
    code, _, _, param = A.ACTS[name]
    r = fp32_refs[dname, name]
    ref, ref32 = r[1, torch.float64], r[1, torch.float32]
    mean, rstd = ref["mean"].float(), ref["rstd"].float()
    kw = dict(eps=r["eps"], slope=param)
    lay = dict(c_pre=0, c_post=0, extra=1) if layout == "strided" else None
    inp = (lambda t: hip.slot(t, **lay)) if lay else (lambda t: t)
    out = (lambda shape=(N, Cc, D, H, W): hip.slot(shape, **lay)) if lay else (lambda shape=None: None)
    res = (lambda t: t.check_output(dname)) if lay else (lambda t: t)
    x, dy, add, gamma, beta = inp(r["x"]), inp(r["dy"]), inp(r["add"]), r["gamma"], r["beta"]
    tag = f"{name} {dname}"
    y = res(hip.norm_act_fwd(x, mean, rstd, gamma, beta, groups, code, out=out(), **kw))
    check(y, ref["y"], 2e-5, 2e-5, f"{tag} pass 1 fwd", ref32["y"])
    y = res(hip.norm_act_fwd(x, mean, rstd, gamma, beta, groups, code, add, out=out(), **kw))
    check(y, r["y_add"], 2e-5, 2e-5, f"{tag} pass 1 fwd + add")
    if D % 2 == 0 and H % 2 == 0 and W % 2 == 0:
        y, pooled = hip.norm_act_pool_fwd(x, mean, rstd, gamma, beta, groups, code, **kw)
        check(y, ref["y"], 2e-5, 2e-5, f"{tag} pass 4 fwd")
        check(pooled, F.avg_pool3d(ref["y"], 2, 2), 2e-5, 2e-5, f"{tag} pass 4 pooled")
    for training in ((1,) if groups else (1, 0)):
        ref, ref32 = r[training, torch.float64], r[training, torch.float32]
        dx, dg, db = hip.norm_act_bwd(x, dy, mean, rstd, gamma, beta, groups, code, training, out=out(), **kw)
        dx = res(dx)
        check(dx, ref["dx"], 2e-5, 2e-5, f"{tag} pass 5+6 dx training={training}", ref32["dx"])
        if gamma is not None:
            check(dg, ref["dgamma"], 2e-5, 1e-4, f"{tag} pass 5 dgamma training={training}", ref32["dgamma"])
            check(db, ref["dbeta"], 2e-5, 1e-4, f"{tag} pass 5 dbeta training={training}", ref32["dbeta"])
        stat_m, dg2, db2 = hip.norm_act_bwd_reduce(x, dy, mean, rstd, gamma, beta, groups, code, training, **kw)
        dx2, _ = hip.norm_act_bwd_apply(x, dy, mean, rstd, gamma, beta, stat_m, groups, code, out=out(), **kw)
        assert torch.equal(res(dx2).view(torch.int32), dx.view(torch.int32)), "reduce / apply pair != the one-call backward"
        if gamma is not None:
            assert torch.equal(dg2, dg) and torch.equal(db2, db)


# ------------------------------------------------------------------------------------------------ c8 kernels
C8 = {"gn_c12": (2, 12, 2, 4, 6, 4), "bn_c12": (2, 12, 2, 4, 6, 0), "gn_c8": (1, 8, 2, 2, 4, 2)}   # C = 12: a half-empty block


def unpack_c8(t16, Cc, spatial):
    """[N, CB, S, 8] (device) -> fp64 [N, C, D, H, W] on the CPU"""
    t16 = t16.cpu()
    N, CB, S, _ = t16.shape
    return t16.double().permute(0, 1, 3, 2).reshape(N, CB * 8, S)[:, :Cc].reshape((N, Cc) + tuple(spatial))


def pad_lanes_zero(t16, Cc):
    return Cc % 8 == 0 or not bool(t16[:, -1, :, Cc % 8:].cpu().view(torch.int16).any())


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dname", list(C8))
def test_c8_passes(hip, dname, name, compute):
    """passes 2, 3 (with add16), 7, and 8 / 9 with the gradient from dy16, from dpool16 and from both: c8 outputs are one
    rounding of a value within 2e-5 * max |ref| of the fp64 result on the rounded operand values, dgamma / dbeta within
    1e-4 * max |ref|; the lanes past C of the last channel block are zero."""
    N, Cc, D, H, W, groups = C8[dname]
    code, _, _, param = A.ACTS[name]
    act, dt, sp = A.module(name), DT[compute], (D, H, W)
    kw = dict(slope=param)
    x, dy, add = rnd(N, Cc, D, H, W, seed=1) * 1.7 + 0.3, rnd(N, Cc, D, H, W, seed=6), rnd(N, Cc, D, H, W, seed=4)
    dp = rnd(N, Cc, D // 2, H // 2, W // 2, seed=7)
    gamma, beta = rnd(Cc, seed=2) * 0.5 + 1.0, rnd(Cc, seed=3) * 0.1
    rd = lambda t: t.to(dt).float()     # noqa: E731  (the values a c8 tensor holds)
    tag = f"{name} {dname} {PREC[compute]}"

    # pass 2 (fp32 in, c8 + fp32 out) and pass 7 (fp32 backward with the c8 twin of dx): fp32 operands
    ref = A.norm_act_fwd_bwd(x, dy, gamma, beta, groups, 1e-5, act)
    mean, rstd = ref["mean"].float(), ref["rstd"].float()
    y16, y = hip.norm_act_fwd_h16(x, mean, rstd, gamma, beta, groups, code, compute, want_f32=True, **kw)
    check(y, ref["y"], 2e-5, 2e-5, f"{tag} pass 2 fp32 y")
    rounded_check(unpack_c8(y16, Cc, sp), ref["y"], compute, 2e-5 * ref["y"].abs().max().item(), f"{tag} pass 2 y16")
    dx, dg, db, dx16 = hip.norm_act_bwd_h16(x, dy, mean, rstd, gamma, beta, groups, code, compute, **kw)
    check(dx, ref["dx"], 2e-5, 2e-5, f"{tag} pass 7 dx")
    check(dg, ref["dgamma"], 2e-5, 1e-4, f"{tag} pass 5 dgamma (twin)")
    check(db, ref["dbeta"], 2e-5, 1e-4, f"{tag} pass 5 dbeta (twin)")
    rounded_check(unpack_c8(dx16, Cc, sp), ref["dx"], compute, 2e-5 * ref["dx"].abs().max().item(), f"{tag} pass 7 dx16")
    assert pad_lanes_zero(y16, Cc) and pad_lanes_zero(dx16, Cc)

    # passes 3, 8, 9: c8 operands; the reference sees the rounded values
    x16, add16 = hip.act16_pack(x, compute), hip.act16_pack(add, compute)
    xr = rd(x)
    up = 0.125 * rd(dp).repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)
    for src, g in (("dy", rd(dy)), ("pool", up), ("both", rd(dy) + up)):
        ref = A.norm_act_fwd_bwd(xr, g, gamma, beta, groups, 1e-5, act, add=rd(add))
        mean, rstd = ref["mean"].float(), ref["rstd"].float()
        if src == "dy":
            y16 = hip.norm_act_fwd_c8(x16, Cc, mean, rstd, gamma, beta, groups, code, compute, add16=add16, **kw)
            rounded_check(unpack_c8(y16, Cc, sp), ref["y"], compute, 2e-5 * ref["y"].abs().max().item(), f"{tag} pass 3 y16 + add16")
            assert pad_lanes_zero(y16, Cc)
        dy16 = hip.act16_pack(dy, compute) if src != "pool" else None
        dp16 = hip.act16_pack(dp, compute) if src != "dy" else None
        dx16, dg, db = hip.norm_act_bwd_c8(x16, dy16, dp16, Cc, sp, mean, rstd, gamma, beta, groups, code, compute, **kw)
        rounded_check(unpack_c8(dx16, Cc, sp), ref["dx"], compute, 2e-5 * ref["dx"].abs().max().item(), f"{tag} pass 8+9 dx16 from {src}")
        check(dg, ref["dgamma"], 1e-4, 0.0, f"{tag} pass 8 dgamma from {src}")
        check(db, ref["dbeta"], 1e-4, 0.0, f"{tag} pass 8 dbeta from {src}")
        assert pad_lanes_zero(dx16, Cc)


# ------------------------------------------------------------------------------------------------ model
FILTERS = [8, 16, 16]


def _model(cls, params, norm=partial(nn.GroupNorm, 4), residual=False):
    torch.manual_seed(0)        # (an activation has no parameters: every activation_class gives the same weights)
    return ModularUNet(2, 3, FILTERS, 3, block_params={'normalization_class': norm, 'activation_class': cls,
                                                       'activation_params': dict(params), 'residual': residual})


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
    """per activation: the model before and after one fp32-flow training step on the device:
    (state_dict before, model, x, y, probabilities, loss, gradients)"""
    steps = {}
    for name in NAMES:
        _, cls, params, _ = A.ACTS[name]
        model = _model(cls, params).cuda().train()
        sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        x, y = _batch()
        steps[name] = (sd0, model, x, y) + _train_step(model, x.cuda(), y.cuda())
    return steps


def _against_the_cpu(tag, sd0, model, x, y, p, loss, grads, spec, act):
    names = {k for k, _ in model.named_parameters()}
    sd = {k: v.clone().requires_grad_(k in names) for k, v in sd0.items()}
    p_ref = A.unet_forward_act(sd, spec, x, act, training=True)
    loss_ref = R.hybrid_logistic_dice_loss(p_ref, y)["loss"]
    loss_ref.backward()
    err = (p.cpu() - p_ref.detach()).abs().max().item()
    gerr = max(((grads[k].cpu() - sd[k].grad).abs().max() / (1e-3 * sd[k].grad.abs().max() + 1e-7)).item() for k in names)
    print(f"activation_accuracy {tag} fp32 flow vs CPU: max |dp| {err:.3e}, loss {loss.item():.6f} vs {loss_ref.item():.6f}, "
          f"worst gradient error / bound {gerr:.3f}")
    assert set(grads) == names and len(names) > 10
    assert err <= 1e-4
    assert abs(loss.item() - loss_ref.item()) <= 1e-4
    for k in sorted(names):
        g_ref = sd[k].grad
        assert (grads[k].cpu() - g_ref).abs().max().item() <= 1e-3 * g_ref.abs().max().item() + 1e-7, k
    return sd


@pytest.mark.parametrize("name", NAMES)
def test_model_fp32_flow_matches_the_cpu(fp32_steps, name):
    """probabilities and loss within 1e-4 of the CPU formulation (tests/activation_ref.py), every parameter gradient within
    1e-3 * max |g_ref| + 1e-7: smoke()'s bounds"""
    _against_the_cpu(name, *fp32_steps[name], R.UNetSpec(2, 3, FILTERS, 3, norm="group", groups=4), A.module(name))


def test_model_batchnorm_residual_gelu():
    """BatchNorm3d and residual=True: the residual add inside the last pass, at the same bounds; the running statistics
    follow the CPU's, and those of the very first normalisation -- whose input no activation has touched -- are the ReLU
    twin's bit for bit, as is every num_batches_tracked"""
    x, y = _batch()
    sds = {}
    for tag, cls, params in (("gelu", nn.GELU, {}), ("relu", nn.ReLU, {'inplace': True})):
        model = _model(cls, params, norm=nn.BatchNorm3d, residual=True).cuda().train()
        sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        step = _train_step(model, x.cuda(), y.cuda())
        sds[tag] = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        if tag == "gelu":
            sd_ref = _against_the_cpu("gelu BatchNorm residual", sd0, model, x, y, *step,
                                      R.UNetSpec(2, 3, FILTERS, 3, norm="batch", residual=True), nn.GELU())
    running = [k for k in sds["gelu"] if "running_" in k]
    assert len(running) >= 20
    for k in running:
        assert (sds["gelu"][k] - sd_ref[k].detach()).abs().max().item() <= 1e-5 * (1.0 + sd_ref[k].abs().max().item()), k
    first = "down_blocks.0.layers.norm0."
    assert torch.equal(sds["gelu"][first + "running_mean"], sds["relu"][first + "running_mean"])
    assert torch.equal(sds["gelu"][first + "running_var"], sds["relu"][first + "running_var"])
    assert not torch.equal(sds["gelu"]["down_blocks.0.layers.norm1.running_mean"], sds["relu"]["down_blocks.0.layers.norm1.running_mean"])
    assert all(int(sds[t][k]) == 1 for t in sds for k in sds[t] if k.endswith("num_batches_tracked"))


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("name", NAMES)
def test_model_16bit_flows(fp32_steps, name, prec):
    """c8 no-grad flow: finite probabilities that sum to 1 within 1e-5, and a non-zero distance to the fp32 flow of at most
    2x that of the LeakyReLU twin of the same weights on the same input (the same count of rounded values; the factor is
    slack for the different function).  c8 training flow: every parameter gradient finite, cosine with the fp32-flow
    gradient >= 0.95."""
    import segmentation_pipeline_amd as sp
    _, model, x, y, _, _, grads32 = fp32_steps[name]
    xd, yd = x.cuda(), y.cuda()
    twin = _model(nn.LeakyReLU, {}).cuda()
    twin.load_state_dict(model.state_dict())
    dist = {}
    for tag, m in (("new", copy.deepcopy(model)), ("twin", twin)):
        m.eval()
        with torch.no_grad():
            p32 = m(xd)
            with sp.precision(prec):
                p16 = m(xd)
        assert torch.isfinite(p16).all()
        assert (p16.sum(dim=1) - 1).abs().max().item() <= 1e-5
        dist[tag] = (p16 - p32).abs().max().item()
    print(f"activation_accuracy {name} {prec}: max |p16 - p32| {dist['new']:.4e}  LeakyReLU twin {dist['twin']:.4e}  "
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
    print(f"activation_accuracy {name} {prec}: c8 training flow, worst parameter cosine with the fp32 flow {worst_cos[0]:.4f} "
          f"({worst_cos[1]})")
    assert worst_cos[0] >= 0.95, worst_cos


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_graphed_train_step_reproduces_the_eager_losses(prec):
    """trainer.GraphedTrainStep on the SiLU model: three eager warm-up steps, then two replayed ones; the losses equal those
    of five eager steps from the same seed"""
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd.trainer import GraphedTrainStep
    m_e = _model(nn.SiLU, {}).cuda().train()
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
