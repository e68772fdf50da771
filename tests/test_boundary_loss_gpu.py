"""The boundary loss on the device: m355_signed_distance against the brute-force reference of
tests/boundary_ref.py -- bit for bit with unit spacing, within the distance tests' bound otherwise --, the loss kernels
against fp64 torch, criterions.BoundaryLoss on a model against the torch restatement, composed with DeepSupervisionLoss,
and its in-place mixing weights eagerly and under trainer.GraphedTrainStep.  Every figure is printed before it is asserted
(lines starting with `boundary_loss`)."""
import copy
import ctypes
from functools import partial

import numpy as np
import pytest
import torch
from torch import nn

import boundary_ref as B
import deep_supervision_ref as DS
import segmentation_pipeline_amd as sp
from oracle import torch_ref as R
from segmentation_pipeline_amd import _lib, ops
from segmentation_pipeline_amd.criterions import BoundaryLoss, DeepSupervisionLoss, HybridLogisticDiceLoss
from segmentation_pipeline_amd.models import DeepSupervisionUNet, ModularUNet
from segmentation_pipeline_amd.trainer import GraphedTrainStep

pytestmark = pytest.mark.gpu

GN8 = {'normalization_class': partial(nn.GroupNorm, 8)}
CONVT = dict(upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2})


# ------------------------------------------------------------------------------------------------------- the targets
def _random(shape, density, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < density).float()


def _ball_shell_uniform():
    """(1, 3, 24, 22, 24): a ball, a shell (a cavity inside: both signs on both sides of a surface) and a uniform plane"""
    z, y, x = torch.meshgrid(torch.arange(24.), torch.arange(22.), torch.arange(24.), indexing="ij")
    r2 = (z - 11.5) ** 2 + (y - 10.0) ** 2 + (x - 12.5) ** 2
    t = torch.zeros(1, 3, 24, 22, 24)
    t[0, 0] = (r2 <= 6.5 ** 2).float()
    t[0, 1] = ((r2 <= 9.0 ** 2) & (r2 >= 5.0 ** 2)).float()
    return t


def _single(value):
    """(1, 1, 8, 8, 130): one voxel of `value` in a corner of a volume of the other membership"""
    t = torch.full((1, 1, 8, 8, 130), 1.0 - value)
    t[0, 0, 7, 0, 129] = value
    return t


# name -> (target, planes or None).  The shapes are the issue's: one voxel; a row shorter than a chunk; a row longer than
# one 64-voxel chunk and no multiple of it, several rows per wave and more than one wave; 65-voxel rows and a 33-long outer
# axis (more than one block of 32 lines); hundreds of 3-voxel rows per wave; 130-voxel rows with the nearest voxel of the
# other membership up to 129 + 7 + 7 steps away; structures with curved borders.  Random membership at both densities.
def _cases():
    out = {"one_voxel_in": (torch.ones(1, 1, 1, 1, 1), None), "one_voxel_out": (torch.zeros(1, 1, 1, 1, 1), None),
           "corner_inside": (_single(1.0), None), "corner_outside": (_single(0.0), None),
           "ball_shell_uniform": (_ball_shell_uniform(), None),
           # (seven random voxels at density 0.02 or 0.9 are a uniform row: the short row with both memberships by hand)
           "1x2x1x1x7_mixed": (torch.tensor([[0., 1, 1, 0, 0, 1, 0], [1, 1, 0, 1, 1, 1, 1]]).reshape(1, 2, 1, 1, 7), None)}
    for i, shape in enumerate([(1, 2, 1, 1, 7), (2, 3, 3, 5, 70), (1, 2, 33, 2, 65), (1, 1, 5, 40, 3)]):
        for density in (0.02, 0.9):
            planes = [1, 0, 1, 1, 1, 0] if shape[:2] == (2, 3) and density == 0.9 else None
            out["x".join(map(str, shape)) + f"_d{density}"] = (_random(shape, density, 40 + i), planes)
    # rows of one membership each (every value entering the first line pass is +inf, lines hold both memberships), with a
    # slab of one membership (its lines of the first pass offer no candidate at all)
    rows = torch.zeros(1, 1, 4, 6, 70)
    rows[0, 0, :, 1::2, :] = 1.0
    rows[0, 0, 2] = 0.0
    out["uniform_rows_1x1x4x6x70"] = (rows, None)
    # the longest axis the transform takes, on each axis in turn: a line pass then stages 64 KiB of LDS, the sweep's run of
    # 1024 voxels is two rows
    for i, shape in enumerate([(1, 1, 512, 1, 3), (1, 1, 1, 512, 3), (1, 1, 1, 2, 512)]):
        out["x".join(map(str, shape)) + "_d0.02"] = (_random(shape, 0.02, 55 + i), None)
    # soft values on both sides of the threshold, a NaN and infinities: t > 0.5 decides, a NaN is outside
    soft = torch.rand((1, 2, 3, 5, 70), generator=torch.Generator().manual_seed(50))
    soft[0, 0, 1, 2, 3:9] = torch.tensor([float("nan"), 0.5, 0.50001, float("inf"), -float("inf"), 0.49999])
    out["soft_1x2x3x5x70"] = (soft, None)
    return out


CASES = _cases()
_ref_cache = {}


def _ref_f32(name):
    if name not in _ref_cache:
        t, planes = CASES[name]
        _ref_cache[name] = torch.from_numpy(B.signed_distance_f32(t.numpy(), planes))
    return _ref_cache[name]


def _by_edt_sq(t, planes, spacing=(1., 1., 1.)):
    """phi through the code that existed before the batched transform: two ops.edt_sq per plane on the two masks"""
    out = torch.zeros_like(t)
    N, C = t.shape[:2]
    for i in range(N * C):
        if planes is not None and not planes[i]:
            continue
        m = t[i // C, i % C] > 0.5
        if bool(m.all()) or not bool(m.any()):
            continue
        to_in = ops.edt_sqrt(ops.edt_sq(m.to(torch.uint8), spacing))
        to_out = ops.edt_sqrt(ops.edt_sq((~m).to(torch.uint8), spacing))
        out[i // C, i % C] = torch.where(m, 1.0 - to_out, to_in)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_signed_distance_unit_spacing_is_the_reference_bit_for_bit(name):
    t, planes = CASES[name]
    ref = _ref_f32(name)
    tg = t.cuda()
    before = tg.clone()
    phi = ops.signed_distance(tg, planes=planes)
    assert phi.shape == t.shape and phi.dtype == torch.float32 and phi.is_contiguous() and not phi.requires_grad
    diff = (phi.cpu() - ref).abs()
    print(f"boundary_loss signed distance {name}: {int((diff.nan_to_num(1.0) != 0).sum())} of {t.numel()} voxels differ, "
          f"max |phi| {ref.abs().max().item():.4f}")
    assert torch.equal(phi.cpu(), ref)
    assert torch.equal(tg.isnan(), before.isnan()) and torch.equal(tg.nan_to_num(7.0), before.nan_to_num(7.0)), "the target is unchanged"
    assert torch.equal(ops.signed_distance(tg, planes=planes), phi), "a second call gives the same bits"
    if planes is not None:
        N, C = t.shape[:2]
        for i, on in enumerate(planes):
            if not on:
                assert not phi[i // C, i % C].any(), f"plane {i} is off"
        assert torch.equal(ops.signed_distance(tg, planes=torch.tensor(planes).reshape(N, C)), phi)
    assert torch.equal(_by_edt_sq(tg, planes), phi), "the two-transform formulation through ops.edt_sq"


def test_all_planes_off_gives_zeros_and_uniform_planes_need_no_reduction():
    t = _random((2, 2, 3, 5, 70), 0.3, 60).cuda()
    assert not ops.signed_distance(t, planes=[0, 0, 0, 0]).any()
    t[1, 0] = 1.0
    t[0, 1] = 0.0
    phi = ops.signed_distance(t)
    assert not phi[1, 0].any() and not phi[0, 1].any() and phi[0, 0].any() and phi[1, 1].any()


@pytest.mark.parametrize("name", ["2x3x3x5x70_d0.9", "1x2x33x2x65_d0.02", "corner_inside"])
def test_raw_binding_keeps_the_canaries_and_the_target(name):
    """phi starts 5 floats into its buffer and the target 3 floats into its own (4-byte aligned only)"""
    L = _lib.lib()
    t, planes = CASES[name]
    n, n_planes = t.numel(), t.shape[0] * t.shape[1]
    size3 = (ctypes.c_int32 * 3)(*t.shape[2:])
    tbuf = torch.full((n + 6,), -7.0, device="cuda")
    tbuf[3:3 + n] = t.flatten().cuda()
    t_before = tbuf.clone()
    nbytes = int(L.m355_signed_distance_workspace(n_planes, size3))
    on = None if planes is None else (ctypes.c_uint8 * n_planes)(*planes)
    outs = []
    for _ in range(2):
        buf = torch.full((n + 12,), 123.25, device="cuda")
        ws = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        rc = L.m355_signed_distance(ctypes.c_void_p(tbuf.data_ptr() + 12), n_planes, size3, (ctypes.c_float * 3)(1, 1, 1), on,
                                    ctypes.c_void_p(buf.data_ptr() + 20), ctypes.c_void_p(ws.data_ptr()), nbytes,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.m355_last_error()
        torch.cuda.synchronize()
        assert torch.all(buf[:5] == 123.25) and torch.all(buf[5 + n:] == 123.25), "canary floats"
        assert torch.all(ws[nbytes:] == 0x5A), "the workspace's declared size"
        outs.append(buf[5:5 + n].clone())
    assert torch.equal(tbuf, t_before), "target"
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0].cpu(), _ref_f32(name).flatten())


SPACING = (0.7, 1.3, 2.0)


@pytest.mark.parametrize("name", ["2x3x3x5x70_d0.9", "1x2x33x2x65_d0.02", "ball_shell_uniform"])
def test_signed_distance_general_spacing(name):
    """|phi - ref| <= 1e-6 max(|ref|, 1): the bound of the distance tests for non-unit spacing"""
    t, planes = CASES[name]
    ref = torch.from_numpy(B.signed_distance(t.numpy(), SPACING, planes))
    phi = ops.signed_distance(t.cuda(), SPACING, planes)
    ratio = ((phi.cpu().double() - ref).abs() / (1e-6 * ref.abs().clamp(min=1.0))).max().item()
    print(f"boundary_loss signed distance {name} spacing {SPACING}: worst error / bound {ratio:.4f}")
    assert ratio <= 1.0
    assert torch.equal(_by_edt_sq(t.cuda(), planes, SPACING), phi), "the two-transform formulation has the same bits"


# ------------------------------------------------------------------------------------------------------ loss kernels
def _ill_conditioned(shape, seed):
    """values of both signs over six decades, arranged so that the sum cancels to a small fraction of the sum of moduli"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(shape, generator=g) * 10.0 ** (6 * torch.rand(shape, generator=g) - 3)
    flat = v.flatten()
    flat[1::2] = -flat[0::2][:flat[1::2].numel()] * (1 + 1e-3 * torch.randn(flat[1::2].shape, generator=g))
    return flat.reshape(shape).contiguous()


# (shape, class weights).  The issue's two, then the paths they leave out: a row of more than one 8192-element chunk with a
# partial last chunk, and a row of more than 64 chunks (a lane of the finalize kernel adds more than one of them).
LOSS_CASES = [((2, 3, 3, 5, 70), (0.0, 1.0, 2.0)), ((1, 4, 16, 16, 16), None), ((1, 2, 24, 22, 24), (1.0, 0.5)),
              ((1, 1, 65, 64, 130), None)]


@pytest.mark.parametrize("kind", ["transform", "ill_conditioned"])
@pytest.mark.parametrize("shape, weights", LOSS_CASES, ids=["x".join(map(str, s)) for s, _ in LOSS_CASES])
def test_loss_kernels_against_fp64(shape, weights, kind):
    g = torch.Generator().manual_seed(70)
    p = torch.softmax(2 * torch.randn(shape, generator=g), dim=1) if shape[1] > 1 else torch.rand(shape, generator=g)
    if kind == "transform":
        phi = ops.signed_distance(_random(shape, 0.3, 71).cuda()).cpu()
    else:
        phi = _ill_conditioned(shape, 72)
    w = (1.0,) * shape[1] if weights is None else weights
    wt = None if weights is None else torch.tensor(weights, device="cuda")
    ref, mass = B.loss(p, phi, w).item(), B.abs_mass(p, phi, w).item()
    pg = p.cuda().requires_grad_()
    loss = ops.boundary_loss(pg, phi.cuda(), wt)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
    err, bound = abs(loss.double().item() - ref), 2.0 ** -23 * mass
    print(f"boundary_loss loss {shape} {kind}: loss {loss.item():.7e} ref {ref:.7e}  err {err:.3e}  bound {bound:.3e} "
          f"(cancellation {abs(ref) / mass:.2e})")
    assert err <= bound
    dloss = torch.tensor(0.37, device="cuda")
    loss.backward(dloss)
    dref = B.grad(phi, w, dloss.item())
    derr = (pg.grad.cpu().double() - dref).abs()
    worst = (derr / (2.0 ** -22 * dref.abs()).clamp(min=1e-300)).max().item()
    print(f"boundary_loss gradient {shape} {kind}: worst error / bound {worst:.4f}")
    assert bool((derr <= 2.0 ** -22 * dref.abs()).all())
    for c, wc in enumerate(w):
        if wc == 0.0:
            assert not pg.grad[:, c].any(), "a channel without weight gets exactly zero"
    pg2 = p.cuda().requires_grad_()
    again = ops.boundary_loss(pg2, phi.cuda(), wt)
    again.backward(dloss)
    assert torch.equal(again, loss) and torch.equal(pg2.grad, pg.grad), "a second call gives the same bits"
    pg3 = p.cuda().requires_grad_()
    ops.boundary_loss(pg3, phi.cuda(), wt).backward()      # dloss = 1 is another gradient
    assert not torch.equal(pg3.grad, pg.grad)


def test_zero_weight_rows_are_not_read():
    """NaN and infinity in p and phi of a channel without weight reach neither the loss nor the gradient"""
    shape = (2, 3, 3, 5, 70)
    g = torch.Generator().manual_seed(73)
    p = torch.softmax(torch.randn(shape, generator=g), dim=1)
    phi = _ill_conditioned(shape, 74)
    w = (0.0, 1.0, 2.0)
    ref = B.loss(p, phi, w).item()
    p[:, 0, 0, 0, :3] = torch.tensor([float("nan"), float("inf"), -float("inf")])
    phi[:, 0, 1, 1, :2] = torch.tensor([float("nan"), float("inf")])
    pg = p.cuda().requires_grad_()
    loss = ops.boundary_loss(pg, phi.cuda(), torch.tensor(w, device="cuda"))
    loss.backward()
    assert abs(loss.double().item() - ref) <= 2.0 ** -23 * B.abs_mass(p[:, 1:], phi[:, 1:], w[1:]).item()
    assert not pg.grad[:, 0].any() and torch.isfinite(pg.grad).all()


# ----------------------------------------------------------------------------------------------------------- criterion
def _blobs_target():
    """1 x 3 x 16^3 one-hot: two blobs of class 1, class 2 absent"""
    z, y, x = torch.meshgrid(torch.arange(16.), torch.arange(16.), torch.arange(16.), indexing="ij")
    blob = ((z - 4) ** 2 + (y - 5) ** 2 + (x - 4) ** 2 <= 9.5) | ((z - 11) ** 2 + (y - 10) ** 2 + (x - 12) ** 2 <= 5.5)
    t = torch.zeros(1, 3, 16, 16, 16)
    t[0, 1] = blob.float()
    t[0, 0] = 1.0 - t[0, 1]
    return t


def _criterion_model():
    torch.manual_seed(0)
    return ModularUNet(2, 3, [8, 16, 16], 3, block_params={'normalization_class': partial(nn.GroupNorm, 4)})


def test_criterion_matches_the_torch_restatement_fp32():
    model = _criterion_model()
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn((1, 2, 16, 16, 16), generator=torch.Generator().manual_seed(80))
    y = _blobs_target()
    w, bw, rw = (0.0, 1.0, 1.0), 0.05, 0.75
    phi_ref = torch.from_numpy(B.signed_distance_f32(y.numpy()))
    assert phi_ref[0, 1].any() and not phi_ref[0, 2].any()
    spec = R.UNetSpec(2, 3, [8, 16, 16], 3, norm="group", groups=4)
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd0.items()}
    p_ref = R.unet_forward(sd, spec, x, training=True)
    regional_ref = R.hybrid_logistic_dice_loss(p_ref, y)["loss"]
    boundary_ref = B.loss(p_ref, phi_ref, w)
    total_ref = rw * regional_ref.double() + bw * boundary_ref
    total_ref.backward()

    model = model.cuda().train()
    crit = BoundaryLoss(HybridLogisticDiceLoss(), boundary_weight=bw, regional_weight=rw)
    p = model(x.cuda())
    ld = crit(p, y.cuda())
    assert list(ld) == ['loss', 'dice_loss', 'logistic_loss', 'boundary_loss', 'regional_loss', 'boundary_weight', 'regional_weight']
    assert all(torch.is_tensor(v) and v.is_cuda for v in ld.values())
    assert not ld['boundary_loss'].requires_grad and not ld['regional_loss'].requires_grad and ld['loss'].requires_grad
    ld["loss"].backward()
    # the boundary term on the device's own probabilities, within the bound of the kernel test
    own = B.loss(p.detach().cpu(), phi_ref, w).item()
    err, bound = abs(ld['boundary_loss'].double().item() - own), 2.0 ** -23 * B.abs_mass(p.detach().cpu(), phi_ref, w).item()
    print(f"boundary_loss criterion: boundary {ld['boundary_loss'].item():.7e} fp64 {own:.7e} err {err:.3e} bound {bound:.3e}; "
          f"restatement boundary {boundary_ref.item():.7e} total {ld['loss'].item():.7f} vs {total_ref.item():.7f}")
    assert err <= bound
    assert abs(ld['boundary_loss'].item() - boundary_ref.item()) <= 1e-4 and abs(ld['loss'].item() - total_ref.item()) <= 1e-4
    by_hand = ld['regional_weight'] * ld['regional_loss'] + ld['boundary_weight'] * ld['boundary_loss']
    assert torch.equal(ld['loss'].detach(), by_hand)
    assert ld['boundary_weight'].item() == np.float32(bw) and ld['regional_weight'].item() == np.float32(rw)
    worst = 0.0
    for k, v in model.named_parameters():
        ref = sd[k].grad
        e, scale = (v.grad.cpu() - ref).abs().max().item(), ref.abs().max().item()
        worst = max(worst, e / (1e-3 * scale + 1e-7))
        assert e <= 1e-3 * scale + 1e-7, f"grad {k}: {e:.3e} vs scale {scale:.3e}"
    print(f"boundary_loss criterion: worst gradient error / bound {worst:.3f}")


def test_criterion_bf16():
    model = _criterion_model().cuda().train()
    x = torch.randn((1, 2, 16, 16, 16), generator=torch.Generator().manual_seed(80)).cuda()
    crit = BoundaryLoss(HybridLogisticDiceLoss(), boundary_weight=0.05)
    with sp.precision("bf16"):
        ld = crit(model(x), _blobs_target().cuda())
        ld["loss"].backward()
    print(f"boundary_loss criterion bf16: loss {ld['loss'].item():.6f} boundary {ld['boundary_loss'].item():.6f}")
    assert torch.isfinite(ld["loss"]) and torch.isfinite(ld["boundary_loss"])
    for k, v in model.named_parameters():
        assert v.grad is not None and torch.isfinite(v.grad).all() and v.grad.abs().max().item() > 0, k


# --------------------------------------------------------------------------------------------------------- composition
def _batch(shape, classes, seed):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return x, DS.one_hot_target((shape[0], classes) + tuple(shape[2:]), seed + 1)


@pytest.mark.parametrize("mode", ["area", "nearest"])
def test_composition_with_deep_supervision(mode):
    torch.manual_seed(5)
    model = DeepSupervisionUNet(2, 3, [8, 16, 24], 3, aux_levels=1, block_params=dict(GN8), **CONVT).cuda().train()
    x, y = _batch((1, 2, 16, 16, 16), 3, 200)
    x, y = x.cuda(), y.cuda()
    inner = BoundaryLoss(HybridLogisticDiceLoss(), boundary_weight=0.1)
    out = model(x)
    assert len(out) == 2
    ld = DeepSupervisionLoss(inner, target_mode=mode)(out, y)
    assert 'loss_level1' in ld and 'boundary_loss' in ld and 'regional_loss' in ld
    targets = [y] + ops.target_pyramid(y, 1, mode)
    by_hand = [inner(p.detach(), t) for p, t in zip(out, targets)]
    w = DS.default_weights(2)
    total = w[0] * by_hand[0]["loss"]
    total = total + w[1] * by_hand[1]["loss"]
    print(f"boundary_loss composition {mode}: total {ld['loss'].item():.7f} levels {[round(d['loss'].item(), 6) for d in by_hand]} "
          f"boundary terms {[round(d['boundary_loss'].item(), 6) for d in by_hand]}")
    assert torch.equal(ld["loss"].detach(), total)
    assert torch.equal(ld["loss_level1"], by_hand[1]["loss"]) and torch.equal(ld["boundary_loss"], by_hand[0]["boundary_loss"])
    ld["loss"].backward()
    for k, v in model.named_parameters():
        assert v.grad is not None and torch.isfinite(v.grad).all() and v.grad.abs().max().item() > 0, k


# ----------------------------------------------------------------------------------------------------- weights, graphs
def test_set_weights_changes_the_next_loss_in_place():
    g = torch.Generator().manual_seed(90)
    p = torch.softmax(torch.randn((1, 3, 8, 8, 8), generator=g), dim=1).cuda()
    y = DS.one_hot_target((1, 3, 8, 8, 8), 91).cuda()
    crit = BoundaryLoss(HybridLogisticDiceLoss())
    first = crit(p, y)
    ptrs = crit.regional_weight.data_ptr(), crit.boundary_weight.data_ptr()
    assert crit.regional_weight.is_cuda and first['boundary_weight'].item() == np.float32(0.01)
    crit.set_weights(regional=0.5, boundary=0.25)
    second = crit(p, y)
    assert (crit.regional_weight.data_ptr(), crit.boundary_weight.data_ptr()) == ptrs
    assert first['boundary_weight'].item() == np.float32(0.01), "the dict holds its own copy"
    assert torch.equal(second['boundary_loss'], first['boundary_loss']) and torch.equal(second['regional_loss'], first['regional_loss'])
    half, quarter = torch.tensor(0.5, device="cuda"), torch.tensor(0.25, device="cuda")
    assert torch.equal(second['loss'], half * second['regional_loss'] + quarter * second['boundary_loss'])
    assert not torch.equal(second['loss'], first['loss'])


def _train_batches(n, seed=21):
    out = []
    for i in range(n):
        x, y = _batch((2, 4, 16, 16, 16), 3, seed + 10 * i)
        out.append({"X": x.cuda(), "y": y.cuda()})
    return out


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_graphed_train_step_follows_set_weights_like_the_eager_loop(mode):
    """three eager warm-up calls, the capture with its replay and four more replays; the boundary weight changes twice
    between replays: losses and final weights equal the eager loop's with the same changes, bit for bit"""
    torch.manual_seed(0)
    m_e = ModularUNet(4, 3, [8, 16, 24], 3, block_params=dict(GN8), **CONVT).cuda().train()
    m_g = copy.deepcopy(m_e)
    batches = _train_batches(8)
    crit_e = BoundaryLoss(HybridLogisticDiceLoss(), boundary_weight=0.02)
    crit_g = BoundaryLoss(HybridLogisticDiceLoss(), boundary_weight=0.02)
    with sp.precision(mode):
        opt_e = torch.optim.SGD(m_e.parameters(), lr=1e-2, momentum=0.9)
        opt_g = torch.optim.SGD(m_g.parameters(), lr=1e-2, momentum=0.9)
        step = GraphedTrainStep(m_g, crit_g, opt_g, warmup=3)
        losses_e, losses_g, bnd_e, bnd_g, bw_g = [], [], [], [], []
        for i, b in enumerate(batches):
            # calls 0..2 are eager, call 3 captures and replays once, calls 4..7 replay.  The weight changes after the
            # second replay counted with the capture's own (before call 5) and again after the second counted without it
            if i in (5, 6):
                ptr = crit_g.boundary_weight.data_ptr()
                crit_e.set_weights(boundary=0.5 if i == 5 else 0.25)
                crit_g.set_weights(boundary=0.5 if i == 5 else 0.25)
                assert crit_g.boundary_weight.data_ptr() == ptr
            opt_e.zero_grad(set_to_none=True)
            ld = crit_e(m_e(b["X"]), b["y"])
            ld["loss"].backward()
            opt_e.step()
            losses_e.append(ld["loss"].detach().clone())
            bnd_e.append(ld["boundary_loss"].clone())
            got = step(b)
            losses_g.append(got["loss"])
            bnd_g.append(got["boundary_loss"])
            bw_g.append(got["boundary_weight"])
    print(f"boundary_loss graphed {mode}: losses {[round(l.item(), 5) for l in losses_g]}")
    assert torch.equal(torch.stack(losses_e), torch.stack(losses_g))
    assert torch.equal(torch.stack(bnd_e), torch.stack(bnd_g))
    assert [round(v.item(), 6) for v in bw_g] == [0.02] * 5 + [0.5] + [0.25] * 2, "a replay reads the buffer it was captured with"
    for (k, a), (_, b) in zip(m_e.state_dict().items(), m_g.state_dict().items()):
        assert torch.equal(a, b), k
    assert len(step._graphs) == 1 and next(iter(step._graphs.values()))["graph"] is not None
