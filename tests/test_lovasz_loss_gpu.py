"""The segmented radix sort and the Lovasz-softmax loss on the device: m355_segmented_sort_u32 bit for bit against
torch.sort on the CPU; m355_lovasz_loss_fwd / _bwd against the fp64 closed form of tests/lovasz_ref.py in both segment
layouts, both reductions, weighted and not; ties, saturated and tiny probabilities, absent and all-foreground classes,
values outside [0, 1]; determinism, misaligned views and recycled memory; the autograd function, the models in the three
activation flows, the wrappers, and the captured train step that follows set_weights.
The lines starting with `lovasz_loss_accuracy` are what profiles/lovasz_loss_accuracy.txt records."""
import copy
from functools import partial

import pytest
import torch
from torch import nn

import lovasz_ref as V
from raw_ops import PoisonedEmpty, assert_recycled
from segmentation_pipeline_amd import _lib, ops
from segmentation_pipeline_amd.criterions import (BoundaryLoss, DeepSupervisionLoss, HybridBinaryLogisticDiceLoss,
                                                  HybridLogisticDiceLoss, LovaszLoss)
from segmentation_pipeline_amd.models import DeepSupervisionUNet, ModularUNet

pytestmark = pytest.mark.gpu

DLOSS = 0.7
WEIGHTS = {2: [1.0, 2.5], 3: [1.0, 0.5, 2.0], 5: [1.0, 0.5, 2.0, 0.0, 3.0]}


def close(got, ref, rtol, atol, what, torch32=None):
    """tests/test_kernels_gpu.py's close(): max |got - ref| <= atol + rtol * max |ref|; prints the figure first"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, bound = (got - ref).abs().max().item(), atol + rtol * ref.abs().max().item()
    t32 = "" if torch32 is None else f"  torch fp32 on the CPU {(torch32.double() - ref).abs().max().item():.3e}"
    print(f"lovasz_loss_accuracy {what}: max err {err:.3e}  bound {bound:.3e}{t32}")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


# ------------------------------------------------------------------------------------------------------------- the sort
def _as_i32(u):
    """int64 values in [0, 2^32) -> the int32 tensor of the same bits"""
    return torch.where(u >= 1 << 31, u - (1 << 32), u).to(torch.int32)


def _as_u(i32):
    return i32.cpu().long() & 0xffffffff


def _sorted_on_the_cpu(u, end_bit):
    """the stable sort by the bits [0, end_bit): the bits above travel with their key"""
    order = torch.sort(u & ((1 << end_bit) - 1), dim=1, stable=True).indices
    return torch.gather(u, 1, order)


def _patterns(R, M, g):
    rnd = torch.randint(0, 1 << 32, (R, M), generator=g, dtype=torch.int64)
    yield "random", rnd
    yield "all equal", torch.full((R, M), 0x12345678, dtype=torch.int64)
    yield "top digit only", (rnd >> 24) << 24
    yield "bottom digit only", rnd & 0xff
    yield "two values per digit", rnd & 0x01010101
    ordered = torch.sort(rnd & 0x7fffffff, dim=1).values
    yield "sorted", ordered
    yield "reversed", ordered.flip(1)


def _sort_sizes():
    T = V.sort_tile()
    return [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]


@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("which", range(8))
def test_sort_is_torch_sort_bit_for_bit(hip, which, R):
    """M = 1, 63, 64, 65, one tile - 1, one tile, one tile + 1, three tiles and a remainder; end_bit 32, and 31 with the top
    bit as a payload that a stable sort leaves in input order"""
    M = _sort_sizes()[which]
    g = torch.Generator().manual_seed(100 * which + R)
    for name, u in _patterns(R, M, g):
        for end_bit in (31, 32):
            got = _as_u(V.raw_sort(hip, _as_i32(u).cuda(), end_bit))
            assert torch.equal(got, _sorted_on_the_cpu(u, end_bit)), (name, M, R, end_bit)


def test_sort_is_stable_in_every_pass_and_sorts_only_the_low_bits(hip):
    """end_bit 1, 8, 9, 16, 20: the 32 - end_bit bits above are each key's position in the input, so the result is the
    stable sort's or none; more than 64 tiles per segment: the scan kernel's carry along a digit row"""
    T = V.sort_tile()
    R, M = 2, 66 * T + 5
    g = torch.Generator().manual_seed(7)
    for end_bit in (1, 8, 9, 16, 20):
        low = torch.randint(0, 1 << min(end_bit, 3), (R, M), generator=g, dtype=torch.int64)   # few values: long runs of ties
        pos = torch.arange(M, dtype=torch.int64)[None, :] & ((1 << (32 - end_bit)) - 1)
        u = (pos << end_bit) | low
        got = _as_u(V.raw_sort(hip, _as_i32(u).cuda(), end_bit))
        assert torch.equal(got, _sorted_on_the_cpu(u, end_bit)), end_bit


def test_ops_segmented_sort(hip):
    g = torch.Generator().manual_seed(3)
    keys = torch.randint(0, 1 << 31, (3, 5000), generator=g, dtype=torch.int64).to(torch.int32)
    got = ops.segmented_sort(keys.cuda())
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), torch.sort(keys, dim=1).values)
    view = keys.cuda().t().contiguous().t()          # not contiguous
    assert not view.is_contiguous() and torch.equal(ops.segmented_sort(view), got)


# ------------------------------------------------------------------------------------------------ kernels against fp64
_inputs = {}


def inputs(case):
    if case not in _inputs:
        _inputs[case] = V.softmax_inputs(V.CASES[case], sorted(V.CASES).index(case) + 21)
    return _inputs[case]


def _cfg(classes, per_image, weighted, channels):
    return dict(classes=classes, per_image=per_image, class_weights=WEIGHTS[channels] if weighted else None)


def _check(hip, p, t, cfg, tag, key=None):
    """one forward and backward on the device against the closed form; -> (out2, dx, state)"""
    ref = V.closed_form(p, t, DLOSS, key=key, **cfg)
    loss32, dx32 = V.torch32(p, t, DLOSS, key=key, **cfg)
    pd, td = p.cuda(), t.cuda()
    out2, skeys, F, state = V.raw_fwd(hip, pd, td, **cfg)
    dx = V.raw_bwd(hip, pd, td, skeys, F, state, DLOSS, **cfg)
    close(out2[0], ref['loss'], 2e-6, 1e-7, f"{tag} loss", loss32)
    close(dx, ref['dx'], 1e-5, 1e-9, f"{tag} dx", dx32)
    G, _ = V.state_fields(state)
    assert torch.equal(G, ref['G']) and out2[1].item() == ref['count']
    assert bool(torch.isfinite(out2).all()) and bool(torch.isfinite(dx).all())
    return out2, dx, state


FWD_BWD = [pytest.param(case, pi, c, w, id=f"{case}-{'image' if pi else 'batch'}-{c}-{'w' if w else 'ones'}")
           for case in V.CASES for pi in (False, True) for c in V.CLASSES for w in (False, True)]


@pytest.mark.parametrize("case,per_image,classes,weighted", FWD_BWD)
def test_fwd_bwd_against_fp64(hip, case, per_image, classes, weighted):
    """'loss' within close(2e-6, 1e-7), the gradient for dloss = 0.7 within close(1e-5, 1e-9) -- the bounds of
    test_hybrid_loss_fwd_bwd -- and the foreground counts and the number of segments averaged exactly"""
    p, t = inputs(case)
    cfg = _cfg(classes, per_image, weighted, p.shape[1])
    tag = f"{case} {'per image' if per_image else 'batch'} {classes} {'weights' if weighted else 'ones'}"
    _check(hip, p, t, cfg, tag, key=case)


# ------------------------------------------------------------------------------------------------------- ties and edges
EDGE = (2, 3, 11, 13, 17)     # S = 2431: odd rows, less than one tile; M = 4862 for the batch: two tiles


@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "image"])
def test_a_constant_prediction_is_one_group_per_foreground_value(hip, per_image):
    """p = 0.25 everywhere: e = 0.75 on the foreground, 0.25 on the background; every member of a group gets the same
    gradient bits, and loss and gradient are the closed form's.  The background comes after the whole foreground, where
    the Jaccard loss is 1 already: its gradient is 0"""
    _, t = V.softmax_inputs(EDGE, 31)
    p = torch.full(EDGE, 0.25)
    _, dx, _ = _check(hip, p, t, _cfg('present', per_image, False, 3), f"constant {'per image' if per_image else 'batch'}")
    dxs, ts = V.segments(dx.cpu(), per_image), V.segments(t, per_image)
    for r in range(dxs.shape[0]):
        on, off = dxs[r][ts[r] == 1], dxs[r][ts[r] == 0]
        assert bool((on == on[0]).all()) and bool((off == off[0]).all()) and on[0].item() < 0 == off[0].item()


@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "image"])
def test_saturated_and_tiny_probabilities(hip, per_image):
    """a prediction that is exactly 0 or 1 on nine voxels of ten (e = 0 and e = 1 in large groups, the one-sided
    derivative at e = 0), and probabilities from 1e-30 to 1 (keys that differ in every digit)"""
    g = torch.Generator().manual_seed(32)
    p, t = V.softmax_inputs(EDGE, 33)
    hard = (torch.rand(EDGE, generator=g) < 0.5).float()
    sat = torch.where(torch.rand(EDGE, generator=g) < 0.9, hard, p)
    for classes in V.CLASSES:
        _, dx, _ = _check(hip, sat, t, _cfg(classes, per_image, True, 3), f"saturated {'per image' if per_image else 'batch'} {classes}")
    right = (sat == t).cpu() & (t == 1)
    assert int(right.sum()) > 100 and bool((dx.cpu()[right] <= 0).all())
    tiny = torch.pow(10.0, -30 * torch.rand(EDGE, generator=g)).clamp(0, 1)
    assert tiny.min().item() < 1e-25 and tiny.max().item() > 0.5
    _check(hip, tiny, t, _cfg('all', per_image, False, 3), f"1e-30..1 {'per image' if per_image else 'batch'}")


@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "image"])
def test_absent_and_all_foreground_classes(hip, per_image):
    """channel 0 has no foreground, channel 1 only foreground, channel 2 both; then nothing present at all"""
    g = torch.Generator().manual_seed(34)
    p = torch.rand(EDGE, generator=g)
    t = torch.zeros(EDGE)
    t[:, 1] = 1.0
    t[:, 2] = (torch.rand((2, 11, 13, 17), generator=g) < 0.2).float()
    where = 'per image' if per_image else 'batch'
    out_p, dx_p, state = _check(hip, p, t, _cfg('present', per_image, False, 3), f"absent class {where} present")
    assert bool((dx_p[:, 0] == 0).all()) and out_p[1].item() == (4 if per_image else 2)
    assert V.state_fields(state)[1].reshape(-1, 3)[:, 0].abs().max().item() == 0.0
    out_a, dx_a, _ = _check(hip, p, t, _cfg('all', per_image, False, 3), f"absent class {where} all")
    assert bool((dx_a[:, 0] != 0).any()) and out_a[1].item() == (6 if per_image else 3)
    none, dx_n, _ = _check(hip, p, torch.zeros(EDGE), _cfg('present', per_image, True, 3), f"nothing present {where}")
    assert none[0].item() == 0.0 and none[1].item() == 0.0 and bool((dx_n == 0).all())
    if per_image:       # image 1 empty, image 0 not: 0 for it, and it counts in the mean
        t1 = t.clone()
        t1[1] = 0.0
        half, dx_h, _ = _check(hip, p, t1, _cfg('present', True, False, 3), "one empty image")
        assert bool((dx_h[1] == 0).all()) and half[1].item() == 2


def _guarded(n, dtype, guard=64):
    """(whole buffer, the n elements between two guards): 0x5A bytes everywhere"""
    size = torch.empty(0, dtype=dtype).element_size()
    buf = torch.full(((n + 2 * guard) * size,), 0x5A, dtype=torch.uint8, device="cuda")
    return buf, buf.view(dtype)[guard:guard + n]


def _guards_intact(buf, n, dtype, guard=64):
    size = torch.empty(0, dtype=dtype).element_size()
    return bool((buf[:guard * size] == 0x5A).all()) and bool((buf[(guard + n) * size:] == 0x5A).all())


@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "image"])
@pytest.mark.parametrize("bad", [float("nan"), 1.5, -0.25, float("inf")])
def test_a_value_outside_the_unit_interval_gives_nan_and_stays_inside_the_buffers(hip, bad, per_image):
    p, t = inputs("blocks")
    p = p.clone()
    p[1, 2, 3, 4, 5] = bad
    N, C_ = p.shape[:2]
    n, S = p.numel(), p.numel() // (N * C_)
    nbytes = int(_lib.lib().m355_lovasz_loss_workspace(N, C_, S, int(per_image)))
    ws = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    kbuf, skeys = _guarded(n, torch.int32)
    fbuf, F = _guarded(n, torch.int32)
    dbuf, dx = _guarded(n, torch.float32)
    pd, td = p.cuda(), t.cuda()
    out2, _, _, state = V.raw_fwd(hip, pd, td, per_image=per_image, skeys=skeys, F=F, ws=ws[:nbytes])
    V.raw_bwd(hip, pd, td, skeys, F, state, DLOSS, per_image=per_image, out=dx.view(p.shape))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out2[0])) and bool(torch.isnan(dx).all())
    assert bool((ws[nbytes:] == 0x5A).all()), "the workspace's declared size"
    assert _guards_intact(kbuf, n, torch.int32) and _guards_intact(fbuf, n, torch.int32) and _guards_intact(dbuf, n, torch.float32)
    R, M = (N * C_, S) if per_image else (C_, N * S)
    sk = skeys.cpu().reshape(R, M)
    assert bool((sk >= 0).all()) and bool((sk[:, 1:] >= sk[:, :-1]).all()), "every key inside 31 bits, every segment sorted"
    # the next call on the same buffers is clean again: the status word is reset by every forward
    good, _, _, _ = V.raw_fwd(hip, inputs("blocks")[0].cuda(), td, per_image=per_image, skeys=skeys, F=F, ws=ws[:nbytes])
    assert bool(torch.isfinite(good[0]))


# ------------------------------------------------------------------------------------------------- determinism, memory
@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "image"])
@pytest.mark.parametrize("case", ["tiny", "ragged", "blocks"])
def test_determinism_and_misaligned_views(hip, case, per_image):
    """two calls give the same bits; views offset by one element (not 16-byte aligned) give the bits of their aligned
    clones, in every output; the floats around dx stay"""
    p, t = inputs(case)
    cfg = _cfg('present', per_image, True, p.shape[1])
    n = p.numel()
    pd, td = p.cuda(), t.cuda()
    first = V.raw_fwd(hip, pd, td, **cfg)
    second = V.raw_fwd(hip, pd, td, **cfg)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    out2, skeys, F, state = first
    dx = V.raw_bwd(hip, pd, td, skeys, F, state, DLOSS, **cfg)
    assert torch.equal(dx, V.raw_bwd(hip, pd, td, skeys, F, state, DLOSS, **cfg))
    pb, tb = torch.zeros(n + 8, device="cuda"), torch.zeros(n + 8, device="cuda")
    kb, fb = torch.zeros(n + 8, dtype=torch.int32, device="cuda"), torch.zeros(n + 8, dtype=torch.int32, device="cuda")
    pb[1:1 + n], tb[1:1 + n] = pd.flatten(), td.flatten()
    po, to = pb[1:1 + n].view(p.shape), tb[1:1 + n].view(p.shape)
    assert po.data_ptr() % 16 != 0 and to.data_ptr() % 16 != 0 and pd.data_ptr() % 16 == 0
    out2_o, skeys_o, F_o, state_o = V.raw_fwd(hip, po, to, skeys=kb[1:1 + n], F=fb[1:1 + n], **cfg)
    assert torch.equal(out2_o, out2) and torch.equal(skeys_o, skeys) and torch.equal(F_o, F) and torch.equal(state_o, state)
    assert kb[0].item() == 0 and not kb[1 + n:].any() and fb[0].item() == 0 and not fb[1 + n:].any()
    guard = 64
    buf_o = torch.full((n + 2 * guard + 1,), 7.0, device="cuda")
    dx_o = V.raw_bwd(hip, po, to, skeys_o, F_o, state_o, DLOSS, out=buf_o[guard + 1:guard + 1 + n].view(p.shape), **cfg)
    assert dx_o.data_ptr() % 16 != 0 and torch.equal(dx_o, dx)
    assert bool((buf_o[:guard + 1] == 7.0).all()) and bool((buf_o[guard + 1 + n:] == 7.0).all())


@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "image"])
def test_recycled_memory(hip, per_image):
    """tests/raw_ops.py's protocol: the sort and the loss on zeroed, stale, 0xFF and NaN-canary workspaces and outputs
    with a guarded tail give the bits of the clean run"""
    p, t = inputs("blocks")
    p2, t2 = V.softmax_inputs(V.CASES["blocks"], 99)
    cfg = _cfg('all', per_image, True, p.shape[1])
    ref = V.closed_form(p, t, DLOSS, key="blocks", **cfg)
    keys = torch.randint(0, 1 << 31, (3, 9000), generator=torch.Generator().manual_seed(1), dtype=torch.int64).to(torch.int32)

    def run_on(p, t, keys):
        pd, td = p.cuda(), t.cuda()
        out2, skeys, F, state = V.raw_fwd(hip, pd, td, **cfg)
        dx = V.raw_bwd(hip, pd, td, skeys, F, state, DLOSS, **cfg)
        return {'out2': out2, 'skeys': skeys, 'F': F, 'state': state, 'dx': dx, 'sorted': V.raw_sort(hip, keys.cuda(), 31)}

    def reference(got):
        close(got['out2'][0], ref['loss'], 2e-6, 1e-7, f"recycled {'per image' if per_image else 'batch'} loss")
        close(got['dx'], ref['dx'], 1e-5, 1e-9, f"recycled {'per image' if per_image else 'batch'} dx")
        assert torch.equal(got['sorted'].cpu(), torch.sort(keys, dim=1).values)
    assert_recycled(hip, lambda: run_on(p, t, keys), lambda: run_on(p2, t2, keys.flip(1)), reference)


@pytest.mark.parametrize("mode", ["zeros", "ones", "nan"])
def test_the_autograd_function_on_poisoned_allocations(hip, monkeypatch, mode):
    p, t = inputs("ragged")
    cw = torch.tensor(WEIGHTS[3], device="cuda")

    def run():
        pd = p.cuda().requires_grad_(True)
        loss = ops.lovasz_loss(pd, t.cuda(), 'present', True, cw)
        (loss * DLOSS).backward()
        return loss.detach().clone(), pd.grad.clone()
    clean = run()
    with PoisonedEmpty(monkeypatch, mode) as poison:
        got = run()
    assert poison.dirtied >= 5
    assert torch.equal(clean[0], got[0]) and torch.equal(clean[1], got[1])


# --------------------------------------------------------------------------------------------------------- integration
@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "image"])
def test_autograd_function_matches_the_entry_points(hip, per_image):
    p, t = inputs("ragged")
    cfg = _cfg('all', per_image, True, 3)
    pd = p.cuda().requires_grad_(True)
    loss = ops.lovasz_loss(pd, t.cuda(), 'all', per_image, torch.tensor(cfg['class_weights'], device="cuda"))
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad
    (loss * DLOSS).backward()
    out2, skeys, F, state = V.raw_fwd(hip, p.cuda(), t.cuda(), **cfg)
    assert torch.equal(loss.detach(), out2[0])
    assert torch.equal(pd.grad, V.raw_bwd(hip, p.cuda(), t.cuda(), skeys, F, state, DLOSS, **cfg))
    # the criterion alone is lovasz_weight times the op
    crit = LovaszLoss(None, 0.5, classes='all', per_image=per_image, lovasz_class_weights=cfg['class_weights'])
    ld = crit(p.cuda(), t.cuda())
    assert torch.equal(ld['lovasz_loss'], out2[0]) and torch.equal(ld['loss'], 0.5 * out2[0])
    assert set(crit._uploaded) == {"lovasz_class_weights"}


FILTERS = [8, 16]
GN4 = {'normalization_class': partial(nn.GroupNorm, 4)}


def _unet(head=nn.Softmax, params=None):
    torch.manual_seed(0)
    return ModularUNet(2, 3, FILTERS, 2, block_params=dict(GN4), hypothesis_class=head,
                       hypothesis_params={"dim": 1} if params is None else params)


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
def test_model_step_equals_the_raw_op_path(prec):
    """one training step of the ModularUNet in each activation flow with LovaszLoss(HybridLogisticDiceLoss()): loss and
    every parameter gradient finite and, bit for bit, those of the same step with the two terms taken through ops"""
    import segmentation_pipeline_amd as sp
    model = _unet().cuda().train()
    x, y = _batch(2, 3)
    x, y = x.cuda(), y.cuda()
    crit = LovaszLoss(HybridLogisticDiceLoss(), 0.75, 0.5, lovasz_class_weights=[1, 2, 3])
    cw = torch.tensor([1.0, 2.0, 3.0], device="cuda")
    wl, wr = torch.tensor(0.75, device="cuda"), torch.tensor(0.5, device="cuda")

    def raw(out, target):
        regional = ops.hybrid_logistic_dice_loss(out, target)[0]
        return {'loss': wr * regional + wl * ops.lovasz_loss(out, target, 'present', False, cw)}
    with sp.precision(prec):
        ops.fp16_overflow()
        ld, grads = _step(model, crit, x, y)
        ld_raw, grads_raw = _step(model, raw, x, y)
    print(f"lovasz_loss_accuracy unet {prec}: loss {ld['loss'].item():.6f} regional {ld['regional_loss'].item():.6f} "
          f"lovasz {ld['lovasz_loss'].item():.6f}")
    assert all(bool(torch.isfinite(v)) for v in ld.values()) and len(grads) > 10
    assert 0 < ld['lovasz_loss'].item() <= 1
    assert torch.equal(ld['loss'], ld_raw['loss'])
    for k, g in grads.items():
        assert bool(torch.isfinite(g).all()) and torch.equal(g, grads_raw[k]), k
    assert any(g.abs().max().item() > 0 for g in grads.values())


def test_a_sigmoid_head_model_runs():
    model = _unet(nn.Sigmoid, {}).cuda().train()
    x, y = _batch(2, 3)
    ld, grads = _step(model, LovaszLoss(HybridBinaryLogisticDiceLoss(), per_image=True), x.cuda(), y.cuda())
    assert {'loss', 'dice_loss', 'logistic_loss', 'lovasz_loss', 'regional_loss'} <= set(ld)
    assert all(bool(torch.isfinite(v)) for v in ld.values()) and 0 < ld['lovasz_loss'].item() <= 1
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and any(g.abs().max().item() > 0 for g in grads.values())


def test_inside_deep_supervision_and_boundary_loss():
    torch.manual_seed(5)
    model = DeepSupervisionUNet(2, 3, [8, 16, 24], 3, aux_levels=1, block_params=dict(GN4),
                                upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2}).cuda().train()
    x, y = _batch(2, 3, seed=200, size=(8, 16, 16))
    x, y = x.cuda(), y.cuda()
    for crit in (DeepSupervisionLoss(LovaszLoss(HybridLogisticDiceLoss(), 0.5)),
                 DeepSupervisionLoss(BoundaryLoss(LovaszLoss(HybridLogisticDiceLoss(), 0.5)))):
        model.zero_grad(set_to_none=True)
        ld = crit(model(x), y)
        assert {'loss', 'lovasz_loss', 'regional_loss', 'loss_level0', 'loss_level1'} <= set(ld)
        assert bool(torch.isfinite(ld['loss'])) and ld['lovasz_loss'].item() > 0
        ld["loss"].backward()
        for k, v in model.named_parameters():
            assert v.grad is not None and bool(torch.isfinite(v.grad).all()) and v.grad.abs().max().item() > 0, k


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_graphed_train_step_follows_set_weights(prec):
    """trainer.GraphedTrainStep with the criterion: two eager warm-up steps, then four replayed ones, the Lovasz term
    faded in (0 -> 0.5, regional 1 -> 0.5) before the last two.  The loss dicts equal those of six eager steps from the
    same seed bit for bit, and the step was captured once"""
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd.trainer import GraphedTrainStep
    m_e = _unet().cuda().train()
    m_g = copy.deepcopy(m_e)
    batches = []
    for i in range(6):
        x, y = _batch(2, 3, seed=100 + i)
        batches.append({"X": x.cuda(), "y": y.cuda()})
    crit = LovaszLoss(HybridLogisticDiceLoss(), 0.0, 1.0, per_image=True)
    with sp.precision(prec):
        opt_e = torch.optim.SGD(m_e.parameters(), lr=1e-2, momentum=0.9)
        opt_g = torch.optim.SGD(m_g.parameters(), lr=1e-2, momentum=0.9)
        step = GraphedTrainStep(m_g, crit, opt_g, warmup=2)
        losses_e, losses_g = [], []
        for i, b in enumerate(batches):
            if i == 4:
                crit.set_weights(regional=0.5, lovasz=0.5)
            opt_e.zero_grad(set_to_none=True)
            ld = crit(m_e(b["X"]), b["y"])
            ld["loss"].backward()
            opt_e.step()
            losses_e.append(torch.stack([v.detach().clone() for v in ld.values()]))
            losses_g.append(torch.stack([v.detach().clone() for v in step(b).values()]))
            names = list(ld)
    w = names.index('lovasz_weight')
    print(f"lovasz_loss_accuracy graphed {prec}: lovasz_loss per step "
          f"{[round(v[names.index('lovasz_loss')].item(), 6) for v in losses_g]} weight {[v[w].item() for v in losses_g]}")
    assert torch.equal(torch.stack(losses_e), torch.stack(losses_g))
    assert [v[w].item() for v in losses_g] == [0.0] * 4 + [0.5] * 2
    i_loss, i_reg, i_lov = names.index('loss'), names.index('regional_loss'), names.index('lovasz_loss')
    assert torch.equal(losses_g[3][i_loss], losses_g[3][i_reg])
    assert torch.equal(losses_g[5][i_loss], 0.5 * losses_g[5][i_reg] + 0.5 * losses_g[5][i_lov])
    assert len(step._graphs) == 1 and next(iter(step._graphs.values()))["graph"] is not None
