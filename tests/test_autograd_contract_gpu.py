"""The autograd contract of segmentation_pipeline_amd.ops: every differentiable public op through its public function,
with frozen inputs and with upstream gradients in the layouts autograd really hands over.

Part 1, op by op (tests/autograd_cases.py: the table, the fp64 restatements and the tolerances with the lines they come
from), in precision "fp32" and "fp32_mfma", N = 2 throughout:
  (a) outputs and all gradients against fp64 torch autograd on the CPU, at the tolerance tests/test_kernels_gpu.py applies
      to the same kernel against the C oracle;
  (b) every non-empty subset of the differentiable inputs requiring grad: gradients inside the subset bit-identical to the
      all-inputs run, `.grad is None` outside it, the forward bit-identical; the empty subset under enable_grad gives an
      output that does not require grad;
  (c) the same gradient values arriving dense, expanded from a scalar (`y.sum()`), batch-expanded (`y.sum(dim=0)`: batch
      stride 0), as a channel slice of a wider tensor, as a `[::2]` batch slice, and as the sum of two consumers: every
      input gradient bit-identical to the dense run.  A hook on the output asserts that the layout really arrived.

The two references agree far inside the tolerances (tests/test_autograd_refs_cpu.py asserts <= 0.1 of each).  Measured
there, C oracle vs fp64 restatement (rounded once to fp32, as the oracle's results are) as a fraction of the tolerance,
worst entry per family: conv3d 0.0029 (forward of conv3d_out_softmax_unfused), conv_transpose3d 0 (the same fp32 values),
norm_act 0.0058 (dgamma of norm_act_bn_eval_ragged_add), norm_act_pool 0.0082 (the pooled output), avgpool3d_2x and
avgpool3d_2x_with_skip 0, upsample_trilinear2x 0.094 (forward: the oracle interpolates in fp32), softmax_channels 0.028
(inner = C forward), hybrid_logistic_dice_loss 0.0077 (dp), copy_into / space_to_depth2 / depth_to_space2 0,
blur_weight 0.0045 (dw, standardised), weight_standardize 0.00077 (dw).  Ops without an oracle entry (max pool, nearest /
half-pixel upsampling, sigmoid, channel_scale, add) are held to the bounds of their own kernel tests.

Part 2, the four precisions through one small ModularUNet (two levels, filters [8, 16], GroupNorm, biased convolutions,
N = 2, 2 x 16^3 input, HybridLogisticDiceLoss): ConvTranspose3d, the default trilinear / AvgPool, a MaxPool variant, and
ConvTranspose3d with widths [12, 20]; the freezing patterns encoder / decoder / norm affines / biases / convolution
weights / everything but the input / everything but the norm affines, each against the nothing-frozen run of the same
mode; the loss consumed twice; and (fp32 modes) a head that hands the fused softmax output convolution a batch-expanded
gradient.  In the 16-bit modes the Functions of the first three variants are the c8 ones (_Conv3dC8Fn, _NormActC8Fn,
_ConvTC8Fn, _UpsampleC8Fn, _MaxPoolC8Fn, _PackFn); widths that are no multiples of 8 keep fp32 tensors between the layers
and run _Conv3dFn / _NormActFn / _ConvT3dFn / _PoolSkipFn with 16-bit operands.  The anchor test asserts from the autograd
graph that each variant still runs the Functions it is here for.

16-bit tensors accepted on the 3e-5 "same rounded operands, other accumulation order" bound: NONE.  Freezing changes
which code records or launches an op -- ops.conv3d: `_conv3d_act16` instead of `_Conv3dC8Fn` for frozen parameters on an
input without history; ModularUNet._forward: avgpool3d_2x instead of avgpool3d_2x_with_skip; `_Conv3dFn.forward` (the
[12, 20] variant): m355_conv3d_fwd_h16 on a c8 twin packed by the Function only when the weight needs a gradient, else
m355_conv3d_fwd, which stages the same copy inside the library -- but each pair computes the same products in the same
order, and a backward launches one kernel for weight and bias gradient whichever of them is wanted.  Measured on the
device: every tensor of every pattern is bit-identical in all four modes, so bit-identity is what is asserted.
"""
import copy
import itertools
from functools import partial

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import autograd_cases as A
import maxpool_ref as M
from oracle import torch_ref as R
from segmentation_pipeline_amd import ops
from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss
from segmentation_pipeline_amd.models import ModularUNet

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
MODES = ["fp32", "fp32_mfma"]
LAYOUTS = ["scalar_expanded", "batch_expanded", "channel_slice", "batch_slice", "consumed_twice"]
CASE_IDS = [c.name for c in A.CASES]


# ------------------------------------------------------------------------------------------------ part 1: op by op
def _assert_plan(case, mode):
    """a conv case names the kernel families it was written for: a planner change cannot quietly move it off its route"""
    if case.plans is None:
        return
    cin, cout, D, H, W = case.desc
    d = ops._conv_desc(A.N, cin, cout, D, H, W, 3, 1, 1, 0, 0, compute=ops._COMPUTE[mode])
    got = tuple(ops.conv_plan(d, which)[0] for which in (0, 1, 2))
    want = case.plans[mode if ops.FP32_SPLIT else "fp32_mfma"]
    assert got == want, f"{case.name} in {mode}: (forward, data-gradient, weight-gradient) families {got}, written for {want}"


def _values(layout, dys):
    """the gradient VALUES a layout delivers, as dense fp32 CPU tensors (what the dense baseline of the layout is fed)"""
    if layout == "scalar_expanded":
        return [torch.ones_like(d) for d in dys]
    if layout == "batch_expanded":
        return [d[:1].expand_as(d).contiguous() if d.dim() else d for d in dys]
    if layout == "consumed_twice":
        return [d + d * 0.5 for d in dys]
    return dys


def _deliver(layout, outs, dys, seen):
    """backward through `outs` so that each producer receives the values of _values(layout, dys) in the layout's strides"""
    for i, o in enumerate(outs):
        o.register_hook(lambda g, i=i: seen.append((i, tuple(g.shape), tuple(g.stride()))))
    dys = [d.to(DEVICE) for d in dys]
    if layout == "dense":
        torch.autograd.backward(outs, [d.clone() for d in dys])
    elif layout == "scalar_expanded":              # SumBackward expands a 0-dim gradient: every stride 0
        sum(o.sum() for o in outs).backward()
    elif layout == "batch_expanded":               # SumBackward1 expands along the batch: stride 0 there
        torch.autograd.backward([o.sum(dim=0) if o.dim() else o for o in outs], [d[0].clone() if d.dim() else d for d in dys])
    elif layout == "channel_slice":                # what torch.cat([z, y, z'], 1) hands y: a [:, a:b] view of the wider gradient
        views = []
        for d in dys:
            if d.dim() < 2:
                views.append(d.clone())
                continue
            wide = torch.zeros((d.shape[0], d.shape[1] + 5) + tuple(d.shape[2:]), dtype=d.dtype, device=d.device)
            wide[:, 2:2 + d.shape[1]] = d
            views.append(wide[:, 2:2 + d.shape[1]])
        torch.autograd.backward(outs, views)
    elif layout == "batch_slice":                  # every other sample of a batch twice as large
        views = []
        for d in dys:
            if d.dim() < 1:
                views.append(d.clone())
                continue
            big = torch.zeros((2 * d.shape[0],) + tuple(d.shape[1:]), dtype=d.dtype, device=d.device)
            big[::2] = d
            views.append(big[::2])
        torch.autograd.backward(outs, views)
    elif layout == "consumed_twice":               # two consumers: the engine adds their gradients before the producer runs
        torch.autograd.backward([o.view_as(o) for o in outs] + [o.view_as(o) for o in outs], dys + [d * 0.5 for d in dys])
    else:
        raise ValueError(layout)


def _assert_layout_arrived(layout, seen, outs):
    assert len(seen) == len(outs), (layout, seen)
    for i, shape, stride in seen:
        if len(shape) < 5 or shape[0] < 2:
            continue
        inner = 1
        for v in shape[1:]:
            inner *= v
        if layout == "scalar_expanded":
            assert all(s == 0 for s in stride), (layout, stride)
        elif layout == "batch_expanded":
            assert stride[0] == 0 and stride[1] > 0, (layout, stride)
        elif layout == "channel_slice":
            assert stride[0] == inner // shape[1] * (shape[1] + 5), (layout, shape, stride)
        elif layout == "batch_slice":
            assert stride[0] == 2 * inner, (layout, shape, stride)


def _run(case, mode, requires, layout="dense", dys=None):
    """one forward (+ backward when anything requires grad) -> (forward outputs, {input: .grad}, outputs' requires_grad)"""
    t = {k: v.clone().to(DEVICE).requires_grad_(k in requires) for k, v in case.inputs.items()}
    t.update({k: v.clone().to(DEVICE) for k, v in case.consts.items()})
    seen = []
    with ops.precision(mode), torch.enable_grad():
        outs = A._tuple(case.run(t))
        fwd = [o.detach().clone() for o in outs]
        flags = [o.requires_grad for o in outs]
        if requires:
            assert all(flags), f"{case.name}: outputs {flags} with {sorted(requires)} requiring grad"
            _deliver(layout, outs, A.reference(case)["dys"] if dys is None else dys, seen)
            _assert_layout_arrived(layout, seen, outs)
    if DEVICE == "cuda":
        torch.cuda.synchronize()
    return fwd, {k: t[k].grad for k in case.inputs}, flags


_BASE = {}


def _baseline(case, mode, layout="dense"):
    """all inputs requiring grad, the values of `layout` as dense clones; computed once and shared"""
    key = (case.name, mode, layout if layout in ("scalar_expanded", "batch_expanded", "consumed_twice") else "dense")
    if key not in _BASE:
        _BASE[key] = _run(case, mode, set(case.inputs), "dense", _values(layout, A.reference(case)["dys"]))
    return _BASE[key]


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", A.CASES, ids=CASE_IDS)
def test_full_gradients_against_fp64_torch(case, mode):
    """(a): outputs and every input gradient within the kernel tests' tolerance of fp64 torch autograd"""
    _assert_plan(case, mode)
    ref = A.reference(case)
    fwd, grads, _ = _baseline(case, mode)
    assert len(fwd) == len(ref["outs"])
    rows, bad = [], []
    for i, (got, want) in enumerate(zip(fwd, ref["outs"])):
        rows.append((f"out{i}", A.excess(case, f"out{i}", got, want, ref)))
    for k in case.inputs:
        assert grads[k] is not None, f"{case.name}: no gradient for {k}"
        rows.append((k, A.excess(case, k, grads[k], ref["grads"][k], ref)))
    print(f"{case.name} {mode}: fraction of the tolerance vs fp64: " + ", ".join(f"{k} {v:.3g}" for k, v in rows))
    bad = [(k, v) for k, v in rows if not v <= 1.0]
    assert not bad, f"{case.name} {mode}: outside the tolerance (fraction of it): {bad}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", A.CASES, ids=CASE_IDS)
def test_every_subset_of_inputs_requiring_grad(case, mode):
    """(b): which gradients are wanted changes neither the forward nor the gradients that are computed"""
    _assert_plan(case, mode)
    fwd0, grads0, _ = _baseline(case, mode)
    names = list(case.inputs)
    assert len(names) <= 5
    fwd, grads, flags = _run(case, mode, set())
    assert not any(flags), f"{case.name}: nothing requires grad, outputs say {flags}"
    assert all(g is None for g in grads.values())
    assert all(_same_bits(a, b) for a, b in zip(fwd, fwd0)), f"{case.name}: forward differs with nothing requiring grad"
    bad = []
    for r in range(1, len(names) + 1):
        for subset in itertools.combinations(names, r):
            fwd, grads, _ = _run(case, mode, set(subset))
            if not all(_same_bits(a, b) for a, b in zip(fwd, fwd0)):
                bad.append((subset, "forward"))
            for k in names:
                if k in subset:
                    if grads[k] is None or not _same_bits(grads[k], grads0[k]):
                        bad.append((subset, k, "missing" if grads[k] is None else
                                    f"differs by {(grads[k] - grads0[k]).abs().max().item():.3e}"))
                elif grads[k] is not None:
                    bad.append((subset, k, "has a gradient without requiring one"))
    assert not bad, f"{case.name} {mode}: {bad}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", A.CASES, ids=CASE_IDS)
def test_gradient_layouts(case, layout, mode):
    """(c): the layout the upstream gradient arrives in does not change a bit of any input gradient"""
    _assert_plan(case, mode)
    fwd0, grads0, _ = _baseline(case, mode, layout)
    fwd, grads, _ = _run(case, mode, set(case.inputs), layout)
    assert all(_same_bits(a, b) for a, b in zip(fwd, fwd0))
    bad = [(k, "missing" if grads[k] is None else f"differs by {(grads[k] - grads0[k]).abs().max().item():.3e}")
           for k in case.inputs if grads[k] is None or not _same_bits(grads[k], grads0[k])]
    assert not bad, f"{case.name} {mode} {layout}: {bad}"


# ------------------------------------------------------------------------------------------- part 2: through a model
ALL_MODES = ["fp32", "fp32_mfma", "bf16", "fp16"]
FILTERS = [8, 16]
GROUPS = 4
VARIANTS = {
    "convt": lambda: dict(upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2}),
    "default": lambda: {},                                             # trilinear upsampling, average pool
    "maxpool": lambda: dict(downsample_class=nn.MaxPool3d, downsample_params={'kernel_size': 2, 'stride': 2}),
    # widths that are no multiples of 8: the 16-bit modes then keep fp32 tensors between the layers (ModularUNet._forward
    # drops the c8 flow) and run _Conv3dFn / _NormActFn / _ConvT3dFn with c8 twins of the conv operands
    "convt_12_20": lambda: dict(upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2}),
}
WIDTHS = {"convt_12_20": [12, 20]}


def _model(variant):
    torch.manual_seed(0)
    block = {'normalization_class': partial(nn.GroupNorm, GROUPS), 'conv_params': {'bias': True, 'kernel_size': 3, 'padding': 1}}
    return ModularUNet(2, 3, list(WIDTHS.get(variant, FILTERS)), 2, block_params=block, **VARIANTS[variant]())


def _batch():
    g = torch.Generator().manual_seed(1234)
    x = torch.randn((2, 2, 16, 16, 16), generator=g)
    lab = torch.randint(0, 3, (2, 16, 16, 16), generator=g)
    return x, F.one_hot(lab, 3).permute(0, 4, 1, 2, 3).float().contiguous()


def _is_conv(m):
    return isinstance(m, (nn.Conv3d, nn.ConvTranspose3d))


def _named(model, pick):
    return {f"{mn}.{pn}" if mn else pn for mn, m in model.named_modules() for pn, _ in m.named_parameters(recurse=False)
            if pick(mn, m, pn)}


# name -> (model -> the parameter names to freeze, does the input require grad)
FREEZE = {
    "encoder": (lambda m: _named(m, lambda mn, mod, pn: mn.startswith("down_blocks.")), False),
    "decoder": (lambda m: _named(m, lambda mn, mod, pn: not mn.startswith("down_blocks.")), False),
    "norm_affines": (lambda m: _named(m, lambda mn, mod, pn: isinstance(mod, nn.GroupNorm)), False),
    "biases": (lambda m: _named(m, lambda mn, mod, pn: _is_conv(mod) and pn == "bias"), False),
    "conv_weights": (lambda m: _named(m, lambda mn, mod, pn: _is_conv(mod) and pn == "weight"), False),
    "all_but_the_input": (lambda m: _named(m, lambda mn, mod, pn: True), True),
    # beyond the issue's list: the first normalisation then follows a convolution without any autograd history
    "all_but_norm_affines": (lambda m: _named(m, lambda mn, mod, pn: not isinstance(mod, nn.GroupNorm)), False),
}


def _step(variant, mode, frozen=(), input_grad=False, head="loss"):
    """one forward / backward of a fresh copy of the seeded model -> (p, loss, {parameter: grad or None}, input grad)"""
    model = _model(variant).to(DEVICE).train()
    for k, v in model.named_parameters():
        v.requires_grad_(k not in frozen)
    x, y = _batch()
    x, y = x.to(DEVICE).requires_grad_(input_grad), y.to(DEVICE)
    # fp16: the loss scale is calibrated on the gradient that enters the c8 flow and cached per (id(out conv weight),
    # shape).  An id is reused once a model is freed, so a step could meet the calibration of an earlier model whose
    # gradient was twice as large (the loss_twice head) and travel at another power of two than the run it is compared
    # with -- identical up to fp16 subnormals, not bit for bit.  Every step here calibrates on its own gradient.
    ops._fp16_calibration.clear()
    with ops.precision(mode):
        p = model(x)
        if not frozen:
            _NODES[(variant, mode, input_grad)] = _graph_nodes(p)
        if head == "loss":
            loss = HybridLogisticDiceLoss()(p, y)["loss"]
            loss.backward()
        elif head == "loss_twice":
            loss = HybridLogisticDiceLoss()(p, y)["loss"]
            (loss + loss).backward()
        elif head == "loss_doubled":
            loss = HybridLogisticDiceLoss()(p, y)["loss"]
            (2 * loss).backward()
        else:   # a quadratic loss on the batch sum: "sum_dim0" hands the producer of p a batch-expanded gradient
            q = p.sum(dim=0) if head == "sum_dim0" else (p * 1.0).sum(dim=0)
            loss = ((q - y.sum(dim=0)) ** 2).mean()
            loss.backward()
    if DEVICE == "cuda":
        torch.cuda.synchronize()
    return (p.detach(), loss.detach(), {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in model.named_parameters()},
            None if x.grad is None else x.grad.detach().clone())


_NODES = {}


def _graph_nodes(t):
    """names of the autograd nodes behind a tensor"""
    seen, names, stack = set(), set(), [t.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        stack.extend(f for f, _ in fn.next_functions)
    return names


def _expected_nodes(variant, mode, input_grad):
    """the autograd Functions a variant is in the table for"""
    c8 = mode in ("bf16", "fp16") and variant not in WIDTHS
    want = {"_Conv3dC8FnBackward", "_NormActC8FnBackward"} if c8 else {"_Conv3dFnBackward", "_NormActFnBackward"}
    if variant.startswith("convt"):
        want.add("_ConvTC8FnBackward" if c8 else "_ConvT3dFnBackward")
    else:
        want.add("_UpsampleC8FnBackward" if c8 else "_UpsampleFnBackward")
    if variant == "maxpool":
        want.add("_MaxPoolC8FnBackward" if c8 else "_MaxPoolSkipFnBackward")
    elif not c8:   # the encoder block's last pass emits the pooled tensor in the fp32 modes only
        want.add("_NormActPoolFnBackward" if mode in MODES else "_PoolSkipFnBackward")
    if c8 and input_grad:
        want.add("_PackFnBackward")
    return want


_STEPS = {}


def _unfrozen(variant, mode, input_grad=False, head="loss"):
    key = (variant, mode, input_grad, head)
    if key not in _STEPS:
        _STEPS[key] = _step(variant, mode, input_grad=input_grad, head=head)
    return _STEPS[key]


def _differing(got, want):
    """[(name, max |difference| / max |want|)] of the tensors that are not bit-identical"""
    out = []
    for k, g in got.items():
        if g is None:
            continue
        if want[k] is None or not _same_bits(g, want[k]):
            out.append((k, float("nan") if want[k] is None else
                        (g - want[k]).abs().max().item() / max(want[k].abs().max().item(), 1e-300)))
    return out


def _cpu_reference(variant, mode):
    """oracle.torch_ref on the CPU, rounding where the mode's flow rounds: (p, loss, {parameter: grad})"""
    model = _model(variant)
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}
    x, y = _batch()
    spec = R.UNetSpec(2, 3, list(WIDTHS.get(variant, FILTERS)), 2, norm="group", groups=GROUPS,
                      up="convT" if variant.startswith("convt") else "trilinear",
                      rounding=mode if mode in ("bf16", "fp16") else None)
    if variant == "maxpool":     # (tests/maxpool_ref.py has no rounding: the fp32 arithmetic, forward only)
        spec.rounding = None
        with torch.no_grad():
            return M.unet_forward_maxpool(sd, spec, x, training=True), None, None
    p = R.unet_forward(sd, spec, x, training=True)
    loss = R.hybrid_logistic_dice_loss(p, y)["loss"]
    loss.backward()
    return p.detach(), loss.detach(), {k: v.grad for k, v in sd.items() if v.grad is not None}


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_model_unfrozen_step_is_anchored_to_the_cpu_oracle(variant, mode):
    """the run every freezing pattern is compared with.  fp32 modes: smoke()'s bounds (probabilities and loss 1e-4, every
    gradient 1e-3 of its scale).  16-bit modes: the bounds of test_c8_training_flow_architectures_with_fallback_ops
    (tests/test_kernels_gpu.py:1465-1487) against oracle.torch_ref.unet_forward with rounding=mode: probabilities 2e-2
    (bf16) / 5e-3 (fp16), every parameter gradient's cosine >= 0.9 / 0.97, all parameters together >= 0.995 / 0.9995.  The
    MaxPool variant has no rounding-matched restatement and routes near-ties its own way: probabilities only, against the
    fp32 formulation at the mode's bound (as that test compares with the fp32 golden)."""
    p, loss, grads, _ = _unfrozen(variant, mode)
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values()) and len(grads) >= 20
    missing = _expected_nodes(variant, mode, False) - _NODES[(variant, mode, False)]
    assert not missing, f"{variant} {mode} no longer runs {missing}: {sorted(_NODES[(variant, mode, False)])}"
    p_ref, loss_ref, g_ref = _cpu_reference(variant, mode)
    tol = {"fp32": 1e-4, "fp32_mfma": 1e-4, "bf16": 2e-2, "fp16": 5e-3}[mode]
    err = (p.cpu() - p_ref).abs().max().item()
    print(f"{variant} {mode}: max |p - p_ref| {err:.3e} (bound {tol:.0e})")
    assert err <= tol
    if g_ref is None:
        return
    assert set(g_ref) == set(grads)
    if mode in ("fp32", "fp32_mfma"):
        assert abs(loss.item() - loss_ref.item()) <= 1e-4
        for k, ref in g_ref.items():
            e = (grads[k].cpu() - ref).abs().max().item()
            assert e <= 1e-3 * ref.abs().max().item() + 1e-7, f"grad {k}: {e}"
        return
    dot = na = nb = 0.0
    worst = (2.0, None)
    top = max(float(r.double().norm()) for r in g_ref.values())
    for k, ref in g_ref.items():
        a, b = grads[k].cpu().double().flatten(), ref.double().flatten()
        if float(b.norm()) < 1e-9 * top:
            continue
        worst = min(worst, (float(a @ b / (a.norm() * b.norm() + 1e-300)), k))
        dot, na, nb = dot + float(a @ b), na + float(a @ a), nb + float(b @ b)
    total = dot / (na * nb) ** 0.5
    print(f"{variant} {mode}: worst parameter cosine {worst[0]:.4f} ({worst[1]}), all parameters {total:.5f}")
    assert worst[0] >= (0.9 if mode == "bf16" else 0.97), worst
    assert total >= (0.995 if mode == "bf16" else 0.9995), total


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("pattern", list(FREEZE))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_model_freezing_patterns(variant, pattern, mode):
    """frozen parameters get no gradient; every remaining gradient (and the forward) is bit-identical to the nothing-frozen
    run of the same mode -- in all four modes: see the module docstring for why no 16-bit tensor is given the 3e-5 bound"""
    pick, input_grad = FREEZE[pattern]
    frozen = pick(_model(variant))
    p0, loss0, grads0, dx0 = _unfrozen(variant, mode, input_grad=input_grad)
    assert frozen and (input_grad or len(frozen) < len(grads0)) and frozen <= set(grads0)
    if input_grad:      # asking for the input's gradient as well does not change a bit of any parameter gradient
        assert dx0 is not None and bool(torch.isfinite(dx0).all()) and dx0.abs().max().item() > 0
        assert _expected_nodes(variant, mode, True) <= _NODES[(variant, mode, True)], sorted(_NODES[(variant, mode, True)])
        assert not _differing(grads0, _unfrozen(variant, mode)[2])
    p, loss, grads, dx = _step(variant, mode, frozen=frozen, input_grad=input_grad)
    assert _same_bits(p, p0) and _same_bits(loss, loss0), "the forward depends on what is frozen"
    assert [k for k in frozen if grads[k] is not None] == [], "a frozen parameter has a gradient"
    assert [k for k in grads if k not in frozen and grads[k] is None] == [], "a trainable parameter has no gradient"
    diff = _differing(grads, grads0)
    if input_grad:
        diff += _differing({"input": dx}, {"input": dx0})
    assert not diff, f"{variant} {mode} {pattern}: not bit-identical to the unfrozen run (relative difference): {diff}"


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("variant", ["convt", "default"])
def test_model_loss_consumed_twice(variant, mode):
    """(l + l).backward() == (2 * l).backward(): autograd adds the two unit gradients before the loss node runs"""
    _, _, twice, _ = _step(variant, mode, head="loss_twice")
    _, _, doubled, _ = _step(variant, mode, head="loss_doubled")
    assert all(g is not None and g.abs().max().item() > 0 for g in twice.values())
    assert not _differing(twice, doubled)
    # ... and really twice the plain step's (a power of two: exact wherever nothing rounds to 16 bits on the way)
    if mode in ("fp32", "fp32_mfma"):
        plain = _unfrozen(variant, mode)[2]
        assert not _differing(twice, {k: 2.0 * g for k, g in plain.items()})


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", ["convt", "default"])
def test_model_batch_expanded_gradient_into_the_softmax_head(variant, mode):
    """p.sum(dim=0) hands the fused softmax output convolution a gradient with batch stride 0; (p * 1.0).sum(dim=0) the
    same values densely"""
    p_e, loss_e, expanded, _ = _step(variant, mode, head="sum_dim0")
    p_d, loss_d, dense, _ = _step(variant, mode, head="sum_dim0_dense")
    assert _same_bits(p_e, p_d) and _same_bits(loss_e, loss_d)
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in expanded.values())
    assert max(g.abs().max().item() for g in expanded.values()) > 0
    assert not _differing(expanded, dense)
