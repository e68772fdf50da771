"""Nested criteria on the device against the composed fp64 reference of tests/criterion_compositions.py (DESIGN §4.30,
*Composition*).  For every case of the table:

1. terms: every named entry of the returned dict against the fp64 reference of its term on the same level's inputs, at the
   tolerance of that term's own GPU test (copied in criterion_compositions.py, each with its source); counts exactly;
   'loss' (and the level loss under DeepSupervisionLoss) bit for bit as the weighted sum of the dict's own entries;
2. gradient: loss.backward() with the predictions of all levels as leaves; at every element of every level
   |got - ref| <= sum_k |c_k| (rtol_k max |dterm_k| + atol_k), the tolerances of the terms' own tests;
3. isolation: with every mixing weight on the path but one term's set to zero through set_weights (and weights=(0, 1) or
   (1, 0) for DeepSupervisionLoss), the gradient is torch.equal to that term's own gradient through ops.*, taken with the
   coefficient formed by the same fp32 products in the same order -- what a weight applied twice, a level weight that
   misses the gradient or a buffer shared between two backward functions cannot pass, whatever the tolerance of 2;
4. schedules: after set_weights on every wrapper and set_top_k(0.5), the same criterion objects pass 1 and 2 with the new
   coefficients, and their buffers keep their addresses;
5. repeatability: a second run gives the same bits in every entry and every gradient; the four-deep nest also on
   allocations filled with NaN (raw_ops.PoisonedEmpty).

Then the three terms that binarise a soft target on the level-1 'area' target, with the cells of exactly 1/2 moved to
1/2 +- 2^-20: `>=` for Lovasz, `>` for blob and boundary; the four-deep nest on a DeepSupervisionUNet under
trainer.GraphedTrainStep in fp32 and bf16 and through trainer.train_step in fp16; and its deepcopy / pickle round trip.

Worst measured err / bound per case on an MI355X (profiles/criterion_compositions.txt; set M355_CRITERION_COVERAGE_OUT to
a path to write the table again) -- the gradient of check 2 and 4, and the worst named value of check 1 and 4:
  ds(hybrid)                                   gradient  0.0092 initial level 0          value  0.0349 loss_level1
  ds(binary)                                   gradient  0.0167 initial level 0          value  0.0390 loss_level1
  ds(focal_tversky)                            gradient  0.0078 initial level 0          value  0.0232 loss_level1
  ds(topk)                                     gradient  0.0085 initial level 0          value  0.5000 topk_threshold
  boundary(hybrid)                             gradient  0.0066 initial level 0          value  0.0392 logistic_loss
  boundary(binary)                             gradient  0.0114 scheduled level 0        value  0.0376 boundary_loss
  boundary(focal_tversky)                      gradient  0.0181 initial level 0          value  0.2611 boundary_loss
  boundary(topk)                               gradient  0.0035 initial level 0          value  0.5000 topk_threshold
  blob(hybrid)                                 gradient  0.0089 initial level 0          value  0.3778 blob_loss
  blob(binary)                                 gradient  0.0149 initial level 0          value  0.3009 blob_loss
  blob(focal_tversky)                          gradient  0.0253 initial level 0          value  0.1034 blob_loss
  blob(topk)                                   gradient  0.0075 initial level 0          value  0.5000 topk_threshold
  lovasz(hybrid)                               gradient  0.0104 initial level 0          value  0.0290 loss
  lovasz(binary)                               gradient  0.0151 initial level 0          value  0.0349 logistic_loss
  lovasz(focal_tversky)                        gradient  0.0142 initial level 0          value  0.0163 loss
  lovasz(topk)                                 gradient  0.0070 initial level 0          value  0.5000 topk_threshold
  boundary(blob(hybrid))                       gradient  0.0046 scheduled level 0        value  0.3784 boundary_loss
  boundary(lovasz(hybrid))                     gradient  0.0030 scheduled level 0        value  0.0393 loss
  blob(boundary(hybrid))                       gradient  0.0019 initial level 0          value  0.3546 boundary_loss
  blob(lovasz(hybrid))                         gradient  0.0050 scheduled level 0        value  0.5323 blob_loss
  lovasz(boundary(hybrid))                     gradient  0.0030 initial level 0          value  0.3677 boundary_loss
  lovasz(blob(hybrid))                         gradient  0.0107 scheduled level 0        value  0.2598 blob_loss
  ds(boundary(hybrid))                         gradient  0.0083 initial level 0          value  0.2134 boundary_loss
  ds(blob(hybrid))                             gradient  0.0139 scheduled level 1        value  0.2431 blob_loss
  ds(lovasz(hybrid))                           gradient  0.0224 scheduled level 1        value  0.0273 logistic_loss
  ds(boundary(blob(hybrid)))                   gradient  0.0110 scheduled level 0        value  0.3808 blob_loss
  ds(boundary(lovasz(hybrid)))                 gradient  0.0073 scheduled level 0        value  0.1502 boundary_loss
  ds(blob(boundary(hybrid)))                   gradient  0.0065 scheduled level 1        value  0.2394 blob_loss
  ds(blob(lovasz(hybrid)))                     gradient  0.0045 scheduled level 0        value  0.0425 blob_loss
  ds(lovasz(boundary(hybrid)))                 gradient  0.0126 initial level 0          value  0.1812 boundary_loss
  ds(lovasz(blob(hybrid)))                     gradient  0.0121 initial level 1          value  0.2478 blob_loss
  ds(boundary(lovasz(blob(topk))))             gradient  0.0089 scheduled level 1        value  0.5000 topk_threshold
  lovasz(None)                                 gradient  0.0120 initial level 0          value  0.0013 lovasz_loss
  lovasz(binary) C=1                           gradient  0.0105 scheduled level 0        value  0.0161 loss
  boundary(binary) C=1                         gradient  0.0085 initial level 0          value  0.3525 boundary_loss
  ds(binary from_logits)                       gradient  0.0195 initial level 0          value  0.0167 loss_level0
  ds(focal_tversky from_logits)                gradient  0.0187 initial level 1          value  0.0184 loss
  ds(topk from_logits)                         gradient  0.0134 scheduled level 1        value  0.0299 loss_level1
"""
import copy
import os
import pickle
from functools import partial

import numpy as np
import pytest
import torch
from torch import nn

import blob_loss_ref as BR
import boundary_ref as B
import criterion_compositions as CC
import deep_supervision_ref as DS
import lovasz_ref as V
import segmentation_pipeline_amd as sp
from raw_ops import PoisonedEmpty
from segmentation_pipeline_amd import ops
from segmentation_pipeline_amd.models import DeepSupervisionUNet
from segmentation_pipeline_amd.prediction import StandardPredict
from segmentation_pipeline_amd.trainer import GraphedTrainStep, train_step

pytestmark = pytest.mark.gpu

WORST = {}      # case name -> {"gradient": (err / bound, what), "value": (err / bound, what)}


@pytest.fixture(scope="module", autouse=True)
def results_table():
    yield
    lines = [f"{name:44s} gradient {w['gradient'][0]:7.4f} {w['gradient'][1]:24s} value {w['value'][0]:7.4f} {w['value'][1]}"
             for name, w in WORST.items()]
    print("\nworst err / bound per case\n" + "\n".join(lines))
    path = os.environ.get("M355_CRITERION_COVERAGE_OUT")
    if path:
        with open(path, "w") as f:
            f.write("# tests/test_criterion_compositions_gpu.py on an MI355X: worst err / bound per case -- of the gradient against\n"
                    "# sum_k |c_k| (rtol_k max|dterm_k| + atol_k), and of the named values against their terms' own bounds\n")
            f.write("\n".join(lines) + "\n")


def note(name, family, ratio, what):
    held = WORST.setdefault(name, {"gradient": (-1.0, "-"), "value": (-1.0, "-")})
    if ratio > held[family][0]:
        held[family] = (ratio, what)


def _dev(values):
    return None if values is None else torch.tensor([float(v) for v in values], dtype=torch.float32, device="cuda")


def ulps(a, b):
    """the distance of two fp32 values of one sign in units of the last place (test_topk_loss_gpu.py's)"""
    ia, ib = (torch.tensor(float(v), dtype=torch.float32).view(torch.int32).item() for v in (a, b))
    return abs(ia - ib)


# ---------------------------------------------------------------------------------------------------------- one run
def run(crit, case, ps, t):
    """forward and backward with the predictions of all levels as leaves -> (dict, [gradient or None per level])"""
    leaves = [p.cuda().requires_grad_(True) for p in ps]
    ld = crit(tuple(leaves) if "ds" in [w.kind for w in case.wrappers] else leaves[0], t.cuda())
    assert ld["loss"].dim() == 0 and ld["loss"].dtype == torch.float32
    ld["loss"].backward()
    return {k: v.detach().clone() for k, v in ld.items()}, [None if p.grad is None else p.grad.clone() for p in leaves]


def same_bits(a, b):
    (da, ga), (db, gb) = a, b
    assert list(da) == list(db)
    for k in da:
        assert da[k].dtype == db[k].dtype and torch.equal(da[k], db[k]), k
    for j, (x, y) in enumerate(zip(ga, gb)):
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), f"gradient of level {j}"


def _mix_by_hand(kind, ld, alone):
    inner_w, term_w = CC.MIX_NAMES[kind]
    if alone:
        return ld[term_w] * ld[CC.TERM_KEY[kind]]
    return ld[inner_w] * ld[CC.INNER_KEY[kind]] + ld[term_w] * ld[CC.TERM_KEY[kind]]


def check_values(case, mix, ld, ref, tag):
    """check 1"""
    name = case.name
    for term in ref.terms:
        if term.level != ref.first:
            continue
        for key, spec in term.named.items():
            assert key in ld, (key, list(ld))
            if spec[0] == "exact":
                print(f"criterion_compositions {name} {tag} {key}: {ld[key].item()} (reference {spec[1]})")
                assert ld[key].item() == spec[1] and not ld[key].dtype.is_floating_point
            elif spec[0] == "ulps":
                d = ulps(ld[key].item(), spec[1])
                print(f"criterion_compositions {name} {tag} {key}: {ld[key].item():.9g} vs {spec[1]:.9g} ({d} ulp of {spec[2]})")
                note(name, "value", d / spec[2], key)
                assert d <= spec[2], f"{key}: {d} ulp"
            else:
                want, bound = spec
                err = abs(ld[key].double().item() - want)
                print(f"criterion_compositions {name} {tag} {key}: {ld[key].item():.9e} fp64 {want:.9e} err {err:.3e} bound {bound:.3e}")
                note(name, "value", err / bound, key)
                assert err <= bound, f"{key}: {err:.3e} > {bound:.3e}"
    kinds = [w.kind for w in case.wrappers]
    composed = [("loss", ref.loss, ref.loss_bound)]
    if kinds[0] == "ds":
        composed += [(f"loss_level{j}", ref.level_loss[j], ref.level_bound[j]) for j in ref.level_loss]
        assert [k for k in ld if k.startswith("loss_level")] == [f"loss_level{j}" for j in ref.level_loss]
    for key, want, bound in composed:
        err = abs(ld[key].double().item() - want)
        print(f"criterion_compositions {name} {tag} {key}: {ld[key].item():.9e} fp64 {want:.9e} err {err:.3e} bound {bound:.3e}")
        note(name, "value", err / bound, key)
        assert err <= bound, f"{key}: {err:.3e} > {bound:.3e}"
    # 'loss' bit for bit from the dict's own weights and terms
    if kinds[0] == "ds":
        total = None
        for j, w in enumerate(mix["ds"]):
            if w == 0.0:
                continue
            part = w * ld[f"loss_level{j}"]
            total = part if total is None else total + part
        assert torch.equal(ld["loss"], total)
        if len(kinds) > 1:       # the dict is the finest evaluated level's: its outermost mix is that level's loss
            assert torch.equal(ld[f"loss_level{ref.first}"], _mix_by_hand(kinds[1], ld, case.leaf is None and len(kinds) == 2))
    else:
        assert torch.equal(ld["loss"], _mix_by_hand(kinds[0], ld, case.leaf is None and len(kinds) == 1))
    outer = kinds[1] if kinds[0] == "ds" and len(kinds) > 1 else kinds[0]
    if outer != "ds":
        for key, v in zip(CC.MIX_NAMES[outer], mix[outer]):
            assert ld[key].item() == np.float32(v), key


def check_gradients(case, grads, ref, tag):
    """check 2"""
    for j, g in enumerate(grads):
        if j not in ref.grads:
            assert g is None or not g.any(), f"level {j} has weight 0"
            continue
        err = (g.cpu().double() - ref.grads[j]).abs().max().item()
        bound = ref.grad_bounds[j]
        parts = ", ".join(f"{k.kind} {abs(k.coef) * (k.rtol * k.grad.abs().max().item() + k.atol):.2e}" for k in ref.terms if k.level == j)
        print(f"criterion_compositions {case.name} {tag} gradient of level {j}: max err {err:.3e} bound {bound:.3e} ({parts}) "
              f"max |ref| {ref.grads[j].abs().max().item():.3e}")
        note(case.name, "gradient", err / bound, f"{tag} level {j}")
        assert bool(torch.isfinite(g).all()) and err <= bound, f"level {j}: {err:.3e} > {bound:.3e}"


# ------------------------------------------------------------------------------------------------------- one term alone
def term_alone(case, i, leaf, p, t, top_k):
    """term i of the chain (the wrappers inside DeepSupervisionLoss, then the leaf) through ops.* on device tensors"""
    inner = [w for w in case.wrappers if w.kind != "ds"]
    n, channels = p.shape[:2]
    if i == len(inner):
        cw = _dev(leaf.logistic_class_weights)
        if case.leaf.kind == "hybrid":
            return ops.hybrid_logistic_dice_loss(p, t, leaf.dice_weight, cw, leaf.square_dice)[0]
        if case.leaf.kind == "binary":
            return ops.binary_logistic_dice_loss(p, t, leaf.dice_weight, cw, _dev(leaf.pos_weight), leaf.square_dice,
                                                 leaf.from_logits)[0]
        if case.leaf.kind == "focal_tversky":
            return ops.focal_tversky_loss(p, t, leaf.tversky_weight, leaf.alpha, leaf.beta, leaf.tversky_power,
                                          leaf.focal_gamma, cw, _dev(leaf.tversky_class_weights), leaf.from_logits)[0]
        return ops.topk_logistic_dice_loss(p, t, top_k, leaf.dice_weight, cw, leaf.square_dice, leaf.from_logits)[0]
    w = inner[i]
    values = CC.class_weights(w.kind, w.kw, channels)
    if w.kind == "boundary":
        phi = ops.signed_distance(t.contiguous(), planes=[v != 0.0 for v in values] * n)
        return ops.boundary_loss(p, phi, _dev(values))
    if w.kind == "blob":
        return ops.blob_dice_loss(p, t, _dev(values), w.kw.get("square_dice", True), w.kw.get("connectivity", 3),
                                  planes=[v != 0.0 for v in values] * n)[0]
    return ops.lovasz_loss(p, t, w.kw.get("classes", "present"), w.kw.get("per_image", False), _dev(values))


def check_isolation(case, ps, t):
    """check 3.  The coefficient is formed as autograd forms it: ones, times the level weight (a Python scalar), times the
    fp32 device scalars on the path from the outside in -- the same products in the same order, so torch.equal."""
    inner = [w for w in case.wrappers if w.kind != "ds"]
    has_ds = len(inner) != len(case.wrappers)
    chain = len(inner) + (case.leaf is not None)
    td = t.cuda()
    targets = [td] + (ops.target_pyramid(td, case.levels - 1, "area") if case.levels > 1 else [])
    base = CC.initial_mix(case)
    for level in range(case.levels):
        ds_weights = [1.0 if j == level else 0.0 for j in range(case.levels)] if has_ds else None
        for i in range(chain):
            mix = dict(base)
            for m, w in enumerate(inner[:i + 1]):
                mix[w.kind] = (base[w.kind][0], 0.0) if m < i else (0.0, base[w.kind][1])
            crit = CC.build(case, ds_weights)
            CC.apply_mix(crit, case, mix)
            mods, leaf = CC.modules(crit, case)
            got_dict, got = run(crit, case, ps, t)
            for j, g in enumerate(got):
                assert j == level or g is None, f"level {j} has weight 0 and gets no gradient"
            coefficient = torch.ones((), dtype=torch.float32, device="cuda")
            if has_ds:
                coefficient = coefficient * ds_weights[level]
                mods = mods[1:]
            for m, (w, mod) in enumerate(zip(inner[:i + 1], mods)):
                coefficient = coefficient * getattr(mod, CC.MIX_NAMES[w.kind][0 if m < i else 1])
            p = ps[level].cuda().requires_grad_(True)
            term_alone(case, i, leaf, p, targets[level], CC.top_k_of(case)).backward(coefficient)
            what = inner[i].kind if i < len(inner) else case.leaf.kind
            differ = int((got[level] != p.grad).sum())
            print(f"criterion_compositions {case.name} isolation of {what} at level {level}: coefficient {coefficient.item():.9g}, "
                  f"{differ} of {p.grad.numel()} elements differ, max |gradient| {p.grad.abs().max().item():.3e}")
            assert p.grad.abs().max().item() > 0 and bool(torch.isfinite(got[level]).all())
            assert torch.equal(got[level], p.grad), f"{what} at level {level}: {differ} elements differ"


# ----------------------------------------------------------------------------------------------------------- the cases
def _buffers(crit, case):
    mods, leaf = CC.modules(crit, case)
    out = [getattr(m, n) for w, m in zip(case.wrappers, mods) if w.kind != "ds" for n in CC.MIX_NAMES[w.kind]]
    if leaf is not None and hasattr(leaf, "_counts"):
        out += list(leaf._counts.values())
    return out


@pytest.mark.parametrize("case", CC.CASES, ids=[c.name for c in CC.CASES])
def test_case(case, monkeypatch):
    ps, t = CC.inputs(case)
    crit = CC.build(case)
    mix, top_k = CC.initial_mix(case), CC.top_k_of(case)
    first = run(crit, case, ps, t)
    ref = CC.reference(case, mix, ps, t, top_k)
    check_values(case, mix, first[0], ref, "initial")
    check_gradients(case, first[1], ref, "initial")
    # 5: the same bits again, and on allocations filled with NaN
    same_bits(first, run(crit, case, ps, t))
    if case.name == CC.FOUR_DEEP:
        with PoisonedEmpty(monkeypatch, "nan") as poison:
            poisoned = run(crit, case, ps, t)
        print(f"criterion_compositions {case.name}: {poison.dirtied} allocations filled with NaN")
        assert poison.dirtied >= 20
        same_bits(first, poisoned)
    # 3
    check_isolation(case, ps, t)
    # 4: the schedule on the same objects
    buffers = _buffers(crit, case)
    assert all(b.is_cuda for b in buffers)
    ptrs = [b.data_ptr() for b in buffers]
    mix2 = CC.scheduled_mix(case)
    CC.apply_mix(crit, case, mix2)
    if top_k is not None:
        CC.modules(crit, case)[1].set_top_k(CC.SCHEDULE_TOP_K)
        top_k = CC.SCHEDULE_TOP_K
    second = run(crit, case, ps, t)
    assert [b.data_ptr() for b in _buffers(crit, case)] == ptrs
    ref2 = CC.reference(case, mix2, ps, t, top_k)
    check_values(case, mix2, second[0], ref2, "scheduled")
    check_gradients(case, second[1], ref2, "scheduled")
    if mix2 != mix or top_k != CC.top_k_of(case):
        assert not torch.equal(second[0]["loss"], first[0]["loss"])
    same_bits(second, run(crit, case, ps, t))


# -------------------------------------------------------------------------- soft targets in the terms that binarise them
def close(got, ref, rtol, atol, what):
    """tests/test_kernels_gpu.py's close(): max |got - ref| <= atol + rtol * max |ref|; prints the figure first"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, bound = (got - ref).abs().max().item(), atol + rtol * ref.abs().max().item()
    print(f"criterion_compositions soft target {what}: max err {err:.3e}  bound {bound:.3e}")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def _soft_inputs():
    """(p, {name: level-1 target}) on the host: the 'area' target of the device, equal to torch's pooling, and the same with
    the cells of exactly 1/2 moved by 2^-20 either way"""
    t0 = CC.target()
    t1 = ops.target_pyramid(t0.cuda(), 1, "area")[0].cpu()
    assert torch.equal(t1, DS.pyramid(t0, 1, "area")[0])
    half = CC.half_cells(t1)
    assert int(half[:, 1].sum()) >= 8 and int(half[:, 2].sum()) >= 8
    p = torch.softmax(2 * torch.randn(t1.shape, generator=torch.Generator().manual_seed(77)), dim=1).contiguous()
    above, below = t1.clone(), t1.clone()
    above[half], below[half] = 0.5 + 2.0 ** -20, 0.5 - 2.0 ** -20
    assert bool((above[half] > 0.5).all()) and bool((below[half] < 0.5).all())
    return p, {"area": t1, "above": above, "below": below}


DLOSS = 0.7


@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "image"])
def test_soft_target_lovasz_takes_one_half_as_foreground(per_image):
    """t >= 0.5 (lovasz_loss.hip's lv_key, lovasz_ref): 1/2 + 2^-20 changes nothing, 1/2 - 2^-20 does; value and gradient of
    all three against the closed form at test_lovasz_loss_gpu.py's close(2e-6, 1e-7) and close(1e-5, 1e-9)"""
    p, targets = _soft_inputs()
    got = {}
    for name, t in targets.items():
        pd = p.cuda().requires_grad_(True)
        loss = ops.lovasz_loss(pd, t.cuda(), "present", per_image, None)
        (loss * DLOSS).backward()
        ref = V.closed_form(p, t, DLOSS, "present", per_image, None)
        close(loss, ref["loss"], 2e-6, 1e-7, f"lovasz {name} loss")
        close(pd.grad, ref["dx"], 1e-5, 1e-9, f"lovasz {name} dx")
        got[name] = (loss.detach().clone(), pd.grad.clone())
    assert torch.equal(got["above"][0], got["area"][0]) and torch.equal(got["above"][1], got["area"][1])
    assert not torch.equal(got["below"][0], got["area"][0]) and not torch.equal(got["below"][1], got["area"][1])


def test_soft_target_blob_takes_one_half_as_no_member():
    """t > 0.5 (blob_loss_ref.membership and BlobLoss's docstring): 1/2 - 2^-20 changes nothing, 1/2 + 2^-20 does; value,
    count and gradient against the closed form within test_blob_loss_gpu.py's bounds"""
    p, targets = _soft_inputs()
    cw = BR.default_weights(p.shape[1])
    planes = [v > 0 for v in cw] * p.shape[0]
    got = {}
    for name, t in targets.items():
        pd = p.cuda().requires_grad_(True)
        loss, count = ops.blob_dice_loss(pd, t.cuda(), cw, True, 3)
        loss.backward(torch.tensor(DLOSS, device="cuda"))
        ref, ref_grad = BR.blob_dice_closed_form(p, t, cw, True, 3)
        want_n = BR.stacked_labels(t, planes, 3)[2]
        err, bound = abs(loss.double().item() - ref.item()), 2.0 ** -31 + 2.0 ** -24 * abs(ref.item())
        print(f"criterion_compositions soft target blob {name}: components {count.item()} (scipy {want_n}) loss {loss.item():.9e} "
              f"fp64 {ref.item():.12e} err {err:.3e} bound {bound:.3e}")
        assert count.item() == want_n and err <= bound
        g, w = pd.grad.double().cpu().numpy(), (ref_grad * DLOSS).numpy()
        worst = 0.0
        for i, on in enumerate(planes):
            gi, wi = g[i // 3, i % 3], w[i // 3, i % 3]
            if not on:
                assert not gi.any() and not wi.any()
            elif np.abs(wi).max() > 0:      # 4 ulps of the plane's largest magnitude (the square form)
                tol = 4.0 * np.spacing(np.float32(np.abs(wi).max())).astype(np.float64)
                worst = max(worst, float((np.abs(gi - wi) / tol).max()))
            else:
                assert not gi.any()
        print(f"criterion_compositions soft target blob {name}: worst gradient |error| / (4 ulp bound) {worst:.3f}")
        assert worst <= 1.0
        got[name] = (loss.detach().clone(), count.clone(), pd.grad.clone())
    assert all(torch.equal(a, b) for a, b in zip(got["below"], got["area"]))
    assert not torch.equal(got["above"][0], got["area"][0]) and not torch.equal(got["above"][2], got["area"][2])
    # the component smaller than a coarse cell is gone at level 1: fewer components than at level 0
    assert got["area"][1].item() < ops.blob_dice_loss(torch.rand(CC.target().shape, device="cuda"), CC.target().cuda(), cw)[1].item()


def test_soft_target_boundary_takes_one_half_as_outside():
    """t > 0.5 (boundary_ref.membership and BoundaryLoss's docstring): 1/2 - 2^-20 changes nothing, 1/2 + 2^-20 does; the
    map bit for bit, value and gradient within test_boundary_loss_gpu.py's bounds"""
    p, targets = _soft_inputs()
    cw = BR.default_weights(p.shape[1])
    planes = [v != 0.0 for v in cw] * p.shape[0]
    got = {}
    for name, t in targets.items():
        phi = ops.signed_distance(t.cuda(), planes=planes)
        want = torch.from_numpy(B.signed_distance_f32(t.numpy(), planes))
        assert torch.equal(phi.cpu(), want), f"{name}: {int((phi.cpu() != want).sum())} voxels of the map differ"
        pd = p.cuda().requires_grad_(True)
        loss = ops.boundary_loss(pd, phi, _dev(cw))
        loss.backward(torch.tensor(DLOSS, device="cuda"))
        ref, mass = B.loss(p, want, cw).item(), B.abs_mass(p, want, cw).item()
        err, bound = abs(loss.double().item() - ref), 2.0 ** -23 * mass
        dref = B.grad(want, cw, np.float32(DLOSS))
        derr = (pd.grad.cpu().double() - dref).abs()
        worst = (derr / (2.0 ** -22 * dref.abs()).clamp(min=1e-300)).max().item()
        print(f"criterion_compositions soft target boundary {name}: loss {loss.item():.7e} ref {ref:.7e} err {err:.3e} bound {bound:.3e}; "
              f"gradient worst error / bound {worst:.4f}")
        assert err <= bound and bool((derr <= 2.0 ** -22 * dref.abs()).all())
        got[name] = (phi.clone(), loss.detach().clone(), pd.grad.clone())
    assert all(torch.equal(a, b) for a, b in zip(got["below"], got["area"]))
    assert all(not torch.equal(a, b) for a, b in zip(got["above"], got["area"]))


# ------------------------------------------------------------------------------------- the four-deep nest under a model
GN4 = {'normalization_class': partial(nn.GroupNorm, 4)}
CONVT = dict(upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2})


def _model():
    torch.manual_seed(5)
    return DeepSupervisionUNet(2, 3, [8, 16, 24], 3, aux_levels=1, block_params=dict(GN4), **CONVT).cuda().train()


def _batch(i):
    """an 8 x 16 x 16 input and the hand-built label map of image 0 inside it, moved along x by i"""
    x = torch.randn((1, 2, 8, 16, 16), generator=torch.Generator().manual_seed(300 + i))
    lab = torch.zeros((1, 8, 16, 16), dtype=torch.int64)
    lab[0, :6, :10, :14] = CC.label_map()[0]
    y = torch.nn.functional.one_hot(torch.roll(lab, i, dims=3), 3).permute(0, 4, 1, 2, 3).float().contiguous()
    return {"X": x.cuda(), "y": y.cuda()}


def _schedule(crit, case):
    CC.apply_mix(crit, case, CC.scheduled_mix(case))
    CC.modules(crit, case)[1].set_top_k(CC.SCHEDULE_TOP_K)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_graphed_train_step_follows_all_four_schedules(prec):
    """the pattern of test_lovasz_loss_gpu.py::test_graphed_train_step_follows_set_weights: two eager warm-up steps, four
    replays, all three set_weights and set_top_k before the last two; the loss dicts equal those of six eager steps bit
    for bit and one graph was captured"""
    case = CC.BY_NAME[CC.FOUR_DEEP]
    m_e = _model()
    m_g = copy.deepcopy(m_e)
    crit = CC.build(case)
    batches = [_batch(i) for i in range(6)]
    with sp.precision(prec):
        opt_e = torch.optim.SGD(m_e.parameters(), lr=1e-2, momentum=0.9)
        opt_g = torch.optim.SGD(m_g.parameters(), lr=1e-2, momentum=0.9)
        step = GraphedTrainStep(m_g, crit, opt_g, warmup=2)
        eager, graphed = [], []
        for i, b in enumerate(batches):
            if i == 4:
                _schedule(crit, case)
            opt_e.zero_grad(set_to_none=True)
            ld = crit(m_e(b["X"]), b["y"])
            ld["loss"].backward()
            opt_e.step()
            eager.append({k: v.detach().clone() for k, v in ld.items()})
            graphed.append({k: v.clone() for k, v in step(b).items()})
    print(f"criterion_compositions graphed {prec}: loss per step {[round(d['loss'].item(), 6) for d in graphed]} "
          f"boundary weight {[d['boundary_weight'].item() for d in graphed]} threshold {[round(d['topk_threshold'].item(), 5) for d in graphed]}")
    for i, (a, b) in enumerate(zip(eager, graphed)):
        assert list(a) == list(b)
        for k in a:
            assert bool(torch.isfinite(a[k].float())) and torch.equal(a[k], b[k]), (i, k)
    for key, kind, which in (("boundary_weight", "boundary", 1), ("blob_weight", "blob", 1), ("lovasz_weight", "lovasz", 1)):
        before, after = CC.initial_mix(case)[kind][which], CC.SCHEDULE[kind][which]
        assert [d[key].item() for d in graphed] == [np.float32(before)] * 4 + [np.float32(after)] * 2
    assert all(d["blob_count"].item() > 0 for d in graphed)
    assert len(step._graphs) == 1 and next(iter(step._graphs.values()))["graph"] is not None


def test_fp16_train_step_equals_the_raw_op_path():
    """one step of trainer.train_step in the fp16 flow with the four-deep nest: loss and every parameter gradient finite and,
    bit for bit, those of the same step with the terms taken through ops.* in the order the modules call them (the
    pattern of test_lovasz_loss_gpu.py::test_model_step_equals_the_raw_op_path)"""
    case = CC.BY_NAME[CC.FOUR_DEEP]
    crit = CC.build(case)
    mix = CC.initial_mix(case)
    dev = {k: tuple(torch.tensor(v, dtype=torch.float32, device="cuda") for v in mix[k]) for k in ("boundary", "lovasz", "blob")}
    cw = BR.default_weights(3)
    on = [v != 0.0 for v in cw]
    per_image = CC.LOVASZ["per_image"]

    def level(p, t):      # BoundaryLoss.forward > LovaszLoss.forward > BlobLoss.forward > HybridTopKDiceLoss.forward
        lovasz = ops.lovasz_loss(p, t, "present", per_image, None)
        leaf = ops.topk_logistic_dice_loss(p, t, 0.25)[0]
        blob = ops.blob_dice_loss(p, t, _dev(cw), True, 3, planes=on * p.shape[0])[0]
        inner = dev["blob"][0] * leaf + dev["blob"][1] * blob
        inner = dev["lovasz"][0] * inner + dev["lovasz"][1] * lovasz
        boundary = ops.boundary_loss(p, ops.signed_distance(t.contiguous(), planes=on * p.shape[0]), _dev(cw))
        return dev["boundary"][0] * inner + dev["boundary"][1] * boundary

    def raw(out, y):
        total = None
        for w, p, t in zip(mix["ds"], out, [y] + ops.target_pyramid(y, 1, "area")):
            part = w * level(p, t)
            total = part if total is None else total + part
        return {"loss": total}
    model = _model()
    twin = copy.deepcopy(model)
    b = _batch(0)
    results = []
    with sp.precision("fp16"):
        for m, c in ((model, crit), (twin, raw)):
            ops.fp16_overflow()
            ld, _ = train_step(m, c, torch.optim.SGD(m.parameters(), lr=0.0), StandardPredict(), dict(b), torch.device("cuda"))
            results.append((ld["loss"].detach().clone(), {k: v.grad.detach().clone() for k, v in m.named_parameters()}))
    (loss, grads), (loss_raw, grads_raw) = results
    print(f"criterion_compositions fp16 step: loss {loss.item():.6f} raw {loss_raw.item():.6f}, {len(grads)} parameters")
    assert bool(torch.isfinite(loss)) and torch.equal(loss, loss_raw) and len(grads) > 10
    for k, g in grads.items():
        assert bool(torch.isfinite(g).all()) and torch.equal(g, grads_raw[k]), k
    assert any(g.abs().max().item() > 0 for g in grads.values())


def test_deepcopy_and_pickle_after_a_run_on_the_device():
    """the four-deep nest after it has run (weights uploaded, k on the device, buffers moved) and after its schedule:
    a deepcopy and a pickle round trip give criteria whose first forward returns the original's bits"""
    case = CC.BY_NAME[CC.FOUR_DEEP]
    ps, t = CC.inputs(case)
    crit = CC.build(case)
    run(crit, case, ps, t)
    _schedule(crit, case)
    want = run(crit, case, ps, t)
    for what, twin in (("deepcopy", copy.deepcopy(crit)), ("pickle", pickle.loads(pickle.dumps(crit)))):
        assert twin is not crit and CC.modules(twin, case)[1].top_k == CC.SCHEDULE_TOP_K, what
        same_bits(want, run(twin, case, ps, t))
    same_bits(want, run(crit, case, ps, t))
