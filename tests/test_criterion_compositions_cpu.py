"""The composition table and its fp64 reference without a GPU (tests/criterion_compositions.py): the properties the
hand-built target was built for; the wrapper x leaf pairs and wrapper orders the table must keep; the reference of every
case under both sets of mixing weights (its margins hold: the seeds of the table are good); the coefficient bookkeeping of
the reference against fp64 autograd through the literal composition; and the constructors that refuse logits."""
import itertools

import numpy as np
import pytest
import torch

import binary_loss_ref as BIN
import blob_loss_ref as BR
import boundary_ref as B
import criterion_compositions as CC
import focal_tversky_ref as FT
import lovasz_ref as V
import topk_loss_ref as T
from oracle import torch_ref as R
from segmentation_pipeline_amd.criterions import (BlobLoss, BoundaryLoss, DeepSupervisionLoss, HybridBinaryLogisticDiceLoss,
                                                  HybridFocalTverskyLoss, HybridLogisticDiceLoss, HybridTopKDiceLoss,
                                                  LovaszLoss)


# ----------------------------------------------------------------------------------------------------------- the target
def _components(plane):
    lab, n = BR.plane_labels(plane, 3)
    return sorted(int((lab == k).sum()) for k in range(1, n + 1))


def test_target_is_one_hot_and_has_the_shape_of_the_issue():
    t = CC.target()
    assert tuple(t.shape) == (2, 3, 6, 10, 14) and t.dtype == torch.float32
    assert bool(((t == 0) | (t == 1)).all()) and bool((t.sum(1) == 1).all())
    t1 = CC.level_targets(t, 2)[1]
    assert tuple(t1.shape) == (2, 3, 3, 5, 7) and t1[0, 0].numel() % 2 == 1
    assert torch.equal(CC.target(1), t[:, 1:2])


def test_a_one_plane_holds_at_least_three_components_of_different_sizes():
    sizes = _components(BR.membership(CC.target())[0, 1])
    print(f"criterion_compositions target: components of (0, 1): {sizes}, of (0, 2): {_components(BR.membership(CC.target())[0, 2])}")
    assert len(sizes) >= 3 and len(set(sizes)) >= 3


def test_b_one_class_is_absent_from_image_1():
    t = CC.target()
    assert not t[1, 2].any() and t[0, 2].any() and t[1, 1].any() and t[0, 1].any()


def test_c_level_1_has_cells_of_one_half_one_eighth_and_seven_eighths_in_every_foreground_channel():
    t1 = CC.level_targets(CC.target(), 2)[1]
    for c in (1, 2):
        counts = {v: int((t1[:, c] == v).sum()) for v in (0.5, 0.125, 0.875)}
        print(f"criterion_compositions target: level-1 cells of channel {c}: {counts}")
        assert counts[0.5] >= 8 and counts[0.125] >= 1 and counts[0.875] >= 1
    assert int((CC.level_targets(CC.target(1), 2)[1] == 0.5).sum()) >= 8


def test_d_a_component_smaller_than_a_cell_leaves_the_level_1_membership():
    t0, t1 = CC.level_targets(CC.target(), 2)
    flags = [False, True, True] * 2
    n0, n1 = BR.stacked_labels(t0, flags)[2], BR.stacked_labels(t1, flags)[2]
    print(f"criterion_compositions target: components at level 0: {n0}, at level 1: {n1}")
    assert n1 < n0
    assert 1 in _components(BR.membership(t0)[0, 1]), "a single voxel: 1/8 of its coarse cell"
    # the cells of exactly 1/2 are where the thresholds part: foreground for t >= 0.5, no member for t > 0.5
    half = CC.half_cells(t1)
    assert not BR.membership(t1)[half.numpy()].any() and not B.membership(t1.numpy())[half.numpy()].any()
    assert bool((t1 >= 0.5)[half].all())


# ------------------------------------------------------------------------------------------------------------ the table
def _shape(case):
    return tuple(w.kind for w in case.wrappers), None if case.leaf is None else case.leaf.kind, \
        bool(case.leaf is not None and case.leaf.kw.get("from_logits", False))


def test_the_table_keeps_every_pair_and_every_order():
    have = {_shape(c): c for c in CC.CASES}
    leaves = ("hybrid", "binary", "focal_tversky", "topk")
    for w, l in itertools.product(("ds", "boundary", "blob", "lovasz"), leaves):
        assert ((w,), l, False) in have, (w, l)
    three = ("boundary", "blob", "lovasz")
    pairs = [(a, b) for a in three for b in three if a != b]
    assert len(pairs) == 6
    for pair in pairs:
        assert (pair, "hybrid", False) in have, pair
        assert (("ds",) + pair, "hybrid", False) in have and have[("ds",) + pair, "hybrid", False].levels == 2, pair
    for w in three:
        assert have[("ds", w), "hybrid", False].levels == 2
    four = have[("ds", "boundary", "lovasz", "blob"), "topk", False]
    assert four.name == CC.FOUR_DEEP and four.levels == 2 and four.leaf.kw["top_k"] == 0.25
    assert (("lovasz",), None, False) in have
    for w in ("lovasz", "boundary"):
        assert any(_shape(c) == ((w,), "binary", False) and c.channels == 1 for c in CC.CASES), w
    for l in ("binary", "focal_tversky", "topk"):
        assert have[("ds",), l, True].levels == 2 and have[("ds",), l, True].head == "logits"
    # a logits leaf stands directly under DeepSupervisionLoss and nowhere else
    assert all(_shape(c)[0] == ("ds",) for c in CC.CASES if _shape(c)[2])
    assert len({c.seed for c in CC.CASES}) == len(CC.CASES)


@pytest.mark.parametrize("case", CC.CASES, ids=[c.name for c in CC.CASES])
def test_every_case_builds_and_its_reference_forms_under_both_mixes(case):
    """the margins of topk_loss_ref.expected hold for both fractions (else: another seed in the table), the criterion has
    the nesting the case names, and the coefficients of a level sum as the mixing weights say"""
    crit = CC.build(case)
    mods, leaf = CC.modules(crit, case)
    assert [type(m) for m in mods] == [CC.WRAPPERS[w.kind] for w in case.wrappers]
    assert (leaf is None) == (case.leaf is None) and (leaf is None or type(leaf) is CC.LEAVES[case.leaf.kind])
    ps, t = CC.inputs(case)
    assert len(ps) == case.levels and ps[0].shape == t.shape
    for mix, top_k in ((CC.initial_mix(case), CC.top_k_of(case)),
                       (CC.scheduled_mix(case), CC.SCHEDULE_TOP_K if CC.top_k_of(case) else None)):
        ref = CC.reference(case, mix, ps, t, top_k)
        kinds = [w.kind for w in case.wrappers if w.kind != "ds"] + ([] if case.leaf is None else [case.leaf.kind])
        assert [k.kind for k in ref.terms] == kinds * case.levels
        assert all(np.isfinite(k.value) and bool(torch.isfinite(k.grad).all()) for k in ref.terms)
        assert all(g.abs().max().item() > 0 and ref.grad_bounds[j] > 0 for j, g in ref.grads.items())
        assert ref.first == 0 and sorted(ref.grads) == list(range(case.levels))
    if "ds" in CC.initial_mix(case):
        only = CC.reference(case, dict(CC.initial_mix(case), ds=[0.0, 1.0]), ps, t, CC.top_k_of(case))
        assert only.first == 1 and list(only.grads) == [1] and all(k.coef == k.local for k in only.terms)


# ------------------------------------------------------------------------- the reference against the literal composition
def _leaf_literal(leaf, p, t, top_k):
    cfg = CC.leaf_cfg(leaf, top_k)
    fn = {"hybrid": R.hybrid_logistic_dice_loss, "binary": BIN.binary_loss, "focal_tversky": FT.focal_tversky,
          "topk": T.topk_dice}[leaf.kind]
    return fn(p, t.double(), **cfg)["loss"]


def _term_literal(w, p, t):
    cw = CC.class_weights(w.kind, w.kw, p.shape[1])
    if w.kind == "boundary":
        phi = torch.from_numpy(B.signed_distance_f32(t.numpy(), [v != 0.0 for v in cw] * p.shape[0]))
        return B.loss(p, phi, cw)
    if w.kind == "blob":
        return BR.blob_dice_literal(p, t, cw, w.kw.get("square_dice", True), w.kw.get("connectivity", 3))[0]
    return V.berman(p, t.double(), w.kw.get("classes", "present"), w.kw.get("per_image", False), cw)


def literal(case, mix, predictions, t, top_k):
    """the nest written out in fp64 torch, from the inside out, as the modules' forward methods compose it"""
    targets = CC.level_targets(t, case.levels)
    inner = [w for w in case.wrappers if w.kind != "ds"]

    def level(p, tj):
        loss = None if case.leaf is None else _leaf_literal(case.leaf, p, tj, top_k)
        for w in reversed(inner):
            w_inner, w_term = (CC.f32(v) for v in mix[w.kind])
            term = w_term * _term_literal(w, p, tj)
            loss = term if loss is None else w_inner * loss + term
        return loss
    if "ds" not in mix:
        return level(predictions[0], targets[0])
    return sum(CC.f32(w) * level(p, tj) for w, p, tj in zip(mix["ds"], predictions, targets) if w != 0.0)


# seeds of the untied predictions; a case whose top-k margin fails on one seed gets another here, never a lower margin
UNTIED_SEEDS = {"lovasz(topk)": 2, CC.FOUR_DEEP: 2}


def _untied(case):
    """predictions without two equal Lovasz errors: lovasz_ref.untied_inputs' values k / 4096 and 1 - k / 4096 with
    k <= N S < 2048, so |fg - p| has no tie whatever the foreground is; the target stays the hand-built one"""
    seed = UNTIED_SEEDS.get(case.name, 1)
    return [V.untied_inputs((CC.N, case.channels) + tuple(d >> j for d in CC.SIZE), seed + j)[0] for j in range(case.levels)]


@pytest.mark.parametrize("mixes", ["initial", "scheduled"])
@pytest.mark.parametrize("case", CC.CASES, ids=[c.name for c in CC.CASES])
def test_reference_gradient_equals_autograd_through_the_literal_composition(case, mixes):
    """sum_k c_k dterm_k/dp of the reference against fp64 autograd through the nest written out with the differentiable
    forms of the terms (topk_dice, focal_tversky, binary_loss, blob_dice_literal, boundary_ref.loss, the hybrid loss), to
    1e-12 relative; a nest with a Lovasz term against `berman` on inputs without ties.  This is the proof of the
    coefficient bookkeeping: every term's gradient is already tested against its own literal form."""
    has_lovasz = any(w.kind == "lovasz" for w in case.wrappers)
    ps, t = CC.inputs(case)
    if has_lovasz:
        assert case.head != "logits"
        ps = _untied(case)
        for p, tj in zip(ps, CC.level_targets(t, case.levels)):
            e = ((tj >= 0.5).float() - p).abs().reshape(CC.N, case.channels, -1).transpose(0, 1).reshape(case.channels, -1)
            assert all(len(torch.unique(row)) == row.numel() for row in e), "the Lovasz errors are untied"
    mix = CC.initial_mix(case) if mixes == "initial" else CC.scheduled_mix(case)
    top_k = CC.top_k_of(case) if mixes == "initial" or CC.top_k_of(case) is None else CC.SCHEDULE_TOP_K
    ref = CC.reference(case, mix, ps, t, top_k)
    leaves = [p.double().requires_grad_(True) for p in ps]
    total = literal(case, mix, leaves, t, top_k)
    total.backward()
    assert abs(total.item() - ref.loss) <= 1e-12 * max(abs(ref.loss), 1e-30), (total.item(), ref.loss)
    for j, p in enumerate(leaves):
        err, scale = (p.grad - ref.grads[j]).abs().max().item(), p.grad.abs().max().item()
        print(f"criterion_compositions reference {case.name} {mixes} level {j}: |reference - autograd| {err:.3e} of {scale:.3e}")
        assert scale > 0 and err <= 1e-12 * scale


# ------------------------------------------------------------------------------------------------------- the logits fix
LOGITS_LEAVES = [HybridBinaryLogisticDiceLoss, HybridFocalTverskyLoss, HybridTopKDiceLoss]


@pytest.mark.parametrize("leaf", LOGITS_LEAVES, ids=lambda c: c.__name__)
@pytest.mark.parametrize("wrapper", [BoundaryLoss, BlobLoss, LovaszLoss], ids=lambda c: c.__name__)
def test_a_probability_wrapper_refuses_a_logits_criterion(wrapper, leaf):
    with pytest.raises(ValueError) as info:
        wrapper(leaf(from_logits=True))
    text = str(info.value)
    assert wrapper.__name__ in text and leaf.__name__ in text and "from_logits=False" in text
    assert "softmax or sigmoid" in text and "outside" in text
    assert isinstance(wrapper(leaf(from_logits=False)), wrapper)


@pytest.mark.parametrize("wrapper", [BoundaryLoss, BlobLoss, LovaszLoss], ids=lambda c: c.__name__)
def test_the_refusal_looks_at_every_depth(wrapper):
    for nest in (lambda leaf: DeepSupervisionLoss(leaf),
                 lambda leaf: DeepSupervisionLoss(DeepSupervisionLoss(leaf))):
        with pytest.raises(ValueError, match="HybridTopKDiceLoss"):
            wrapper(nest(HybridTopKDiceLoss(from_logits=True)))
        assert isinstance(wrapper(nest(HybridTopKDiceLoss())), wrapper)
    # through the other probability wrappers too: the logits flag is set after they were built
    for middle in (BoundaryLoss, BlobLoss, LovaszLoss):
        inner = middle(HybridFocalTverskyLoss())
        inner.criterion.from_logits = True
        with pytest.raises(ValueError, match="HybridFocalTverskyLoss"):
            wrapper(inner)


def test_what_stays_legal():
    for leaf in LOGITS_LEAVES:
        assert DeepSupervisionLoss(leaf(from_logits=True)).criterion.from_logits is True
    assert LovaszLoss(None).criterion is None and LovaszLoss().criterion is None
    nest = DeepSupervisionLoss(BoundaryLoss(LovaszLoss(BlobLoss(HybridTopKDiceLoss(0.25)))))
    assert nest.criterion.criterion.criterion.criterion.from_logits is False
    assert isinstance(BoundaryLoss(HybridLogisticDiceLoss()), BoundaryLoss)       # (no from_logits attribute at all)
    # a callable that is no module, as the trainers accept
    assert BlobLoss(lambda p, t: {"loss": p.sum()}).criterion is not None
