"""LovaszLoss and the segmented sort: what can be checked without a GPU -- the criterion's interface, mixing weights and
pickled state, the bindings, the argument checks of every entry point (no launches) and of the ops wrappers, the
workspace queries, and the closed form of tests/lovasz_ref.py (what the kernels implement) against Berman's formula."""
import ctypes
import inspect
import os
import pickle

import pytest
import torch

import lovasz_ref as V
from conftest import ROOT
from segmentation_pipeline_amd import _lib, criterions, ops
from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss, LovaszLoss

SYMBOLS = ["m355_segmented_sort_workspace", "m355_segmented_sort_tile", "m355_segmented_sort_u32",
           "m355_lovasz_loss_workspace", "m355_lovasz_loss_tile", "m355_lovasz_loss_fwd", "m355_lovasz_loss_bwd"]
P = ctypes.c_void_p


# ------------------------------------------------------------------------------------------------------- the criterion
def test_constructor_defaults_and_export():
    assert criterions.LovaszLoss is LovaszLoss
    sig = inspect.signature(LovaszLoss.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ("criterion", None), ("lovasz_weight", 1.0), ("regional_weight", 1.0), ("classes", 'present'), ("per_image", False),
        ("lovasz_class_weights", None)]
    crit = LovaszLoss()
    assert (crit.criterion, crit.classes, crit.per_image, crit.lovasz_class_weights) == (None, 'present', False, None)
    assert crit.lovasz_weight.item() == 1.0 and crit.regional_weight.item() == 1.0
    assert isinstance(crit, criterions._device_weights.DeviceWeightsCriterion)
    assert [(k, v.default) for k, v in inspect.signature(ops.lovasz_loss).parameters.items()] == [
        ("prediction", inspect.Parameter.empty), ("target", inspect.Parameter.empty), ("classes", 'present'),
        ("per_image", False), ("class_weights", None)]


def test_constructor_argument_checks():
    with pytest.raises(ValueError, match="classes"):
        LovaszLoss(classes="some")
    for name in ("lovasz_weight", "regional_weight"):
        with pytest.raises(ValueError, match=name):
            LovaszLoss(**{name: float("nan")})
    for bad in ([], [1.0, -1.0], [float("inf")], torch.ones(2, 2)):
        with pytest.raises(ValueError, match="lovasz_class_weights"):
            LovaszLoss(lovasz_class_weights=bad)
    assert LovaszLoss(lovasz_class_weights=torch.tensor([0.0, 2.0])).lovasz_class_weights == (0.0, 2.0)


def test_set_weights_keeps_the_buffers():
    crit = LovaszLoss(HybridLogisticDiceLoss(), 0.0, 1.0)
    assert set(dict(crit.named_buffers(recurse=False))) == {"regional_weight", "lovasz_weight"}
    r, l = crit.regional_weight, crit.lovasz_weight
    ptrs = (r.data_ptr(), l.data_ptr())
    crit.set_weights(regional=0.75, lovasz=0.25)
    assert crit.regional_weight is r and crit.lovasz_weight is l and (r.data_ptr(), l.data_ptr()) == ptrs
    assert (r.item(), l.item()) == (0.75, 0.25)
    crit.set_weights(lovasz=0.5)
    assert (r.item(), l.item()) == (0.75, 0.5)
    with pytest.raises(ValueError, match="finite"):
        crit.set_weights(lovasz=float("inf"))
    assert l.item() == 0.5


def test_forward_mixes_the_terms_and_hands_over_its_arguments(monkeypatch):
    seen = []

    def fake(prediction, target, classes, per_image, class_weights):
        seen.append((classes, per_image, class_weights, target.requires_grad))
        return prediction.sum() * 0 + 2.0
    monkeypatch.setattr(ops, "lovasz_loss", fake)
    inner = lambda p, t: {'loss': p.sum() * 0 + 3.0, 'dice_loss': torch.tensor(9.0)}   # noqa: E731
    crit = LovaszLoss(inner, 0.5, 0.25, 'all', True, [1, 2, 3])
    x = torch.zeros(2, 3, 4, 4, 4, requires_grad=True)
    out = crit(x, torch.zeros(2, 3, 4, 4, 4))
    assert list(out) == ['loss', 'dice_loss', 'lovasz_loss', 'regional_loss', 'lovasz_weight', 'regional_weight']
    assert out['loss'].item() == 0.25 * 3.0 + 0.5 * 2.0 and out['loss'].requires_grad
    assert (out['lovasz_loss'].item(), out['regional_loss'].item(), out['dice_loss'].item()) == (2.0, 3.0, 9.0)
    assert not out['lovasz_loss'].requires_grad and not out['regional_loss'].requires_grad
    assert (out['lovasz_weight'].item(), out['regional_weight'].item()) == (0.5, 0.25)
    assert out['lovasz_weight'] is not crit.lovasz_weight
    classes, per_image, cw, _ = seen[0]
    assert (classes, per_image) == ('all', True) and cw.tolist() == [1.0, 2.0, 3.0] and cw.dtype == torch.float32
    crit(x, torch.zeros(2, 3, 4, 4, 4))
    assert seen[1][2] is cw, "the weights are uploaded once per (values, device)"
    alone = LovaszLoss(lovasz_weight=0.5)(x, torch.zeros(2, 3, 4, 4, 4))
    assert list(alone) == ['loss', 'lovasz_loss', 'regional_loss', 'lovasz_weight', 'regional_weight']
    assert alone['loss'].item() == 1.0 and alone['regional_loss'].item() == 0.0 and seen[2][2] is None


def test_forward_errors():
    x = torch.zeros(1, 3, 2, 2, 2)
    with pytest.raises(_lib.M355Error, match=r"LovaszLoss takes one prediction tensor.*DeepSupervisionLoss\(LovaszLoss"):
        LovaszLoss()((x, x), x)
    with pytest.raises(_lib.M355Error, match="expected one shape"):
        LovaszLoss()(x, torch.zeros(1, 3, 2, 2, 3))
    with pytest.raises(_lib.M355Error, match="lovasz_class_weights of 2 values for 3 channels"):
        LovaszLoss(lovasz_class_weights=[1, 2])(x, x)


def test_pickled_state_holds_no_device_tensor(monkeypatch):
    monkeypatch.setattr(ops, "lovasz_loss", lambda p, *a: p.sum() * 0)
    crit = LovaszLoss(None, 0.3, 0.9, 'all', True, [1, 2])
    x = torch.zeros(1, 2, 2, 2, 2)
    crit(x, x)
    assert set(crit._uploaded) == {"lovasz_class_weights"}
    state = crit.__getstate__()
    assert state["_uploaded"] == {} and all(v.device.type == "cpu" for v in state["_buffers"].values())
    assert not any(torch.is_tensor(v) for v in state.values())
    back = pickle.loads(pickle.dumps(crit))
    assert back._uploaded == {} and (back.classes, back.per_image, back.lovasz_class_weights) == ('all', True, (1.0, 2.0))
    assert abs(back.lovasz_weight.item() - 0.3) < 1e-7 and abs(back.regional_weight.item() - 0.9) < 1e-7
    assert set(crit._uploaded) == {"lovasz_class_weights"}        # pickling leaves the live object alone
    assert back(x, x)['loss'].item() == 0.0


# ---------------------------------------------------------------------------------------------------------- the bindings
def test_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "m355seg.h")).read()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert getattr(_lib.lib(), s) is not None
        assert f"{s}(" in header, s
    assert len(_lib.SIGNATURES["m355_segmented_sort_u32"][1]) == 8
    assert len(_lib.SIGNATURES["m355_lovasz_loss_fwd"][1]) == 15 and len(_lib.SIGNATURES["m355_lovasz_loss_bwd"][1]) == 12
    assert V.sort_tile() > 0 and V.sort_tile() % 256 == 0 and V.loss_tile() > 0 and V.loss_tile() % 1024 == 0


def test_workspace_queries():
    L = _lib.lib()
    for bad in [(0, 5), (5, 0), (-1, 5), (5, -1)]:
        assert L.m355_segmented_sort_workspace(*bad) == 0, bad
    for bad in [(0, 3, 100), (2, 0, 100), (2, 3, 0), (-1, 3, 100), (2, 3, -5)]:
        assert L.m355_lovasz_loss_workspace(*bad, 0) == 0 and L.m355_lovasz_loss_workspace(*bad, 1) == 0, bad
    up = lambda v: (v + 255) // 256 * 256   # noqa: E731
    for R, M in ((1, 1), (5, 4097), (3, 10 ** 6)):
        tiles = -(-M // V.sort_tile())
        assert L.m355_segmented_sort_workspace(R, M) == up(4 * R * M) + 4 * 256 * R * (tiles + 1) + 256, (R, M)
    for N, C, S, per_image in ((1, 3, 100, 0), (2, 3, 5000, 0), (2, 3, 5000, 1), (1, 4, 128 ** 3, 0)):
        R, M = (N * C, S) if per_image else (C, N * S)
        T = -(-M // V.loss_tile())
        want = up(4 * R * M) + up(L.m355_segmented_sort_workspace(R, M)) + up(4 * R * T) + 8 * R * T + 8 * R + 256
        assert L.m355_lovasz_loss_workspace(N, C, S, per_image) == want, (N, C, S, per_image)


def test_sort_argument_checks_reject_before_any_launch():
    L = _lib.lib()
    a, b = P(64), P(1 << 20)
    ws = L.m355_segmented_sort_workspace(2, 100)

    def sort(keys=a, out=b, R=2, M=100, end_bit=31, w=a, nbytes=ws):
        return L.m355_segmented_sort_u32(keys, out, R, M, end_bit, w, nbytes, None)
    for kw in (dict(keys=None), dict(out=None), dict(w=None)):
        assert sort(**kw) == -1 and b"segmented_sort_u32: null pointer" in L.m355_last_error(), kw
    for kw in (dict(R=0), dict(M=0), dict(R=-1), dict(M=-7)):
        assert sort(**kw) == -1 and b"segmented_sort_u32: non-positive size" in L.m355_last_error(), kw
    for end_bit in (0, -1, 33):
        assert sort(end_bit=end_bit) == -1 and b"end_bit outside [1, 32]" in L.m355_last_error()
    assert sort(out=a) == -1 and b"overlap" in L.m355_last_error()
    assert sort(R=65536, nbytes=1 << 40) == -2 and b"segmented_sort_u32: R > 65535" in L.m355_last_error()
    assert sort(M=1 << 31, nbytes=1 << 50) == -2 and b"segmented_sort_u32: M > 2^31 - 1" in L.m355_last_error()
    assert sort(nbytes=ws - 1) == -4 and b"segmented_sort_u32: workspace too small" in L.m355_last_error()
    assert sort(nbytes=0) == -4


@pytest.mark.parametrize("per_image", [0, 1])
def test_loss_argument_checks_reject_before_any_launch(per_image):
    L = _lib.lib()
    a = P(64)
    ws = L.m355_lovasz_loss_workspace(2, 3, 100, per_image)

    def fwd(p=a, t=a, N=2, C=3, S=100, out2=a, skeys=a, F=a, state=a, w=a, nbytes=ws):
        return L.m355_lovasz_loss_fwd(p, t, N, C, S, per_image, 0, None, out2, skeys, F, state, w, nbytes, None)

    def bwd(p=a, t=a, skeys=a, F=a, state=a, dloss=a, N=2, C=3, S=100, dx=a):
        return L.m355_lovasz_loss_bwd(p, t, skeys, F, state, dloss, N, C, S, per_image, dx, None)
    for kw in (dict(p=None), dict(t=None), dict(out2=None), dict(skeys=None), dict(F=None), dict(state=None), dict(w=None)):
        assert fwd(**kw) == -1 and b"lovasz_loss_fwd: null pointer" in L.m355_last_error(), kw
    for kw in (dict(p=None), dict(t=None), dict(skeys=None), dict(F=None), dict(state=None), dict(dloss=None), dict(dx=None)):
        assert bwd(**kw) == -1 and b"lovasz_loss_bwd: null pointer" in L.m355_last_error(), kw
    for kw in (dict(N=0), dict(C=0), dict(S=0), dict(N=-2), dict(S=-1)):
        assert fwd(**kw) == -1 and b"lovasz_loss_fwd: non-positive size" in L.m355_last_error(), kw
        assert bwd(**kw) == -1 and b"lovasz_loss_bwd: non-positive size" in L.m355_last_error(), kw
    assert fwd(N=256, C=256, nbytes=1 << 40) == -2 and b"lovasz_loss_fwd: N*C > 65535" in L.m355_last_error()
    assert bwd(N=65536, C=1) == -2 and b"lovasz_loss_bwd: N*C > 65535" in L.m355_last_error()
    assert fwd(S=1 << 31, nbytes=1 << 50) == -2 and b"2^31 - 1" in L.m355_last_error()
    if not per_image:
        assert fwd(N=2, S=1 << 30, nbytes=1 << 50) == -2 and b"lovasz_loss_fwd: N*S > 2^31 - 1" in L.m355_last_error()
        assert bwd(N=2, S=1 << 30) == -2 and b"lovasz_loss_bwd: N*S > 2^31 - 1" in L.m355_last_error()
    assert fwd(nbytes=ws - 1) == -4 and b"lovasz_loss_fwd: workspace too small" in L.m355_last_error()
    assert fwd(nbytes=0) == -4
    assert fwd(S=5000, nbytes=ws) == -4


def test_ops_wrapper_errors():
    """raised on the host before the device is looked at: the same without a GPU"""
    x = torch.zeros(2, 3, 4, 4, 4)
    with pytest.raises(ValueError, match="classes"):
        ops.lovasz_loss(x, x, classes="none")
    with pytest.raises(_lib.M355Error, match=r"class_weights of shape \(4,\) for 3 channels"):
        ops.lovasz_loss(x, x, class_weights=torch.ones(4))
    with pytest.raises(_lib.M355Error, match=r"prediction \(2, 3, 4, 4, 4\) and target \(2, 3, 4, 4, 5\)"):
        ops.lovasz_loss(x, torch.zeros(2, 3, 4, 4, 5))
    with pytest.raises(_lib.M355Error, match="prediction: expected torch.float32, got torch.float16"):
        ops.lovasz_loss(x.half(), x)
    with pytest.raises(_lib.M355Error, match="no CPU fallback"):      # valid arguments, host tensors: no quiet fall-back
        ops.lovasz_loss(x, x, 'all', True)
    with pytest.raises(_lib.M355Error, match="expected torch.int32"):
        ops.segmented_sort(torch.zeros(2, 3))
    with pytest.raises(_lib.M355Error, match=r"non-empty \[R, M\]"):
        ops.segmented_sort(torch.zeros(6, dtype=torch.int32))
    with pytest.raises(_lib.M355Error, match="no CPU fallback"):
        ops.segmented_sort(torch.zeros(2, 3, dtype=torch.int32))


# --------------------------------------------------------------------------------- the closed form against Berman's code
CONFIGS = [dict(classes=c, per_image=pi, class_weights=w) for c in V.CLASSES for pi in (False, True)
           for w in (None, [1.0, 0.5, 2.0])]
SHAPE = (2, 3, 5, 4, 6)


def _both(p, t, cfg, dloss=0.7):
    loss, dx = V.berman_run(p, t, dloss, torch.float64, **cfg)
    return loss, dx, V.closed_form(p, t, dloss, **cfg)


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"{c['classes']}-{'image' if c['per_image'] else 'batch'}-"
                                                      f"{'w' if c['class_weights'] else 'ones'}")
def test_closed_form_is_bermans_loss_and_gradient_without_ties(cfg):
    p, t = V.untied_inputs(SHAPE, 5)
    loss, dx, mine = _both(p, t, cfg)
    assert abs(mine['loss'].item() - loss.item()) <= 1e-13 * abs(loss.item())
    assert (mine['dx'] - dx).abs().max().item() <= 1e-13 * dx.abs().max().item()
    assert dx.abs().max().item() > 0 and mine['count'] > 0


@pytest.mark.parametrize("cfg", CONFIGS[::3], ids=["a", "b", "c"])
def test_closed_form_is_bermans_loss_with_ties_and_shares_the_group_sums(cfg):
    """tied errors: the same loss; the gradient summed over each group of (segment, error value, foreground or not) is
    Berman's -- his sort hands the group's subgradients out in some order, the closed form gives every member their
    mean.  e = 0 elements are left out of the sums: torch's abs has gradient 0 there, the closed form the one-sided one."""
    p, t = V.tied_inputs(SHAPE, 6)
    loss, dx, mine = _both(p, t, cfg)
    assert abs(mine['loss'].item() - loss.item()) <= 1e-13 * abs(loss.item())
    pi = cfg['per_image']
    ps, ts, a, b = V.segments(p, pi), V.segments(t, pi), V.segments(dx, pi), V.segments(mine['dx'], pi)
    fg = ts >= 0.5
    e = (fg.float() - ps).abs()
    groups = 0
    for r in range(ps.shape[0]):
        for v in e[r].unique():
            if v.item() == 0:
                continue
            m = e[r] == v
            # de/dp is -1 on foreground and +1 on background: undo the sign, then the group is one group of dL/de
            sa = torch.where(fg[r][m], -a[r][m], a[r][m]).sum().item()
            sb = torch.where(fg[r][m], -b[r][m], b[r][m])
            assert abs(sa - sb.sum().item()) <= 1e-12 * max(abs(sa), 1e-3), (r, v)
            assert (sb - sb[0]).abs().max().item() <= 1e-15, "every member of a group gets the same dL/de"
            groups += 1
    assert groups >= 2 * ps.shape[0]


def test_closed_form_at_zero_error_has_the_one_sided_derivative():
    p = torch.tensor([1.0, 0.0, 0.25, 0.75]).reshape(1, 1, 4)
    t = torch.tensor([1.0, 0.0, 1.0, 0.0]).reshape(1, 1, 4)
    mine = V.closed_form(p, t, 1.0)
    assert mine['dx'][0, 0, 0].item() < 0 < mine['dx'][0, 0, 1].item()     # e = 0: -1 for foreground, +1 for background
    assert V.berman_run(p, t, 1.0, torch.float64)[1][0, 0, :2].abs().max().item() == 0.0   # torch's abs gives 0 there


def test_reductions():
    """two images, three channels; image 1 has no foreground at all, channel 2 none anywhere"""
    g = torch.Generator().manual_seed(8)
    p = torch.rand((2, 3, 40), generator=g)
    t = torch.zeros(2, 3, 40)
    t[0, 0, :7] = 1.0
    t[0, 1, 20:23] = 1.0
    Lb, _, Gb = V.closed_form_segments(p, t, False)
    Li, _, Gi = V.closed_form_segments(p, t, True)
    assert Gb.tolist() == [7, 3, 0] and Gi.tolist() == [7, 3, 0, 0, 0, 0]
    w = [1.0, 3.0, 5.0]
    loss = lambda **cfg: V.closed_form(p, t, 1.0, **cfg)   # noqa: E731
    assert loss()['loss'].item() == pytest.approx(((Lb[0] + Lb[1]) / 2).item(), rel=1e-14) and loss()['count'] == 2
    assert loss(classes='all')['loss'].item() == pytest.approx(Lb.mean().item(), rel=1e-14)
    assert loss(class_weights=w)['loss'].item() == pytest.approx(((Lb[0] + 3 * Lb[1]) / 4).item(), rel=1e-14)
    assert loss(classes='all', class_weights=w)['loss'].item() == pytest.approx(((Lb[0] + 3 * Lb[1] + 5 * Lb[2]) / 9).item(), rel=1e-14)
    # per image: the empty image gives 0 and still counts in the mean over the images
    r = loss(per_image=True)
    assert r['loss'].item() == pytest.approx(((Li[0] + Li[1]) / 2 / 2).item(), rel=1e-14) and r['count'] == 2
    assert r['dx'][1].abs().max().item() == 0.0 and r['dx'][0, 2].abs().max().item() == 0.0
    assert r['dx'][0, 0].abs().max().item() > 0 and r['dx'][0, 1].abs().max().item() > 0
    assert loss(per_image=True, classes='all')['loss'].item() == pytest.approx(Li.mean().item(), rel=1e-14)
    # an absent class under 'all' costs its largest error: J jumps to 1 at the first element
    assert Lb[2].item() == pytest.approx(p[:, 2].max().item(), rel=1e-7)
    # nothing present at all: loss 0, gradient 0
    none = V.closed_form(p, torch.zeros_like(t), 1.0)
    assert none['loss'].item() == 0.0 and none['count'] == 0 and none['dx'].abs().max().item() == 0.0
    assert V.berman(p.double(), torch.zeros_like(t).double()).item() == 0.0
    # weights that are all zero on the present classes: the same
    assert loss(class_weights=[0.0, 0.0, 1.0])['loss'].item() == 0.0
