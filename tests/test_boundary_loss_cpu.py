"""BoundaryLoss and the batched signed distance: what can be checked without a GPU -- exports and bindings, every argument
check of the five entry points (they return before a launch; pointers are integers that are never followed), the
criterion's constructor, default class weights and pickled state, the ops wrappers' argument errors, and the brute-force
reference of tests/boundary_ref.py against scipy's two-transform formula."""
import ctypes
import inspect
import os
import pickle

import numpy as np
import pytest
import torch

import boundary_ref as B
from conftest import ROOT
from segmentation_pipeline_amd import _lib, criterions, ops
from segmentation_pipeline_amd.criterions import BoundaryLoss, HybridLogisticDiceLoss

SYMBOLS = ["m355_signed_distance_workspace", "m355_signed_distance", "m355_boundary_loss_workspace",
           "m355_boundary_loss_fwd", "m355_boundary_loss_bwd"]
P = ctypes.c_void_p
I3 = ctypes.c_int32 * 3
F3 = ctypes.c_float * 3
CHUNK = 8192   # elements of a row per partial sum


# ------------------------------------------------------------------------------------------------ exports, bindings
def test_exports_and_signatures():
    assert criterions.BoundaryLoss is BoundaryLoss
    sig = inspect.signature(BoundaryLoss.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[2:]] == [
        ("boundary_weight", 0.01), ("regional_weight", 1.0), ("boundary_class_weights", None), ("spacing", (1., 1., 1.))]
    assert [(k, v.default) for k, v in inspect.signature(ops.signed_distance).parameters.items()][1:] == [
        ("spacing", (1., 1., 1.)), ("planes", None)]
    assert list(inspect.signature(ops.boundary_loss).parameters) == ["p", "phi", "class_weights"]
    assert [k for k in inspect.signature(BoundaryLoss.set_weights).parameters] == ["self", "regional", "boundary"]


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "m355seg.h")).read()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert getattr(_lib.lib(), s) is not None
        assert f"{s}(" in header, s
    assert len(_lib.SIGNATURES["m355_signed_distance"][1]) == 9
    assert len(_lib.SIGNATURES["m355_boundary_loss_fwd"][1]) == 10 and len(_lib.SIGNATURES["m355_boundary_loss_bwd"][1]) == 8
    assert _lib.lib().m355_version() == 3


# ------------------------------------------------------------------------------------------- entry points, no launch
def test_workspace_queries():
    L = _lib.lib()
    assert L.m355_signed_distance_workspace(0, I3(4, 4, 4)) == 0
    assert L.m355_signed_distance_workspace(-1, I3(4, 4, 4)) == 0
    assert L.m355_signed_distance_workspace(2, None) == 0
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, -1)):
        assert L.m355_signed_distance_workspace(2, I3(*bad)) == 0, bad
    assert L.m355_signed_distance_workspace(1, I3(1, 1, 1)) == 256                      # two bytes a voxel, in 256-byte steps
    assert L.m355_signed_distance_workspace(6, I3(3, 5, 70)) == -(-6 * 1050 * 2 // 256) * 256
    assert L.m355_signed_distance_workspace(16, I3(96, 88, 24)) == 16 * 96 * 88 * 24 * 2
    for bad in ((0, 3, 100), (2, 0, 100), (2, 3, 0), (-1, 3, 100), (2, 3, -5)):
        assert L.m355_boundary_loss_workspace(*bad) == 0, bad
    one = L.m355_boundary_loss_workspace(2, 3, 1)
    assert one >= 2 * 3 * 8
    assert L.m355_boundary_loss_workspace(2, 3, CHUNK) == one
    assert L.m355_boundary_loss_workspace(2, 3, CHUNK + 1) - one == 2 * 3 * 8
    assert L.m355_boundary_loss_workspace(1, 4, 128 ** 3) - one == (4 * 256 - 6) * 8


def test_signed_distance_argument_checks_reject_before_any_launch():
    L = _lib.lib()
    a = P(64)
    big = 1 << 40

    def call(target=a, planes=2, size=(3, 5, 70), spacing=(1.0, 1.0, 1.0), on=None, phi=a, ws=a, nbytes=big,
             size_ptr=True, spacing_ptr=True):
        return L.m355_signed_distance(target, planes, I3(*size) if size_ptr else None, F3(*spacing) if spacing_ptr else None,
                                      on, phi, ws, nbytes, None)
    for kw in (dict(target=None), dict(phi=None), dict(ws=None), dict(size_ptr=False), dict(spacing_ptr=False)):
        assert call(**kw) == -1 and b"signed_distance: null pointer" in L.m355_last_error(), kw
    for planes in (0, -3):
        assert call(planes=planes) == -1 and b"signed_distance: %d planes" % planes in L.m355_last_error()
    for size in ((0, 5, 70), (3, -1, 70), (3, 5, 0)):
        assert call(size=size) == -1 and b"signed_distance: size" in L.m355_last_error(), size
    assert call(size=(2048, 2048, 512)) == -1 and b"fewer than 2^31" in L.m355_last_error()
    for spacing in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0)):
        assert call(spacing=spacing) == -1 and b"signed_distance: spacing" in L.m355_last_error(), spacing
    for axis, size in enumerate(((513, 2, 2), (2, 513, 2), (2, 2, 513))):
        assert call(size=size) == -2 and b"signed_distance: size 513 on axis %d" % axis in L.m355_last_error(), size
    need = L.m355_signed_distance_workspace(2, I3(3, 5, 70))
    assert call(nbytes=need - 1) == -4 and b"signed_distance: workspace" in L.m355_last_error()
    assert call(nbytes=0) == -4
    assert call(planes=3, nbytes=need) == -4      # a third plane needs more


def test_boundary_loss_argument_checks_reject_before_any_launch():
    L = _lib.lib()
    a = P(64)
    ws = L.m355_boundary_loss_workspace(2, 3, 100)

    def fwd(p=a, phi=a, w=None, N=2, C=3, S=100, loss=a, work=a, nbytes=ws):
        return L.m355_boundary_loss_fwd(p, phi, w, N, C, S, loss, work, nbytes, None)
    for kw in (dict(p=None), dict(phi=None), dict(loss=None), dict(work=None)):
        assert fwd(**kw) == -1 and b"boundary_loss_fwd: null pointer" in L.m355_last_error(), kw
    for kw in (dict(N=0), dict(C=0), dict(S=0), dict(N=-2), dict(S=-1)):
        assert fwd(**kw) == -1 and b"boundary_loss_fwd: non-positive size" in L.m355_last_error(), kw
    assert fwd(N=256, C=256, nbytes=1 << 40) == -2 and b"boundary_loss_fwd: N*C > 65535" in L.m355_last_error()
    assert fwd(nbytes=ws - 1) == -4 and b"boundary_loss_fwd: workspace too small" in L.m355_last_error()
    assert fwd(S=CHUNK + 1, nbytes=ws) == -4

    def bwd(phi=a, dloss=a, w=None, N=2, C=3, S=100, dp=a):
        return L.m355_boundary_loss_bwd(phi, dloss, w, N, C, S, dp, None)
    for kw in (dict(phi=None), dict(dloss=None), dict(dp=None)):
        assert bwd(**kw) == -1 and b"boundary_loss_bwd: null pointer" in L.m355_last_error(), kw
    for kw in (dict(N=0), dict(C=-1), dict(S=0)):
        assert bwd(**kw) == -1 and b"boundary_loss_bwd: non-positive size" in L.m355_last_error(), kw
    assert bwd(N=65536, C=1) == -2 and b"boundary_loss_bwd: N*C > 65535" in L.m355_last_error()


# ------------------------------------------------------------------------------------------------------ ops wrappers
def test_ops_wrapper_errors_come_before_the_device_check():
    x = torch.zeros(2, 3, 4, 4, 4)
    with pytest.raises(_lib.M355Error, match="signed_distance: target: element type torch.float16"):
        ops.signed_distance(x.half())
    with pytest.raises(_lib.M355Error, match="signed_distance: target: element type ndarray"):
        ops.signed_distance(np.zeros((1, 1, 2, 2, 2), dtype=np.float32))
    with pytest.raises(_lib.M355Error, match=r"expected \[N, C, D, H, W\], got shape \(3, 4, 4, 4\)"):
        ops.signed_distance(x[0])
    with pytest.raises(_lib.M355Error, match="a number or three numbers"):
        ops.signed_distance(x, spacing=(1.0, 2.0))
    with pytest.raises(_lib.M355Error, match="5 plane flags for N . C = 6 planes"):
        ops.signed_distance(x, planes=[1, 0, 1, 1, 0])
    with pytest.raises(_lib.M355Error, match="expected a contiguous tensor"):
        ops.signed_distance(x.permute(0, 1, 4, 3, 2))
    with pytest.raises(_lib.M355Error, match="signed_distance: target: expected a device tensor"):     # no quiet fall-back
        ops.signed_distance(x, planes=[1] * 6)
    with pytest.raises(_lib.M355Error, match=r"class_weights of shape \(2,\) for 3 channels"):
        ops.boundary_loss(x, x, torch.ones(2))
    with pytest.raises(_lib.M355Error, match=r"prediction \(2, 3, 4, 4, 4\) and phi \(2, 3, 4, 4, 5\)"):
        ops.boundary_loss(x, torch.zeros(2, 3, 4, 4, 5))
    with pytest.raises(_lib.M355Error, match="prediction: expected torch.float32, got torch.float16"):
        ops.boundary_loss(x.half(), x)
    with pytest.raises(_lib.M355Error, match="phi: expected torch.float32, got torch.float64"):
        ops.boundary_loss(x, x.double())
    with pytest.raises(_lib.M355Error, match="class_weights: expected torch.float32, got torch.int64"):
        ops.boundary_loss(x, x, torch.ones(3, dtype=torch.int64))
    with pytest.raises(_lib.M355Error, match="no CPU fallback"):
        ops.boundary_loss(x, x, torch.ones(3))


# --------------------------------------------------------------------------------------------------------- criterion
@pytest.mark.parametrize("kw, match", [
    (dict(boundary_weight=float("nan")), "boundary_weight"), (dict(regional_weight=float("inf")), "regional_weight"),
    (dict(boundary_class_weights=[]), "boundary_class_weights"), (dict(boundary_class_weights=[1.0, -0.5]), "finite values >= 0"),
    (dict(boundary_class_weights=[1.0, float("nan")]), "finite values >= 0"),
    (dict(boundary_class_weights=[float("inf"), 1.0]), "finite values >= 0"),
    (dict(boundary_class_weights=[0.0, 0.0]), "positive weight"), (dict(boundary_class_weights=torch.ones(2, 2)), "expected .C."),
    (dict(spacing=(1.0, 0.0, 1.0)), "spacing"), (dict(spacing=(1.0, float("nan"), 1.0)), "spacing")],
    ids=lambda v: v if isinstance(v, str) else "_".join(v))
def test_invalid_parameters_raise_at_construction(kw, match):
    with pytest.raises(ValueError, match=match):
        BoundaryLoss(HybridLogisticDiceLoss(), **kw)


def test_spacing_of_the_wrong_length_raises():
    with pytest.raises(_lib.M355Error, match="a number or three numbers"):
        BoundaryLoss(HybridLogisticDiceLoss(), spacing=(1.0, 2.0))


def _fake_ops(monkeypatch, seen):
    def fake_sd(target, spacing=(1., 1., 1.), planes=None):
        seen.update(spacing=spacing, planes=list(planes))
        return torch.zeros_like(target)

    def fake_bl(p, phi, class_weights=None):
        seen.update(class_weights=class_weights)
        return torch.tensor(2.0)
    monkeypatch.setattr(ops, "signed_distance", fake_sd)
    monkeypatch.setattr(ops, "boundary_loss", fake_bl)
    monkeypatch.setattr(ops, "hybrid_logistic_dice_loss", lambda *a: (torch.tensor(1.0), torch.tensor(0.25), torch.tensor(0.75)))


def test_forward_dict_default_weights_and_in_place_mixing_weights(monkeypatch):
    seen = {}
    _fake_ops(monkeypatch, seen)
    crit = BoundaryLoss(HybridLogisticDiceLoss(), boundary_weight=0.5, spacing=(0.7, 1.3, 2.0))
    assert isinstance(crit, torch.nn.Module) and set(dict(crit.named_buffers())) == {"regional_weight", "boundary_weight"}
    x = torch.zeros(2, 3, 2, 2, 2)
    out = crit(x, x)
    assert list(out) == ['loss', 'dice_loss', 'logistic_loss', 'boundary_loss', 'regional_loss', 'boundary_weight',
                         'regional_weight']
    assert all(torch.is_tensor(v) for v in out.values())
    assert [v.item() for v in out.values()] == [2.0, 0.25, 0.75, 2.0, 1.0, 0.5, 1.0]
    # the background is dropped by default when there is more than one channel: its planes are not transformed
    assert seen["class_weights"].tolist() == [0.0, 1.0, 1.0] and seen["class_weights"].dtype == torch.float32
    assert seen["planes"] == [False, True, True] * 2 and seen["spacing"] == (0.7, 1.3, 2.0)
    first = seen["class_weights"]
    ptrs = crit.regional_weight.data_ptr(), crit.boundary_weight.data_ptr()
    crit.set_weights(regional=0.25)
    crit.set_weights(boundary=2.0)
    crit.set_weights()
    assert (crit.regional_weight.data_ptr(), crit.boundary_weight.data_ptr()) == ptrs
    out2 = crit(x, x)
    assert out2['loss'].item() == 0.25 * 1.0 + 2.0 * 2.0 and out['boundary_weight'].item() == 0.5
    assert seen["class_weights"] is first, "the weights are uploaded once per (values, device)"
    with pytest.raises(ValueError, match="finite"):
        crit.set_weights(boundary=float("nan"))
    one = torch.zeros(1, 1, 2, 2, 2)
    BoundaryLoss(HybridLogisticDiceLoss())(one, one)
    assert seen["class_weights"].tolist() == [1.0] and seen["planes"] == [True]       # a single channel keeps its weight
    BoundaryLoss(HybridLogisticDiceLoss(), boundary_class_weights=torch.tensor([2.0, 0.0, 0.5]))(x, x)
    assert seen["class_weights"].tolist() == [2.0, 0.0, 0.5] and seen["planes"] == [True, False, True] * 2


def test_shape_and_length_errors_of_the_criterion(monkeypatch):
    _fake_ops(monkeypatch, {})
    x = torch.zeros(1, 3, 2, 2, 2)
    with pytest.raises(_lib.M355Error, match="boundary_class_weights of 2 values for 3 channels"):
        BoundaryLoss(HybridLogisticDiceLoss(), boundary_class_weights=[1, 2])(x, x)
    with pytest.raises(_lib.M355Error, match="DeepSupervisionLoss.BoundaryLoss"):
        BoundaryLoss(HybridLogisticDiceLoss())((x, x), x)
    with pytest.raises(_lib.M355Error, match=r"expected one shape \[N, C, D, H, W\]"):
        BoundaryLoss(HybridLogisticDiceLoss())(x, torch.zeros(1, 3, 2, 2, 3))


def test_pickled_state_holds_no_device_tensor(monkeypatch):
    _fake_ops(monkeypatch, {})
    crit = BoundaryLoss(HybridLogisticDiceLoss(logistic_class_weights=[1, 2]), 0.25, 0.75, [0, 3], (1.0, 1.0, 2.5))
    x = torch.zeros(1, 2, 2, 2, 2)
    crit(x, x)
    assert set(crit._uploaded) == {"boundary_class_weights"}
    state = crit.__getstate__()
    assert state["_uploaded"] == {}
    assert all(v.device.type == "cpu" for v in state["_buffers"].values())
    assert not any(torch.is_tensor(v) for k, v in state.items() if not k.startswith("_"))
    back = pickle.loads(pickle.dumps(crit))
    assert back._uploaded == {} and back.boundary_class_weights == (0.0, 3.0) and back.spacing == (1.0, 1.0, 2.5)
    assert (back.boundary_weight.item(), back.regional_weight.item()) == (0.25, 0.75)
    assert back.criterion.logistic_class_weights == [1, 2] and back.criterion._uploaded == {}
    assert set(crit._uploaded) == {"boundary_class_weights"}        # pickling leaves the live object alone


# ----------------------------------------------------------------------------------- the reference against scipy
@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), (0.7, 1.3, 2.0)], ids=["unit", "aniso"])
def test_brute_force_reference_is_the_published_two_transform_formula(spacing):
    pytest.importorskip("scipy")
    rng = np.random.default_rng(5)
    worst = 0.0
    for shape in ((1, 1, 1), (1, 1, 7), (3, 5, 9), (6, 2, 8), (4, 7, 5)):
        for density in (0.0, 0.02, 0.3, 0.5, 0.9, 1.0):
            t = (rng.random((2, 2) + shape) < density).astype(np.float32)
            mine, ref = B.signed_distance(t, spacing), B.scipy_signed_distance(t, spacing)
            worst = max(worst, float(np.abs(mine - ref).max()))
            if spacing == (1.0, 1.0, 1.0):   # the fp32 value: the root rounded once (2^-24 relative), the subtraction exact
                f32 = B.signed_distance_f32(t).astype(np.float64)
                assert np.all(np.abs(f32 - mine) <= 2.0 ** -24 * (np.abs(mine) + 1.0))
    print(f"boundary_loss reference vs scipy, spacing {spacing}: max difference {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), (0.7, 1.3, 2.0)], ids=["unit", "aniso"])
def test_reference_is_distance_ref_edt_sq_on_the_two_masks(spacing):
    """the reference restricts distance_ref.edt_sq's minimum to the voxels that need it: the same values bit for bit"""
    rng = np.random.default_rng(6)
    for shape in ((1, 1, 7), (3, 5, 9), (6, 2, 8)):
        for density in (0.0, 0.05, 0.5, 0.95, 1.0):
            m = rng.random(shape) < density
            full, mine = B.plane_d2_full(m, spacing), B._plane_d2(m, spacing)
            assert (full is None and mine is None) or np.array_equal(full, mine)


def test_reference_conventions():
    t = np.zeros((1, 3, 1, 1, 5), dtype=np.float32)
    t[0, 0, 0, 0, 1:4] = 1.0                       # o i i i o
    t[0, 1] = 1.0                                  # all inside
    t[0, 2, 0, 0, 0] = np.nan                      # NaN is outside, 0.5 is outside, above it inside
    t[0, 2, 0, 0, 1:] = (0.5, 0.50001, 0.2, 1.0)
    phi = B.signed_distance(t)
    assert phi[0, 0, 0, 0].tolist() == [1.0, 0.0, -1.0, 0.0, 1.0]
    assert not phi[0, 1].any()
    assert phi[0, 2, 0, 0].tolist() == [2.0, 1.0, 0.0, 1.0, 0.0]
    assert not B.signed_distance(t, planes=[0, 1, 0]).any()
    p = torch.rand((1, 3, 1, 1, 5), dtype=torch.float64, requires_grad=True)
    l = B.loss(p, torch.from_numpy(phi), [0.0, 1.0, 2.0])
    l.backward()
    assert torch.allclose(p.grad, B.grad(torch.from_numpy(phi), [0.0, 1.0, 2.0]), rtol=1e-14, atol=0)
    assert abs(l.item() - 2.0 * float((p.detach()[0, 2] * torch.from_numpy(phi)[0, 2]).sum()) / (5 * 3.0)) <= 1e-15
