"""HybridFocalTverskyLoss: what can be checked without a GPU -- the criterion's interface and pickled state, the bindings,
the argument checks of the three entry points (no launches) and of the ops wrapper, the workspace query, and the fp64
formulas of tests/focal_tversky_ref.py against the oracle's loss, the recorded fixture and autograd."""
import ctypes
import inspect
import os
import pickle

import numpy as np
import pytest
import torch

import focal_tversky_ref as F
from conftest import ROOT
from oracle import torch_ref as R
from segmentation_pipeline_amd import _lib, criterions, ops
from segmentation_pipeline_amd.criterions import HybridFocalTverskyLoss

SYMBOLS = ["m355_focal_tversky_workspace", "m355_focal_tversky_fwd", "m355_focal_tversky_bwd"]
P = ctypes.c_void_p
CHUNK = 4096   # voxels per partial sum of the logits mode, the smaller of the two chunks: the workspace is sized by it


def test_constructor_defaults_and_export():
    assert criterions.HybridFocalTverskyLoss is HybridFocalTverskyLoss
    sig = inspect.signature(HybridFocalTverskyLoss.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ("tversky_weight", 0.5), ("alpha", 0.5), ("beta", 0.5), ("tversky_power", 1.0), ("focal_gamma", 0.0),
        ("logistic_class_weights", None), ("tversky_class_weights", None), ("from_logits", False)]
    crit = HybridFocalTverskyLoss()
    assert (crit.tversky_weight, crit.alpha, crit.beta, crit.tversky_power, crit.focal_gamma, crit.logistic_class_weights,
            crit.tversky_class_weights, crit.from_logits) == (0.5, 0.5, 0.5, 1.0, 0.0, None, None, False)
    assert isinstance(crit, torch.nn.Module)
    doc = inspect.getmodule(HybridFocalTverskyLoss).__doc__
    assert "positive half" in doc and "HybridBinaryLogisticDiceLoss" in doc
    assert [(k, v.default) for k, v in list(inspect.signature(ops.focal_tversky_loss).parameters.items())[2:]] == [
        ("tversky_weight", 0.5), ("alpha", 0.5), ("beta", 0.5), ("tversky_power", 1.0), ("focal_gamma", 0.0),
        ("focal_class_weights", None), ("tversky_class_weights", None), ("from_logits", False)]


def test_forward_returns_the_three_keys(monkeypatch):
    """the arguments handed to ops.focal_tversky_loss in its order; the weights are uploaded once"""
    seen = {}

    def fake(x, t, tversky_weight, alpha, beta, tversky_power, focal_gamma, focal_class_weights, tversky_class_weights,
             from_logits):
        seen.update(tversky_weight=tversky_weight, alpha=alpha, beta=beta, tversky_power=tversky_power,
                    focal_gamma=focal_gamma, focal_class_weights=focal_class_weights,
                    tversky_class_weights=tversky_class_weights, from_logits=from_logits)
        return torch.tensor(1.0), torch.tensor(2.0), torch.tensor(3.0)
    monkeypatch.setattr(ops, "focal_tversky_loss", fake)
    crit = HybridFocalTverskyLoss(0.3, 0.2, 0.8, 0.75, 2.0, [1, 2, 3], (0, 1, 1), True)
    out = crit(torch.zeros(2, 3, 4, 4, 4), torch.zeros(2, 3, 4, 4, 4))
    assert list(out) == ['loss', 'tversky_loss', 'focal_loss']
    assert [v.item() for v in out.values()] == [1.0, 2.0, 3.0]
    assert (seen["tversky_weight"], seen["alpha"], seen["beta"], seen["tversky_power"], seen["focal_gamma"]) == \
        (0.3, 0.2, 0.8, 0.75, 2.0)
    assert seen["from_logits"] is True
    assert seen["focal_class_weights"].tolist() == [1.0, 2.0, 3.0] and seen["focal_class_weights"].dtype == torch.float32
    assert seen["tversky_class_weights"].tolist() == [0.0, 1.0, 1.0]
    first = seen["focal_class_weights"], seen["tversky_class_weights"]
    crit(torch.zeros(2, 3, 4, 4, 4), torch.zeros(2, 3, 4, 4, 4))
    assert seen["focal_class_weights"] is first[0] and seen["tversky_class_weights"] is first[1], \
        "the weights are uploaded once per (values, device)"


def test_weight_length_is_checked_by_the_criterion():
    x = torch.zeros(1, 3, 2, 2, 2)
    with pytest.raises(_lib.M355Error, match="tversky_class_weights of 2 values for 3 channels"):
        HybridFocalTverskyLoss(tversky_class_weights=[1, 2])(x, x)
    with pytest.raises(_lib.M355Error, match="logistic_class_weights of shape"):
        HybridFocalTverskyLoss(logistic_class_weights=torch.ones(4))(x, x)


def test_pickled_state_holds_no_device_tensor(monkeypatch):
    monkeypatch.setattr(ops, "focal_tversky_loss", lambda *a: (torch.tensor(0.0),) * 3)
    crit = HybridFocalTverskyLoss(0.3, 0.3, 0.7, 0.75, 2.0, logistic_class_weights=[1, 2], tversky_class_weights=[0, 1])
    crit(torch.zeros(1, 2, 2, 2, 2), torch.zeros(1, 2, 2, 2, 2))
    assert set(crit._uploaded) == {"logistic_class_weights", "tversky_class_weights"}
    state = crit.__getstate__()
    assert state["_uploaded"] == {}
    assert not any(torch.is_tensor(v) for v in state.values())
    back = pickle.loads(pickle.dumps(crit))
    assert back._uploaded == {} and back.tversky_class_weights == [0, 1] and back.logistic_class_weights == [1, 2]
    assert (back.tversky_weight, back.alpha, back.beta, back.tversky_power, back.focal_gamma, back.from_logits) == \
        (0.3, 0.3, 0.7, 0.75, 2.0, False)
    assert set(crit._uploaded) == {"logistic_class_weights", "tversky_class_weights"}   # pickling leaves the live object alone


@pytest.mark.parametrize("kw", [dict(focal_gamma=0.5), dict(tversky_power=0.0), dict(alpha=-1.0), dict(beta=-0.1),
                                dict(focal_gamma=float("nan")), dict(tversky_power=float("inf")), dict(alpha=float("inf"))],
                         ids=lambda kw: "_".join(f"{k}={v}" for k, v in kw.items()))
def test_invalid_parameters_raise_at_construction(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        HybridFocalTverskyLoss(**kw)


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "m355seg.h")).read()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert getattr(_lib.lib(), s) is not None
        assert f"{s}(" in header, s
    assert len(_lib.SIGNATURES["m355_focal_tversky_fwd"][1]) == 18 and len(_lib.SIGNATURES["m355_focal_tversky_bwd"][1]) == 17


def test_workspace_query():
    L = _lib.lib()
    for bad in [(0, 3, 100), (2, 0, 100), (2, 3, 0), (-1, 3, 100), (2, 3, -5)]:
        assert L.m355_focal_tversky_workspace(*bad) == 0, bad
    one = L.m355_focal_tversky_workspace(2, 3, 1)
    assert one >= 2 * 3 * 4 * 8
    assert L.m355_focal_tversky_workspace(2, 3, CHUNK) == one                # one chunk up to CHUNK voxels ...
    two = L.m355_focal_tversky_workspace(2, 3, CHUNK + 1)                    # ... two from CHUNK + 1 on
    assert two - one == 2 * 3 * 4 * 8
    assert L.m355_focal_tversky_workspace(2, 3, 17391) - one == 4 * 2 * 3 * 4 * 8      # ceil(17391 / 4096) = 5
    assert L.m355_focal_tversky_workspace(1, 4, 128 ** 3) - one == (4 * 512 - 6) * 4 * 8


# (tversky_weight, alpha, beta, tversky_power, focal_gamma) the entry points refuse, and the message
BAD_PARAMS = [((0.5, -1.0, 0.5, 1.0, 0.0), b"alpha and beta"), ((0.5, 0.5, -0.5, 1.0, 0.0), b"alpha and beta"),
              ((0.5, float("nan"), 0.5, 1.0, 0.0), b"alpha and beta"), ((0.5, 0.5, float("inf"), 1.0, 0.0), b"alpha and beta"),
              ((0.5, 0.5, 0.5, 0.0, 0.0), b"tversky_power"), ((0.5, 0.5, 0.5, -1.0, 0.0), b"tversky_power"),
              ((0.5, 0.5, 0.5, float("nan"), 0.0), b"tversky_power"),
              ((0.5, 0.5, 0.5, 1.0, 0.5), b"focal_gamma"), ((0.5, 0.5, 0.5, 1.0, -1.0), b"focal_gamma"),
              ((0.5, 0.5, 0.5, 1.0, 0.999), b"focal_gamma"), ((0.5, 0.5, 0.5, 1.0, float("nan")), b"focal_gamma"),
              ((0.5, 0.5, 0.5, 1.0, float("inf")), b"focal_gamma")]
GOOD = (0.5, 0.3, 0.7, 0.75, 2.0)


@pytest.mark.parametrize("from_logits", [0, 1])
def test_forward_argument_checks_reject_before_any_launch(from_logits):
    L = _lib.lib()
    a = P(64)
    ws = L.m355_focal_tversky_workspace(2, 3, 100)

    def fwd(x=a, t=a, N=2, C=3, S=100, par=GOOD, out3=a, sums=a, w=a, nbytes=ws):
        return L.m355_focal_tversky_fwd(x, t, N, C, S, *par, None, None, from_logits, out3, sums, w, nbytes, None)
    for kw in (dict(x=None), dict(t=None), dict(out3=None), dict(sums=None), dict(w=None)):
        assert fwd(**kw) == -1 and b"focal_tversky_fwd: null pointer" in L.m355_last_error(), kw
    for kw in (dict(N=0), dict(C=0), dict(S=0), dict(N=-2), dict(S=-1)):
        assert fwd(**kw) == -1 and b"focal_tversky_fwd: non-positive size" in L.m355_last_error(), kw
    for par, msg in BAD_PARAMS:
        assert fwd(par=par) == -1 and b"focal_tversky_fwd: " + msg in L.m355_last_error(), par
    assert fwd(N=256, C=256, nbytes=1 << 40) == -2 and b"focal_tversky_fwd: N*C > 65535" in L.m355_last_error()
    assert fwd(nbytes=ws - 1) == -4 and b"focal_tversky_fwd: workspace too small" in L.m355_last_error()
    assert fwd(nbytes=0) == -4
    assert fwd(S=4097, nbytes=ws) == -4     # two chunks need more than one chunk's workspace


@pytest.mark.parametrize("from_logits", [0, 1])
def test_backward_argument_checks_reject_before_any_launch(from_logits):
    L = _lib.lib()
    a = P(64)

    def bwd(x=a, t=a, sums=a, dloss=a, N=2, C=3, S=100, par=GOOD, dx=a):
        return L.m355_focal_tversky_bwd(x, t, sums, dloss, N, C, S, *par, None, None, from_logits, dx, None)
    for kw in (dict(x=None), dict(t=None), dict(sums=None), dict(dloss=None), dict(dx=None)):
        assert bwd(**kw) == -1 and b"focal_tversky_bwd: null pointer" in L.m355_last_error(), kw
    for kw in (dict(N=0), dict(C=0), dict(S=0), dict(C=-1)):
        assert bwd(**kw) == -1 and b"focal_tversky_bwd: non-positive size" in L.m355_last_error(), kw
    for par, msg in BAD_PARAMS:
        assert bwd(par=par) == -1 and b"focal_tversky_bwd: " + msg in L.m355_last_error(), par
    assert bwd(N=65536, C=1) == -2 and b"focal_tversky_bwd: N*C > 65535" in L.m355_last_error()


def test_ops_wrapper_errors():
    """raised on the host before the device is looked at: the same without a GPU"""
    x = torch.zeros(2, 3, 4, 4, 4)
    with pytest.raises(_lib.M355Error, match=r"tversky_class_weights of shape \(2,\) for 3 channels"):
        ops.focal_tversky_loss(x, x, tversky_class_weights=torch.ones(2))
    with pytest.raises(_lib.M355Error, match=r"focal_class_weights of shape \(4,\) for 3 channels"):
        ops.focal_tversky_loss(x, x, focal_class_weights=torch.ones(4))
    with pytest.raises(_lib.M355Error, match=r"prediction \(2, 3, 4, 4, 4\) and target \(2, 3, 4, 4, 5\)"):
        ops.focal_tversky_loss(x, torch.zeros(2, 3, 4, 4, 5))
    with pytest.raises(_lib.M355Error, match="prediction: expected torch.float32, got torch.float16"):
        ops.focal_tversky_loss(x.half(), x)
    with pytest.raises(_lib.M355Error, match="target: expected torch.float32, got torch.bool"):
        ops.focal_tversky_loss(x, x.bool())
    with pytest.raises(_lib.M355Error, match="focal_class_weights: expected torch.float32, got torch.float64"):
        ops.focal_tversky_loss(x, x, focal_class_weights=torch.ones(3, dtype=torch.float64))
    with pytest.raises(_lib.M355Error, match="no CPU fallback"):      # valid arguments, host tensors: no quiet fall-back
        ops.focal_tversky_loss(x, x, from_logits=True)


# ---------------------------------------------------------------------------------------- the reference against itself
def _random_case(shape=(2, 3, 4, 5, 6), seed=3):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(shape, generator=g, dtype=torch.float64) * 2
    return z, torch.softmax(z, dim=1), torch.rand(shape, generator=g, dtype=torch.float64)


def test_reference_defaults_are_the_hybrid_loss_without_square_dice():
    _, p, t = _random_case()
    for dw, cw in ((0.5, None), (0.3, [1.0, 2.0, 3.0])):
        mine = F.focal_tversky(p, t, tversky_weight=dw, focal_class_weights=cw)
        ref = R.hybrid_logistic_dice_loss(p.reshape(2, 3, 4, 5, 6), t.reshape(2, 3, 4, 5, 6), dw,
                                          cw, square_dice=False)
        for a, b in (("loss", "loss"), ("tversky_loss", "dice_loss"), ("focal_loss", "logistic_loss")):
            assert abs(mine[a].item() - ref[b].item()) <= 1e-12, (a, mine[a].item(), ref[b].item())


def test_reference_reproduces_the_recorded_fixture():
    """hybrid_loss.npz case1 (dice_weight 0.3, no square_dice, class weights 1, 2, 3), recorded from the reference"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "hybrid_loss.npz"))
    assert g["case1.cfg"].tolist() == [0.3, 0.0, 1.0, 2.0, 3.0]
    p, t = torch.from_numpy(g["p"]), torch.from_numpy(g["t"])
    out3, _, dp = F.expected(p, t, 1.0, tversky_weight=0.3, focal_class_weights=[1.0, 2.0, 3.0])
    assert (out3 - torch.from_numpy(g["case1.out"]).double()).abs().max().item() <= 1e-6
    rec = torch.from_numpy(g["case1.dp"]).double()
    assert (dp - rec).abs().max().item() <= 1e-6 * rec.abs().max().item()
    assert torch.allclose(F.closed_form_bwd(p.double(), t.double(), 1.0, tversky_weight=0.3,
                                            focal_class_weights=[1.0, 2.0, 3.0]), dp, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("from_logits", [False, True], ids=["prob", "logits"])
@pytest.mark.parametrize("cfg", [dict(tversky_weight=0.3, alpha=0.3, beta=0.7, tversky_power=0.75, focal_gamma=2.0,
                                      focal_class_weights=[1.0, 2.0, 3.0], tversky_class_weights=[0.0, 1.0, 1.0]),
                                 dict(alpha=0.7, beta=0.3, tversky_power=1.5, focal_gamma=2.5,
                                      focal_class_weights=[1.0, 100.0, 1.0]),
                                 dict(focal_gamma=1.0), dict()], ids=["cfg1", "cfg2", "cfg3", "cfg0"])
def test_closed_form_backward_is_autograds(cfg, from_logits):
    """the backward the kernels implement, in fp64, against autograd through the forward formulas; soft targets"""
    z, p, t = _random_case()
    x = z if from_logits else p
    _, _, dx = F.expected(x, t, 0.7, from_logits=from_logits, **cfg)
    closed = F.closed_form_bwd(x, t, 0.7, from_logits=from_logits, **cfg)
    err = (closed - dx).abs().max().item()
    assert err <= 1e-13 * max(dx.abs().max().item(), 1e-3), err
