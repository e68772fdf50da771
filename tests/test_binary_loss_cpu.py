"""HybridBinaryLogisticDiceLoss: what can be checked without a GPU -- the criterion's interface and pickled state, the
bindings, the argument checks of the three entry points (no launches) and of the ops wrapper, the workspace query."""
import ctypes
import inspect
import os
import pickle

import pytest
import torch

from conftest import ROOT
from segmentation_pipeline_amd import _lib, criterions, ops
from segmentation_pipeline_amd.criterions import HybridBinaryLogisticDiceLoss

SYMBOLS = ["m355_binary_loss_workspace", "m355_binary_loss_fwd", "m355_binary_loss_bwd"]
P = ctypes.c_void_p
CHUNK = 16384   # elements of a row per partial sum


def test_constructor_defaults_and_export():
    assert criterions.HybridBinaryLogisticDiceLoss is HybridBinaryLogisticDiceLoss
    sig = inspect.signature(HybridBinaryLogisticDiceLoss.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ("dice_weight", 0.5), ("logistic_class_weights", None), ("pos_weight", None), ("square_dice", True),
        ("from_logits", False)]
    crit = HybridBinaryLogisticDiceLoss()
    assert (crit.dice_weight, crit.logistic_class_weights, crit.pos_weight, crit.square_dice, crit.from_logits) == \
        (0.5, None, None, True, False)
    assert isinstance(crit, torch.nn.Module)


def test_forward_returns_the_three_keys(monkeypatch):
    """the dict of HybridLogisticDiceLoss, the arguments handed to ops.binary_logistic_dice_loss in its order"""
    seen = {}

    def fake(x, t, dice_weight, class_weights, pos_weight, square_dice, from_logits):
        seen.update(dice_weight=dice_weight, class_weights=class_weights, pos_weight=pos_weight, square_dice=square_dice,
                    from_logits=from_logits)
        return torch.tensor(1.0), torch.tensor(2.0), torch.tensor(3.0)
    monkeypatch.setattr(ops, "binary_logistic_dice_loss", fake)
    crit = HybridBinaryLogisticDiceLoss(0.3, [1, 2, 3], (1, 5, 0.5), False, True)
    out = crit(torch.zeros(2, 3, 4, 4, 4), torch.zeros(2, 3, 4, 4, 4))
    assert list(out) == ['loss', 'dice_loss', 'logistic_loss']
    assert [v.item() for v in out.values()] == [1.0, 2.0, 3.0]
    assert seen["dice_weight"] == 0.3 and seen["square_dice"] is False and seen["from_logits"] is True
    assert seen["class_weights"].tolist() == [1.0, 2.0, 3.0] and seen["class_weights"].dtype == torch.float32
    assert seen["pos_weight"].tolist() == [1.0, 5.0, 0.5]
    first = seen["pos_weight"]
    crit(torch.zeros(2, 3, 4, 4, 4), torch.zeros(2, 3, 4, 4, 4))
    assert seen["pos_weight"] is first, "the weights are uploaded once per (values, device)"


def test_weight_length_is_checked_by_the_criterion():
    x = torch.zeros(1, 3, 2, 2, 2)
    with pytest.raises(_lib.M355Error, match="pos_weight of 2 values for 3 channels"):
        HybridBinaryLogisticDiceLoss(pos_weight=[1, 2])(x, x)
    with pytest.raises(_lib.M355Error, match="logistic_class_weights of shape"):
        HybridBinaryLogisticDiceLoss(logistic_class_weights=torch.ones(4))(x, x)


def test_pickled_state_holds_no_device_tensor(monkeypatch):
    monkeypatch.setattr(ops, "binary_logistic_dice_loss", lambda *a: (torch.tensor(0.0),) * 3)
    crit = HybridBinaryLogisticDiceLoss(logistic_class_weights=[1, 2], pos_weight=[3, 4])
    crit(torch.zeros(1, 2, 2, 2, 2), torch.zeros(1, 2, 2, 2, 2))
    assert set(crit._uploaded) == {"logistic_class_weights", "pos_weight"}
    state = crit.__getstate__()
    assert state["_uploaded"] == {}
    assert not any(torch.is_tensor(v) for v in state.values())
    back = pickle.loads(pickle.dumps(crit))
    assert back._uploaded == {} and back.pos_weight == [3, 4] and back.logistic_class_weights == [1, 2]
    assert (back.dice_weight, back.square_dice, back.from_logits) == (0.5, True, False)
    assert set(crit._uploaded) == {"logistic_class_weights", "pos_weight"}     # pickling leaves the live object alone


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "m355seg.h")).read()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert getattr(_lib.lib(), s) is not None
        assert f"{s}(" in header, s
    assert len(_lib.SIGNATURES["m355_binary_loss_fwd"][1]) == 15 and len(_lib.SIGNATURES["m355_binary_loss_bwd"][1]) == 14


def test_workspace_query():
    L = _lib.lib()
    for bad in [(0, 3, 100), (2, 0, 100), (2, 3, 0), (-1, 3, 100), (2, 3, -5)]:
        assert L.m355_binary_loss_workspace(*bad) == 0, bad
    one = L.m355_binary_loss_workspace(2, 3, 1)
    assert one >= 2 * 3 * 5 * 8
    assert L.m355_binary_loss_workspace(2, 3, CHUNK) == one                # one chunk up to CHUNK elements ...
    two = L.m355_binary_loss_workspace(2, 3, CHUNK + 1)                    # ... two from CHUNK + 1 on
    assert two - one == 2 * 3 * 5 * 8
    assert L.m355_binary_loss_workspace(2, 3, 17391) == two
    assert L.m355_binary_loss_workspace(1, 4, 128 ** 3) - one == (4 * 128 - 6) * 5 * 8


@pytest.mark.parametrize("from_logits", [0, 1])
def test_forward_argument_checks_reject_before_any_launch(from_logits):
    L = _lib.lib()
    a = P(64)
    ws = L.m355_binary_loss_workspace(2, 3, 100)

    def fwd(x=a, t=a, N=2, C=3, S=100, out3=a, sums=a, w=a, nbytes=ws):
        return L.m355_binary_loss_fwd(x, t, N, C, S, 0.5, None, None, 1, from_logits, out3, sums, w, nbytes, None)
    for kw in (dict(x=None), dict(t=None), dict(out3=None), dict(sums=None), dict(w=None)):
        assert fwd(**kw) == -1 and b"binary_loss_fwd: null pointer" in L.m355_last_error(), kw
    for kw in (dict(N=0), dict(C=0), dict(S=0), dict(N=-2), dict(S=-1)):
        assert fwd(**kw) == -1 and b"binary_loss_fwd: non-positive size" in L.m355_last_error(), kw
    assert fwd(N=256, C=256, nbytes=1 << 40) == -2 and b"binary_loss_fwd: N*C > 65535" in L.m355_last_error()
    assert fwd(nbytes=ws - 1) == -4 and b"binary_loss_fwd: workspace too small" in L.m355_last_error()
    assert fwd(nbytes=0) == -4


@pytest.mark.parametrize("from_logits", [0, 1])
def test_backward_argument_checks_reject_before_any_launch(from_logits):
    L = _lib.lib()
    a = P(64)

    def bwd(x=a, t=a, sums=a, dloss=a, N=2, C=3, S=100, dx=a):
        return L.m355_binary_loss_bwd(x, t, sums, dloss, N, C, S, 0.5, None, None, 1, from_logits, dx, None)
    for kw in (dict(x=None), dict(t=None), dict(sums=None), dict(dloss=None), dict(dx=None)):
        assert bwd(**kw) == -1 and b"binary_loss_bwd: null pointer" in L.m355_last_error(), kw
    for kw in (dict(N=0), dict(C=0), dict(S=0), dict(C=-1)):
        assert bwd(**kw) == -1 and b"binary_loss_bwd: non-positive size" in L.m355_last_error(), kw
    assert bwd(N=65536, C=1) == -2 and b"binary_loss_bwd: N*C > 65535" in L.m355_last_error()


def test_ops_wrapper_errors():
    """raised on the host before the device is looked at: the same without a GPU"""
    x = torch.zeros(2, 3, 4, 4, 4)
    with pytest.raises(_lib.M355Error, match=r"pos_weight of shape \(2,\) for 3 channels"):
        ops.binary_logistic_dice_loss(x, x, pos_weight=torch.ones(2))
    with pytest.raises(_lib.M355Error, match=r"class_weights of shape \(4,\) for 3 channels"):
        ops.binary_logistic_dice_loss(x, x, class_weights=torch.ones(4))
    with pytest.raises(_lib.M355Error, match=r"prediction \(2, 3, 4, 4, 4\) and target \(2, 3, 4, 4, 5\)"):
        ops.binary_logistic_dice_loss(x, torch.zeros(2, 3, 4, 4, 5))
    with pytest.raises(_lib.M355Error, match="prediction: expected torch.float32, got torch.float16"):
        ops.binary_logistic_dice_loss(x.half(), x)
    with pytest.raises(_lib.M355Error, match="target: expected torch.float32, got torch.bool"):
        ops.binary_logistic_dice_loss(x, x.bool())
    with pytest.raises(_lib.M355Error, match="pos_weight: expected torch.float32, got torch.float64"):
        ops.binary_logistic_dice_loss(x, x, pos_weight=torch.ones(3, dtype=torch.float64))
    with pytest.raises(_lib.M355Error, match="no CPU fallback"):      # valid arguments, host tensors: no quiet fall-back
        ops.binary_logistic_dice_loss(x, x)
