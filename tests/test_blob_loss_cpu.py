"""BlobLoss and the blob Dice entry points: what can be checked without a GPU -- the two references of tests/blob_loss_ref.py
against each other on the cases of the GPU test (the closed form the kernels implement is the literal definition), exports
and bindings, every host-side argument check of the entry points (they return before a launch; pointers are integers that
are never followed), the capacity bound behind the workspace queries, the criterion's constructor, default class weights
and pickled state, and the ops wrappers' argument errors."""
import ctypes
import inspect
import os
import pickle

import numpy as np
import pytest
import torch

import blob_loss_ref as BR
from conftest import ROOT
from segmentation_pipeline_amd import _lib, criterions, ops
from segmentation_pipeline_amd.criterions import BlobLoss, HybridLogisticDiceLoss

SYMBOLS = ["m355_blob_capacity", "m355_blob_label_workspace", "m355_blob_label", "m355_blob_dice_workspace",
           "m355_blob_dice_tables", "m355_blob_dice_fwd", "m355_blob_dice_bwd"]
P = ctypes.c_void_p
CASES = BR.cases()


def _on(flags):
    return (ctypes.c_uint8 * len(flags))(*flags)


def _up(v, to=256):
    return -(-v // to) * to


# -------------------------------------------------------------------------------------------- the references agree
@pytest.mark.parametrize("square", [False, True], ids=["plain", "square"])
@pytest.mark.parametrize("kind", BR.PREDICTIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_closed_form_is_the_literal_definition(name, kind, square):
    target, weights, planes, conn = CASES[name]
    p = BR.prediction(kind, target.shape).double()
    loss, grad, count = BR.literal_with_grad(p, target, weights, square, conn, planes)
    loss2, grad2 = BR.blob_dice_closed_form(p, target, weights, square, conn, planes)
    scale = grad.abs().max().item()
    dl, dg = abs(loss.item() - loss2.item()), (grad - grad2).abs().max().item()
    print(f"blob_loss refs {name} {kind} square={square}: components {count} loss {loss.item():.12f} |dloss| {dl:.2e} "
          f"|dgrad| {dg:.2e} of {scale:.2e}")
    assert dl <= 1e-12 * max(abs(loss.item()), 1e-300) or dl == 0.0
    assert dg <= 1e-12 * scale or dg == 0.0
    assert count == BR.stacked_labels(target, _flags(target, weights, planes), conn)[2]


def _flags(target, weights, planes):
    N, C = target.shape[:2]
    w = BR.default_weights(C) if weights is None else weights
    return [w[i % C] > 0 and (planes is None or bool(planes[i])) for i in range(N * C)]


def test_reference_conventions():
    t = torch.zeros(1, 2, 1, 1, 7)
    t[0, 1, 0, 0] = torch.tensor([1.0, 0.0, 0.7, 0.5, float("nan"), 0.50001, 1.0])     # components {0}, {2}, {5, 6}
    p = torch.tensor([0.5, 0.25, 1.0, 0.0, 0.125, 0.75, 0.5], dtype=torch.float64).reshape(1, 1, 1, 1, 7).repeat(1, 2, 1, 1, 1)
    lab, ranges, n = BR.stacked_labels(t, [0, 1])
    assert lab.reshape(-1).tolist() == [1, 0, 2, 0, 0, 3, 3] and ranges.tolist() == [[1, 3]] and n == 3
    B = 0.25 + 0.0 + 0.125
    want = sum(1 - 2 * s / (a + s + B + 1e-8) for s, a in ((0.5, 1), (1.0, 1), (1.25, 2))) / 3
    got, count = BR.blob_dice_literal(p, t, None, square_dice=False)
    assert count == 3 and abs(got.item() - want) <= 1e-15
    # the background is off by default, a single channel is on; weights average the planes that have a component
    assert BR.blob_dice_literal(p[:, 1:], t[:, 1:], None, False)[0].item() == got.item()
    both, count = BR.blob_dice_literal(p, t, (3.0, 1.0), False)
    assert count == 3 and abs(both.item() - got.item()) <= 1e-15        # channel 0 has no member: it does not count
    zero, count = BR.blob_dice_literal(p, torch.zeros_like(t), (1.0, 1.0), True)
    assert count == 0 and zero.item() == 0.0


# ------------------------------------------------------------------------------------------------ exports, bindings
def test_exports_and_signatures():
    assert criterions.BlobLoss is BlobLoss
    sig = inspect.signature(BlobLoss.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[2:]] == [
        ("blob_weight", 1.0), ("global_weight", 2.0), ("blob_class_weights", None), ("square_dice", True), ("connectivity", 3)]
    assert [(k, v.default) for k, v in inspect.signature(ops.blob_labels).parameters.items()][1:] == [
        ("planes", None), ("connectivity", 3)]
    assert [(k, v.default) for k, v in inspect.signature(ops.blob_dice_loss).parameters.items()][2:5] == [
        ("class_weights", None), ("square_dice", True), ("connectivity", 3)]
    assert [k for k in inspect.signature(BlobLoss.set_weights).parameters] == ["self", "global_", "blob"]


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "m355seg.h")).read()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert getattr(_lib.lib(), s) is not None
        assert f"{s}(" in header, s
    assert len(_lib.SIGNATURES["m355_blob_label"][1]) == 13
    assert len(_lib.SIGNATURES["m355_blob_dice_fwd"][1]) == 20 and len(_lib.SIGNATURES["m355_blob_dice_bwd"][1]) == 14
    build = open(os.path.join(ROOT, "segmentation-pipeline_amd", "build.py")).read()
    assert '"blob_loss.hip"' in build


# ------------------------------------------------------------------------------------------- entry points, no launch
def test_capacity_bound_and_workspace_queries():
    L = _lib.lib()
    # 26 neighbours: one component per 2 x 2 x 2 cell of a plane (planes do not share cells: the bound is per plane);
    # 6 and 18 neighbours: every other voxel
    assert L.m355_blob_capacity(1, None, 1, 1, 1, 3) == 1 and L.m355_blob_capacity(1, None, 1, 1, 1, 1) == 1
    assert L.m355_blob_capacity(6, _on([1, 0, 1, 1, 1, 0]), 3, 5, 70, 3) == 4 * 2 * 3 * 35
    assert L.m355_blob_capacity(6, None, 3, 5, 70, 3) == 6 * 2 * 3 * 35
    assert L.m355_blob_capacity(1, None, 6, 6, 66, 1) == 1188 and L.m355_blob_capacity(1, None, 6, 6, 66, 2) == 1188
    assert L.m355_blob_capacity(1, None, 6, 6, 66, 3) == 3 * 3 * 33
    assert L.m355_blob_capacity(3, None, 3, 3, 3, 1) == 3 * 14
    assert L.m355_blob_capacity(4, _on([0, 1, 1, 1]), 128, 128, 128, 3) == 3 * 64 ** 3
    # the bound holds on the cases of the GPU test, and is reached by both checkerboards' densest relatives
    for name, (target, weights, planes, conn) in CASES.items():
        flags = _flags(target, weights, planes)
        n = BR.stacked_labels(target, flags, conn)[2]
        cap = L.m355_blob_capacity(len(flags), _on(flags), *target.shape[2:], conn)
        assert 0 <= n <= cap, name
    assert BR.stacked_labels(CASES["checkerboard_6conn"][0], None, 1)[2] == 1188
    cells = np.zeros((2, 1, 3, 5, 7), dtype=np.float32)
    cells[:, :, ::2, ::2, ::2] = 1.0                       # one voxel per cell, odd sizes, two planes
    assert BR.stacked_labels(cells, None, 3)[2] == 2 * 2 * 3 * 4 == L.m355_blob_capacity(2, None, 3, 5, 7, 3)
    # sizes: accumulators 24 bytes and tables 16 bytes per component of the capacity, plus the per-slot words
    for planes, on, size, conn in ((1, None, (1, 1, 1), 3), (6, [1, 0, 1, 1, 1, 0], (3, 5, 70), 3), (1, None, (6, 6, 66), 1),
                                   (4, [0, 1, 1, 1], (128, 128, 128), 3)):
        onb = None if on is None else _on(on)
        cap, p_on = L.m355_blob_capacity(planes, onb, *size, conn), planes if on is None else sum(on)
        assert L.m355_blob_dice_workspace(planes, onb, *size, conn) == 2 * _up(p_on * 8) + 24 * cap
        assert L.m355_blob_dice_tables(planes, onb, *size, conn) == 256 + _up(p_on * 8) + 16 * cap
        S = size[0] * size[1] * size[2]
        assert L.m355_blob_label_workspace(planes, onb, *size) == _up(p_on * S * 4) + _up(p_on * 4) + \
            L.m355_ccl_workspace(p_on * size[0], size[1], size[2])
    for query in (L.m355_blob_capacity, L.m355_blob_dice_workspace, L.m355_blob_dice_tables):
        for bad in ((0, None, 4, 4, 4, 3), (-1, None, 4, 4, 4, 3), (2, None, 0, 4, 4, 3), (2, None, 4, -1, 4, 3),
                    (2, None, 4, 4, 0, 3), (2, None, 4, 4, 4, 0), (2, None, 4, 4, 4, 4), (2, _on([0, 0]), 4, 4, 4, 3),
                    (1025, None, 4, 4, 4, 3), (2, None, 1024, 1024, 1024, 3), (1, None, 2048, 1024, 1024, 3)):
            assert query(*bad) == 0, bad
    assert L.m355_blob_label_workspace(0, None, 4, 4, 4) == 0 and L.m355_blob_label_workspace(2, None, 1024, 1024, 1024) == 0


def test_blob_label_argument_checks_reject_before_any_launch():
    L = _lib.lib()
    a = P(64)
    big = 1 << 40

    def call(target=a, planes=6, on=(1, 0, 1, 1, 1, 0), size=(3, 5, 70), conn=3, labels=a, ranges=a, count=a, ws=a, nbytes=big):
        return L.m355_blob_label(target, planes, None if on is None else _on(on), *size, conn, labels, ranges, count, ws,
                                 nbytes, None)
    for kw in (dict(target=None), dict(labels=None), dict(ranges=None), dict(count=None), dict(ws=None)):
        assert call(**kw) == -1 and b"blob_label: null pointer" in L.m355_last_error(), kw
    for planes in (0, -3):
        assert call(planes=planes, on=None) == -1 and b"blob_label: %d planes" % planes in L.m355_last_error()
    for size in ((0, 5, 70), (3, -1, 70), (3, 5, 0)):
        assert call(size=size) == -1 and b"blob_label: non-positive size" in L.m355_last_error(), size
    for conn in (0, 4, -1):
        assert call(conn=conn) == -1 and b"blob_label: connectivity %d not in" % conn in L.m355_last_error()
    assert call(on=(0,) * 6) == -1 and b"blob_label: no plane is on" in L.m355_last_error()
    assert call(planes=1025, on=None) == -2 and b"blob_label: 1025 planes (at most 1024)" in L.m355_last_error()
    assert call(planes=2, on=None, size=(1024, 1024, 1024)) == -1 and b"2^31 voxels or more" in L.m355_last_error()
    assert call(planes=2, on=(1, 0), size=(1024, 1024, 1024), nbytes=0) == -4     # (one plane of 2^30 voxels is accepted)
    need = L.m355_blob_label_workspace(6, _on((1, 0, 1, 1, 1, 0)), 3, 5, 70)
    assert call(nbytes=need - 1) == -4 and b"blob_label: workspace" in L.m355_last_error()
    assert call(nbytes=0) == -4
    assert call(on=None, nbytes=need) == -4      # six planes on need more


def test_blob_dice_argument_checks_reject_before_any_launch():
    L = _lib.lib()
    a = P(64)
    on6 = (1, 0, 1, 1, 1, 0)
    ws = L.m355_blob_dice_workspace(6, _on(on6), 3, 5, 70, 3)
    tb = L.m355_blob_dice_tables(6, _on(on6), 3, 5, 70, 3)

    def fwd(p=a, labels=a, ranges=a, count=a, w=None, N=2, C=3, on=on6, size=(3, 5, 70), conn=3, sq=1, loss=a, total=a,
            tables=a, tbytes=tb, work=a, nbytes=ws):
        return L.m355_blob_dice_fwd(p, labels, ranges, count, w, N, C, None if on is None else _on(on), *size, conn, sq,
                                    loss, total, tables, tbytes, work, nbytes, None)
    for kw in (dict(p=None), dict(labels=None), dict(ranges=None), dict(count=None), dict(loss=None), dict(total=None),
               dict(tables=None), dict(work=None)):
        assert fwd(**kw) == -1 and b"blob_dice_fwd: null pointer" in L.m355_last_error(), kw
    for kw in (dict(N=0, on=None), dict(C=0, on=None), dict(N=-2, on=None)):
        assert fwd(**kw) == -1 and b"blob_dice_fwd: non-positive size" in L.m355_last_error(), kw
    for size in ((0, 5, 70), (3, 5, -2)):
        assert fwd(size=size) == -1 and b"blob_dice_fwd: non-positive size" in L.m355_last_error(), size
    for conn in (0, 4):
        assert fwd(conn=conn) == -1 and b"blob_dice_fwd: connectivity" in L.m355_last_error()
    assert fwd(on=(0,) * 6) == -1 and b"no plane is on" in L.m355_last_error()
    assert fwd(N=41, C=25, on=None) == -2 and b"blob_dice_fwd: N * C = 1025 planes" in L.m355_last_error()
    assert fwd(N=1, C=2, on=None, size=(1024, 1024, 1024)) == -1 and b"2^31 voxels or more" in L.m355_last_error()
    assert fwd(nbytes=ws - 1) == -4 and b"blob_dice_fwd: workspace" in L.m355_last_error()
    assert fwd(tbytes=tb - 1) == -4 and b"blob_dice_fwd: tables" in L.m355_last_error()
    assert fwd(conn=1) == -4                      # 6 neighbours: more components fit a plane, the buffers are larger
    assert fwd(on=None) == -4

    def bwd(p=a, labels=a, tables=a, dloss=a, N=2, C=3, on=on6, size=(3, 5, 70), conn=3, sq=1, dp=a):
        return L.m355_blob_dice_bwd(p, labels, tables, dloss, N, C, None if on is None else _on(on), *size, conn, sq, dp, None)
    for kw in (dict(p=None), dict(labels=None), dict(tables=None), dict(dloss=None), dict(dp=None)):
        assert bwd(**kw) == -1 and b"blob_dice_bwd: null pointer" in L.m355_last_error(), kw
    for kw in (dict(N=0, on=None), dict(C=-1, on=None)):
        assert bwd(**kw) == -1 and b"blob_dice_bwd: non-positive size" in L.m355_last_error(), kw
    assert bwd(size=(3, 0, 70)) == -1 and bwd(conn=5) == -1 and bwd(on=(0,) * 6) == -1
    assert bwd(N=1025, C=1, on=None) == -2 and b"blob_dice_bwd: N * C = 1025 planes" in L.m355_last_error()
    assert bwd(N=1, C=2, on=None, size=(1024, 1024, 1024)) == -1 and b"2^31 voxels or more" in L.m355_last_error()


# ------------------------------------------------------------------------------------------------------ ops wrappers
def test_ops_wrapper_errors_come_before_the_device_check():
    x = torch.zeros(2, 3, 4, 4, 4)
    with pytest.raises(_lib.M355Error, match="blob_labels: target: element type torch.float16"):
        ops.blob_labels(x.half())
    with pytest.raises(_lib.M355Error, match=r"expected \[N, C, D, H, W\], got shape \(3, 4, 4, 4\)"):
        ops.blob_labels(x[0])
    with pytest.raises(_lib.M355Error, match="connectivity 4 not in"):
        ops.blob_labels(x, connectivity=4)
    with pytest.raises(_lib.M355Error, match="5 plane flags for N . C = 6 planes"):
        ops.blob_labels(x, planes=[1, 0, 1, 1, 0])
    with pytest.raises(_lib.M355Error, match="no plane is on"):
        ops.blob_labels(x, planes=[0] * 6)
    with pytest.raises(_lib.M355Error, match="expected a contiguous tensor"):
        ops.blob_labels(x.permute(0, 1, 4, 3, 2))
    with pytest.raises(_lib.M355Error, match="blob_labels: target: expected a device tensor"):     # no quiet fall-back
        ops.blob_labels(x)
    with pytest.raises(_lib.M355Error, match="class_weights of 2 values for 3 channels"):
        ops.blob_dice_loss(x, x, [1.0, 2.0])
    with pytest.raises(_lib.M355Error, match="positive sum"):
        ops.blob_dice_loss(x, x, [0.0, 0.0, 0.0])
    with pytest.raises(_lib.M355Error, match="expected finite values >= 0"):
        ops.blob_dice_loss(x, x, [1.0, -1.0, 0.0])
    with pytest.raises(_lib.M355Error, match="connectivity 0 not in"):
        ops.blob_dice_loss(x, x, connectivity=0)
    with pytest.raises(_lib.M355Error, match="planes goes with a device tensor"):
        ops.blob_dice_loss(x, x, [1.0, 1.0, 1.0], planes=[1] * 6)
    with pytest.raises(_lib.M355Error, match=r"class_weights of shape \(2,\) for 3 channels"):
        ops.blob_dice_loss(x, x, torch.ones(2))
    with pytest.raises(_lib.M355Error, match=r"prediction \(2, 3, 4, 4, 5\) and target \(2, 3, 4, 4, 4\)"):
        ops.blob_dice_loss(torch.zeros(2, 3, 4, 4, 5), x, torch.ones(3))
    with pytest.raises(_lib.M355Error, match="prediction: expected torch.float32, got torch.float16"):
        ops.blob_dice_loss(x.half(), x, torch.ones(3))
    with pytest.raises(_lib.M355Error, match="no CPU fallback"):
        ops.blob_dice_loss(x, x, torch.ones(3))
    with pytest.raises(_lib.M355Error, match="no CPU fallback"):
        ops.blob_dice_loss(x, x)


# --------------------------------------------------------------------------------------------------------- criterion
@pytest.mark.parametrize("kw, match", [
    (dict(blob_weight=float("nan")), "blob_weight"), (dict(global_weight=float("inf")), "global_weight"),
    (dict(blob_class_weights=[]), "blob_class_weights"), (dict(blob_class_weights=[1.0, -0.5]), "finite values >= 0"),
    (dict(blob_class_weights=[1.0, float("nan")]), "finite values >= 0"),
    (dict(blob_class_weights=[float("inf"), 1.0]), "finite values >= 0"),
    (dict(blob_class_weights=[0.0, 0.0]), "positive weight"), (dict(blob_class_weights=torch.ones(2, 2)), "expected .C."),
    (dict(connectivity=0), "connectivity"), (dict(connectivity=4), "connectivity"), (dict(connectivity=2.5), "connectivity")],
    ids=lambda v: v if isinstance(v, str) else "_".join(v))
def test_invalid_parameters_raise_at_construction(kw, match):
    with pytest.raises(ValueError, match=match):
        BlobLoss(HybridLogisticDiceLoss(), **kw)


def _fake_ops(monkeypatch, seen):
    def fake_blob(prediction, target, class_weights=None, square_dice=True, connectivity=3, planes=None):
        seen.update(class_weights=class_weights, square_dice=square_dice, connectivity=connectivity, planes=list(planes))
        return torch.tensor(3.0), torch.tensor(5, dtype=torch.int32)
    monkeypatch.setattr(ops, "blob_dice_loss", fake_blob)
    monkeypatch.setattr(ops, "hybrid_logistic_dice_loss", lambda *a: (torch.tensor(1.0), torch.tensor(0.25), torch.tensor(0.75)))


def test_forward_dict_default_weights_and_in_place_mixing_weights(monkeypatch):
    seen = {}
    _fake_ops(monkeypatch, seen)
    crit = BlobLoss(HybridLogisticDiceLoss(), blob_weight=0.5, square_dice=False, connectivity=1)
    assert isinstance(crit, torch.nn.Module) and set(dict(crit.named_buffers())) == {"global_weight", "blob_weight"}
    x = torch.zeros(2, 3, 2, 2, 2)
    out = crit(x, x)
    assert list(out) == ['loss', 'dice_loss', 'logistic_loss', 'blob_loss', 'global_loss', 'blob_count', 'blob_weight',
                         'global_weight']
    assert all(torch.is_tensor(v) for v in out.values())
    assert [v.item() for v in out.values()] == [2.0 * 1.0 + 0.5 * 3.0, 0.25, 0.75, 3.0, 1.0, 5, 0.5, 2.0]
    assert seen["class_weights"].tolist() == [0.0, 1.0, 1.0] and seen["class_weights"].dtype == torch.float32
    assert seen["planes"] == [False, True, True] * 2 and seen["square_dice"] is False and seen["connectivity"] == 1
    first = seen["class_weights"]
    ptrs = crit.global_weight.data_ptr(), crit.blob_weight.data_ptr()
    crit.set_weights(global_=0.25)
    crit.set_weights(blob=2.0)
    crit.set_weights()
    assert (crit.global_weight.data_ptr(), crit.blob_weight.data_ptr()) == ptrs
    out2 = crit(x, x)
    assert out2['loss'].item() == 0.25 * 1.0 + 2.0 * 3.0 and out['blob_weight'].item() == 0.5
    assert seen["class_weights"] is first, "the weights are uploaded once per (values, device)"
    with pytest.raises(ValueError, match="finite"):
        crit.set_weights(blob=float("nan"))
    one = torch.zeros(1, 1, 2, 2, 2)
    paper = BlobLoss(HybridLogisticDiceLoss())
    d = paper(one, one)
    assert seen["class_weights"].tolist() == [1.0] and seen["planes"] == [True]       # a single channel keeps its weight
    assert seen["square_dice"] is True and seen["connectivity"] == 3
    assert (d['global_weight'].item(), d['blob_weight'].item(), d['loss'].item()) == (2.0, 1.0, 5.0)   # alpha = 2, beta = 1
    BlobLoss(HybridLogisticDiceLoss(), blob_class_weights=torch.tensor([2.0, 0.0, 0.5]))(x, x)
    assert seen["class_weights"].tolist() == [2.0, 0.0, 0.5] and seen["planes"] == [True, False, True] * 2


def test_shape_and_length_errors_of_the_criterion(monkeypatch):
    _fake_ops(monkeypatch, {})
    x = torch.zeros(1, 3, 2, 2, 2)
    with pytest.raises(_lib.M355Error, match="blob_class_weights of 2 values for 3 channels"):
        BlobLoss(HybridLogisticDiceLoss(), blob_class_weights=[1, 2])(x, x)
    with pytest.raises(_lib.M355Error, match="DeepSupervisionLoss.BlobLoss"):
        BlobLoss(HybridLogisticDiceLoss())((x, x), x)
    with pytest.raises(_lib.M355Error, match=r"expected one shape \[N, C, D, H, W\]"):
        BlobLoss(HybridLogisticDiceLoss())(x, torch.zeros(1, 3, 2, 2, 3))


def test_pickled_state_holds_no_device_tensor(monkeypatch):
    _fake_ops(monkeypatch, {})
    crit = BlobLoss(HybridLogisticDiceLoss(logistic_class_weights=[1, 2]), 0.25, 0.75, [0, 3], False, 2)
    x = torch.zeros(1, 2, 2, 2, 2)
    crit(x, x)
    assert set(crit._uploaded) == {"blob_class_weights"}
    state = crit.__getstate__()
    assert state["_uploaded"] == {}
    assert all(v.device.type == "cpu" for v in state["_buffers"].values())
    assert not any(torch.is_tensor(v) for k, v in state.items() if not k.startswith("_"))
    back = pickle.loads(pickle.dumps(crit))
    assert back._uploaded == {} and back.blob_class_weights == (0.0, 3.0)
    assert (back.square_dice, back.connectivity) == (False, 2)
    assert (back.blob_weight.item(), back.global_weight.item()) == (0.25, 0.75)
    assert back.criterion.logistic_class_weights == [1, 2] and back.criterion._uploaded == {}
    assert set(crit._uploaded) == {"blob_class_weights"}        # pickling leaves the live object alone
