"""Calibration and uncertainty: what can be checked without a GPU -- the torch restatements (calibration_ref,
uncertainty_ref) against hand-made truths, the bindings and host-side argument checks of the new entry points (no
launches), CalibrationEvaluator's layout on a stubbed ops.eval_calibration, and the ensembles' CPU-tensor path."""
import ctypes
import math

import pytest
import torch
from torch import nn

import calibration_ref as cref
import uncertainty_ref as uref
from segmentation_pipeline_amd import _lib, evaluators, ops
from segmentation_pipeline_amd.evaluators import CalibrationEvaluator
from segmentation_pipeline_amd.models import ensemble as E

P = ctypes.c_void_p


# ------------------------------------------------------------------------------------------ the reference itself
def test_reference_on_a_hand_made_table():
    """8 voxels, 2 channels, all (0.75, 0.25), half of them right: everything in bin 7 of 10, ECE = 0.25 exactly"""
    scores = torch.tensor([[0.75] * 8, [0.25] * 8])
    target = torch.tensor([0, 1] * 4)
    r = cref.reference(scores, target, 10, 'categorical')
    assert r['top'][7] == [8, 4, 8 * 3 * 2 ** 30] and all(row == [0, 0, 0] for k, row in enumerate(r['top']) if k != 7)
    ece, mce, conf, acc = cref.table_stats(r['top'])
    assert (ece, mce, conf, acc) == (0.25, 0.25, 0.75, 0.5)
    assert r['classwise'][0][7] == [8, 4, 8 * 3 * 2 ** 30] and r['classwise'][1][2] == [8, 4, 8 * 2 ** 30]
    assert r['invalid'] == 0 and r['terms'] == (16, 8)
    # Brier: right voxels 2 * 0.25^2, wrong ones 2 * 0.75^2; NLL: -log of 0.75 or 0.25 through the 1e-8 shift
    assert r['brier'] == 4 * 2 * 0.0625 + 4 * 2 * 0.5625
    want = -4 * math.log((0.75 + 1e-8) / (1 + 1e-8)) - 4 * math.log((0.25 + 1e-8) / (1 + 1e-8))
    assert abs(r['nll'] - want) <= 1e-15 * want
    # the same through a one-hot target, and the evaluator's expression on the integers
    onehot = nn.functional.one_hot(target, 2).T.contiguous().float()
    assert cref.reference(scores, onehot, 10, 'categorical') == r
    stats, per_bin = evaluators.calibration_stats(r['top'])
    assert stats == {'ece': 0.25, 'mce': 0.25, 'confidence': 0.75, 'accuracy': 0.5}
    assert per_bin[7] == (8, 0.5, 0.75) and per_bin[0][0] == 0 and math.isnan(per_bin[0][1])


@pytest.mark.parametrize("B", [10, 15])
def test_a_confidence_on_a_bin_edge(B):
    q = torch.tensor([k / B for k in range(B)] + [1.0], dtype=torch.float32)
    assert cref.bin_index(q, B).tolist() == list(range(B)) + [B - 1]
    assert cref.bin_index(torch.tensor([0.0, 1.0]), 1).tolist() == [0, 0]


def test_invalid_values_enter_nothing():
    scores = torch.tensor([[0.6, float("nan"), 0.7, -0.25, 0.5, 1.5],
                           [0.4, 0.5, 0.3, 0.5, 0.5, 0.25]])
    target = torch.tensor([0, 0, 7, 1, 1, 0])      # voxel 2: an index out of range
    r = cref.reference(scores, target, 4, 'categorical')
    assert r['invalid'] == 4 and r['valid'] == 2 and r['terms'] == (4, 2)
    assert sum(row[0] for row in r['top']) == 2 and all(sum(row[0] for row in t) == 2 for t in r['classwise'])
    assert r['top'][2] == [2, 1, round(0.6000000238418579 * 2 ** 32) + 2 ** 31]     # float32(0.6) and 0.5: first maximum
    b = cref.reference(scores, target, 4, 'binary')
    assert b['invalid'] == [4, 1] and b['valid'] == 2 + 5        # per channel: NaN, index, negative, above 1 | index
    assert [sum(row[0] for row in t) for t in b['classwise']] == [2, 5]
    assert cref.table_stats([[0, 0, 0]] * 4) != cref.table_stats([[0, 0, 0]] * 4)      # empty: NaN


def test_entropy_reference():
    p = torch.tensor([[[0.5], [0.5]], [[1.0], [0.0]], [[float("nan")], [0.5]]]).reshape(3, 2, 1, 1, 1)
    h = uref.entropy(p)
    assert h.shape == (3, 1, 1, 1, 1) and abs(h[0].item() - math.log(2)) < 1e-15 and h[1].item() == 0 and h[2].isnan().all()
    hb = uref.entropy(p, 'binary')
    assert hb.shape == p.shape and hb[1].abs().max() == 0 and abs(hb[0, 0].item() - math.log(2)) < 1e-15
    assert abs(uref.tol_h(4) - 2.0 ** -23 * (4 + 3 * math.log(4))) < 1e-20 and uref.tol_h(1) == 2.0 ** -23


# ------------------------------------------------------------------------------------------ bindings, no launches
def test_symbols_and_descriptor():
    for name in ("m355_eval_calibration", "m355_eval_calibration_workspace", "m355_predictive_entropy",
                 "m355_ensemble_entropy_accumulate", "m355_ensemble_uncertainty_finalize"):
        assert name in _lib.SIGNATURES and getattr(_lib.lib(), name) is not None
    D = _lib.EvalCalibrationDesc
    assert [f[0] for f in D._fields_] == ["scores", "target", "S", "target_dtype"]
    assert (D.scores.offset, D.target.offset, D.S.offset, D.target_dtype.offset) == (0, 8, 16, 24) and ctypes.sizeof(D) == 32
    assert _lib.CAL_MAX_BINS == 32 and _lib.lib().m355_version() == 3
    assert _lib.lib().m355_eval_calibration_workspace(0) == 0 and _lib.lib().m355_eval_calibration_workspace(3) >= 3 * 16
    assert "CalibrationEvaluator" in evaluators.__all__


def _cal(n=1, dev=P(64), sd=_lib.EV_F32, tk=_lib.EV_TARGET_ONEHOT, C=2, bins=15, kind=0, out=P(64), ws=P(64), wsb=1 << 30,
         scores=64, target=64, S=8, tdt=_lib.EV_BOOL):
    L = _lib.lib()
    descs = (_lib.EvalCalibrationDesc * max(n, 1))()
    for d in descs:
        d.scores, d.target, d.S, d.target_dtype = scores, target, S, tdt
    return L.m355_eval_calibration(descs, n, dev, sd, tk, C, bins, kind, out, out, out, out, out, ws, wsb, None), L.m355_last_error()


def test_calibration_argument_checks_reject_before_any_launch():
    for kw, rc, msg in ((dict(C=0), -2, b"0 channels (1 .. 64)"), (dict(C=65), -2, b"65 channels"),
                        (dict(bins=0), -2, b"0 bins (1 .. 32)"), (dict(bins=33), -2, b"33 bins"),
                        (dict(kind=2), -1, b"kind 2"), (dict(n=0), -1, b"0 subjects"), (dict(dev=None), -1, b"null pointer"),
                        (dict(out=None), -1, b"null pointer"), (dict(ws=None), -1, b"null pointer"),
                        (dict(wsb=8), -4, b"workspace too small"), (dict(sd=_lib.EV_I32), -1, b"score type"),
                        (dict(tk=0), -1, b"target kind 0"), (dict(scores=None), -1, b"null scores"),
                        (dict(target=None), -1, b"null target"), (dict(S=0), -1, b"0 voxels"),
                        (dict(tdt=9), -1, b"target element type 9"),
                        (dict(tk=_lib.EV_TARGET_MAP, tdt=_lib.EV_F32), -1, b"index map of element type 6")):
        got, text = _cal(**kw)
        assert got == rc and b"eval_calibration" in text and msg in text, (kw, got, text)


def test_uncertainty_argument_checks_reject_before_any_launch():
    L = _lib.lib()
    i3 = (ctypes.c_int32 * 3)
    assert L.m355_predictive_entropy(P(64), _lib.EV_I32, P(64), None, 1, 2, 8, 0, None) == -1
    assert b"predictive_entropy: element type 4" in L.m355_last_error()
    assert L.m355_predictive_entropy(None, _lib.EV_F32, P(64), None, 1, 2, 8, 0, None) == -1
    assert L.m355_predictive_entropy(P(64), _lib.EV_F32, P(64), None, 1, 2, 8, 2, None) == -1
    assert b"kind 2" in L.m355_last_error()
    assert L.m355_predictive_entropy(P(64), _lib.EV_F32, P(64), None, 1, 0, 8, 0, None) == -1
    assert L.m355_ensemble_entropy_accumulate(P(64), P(64), 1, 2, i3(2, 2, 2), i3(0, 0, 2), 0, 0, 1, None) == -1
    assert b"not a permutation" in L.m355_last_error()
    assert L.m355_ensemble_entropy_accumulate(P(64), None, 1, 2, i3(2, 2, 2), i3(0, 1, 2), 0, 0, 1, None) == -1
    assert L.m355_ensemble_entropy_accumulate(P(64), P(64), 1, 2, i3(2, 2, 2), i3(0, 1, 2), 8, 0, 1, None) == -1
    assert L.m355_ensemble_uncertainty_finalize(P(64), P(64), P(64), P(64), P(64), P(64), 1, 2, 8, 0, 0, None) == -1
    assert b"0 members" in L.m355_last_error()
    assert L.m355_ensemble_uncertainty_finalize(P(64), P(64), P(64), None, P(64), P(64), 1, 2, 8, 3, 0, None) == -1


def test_ops_wrapper_errors():
    s = torch.zeros(2, 3, 3, 3)
    with pytest.raises(_lib.M355Error, match="one target per subject"):
        ops.eval_calibration([], [])
    with pytest.raises(_lib.M355Error, match="one target per subject"):
        ops.eval_calibration([s], [s, s])
    with pytest.raises(_lib.M355Error, match=r"33 bins \(1 .. 32\)"):
        ops.eval_calibration([s], [s], bins=33)
    with pytest.raises(_lib.M355Error, match="kind 'softmax'"):
        ops.eval_calibration([s], [s], kind='softmax')
    with pytest.raises(_lib.M355Error, match=r"65 channels \(1 .. 64\)"):
        ops.eval_calibration([torch.zeros(65, 2, 2, 2)], [torch.zeros(65, 2, 2, 2)])
    with pytest.raises(_lib.M355Error, match="element type torch.int32"):
        ops.eval_calibration([s.int()], [s])
    with pytest.raises(_lib.M355Error, match="expected a device tensor"):
        ops.eval_calibration([s], [s])
    with pytest.raises(_lib.M355Error, match="kind 'soft'"):
        ops.predictive_entropy(s[None], kind='soft')
    with pytest.raises(_lib.M355Error, match="expected a device tensor"):
        ops.predictive_entropy(s[None])
    with pytest.raises(_lib.M355Error, match="element type torch.int64"):
        ops.predictive_entropy(s[None].long())


def test_packed_result_views():
    n, C, B = 2, 3, 4
    packed = torch.arange(n * (B * 3 * (1 + C) + C + 3), dtype=torch.int64)
    r = ops.CalibrationCounts.unpack(packed, n, C, B, 'binary')
    assert r.top.shape == (n, B, 3) and r.classwise.shape == (n, C, B, 3) and r.invalid.shape == (n, C)
    assert r.brier.shape == r.nll.shape == r.voxels.shape == (n,) and r.brier.dtype == torch.float64
    assert r.top[0, 0, 0] == 0 and r.classwise[0, 0, 0, 0] == n * B * 3 and r.voxels[-1] == packed[-1]
    assert ops.CalibrationCounts.unpack(packed, n, C, B, 'categorical').invalid.shape == (n,)


# ------------------------------------------------------------------------------------------ the evaluator
def test_evaluator_layout_on_stubbed_counts(monkeypatch):
    """two subjects, C = 2, 4 bins: the tables of hand-made integers come back as 'top' + channel rows, the reliability
    table as [subject, label, bin, stat]; a subject without a valid voxel is NaN"""
    n, C, B = 2, 2, 4
    packed = torch.zeros(n * (B * 3 * (1 + C) + C + 3), dtype=torch.int64)
    r = ops.CalibrationCounts.unpack(packed, n, C, B, 'categorical')
    r.top[0, 3] = torch.tensor([8, 4, 8 * 3 * 2 ** 30])                    # 8 voxels at 0.75, half right
    r.classwise[0, 0, 3] = torch.tensor([8, 4, 8 * 3 * 2 ** 30])
    r.classwise[0, 1, 1] = torch.tensor([8, 4, 8 * 2 ** 30])
    packed[-6:-2].view(torch.float64).copy_(torch.tensor([5.0, 4.0, 0.0, 0.0]))     # sums of subject 0: brier 5, nll 4
    packed[-2:] = 8
    seen = {}

    def stub(scores, targets, bins, kind):
        seen.update(n=len(scores), bins=bins, kind=kind)
        return r
    monkeypatch.setattr(ops, "eval_calibration", stub)
    ev = CalibrationEvaluator("p", "t", channel_names=["bg", "lesion"], bins=B)
    subjects = [{"name": k, "p": torch.zeros(C, 2, 2, 2), "t": torch.zeros(2, 2, 2, dtype=torch.int64)} for k in "ab"]
    out = ev(subjects)
    assert seen == dict(n=2, bins=B, kind='categorical') and set(out) == {'subject_stats', 'summary_stats', 'reliability'}
    df = out['subject_stats']
    assert list(df['subject']) == ['a'] * 3 + ['b'] * 3 and list(df['label']) == ['top', 'bg', 'lesion'] * 2
    assert list(df.columns) == ['subject', 'label', 'ece', 'mce', 'brier', 'nll', 'confidence', 'accuracy']
    assert list(df['ece'][:3]) == [0.25, 0.25, 0.25] and list(df['accuracy'][:3]) == [0.5] * 3
    assert list(df['confidence'][:3]) == [0.75, 0.75, 0.25] and list(df['brier'][:3]) == [5 / 8] * 3 and list(df['nll'][:3]) == [0.5] * 3
    assert all(math.isnan(v) for k in ('ece', 'mce', 'brier', 'nll', 'confidence', 'accuracy') for v in df[k][3:])
    rel = out['reliability']
    assert rel.dim_names == ['subject', 'label', 'bin', 'stat'] and rel.data.shape == (2, 3, B, 3)
    assert rel['a', 'top', '3'].tolist() == [8, 0.5, 0.75] and rel['a', 'lesion', '1'].tolist() == [8, 0.5, 0.25]
    assert rel['a', 'top', '0', 'count'] == 0 and rel['a', 'top', '0', 'accuracy'].isnan()
    assert out['summary_stats']['mean', 'top', 'ece'] == 0.25      # the NaN subject is left out, as in the other evaluators
    assert isinstance(ev, evaluators.Evaluator) and "bins=4, kind='categorical'" in repr(ev)
    with pytest.raises(ValueError, match="kind must be"):
        CalibrationEvaluator("p", "t", kind='softmax')
    assert CalibrationEvaluator("p", "t")._channel_names(2) == ["0", "1"]


# ------------------------------------------------------------------------------------------ the ensembles
class Head(nn.Module):
    """a stock torch member: a 1x1x1 convolution and a softmax (or sigmoid), so flipped members differ a little"""

    def __init__(self, seed, sigmoid=False):
        super().__init__()
        torch.manual_seed(seed)
        self.conv = nn.Conv3d(1, 3, 3, padding=1)
        self.sigmoid = sigmoid

    def forward(self, x):
        y = self.conv(x)
        return torch.sigmoid(y) if self.sigmoid else torch.softmax(y, dim=1)


def test_ensembles_refuse_uncertainty_with_majority():
    m = Head(0)
    for make in (lambda **kw: E.EnsembleModels([m], **kw), lambda **kw: E.EnsembleFlips(m, **kw),
                 lambda **kw: E.EnsembleOrientations(m, **kw)):
        with pytest.raises(ValueError, match="strategy 'mean'"):
            make(strategy='majority', uncertainty=True)
        with pytest.raises(ValueError, match="uncertainty_kind"):
            make(uncertainty=True, uncertainty_kind='soft')
        assert make(strategy='majority').last_uncertainty is None and make(uncertainty=True).uncertainty_kind == 'categorical'
        assert make().uncertainty_kind is None


@pytest.mark.parametrize("kind", ["categorical", "binary"])
def test_cpu_tensor_path_against_the_formulas(kind):
    x = torch.randn(2, 1, 4, 5, 6, generator=torch.Generator().manual_seed(3))
    model = Head(1, sigmoid=kind == 'binary')
    with torch.no_grad():
        ens = E.EnsembleFlips(model, uncertainty=True, uncertainty_kind=kind)
        out = ens(x)
        plain = E.EnsembleFlips(model)
        assert torch.equal(plain(x), out) and plain.last_uncertainty is None
        members = [E._torch_back(model(E._torch_member(x, (0, 1, 2), E._mask(f))), (0, 1, 2), E._mask(f)) for f in ens.flips]
    want = uref.ensemble_maps(members, kind)
    u = ens.last_uncertainty
    assert tuple(u) == E.UNCERTAINTY_MAPS
    K = 3 if kind == 'binary' else 1
    tol = 2 * uref.tol_h(3) + 8 * 2.0 ** -23 * (1 + math.log(3))
    for k in E.UNCERTAINTY_MAPS:
        assert u[k].shape == (2, 1 if k == 'confidence' else K, 4, 5, 6) and u[k].dtype == torch.float32
        assert (u[k].double() - want[k]).abs().max() <= tol, k
    assert (u['mutual_information'] >= 0).all() and u['mutual_information'].max() > 0
    # one member four times: no disagreement, and the entropy is that of the member
    same = E.EnsembleModels([model] * 4, uncertainty=True, uncertainty_kind=kind)
    with torch.no_grad():
        same(x)
    assert same.last_uncertainty['mutual_information'].abs().max() == 0
