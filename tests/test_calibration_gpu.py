"""Calibration on the device (m355_eval_calibration via ops.eval_calibration, CalibrationEvaluator, TrainLoop; DESIGN
§4.31) against the torch restatement of calibration_ref on the CPU: integers equal, fp64 sums within the bound of an
fp64 sum."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from torch import nn

import calibration_ref as cref
from segmentation_pipeline_amd import _lib, ops
from segmentation_pipeline_amd.criterions import HybridBinaryLogisticDiceLoss, HybridLogisticDiceLoss
from segmentation_pipeline_amd.evaluators import CalibrationEvaluator
from segmentation_pipeline_amd.models import ModularUNet
from segmentation_pipeline_amd.prediction import StandardPredict
from segmentation_pipeline_amd.trainer import ScheduledEvaluation, TrainLoop

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# (5, 7, 9) and (17, 33, 31): odd voxel counts, the element loads; (4, 6, 8) and (16, 16, 16): multiples of 8, the 16-byte
# loads (the rows of a [C, S] map are then aligned as well)
SIZES = {"odd": [(5, 7, 9), (17, 33, 31)], "aligned": [(4, 6, 8), (16, 16, 16)]}
SCORE_DTYPES = [torch.float32, torch.bfloat16, torch.float16]
BINS = [1, 10, 15, _lib.CAL_MAX_BINS]
INDEX_DTYPES = [torch.int64, torch.uint8, torch.int32, torch.int16]
ONEHOT_DTYPES = [torch.float32, torch.bool, torch.bfloat16, torch.uint8]
CASES = [(1, 'binary'), (2, 'categorical'), (5, 'categorical'), (5, 'binary'), (64, 'categorical')]
WORST = {"brier": 0.0, "nll": 0.0}     # the largest error seen, in units of the bound (printed by the last test)


def make_subject(g, C_, size, sdtype, kind):
    """probabilities softmax(2.5 randn) over the channels (one channel, or 'binary': a sigmoid) rounded to sdtype, class
    indices drawn from them; planted: a NaN, a value above 1, a negative one, 0.5 and float32(0.4) = 6/15 on bin edges"""
    S = math.prod(size)
    z = 2.5 * torch.randn((C_, S), generator=g)
    p = torch.sigmoid(z) if (C_ == 1 or kind == 'binary') else torch.softmax(z, dim=0)
    if kind == 'categorical':
        idx = torch.multinomial(p.T.contiguous(), 1, generator=g)[:, 0]
    else:
        idx = torch.where(torch.rand(S, generator=g) < p[0], 0, C_ - 1) if C_ > 1 else torch.zeros(S, dtype=torch.int64)
    p = p.to(sdtype)
    p[0, 3] = float("nan")
    p[C_ - 1, 5] = 1.5
    p[C_ // 2, 6] = -0.125
    p[:, 7] = 0.0
    p[0, 7] = 0.5                                  # top label exactly on an edge of 10 and 32 bins
    p[:, 8] = 0.0
    p[C_ - 1, 8] = torch.tensor(6 / 15, dtype=torch.float32).to(sdtype)     # (exactly 6/15 in float32 only)
    p[:, 10] = 0.0
    p[0, 10] = 1.0                                 # the last bin
    return p.reshape((C_,) + size), idx.reshape(size)


def targets_of(idx, C_, form, dtype, kind):
    """the index map in `dtype` with two indices out of range, or the one-hot map of it ('binary': a second positive
    channel here and there)"""
    if form == "index":
        t = idx.clone()
        t.view(-1)[9] = C_                          # out of range
        if dtype != torch.uint8:
            t.view(-1)[11] = -1
        return t.to(dtype)
    t = nn.functional.one_hot(idx, C_).movedim(-1, 0).contiguous()
    if kind == 'binary' and C_ > 1:
        t[1] |= t[0] & (idx.new_tensor(1))          # channel 1 positive wherever channel 0 is: several labels a voxel
    return t.to(dtype)


def fetch(res, n, C_, B, kind):
    return ops.CalibrationCounts.unpack(res.packed.cpu(), n, C_, B, kind)


def compare(r, i, ref, kind, what):
    """integers equal; sums within relative 4 (n + 2) 2^-53, n the number of summed terms"""
    if kind == 'categorical':
        assert r.top[i].tolist() == ref['top'], what
        assert int(r.invalid[i]) == ref['invalid'], what
    else:
        assert r.top[i].abs().sum() == 0, what
        assert r.invalid[i].tolist() == ref['invalid'], what
    assert r.classwise[i].tolist() == ref['classwise'], what
    for k, (name, got) in enumerate((("brier", r.brier[i].item()), ("nll", r.nll[i].item()))):
        bound = 4 * (ref['terms'][k] + 2) * 2.0 ** -53 * abs(ref[name])
        err = abs(got - ref[name])
        WORST[name] = max(WORST[name], err / bound if bound else float(err != 0))
        print(f"{what} {name}: got {got!r} ref {ref[name]!r} err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (what, name, got, ref[name])


@pytest.mark.parametrize("sdtype", SCORE_DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"C{c[0]}-{c[1]}")
@pytest.mark.parametrize("sizes", list(SIZES))
def test_tables_and_sums_against_torch(sizes, case, sdtype):
    """two subjects of different sizes in one launch, every bin count and both target forms"""
    C_, kind = case
    g = torch.Generator().manual_seed(13 * C_ + len(str(sdtype)) + len(sizes) + len(kind))
    subjects = [make_subject(g, C_, size, sdtype, kind) for size in SIZES[sizes]]
    scores = [p.to(DEV) for p, _ in subjects]
    for k, B in enumerate(BINS):
        for form, dtype in (("index", INDEX_DTYPES[k]), ("onehot", ONEHOT_DTYPES[k])):
            targets = [targets_of(idx, C_, form, dtype, kind) for _, idx in subjects]
            res = ops.eval_calibration(scores, [t.to(DEV) for t in targets], B, kind)
            r = fetch(res, 2, C_, B, kind)
            assert r.voxels.tolist() == [math.prod(size) for size in SIZES[sizes]]
            for i, ((p, _), t) in enumerate(zip(subjects, targets)):
                ref = cref.reference(p, t, B, kind)
                compare(r, i, ref, kind, f"{sizes}[{i}] C={C_} {kind} {sdtype} B={B} {form}:{dtype}")
                if B == 15 and i == 1:
                    tab = ref['top'] if kind == 'categorical' else ref['classwise'][0]
                    assert sum(1 for row in tab if row[0]) >= 5       # an all-in-one-bin input cannot pass
                    assert (ref['invalid'] >= 3) if kind == 'categorical' else (max(ref['invalid']) >= 1)


def _one_case(C_=5, kind='categorical', sizes=((16, 16, 32), (17, 33, 31)), B=15, sdtype=torch.float32, seed=5):
    g = torch.Generator().manual_seed(seed)
    subjects = [make_subject(g, C_, size, sdtype, kind) for size in sizes]
    targets = [targets_of(idx, C_, "index", torch.int64, kind) for _, idx in subjects]
    return subjects, targets


@pytest.mark.parametrize("kind", ["categorical", "binary"])
def test_a_small_grid_takes_several_trips_and_flushes(tuning, kind):
    """M355_CAL_BLOCKS = 2 and 3: so few workgroups per subject walk 8192 (aligned) and 17391 (odd) voxels in several trips
    of the grid-stride loop and all flush into one table; the tables do not depend on the grid"""
    subjects, targets = _one_case(kind=kind)
    scores, dt = [p.to(DEV) for p, _ in subjects], [t.to(DEV) for t in targets]
    base = fetch(ops.eval_calibration(scores, dt, 15, kind), 2, 5, 15, kind)
    for blocks in (2, 3):
        tuning(M355_CAL_BLOCKS=blocks)
        r = fetch(ops.eval_calibration(scores, dt, 15, kind), 2, 5, 15, kind)
        for i, ((p, _), t) in enumerate(zip(subjects, targets)):
            compare(r, i, cref.reference(p, t, 15, kind), kind, f"{blocks} blocks [{i}] {kind}")
        assert torch.equal(r.top, base.top) and torch.equal(r.classwise, base.classwise) and torch.equal(r.invalid, base.invalid)


def _raw_call(scores, targets, B, kind, fill):
    """m355_eval_calibration on buffers of this test's own: every output, the workspace and dev_descs filled by `fill`"""
    n, C_ = len(scores), scores[0].shape[0]
    L = _lib.lib()
    descs = (_lib.EvalCalibrationDesc * n)()
    for d, s, t in zip(descs, scores, targets):
        d.scores, d.target, d.S, d.target_dtype = s.data_ptr(), t.data_ptr(), s[0].numel(), _lib.EV_I64
    bufs = {"dev": torch.empty(C.sizeof(descs), dtype=torch.uint8, device=DEV),
            "top": torch.empty((n, B, 3), dtype=torch.int64, device=DEV),
            "cls": torch.empty((n, C_, B, 3), dtype=torch.int64, device=DEV),
            "inv": torch.empty((n, C_), dtype=torch.int64, device=DEV),
            "sums": torch.empty((n, 2), dtype=torch.float64, device=DEV),
            "vox": torch.empty(n, dtype=torch.int64, device=DEV),
            "ws": torch.empty(L.m355_eval_calibration_workspace(n), dtype=torch.uint8, device=DEV)}
    for b in bufs.values():
        fill(b)
    _lib.check(L.m355_eval_calibration(descs, n, ops._p(bufs["dev"]), _lib.EV_F32, _lib.EV_TARGET_MAP, C_, B,
                                       0 if kind == 'categorical' else 1, *[ops._p(bufs[k]) for k in ("top", "cls", "inv", "sums", "vox")],
                                       ops._p(bufs["ws"]), bufs["ws"].numel(), ops._stream()), "eval_calibration")
    torch.cuda.synchronize()
    return [bufs[k].cpu() for k in ("top", "cls", "inv", "sums", "vox")]


@pytest.mark.parametrize("kind", ["categorical", "binary"])
def test_repeatable_and_indifferent_to_what_the_buffers_held(kind):
    """the same call twice gives the same bits; tables, sums, workspace and dev_descs freshly filled with 0xFF bytes or
    NaNs give them again"""
    subjects, targets = _one_case(kind=kind)
    scores, dt = [p.to(DEV) for p, _ in subjects], [t.to(DEV) for t in targets]
    a = ops.eval_calibration(scores, dt, 15, kind).packed.cpu()
    b = ops.eval_calibration(scores, dt, 15, kind).packed.cpu()
    assert torch.equal(a, b)

    def ones(t):
        t.view(torch.uint8).fill_(0xFF)

    def nans(t):
        if t.dtype == torch.float64:
            t.fill_(float("nan"))
        else:
            t.view(torch.uint8).fill_(0x7F)
    clean = _raw_call(scores, dt, 15, kind, lambda t: t.zero_())
    r = fetch(ops.eval_calibration(scores, dt, 15, kind), 2, 5, 15, kind)
    assert torch.equal(clean[0], r.top) and torch.equal(clean[1], r.classwise)
    assert torch.equal(clean[3][:, 0].view(torch.int64), r.brier.contiguous().view(torch.int64))
    for fill in (ones, nans):
        dirty = _raw_call(scores, dt, 15, kind, fill)
        for x, y in zip(clean, dirty):
            assert torch.equal(x.view(torch.int64), y.view(torch.int64))


def test_evaluator_statistics_are_the_expressions_on_the_reference_integers():
    subjects, targets = _one_case(C_=3, sizes=((5, 7, 9), (16, 16, 16)))
    subs = [{"name": f"s{i}", "p": p.to(DEV), "t": t.to(DEV)} for i, ((p, _), t) in enumerate(zip(subjects, targets))]
    for kind in ("categorical", "binary"):
        out = CalibrationEvaluator("p", "t", channel_names=["a", "b", "c"], bins=10, kind=kind)(subs)
        df = out["subject_stats"]
        labels = (["top"] if kind == "categorical" else []) + ["a", "b", "c"]
        assert list(df["label"]) == labels * 2
        for i, ((p, _), t) in enumerate(zip(subjects, targets)):
            ref = cref.reference(p, t, 10, kind)
            tabs = ([ref["top"]] if kind == "categorical" else []) + ref["classwise"]
            for l, tab in enumerate(tabs):
                ece, mce, conf, acc = cref.table_stats(tab)
                row = i * len(labels) + l
                assert (np.float32(df["ece"][row]), np.float32(df["mce"][row])) == (np.float32(ece), np.float32(mce))
                assert (np.float32(df["confidence"][row]), np.float32(df["accuracy"][row])) == (np.float32(conf), np.float32(acc))
                assert abs(df["brier"][row] - ref["brier"] / ref["valid"]) <= 1e-6 * ref["brier"] / ref["valid"]
                assert abs(df["nll"][row] - ref["nll"] / ref["valid"]) <= 1e-6 * ref["nll"] / ref["valid"]
                rel = out["reliability"].data[i, l]
                assert rel[:, 0].tolist() == [row_[0] for row_ in tab]


def _batches(cout, one_hot):
    g = torch.Generator().manual_seed(7)
    x = torch.randn((2, 2, 16, 16, 16), generator=g)
    if one_hot:
        lab = torch.randint(0, cout, (2, 16, 16, 16), generator=g)
        y = nn.functional.one_hot(lab, cout).permute(0, 4, 1, 2, 3).float().contiguous()
    else:
        y = (torch.rand((2, cout, 16, 16, 16), generator=g) < 0.4).float()
    return [{"X": x.to(DEV), "y": y.to(DEV), "name": ["a", "b"]}] * 2


@pytest.mark.parametrize("head", ["sigmoid", "softmax"])
def test_train_loop_schedules_the_calibration_evaluator(head):
    """label_transform=None and a CalibrationEvaluator on the attached images: every iteration logs a finite ECE"""
    torch.manual_seed(0)
    if head == "sigmoid":
        model = ModularUNet(2, 3, [8, 16], 2, hypothesis_class=nn.Sigmoid, hypothesis_params={}).to(DEV)
        loss, ev, batches = HybridBinaryLogisticDiceLoss(), CalibrationEvaluator("scores", "truth", kind="binary"), _batches(3, False)
    else:
        model = ModularUNet(2, 2, [8, 16], 2).to(DEV)
        loss, ev, batches = HybridLogisticDiceLoss(), CalibrationEvaluator("scores", "truth"), _batches(2, True)
    logs = []
    TrainLoop().run(model, loss, torch.optim.SGD(model.parameters(), lr=0.1), StandardPredict(), iter(batches), DEV, 2,
                    log_fn=logs.append, training_evaluators=[ScheduledEvaluation(ev, "calibration_eval")],
                    label_transform=None, evaluation_images={"scores": "y_pred", "truth": "y"})
    assert len(logs) == 2
    for log in logs:
        df = log["calibration_eval"]["subject_stats"]
        assert list(df["label"]) == ((["top"] if head == "softmax" else []) + [str(c) for c in range(3 if head == "sigmoid" else 2)]) * 2
        for k in ("ece", "mce", "brier", "nll", "confidence", "accuracy"):
            assert np.isfinite(np.asarray(df[k], dtype=np.float64)).all(), k
        assert (np.asarray(df["ece"]) >= 0).all() and (np.asarray(df["ece"]) <= 1).all()
        assert log["calibration_eval"]["reliability"].data.shape[2] == 15


def test_zz_report_worst_errors():
    """(not a check of its own: prints the largest fp64-sum errors the tests above saw, in units of their bound)"""
    print("largest error / bound:", WORST)
    assert WORST["brier"] <= 1 and WORST["nll"] <= 1
