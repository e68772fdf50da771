"""Thresholded multi-label evaluation on the device (m355_eval_multilabel via ops.eval_multilabel, MultiLabelEvaluator,
TrainLoop with label_transform=None) against boolean torch on the CPU."""
import numpy as np
import pytest
import torch
from torch import nn

from segmentation_pipeline_amd import ops
from segmentation_pipeline_amd.criterions import HybridBinaryLogisticDiceLoss, HybridLogisticDiceLoss
from segmentation_pipeline_amd.evaluators import (Evaluator, LabelMap, MultiLabelEvaluator, ScalarImage,
                                                  SegmentationEvaluator, label_counts)
from segmentation_pipeline_amd.models import ModularUNet
from segmentation_pipeline_amd.prediction import StandardPredict
from segmentation_pipeline_amd.trainer import ScheduledEvaluation, TrainLoop
from test_evaluation_cpu import _msseg2_chain, _same

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# (5, 7, 9) and (17, 33, 31): odd voxel counts, the scalar loads; (4, 6, 8) and (16, 16, 16): multiples of 8, the 16-byte
# loads (a [C, S] map's rows are then aligned as well)
SIZES = {"odd": [(5, 7, 9), (17, 33, 31)], "aligned": [(4, 6, 8), (16, 16, 16)]}
SCORE_DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TARGET_DTYPES = [torch.bool, torch.uint8, torch.float32]


def torch_counts(scores, target, thresholds):
    """int64 [C, 3]: TP, FP, FN of torch's own `>` and `!= 0` on the CPU (scores widened exactly)"""
    out = np.zeros((scores.shape[0], 3), np.int64)
    for c in range(scores.shape[0]):
        pred = scores[c].float() > thresholds[c]
        pos = target[c] != 0
        out[c] = [(pred & pos).sum().item(), (pred & ~pos).sum().item(), (~pred & pos).sum().item()]
    return out


def make_subject(g, C, size, sdtype, tdtype):
    """scores in (0, 1) rounded to sdtype with NaNs planted; a target of tdtype (float: soft values, zeros, -0.0, a NaN)"""
    s = torch.rand((C,) + size, generator=g).to(sdtype)
    s.view(-1)[torch.randperm(s.numel(), generator=g)[:max(3, s.numel() // 50)]] = float("nan")
    u = torch.rand((C,) + size, generator=g)
    if tdtype == torch.float32:
        t = torch.where(u < 0.4, u, torch.zeros(()))
        t.view(-1)[1] = -0.0
        t.view(-1)[2] = float("nan")              # positive, as torch's `!= 0`
        t.view(-1)[-1] = float("nan")
    elif tdtype == torch.bool:
        t = u < 0.4
    else:
        t = torch.where(u < 0.4, (u * 600).to(torch.int64) % 255 + 1, torch.zeros((), dtype=torch.int64)).to(tdtype)
    return s, t


@pytest.mark.parametrize("tdtype", TARGET_DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("sdtype", SCORE_DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("sizes", list(SIZES))
def test_counts_against_torch(sizes, C, sdtype, tdtype):
    """two subjects of different sizes in one launch, exact equality with boolean torch; per-channel thresholds, one equal
    to a score that occurs (strict `>` leaves that voxel out), +inf and -inf; NaN scores and a NaN target planted"""
    g = torch.Generator().manual_seed(11 * C + len(str(sdtype)) + 3 * len(str(tdtype)) + len(sizes))
    subjects = [make_subject(g, C, size, sdtype, tdtype) for size in SIZES[sizes]]
    s0 = subjects[0][0][0].float().flatten()
    occurring = s0[~torch.isnan(s0)][7].item()                      # a score of subject 0, channel 0, exact in fp32
    thresholds = [occurring, 0.25, float("inf"), float("-inf"), 0.75][:C]
    counts = ops.eval_multilabel([s.to(DEV) for s, _ in subjects], [t.to(DEV) for _, t in subjects], thresholds)
    assert counts.shape == (2, C, 3) and counts.dtype == torch.int64 and counts.is_cuda
    counts = counts.cpu().numpy()
    for i, (s, t) in enumerate(subjects):
        ref = torch_counts(s, t, thresholds)
        assert np.array_equal(counts[i], ref), (i, counts[i], ref)
        for c in range(C):
            tp, fp, fn = counts[i, c]
            assert tp + fn == (t[c] != 0).sum().item()                         # the target volume
            assert tp + fp == (s[c].float() > thresholds[c]).sum().item()       # the predicted volume
    s0 = subjects[0][0][0].float()
    assert counts[0, 0, 0] + counts[0, 0, 1] == (s0 > occurring).sum().item() < (s0 >= occurring).sum().item()
    if C == 5:
        assert counts[:, 2, :2].sum() == 0                                      # threshold +inf: nothing is predicted
        nan_free = sum(int((~torch.isnan(s[3].float())).sum()) for s, _ in subjects)
        assert counts[:, 3, :2].sum() == nan_free                               # -inf: everything but the NaNs


def test_scalar_threshold_16bit_targets_and_repeatability():
    """a float threshold applies to every channel; bfloat16 / float16 targets count as float32 ones do (-0.0 is not
    positive, a NaN is); a second call gives the same counts"""
    g = torch.Generator().manual_seed(3)
    s, t = make_subject(g, 3, (6, 10, 12), torch.float32, torch.float32)
    ref = torch_counts(s, t, [0.5] * 3)
    first = ops.eval_multilabel([s.to(DEV)], [t.to(DEV)], 0.5)
    assert np.array_equal(first.cpu().numpy()[0], ref)
    assert torch.equal(first, ops.eval_multilabel([s.to(DEV)], [t.to(DEV)], [0.5, 0.5, 0.5]))
    for h in (torch.bfloat16, torch.float16):
        th = torch.where(torch.isnan(t), t, (t != 0).float() * 0.5).to(h)     # every non-zero stays non-zero in 16 bits
        th.view(-1)[1] = -0.0
        assert np.array_equal(ops.eval_multilabel([s.to(DEV)], [th.to(DEV)], 0.5).cpu().numpy()[0], ref), h
        odd = ops.eval_multilabel([s[:, :5, :7, :9].contiguous().to(DEV)], [th[:, :5, :7, :9].contiguous().to(DEV)], 0.5)
        assert np.array_equal(odd.cpu().numpy()[0], torch_counts(s[:, :5, :7, :9], th[:, :5, :7, :9].float(), [0.5] * 3)), h


# ------------------------------------------------------------------------------------------------ evaluator
def reference_stats(tp, fp, fn, size):
    """the reference's float32 expressions (segmentation_evaluator.py) on the counts"""
    TP, FP, FN, TN = (torch.tensor([v], dtype=torch.int64).float() for v in (tp, fp, fn, size - tp - fp - fn))
    return {'target_volume': TP + FN, 'prediction_volume': TP + FP, 'TP': TP, 'FP': FP, 'TN': TN, 'FN': FN,
            'dice': 2 * TP / (2 * TP + FP + FN), 'jaccard': TP / (TP + FP + FN), 'precision': TP / (TP + FP),
            'recall': TP / (TP + FN)}


def test_evaluator_against_the_reference_expressions():
    g = torch.Generator().manual_seed(21)
    stats = ('target_volume', 'prediction_volume', 'TP', 'FP', 'TN', 'FN', 'dice', 'jaccard', 'precision', 'recall')
    names = ["lesion", "edema", "empty"]
    subjects, raw = [], []
    for i, size in enumerate([(5, 7, 9), (8, 8, 8)]):
        s, t = make_subject(g, 3, size, torch.float32, torch.uint8)
        s[2], t[2] = 0.0, 0                     # an empty channel: 0 / 0 statistics
        raw.append((s, t))
        # an image with .data on the device, an image on the host, a bare tensor
        subjects.append({"name": f"s{i}", "scores": ScalarImage(s.to(DEV)) if i == 0 else s,
                         "truth": LabelMap(t) if i == 0 else t.to(DEV)})
    thresholds = [0.5, 0.3, 0.5]
    out = MultiLabelEvaluator("scores", "truth", channel_names=names, threshold=thresholds, stats_to_output=stats)(subjects)
    assert set(out) == {"subject_stats", "summary_stats"}
    df, summary = out["subject_stats"], out["summary_stats"]
    assert list(df.columns) == ["subject", "label"] + list(stats)
    assert list(df["subject"]) == ["s0"] * 3 + ["s1"] * 3 and list(df["label"]) == names * 2
    assert summary.dim_names == ["summary_stat", "label", "stat"]
    assert list(summary.dim_keys[0]) == ['mean', 'std', 'min', 'max'] and summary.dim_keys[1] == names
    for i, (s, t) in enumerate(raw):
        counts = torch_counts(s, t, thresholds)
        for c, name in enumerate(names):
            ref = reference_stats(*(int(v) for v in counts[c]), s[0].numel())
            row = df[(df["subject"] == f"s{i}") & (df["label"] == name)]
            for k in stats:
                assert _same(np.float32(row[k].item()), np.float32(ref[k].item())), (i, name, k)     # NaN matches NaN
    assert np.isnan(df[df["label"] == "empty"]["dice"]).all()
    # the layout of SegmentationEvaluator's output on label maps of the same names
    maps = [{"name": f"s{i}", "p": LabelMap((s[:1] > 0.5).long().to(DEV), {n: k for k, n in enumerate(names)}),
             "t": LabelMap((t[:1] != 0).long().to(DEV), {n: k for k, n in enumerate(names)})} for i, (s, t) in enumerate(raw)]
    seg = SegmentationEvaluator("p", "t", stats_to_output=stats)(maps)
    assert list(seg["subject_stats"].columns) == list(df.columns)
    assert list(seg["subject_stats"]["subject"]) == list(df["subject"])
    assert list(seg["subject_stats"]["label"]) == list(df["label"])
    assert seg["summary_stats"].dim_names == summary.dim_names and seg["summary_stats"].dim_keys == summary.dim_keys
    assert seg["summary_stats"].data.shape == summary.data.shape
    # default names and statistics
    plain = MultiLabelEvaluator("scores", "truth")(subjects)
    assert list(plain["subject_stats"]["label"]) == ["0", "1", "2"] * 2
    assert list(plain["subject_stats"].columns)[2:] == ['target_volume', 'prediction_volume', 'TP', 'FP', 'TN', 'FN', 'dice',
                                                        'precision', 'recall']


# ------------------------------------------------------------------------------------------------ training loop
class Recording(Evaluator):
    """runs `inner` and keeps what it was given: per call, (name, y_pred, y) of every subject on the host"""

    def __init__(self, inner, extra=None):
        self.inner, self.extra, self.calls, self.extras = inner, extra, [], []

    def __call__(self, subjects):
        self.calls.append([(s["name"], s["y_pred"].detach().cpu().clone(), s["y"].detach().cpu().clone()) for s in subjects])
        if self.extra is not None:
            self.extras.append(self.extra(subjects))
        return self.inner(subjects)


def _batches(cout, one_hot):
    g = torch.Generator().manual_seed(7)
    x = torch.randn((2, 2, 16, 16, 16), generator=g)
    if one_hot:
        lab = torch.randint(0, cout, (2, 16, 16, 16), generator=g)
        y = nn.functional.one_hot(lab, cout).permute(0, 4, 1, 2, 3).float().contiguous()
    else:
        y = (torch.rand((2, cout, 16, 16, 16), generator=g) < 0.4).float()
    return [{"X": x.to(DEV), "y": y.to(DEV), "name": ["a", "b"]}] * 3


def test_train_loop_schedules_the_multilabel_evaluator():
    """a sigmoid ModularUNet with the new criterion, label_transform=None and a MultiLabelEvaluator on the attached images:
    three iterations run, each logged mean Dice is the one recomputed on the CPU from that iteration's y_pred and y, and a
    scoring function reading it drives max_score"""
    torch.manual_seed(0)
    model = ModularUNet(2, 3, [8, 16], 2, hypothesis_class=nn.Sigmoid, hypothesis_params={}).to(DEV)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    rec = Recording(MultiLabelEvaluator("scores", "truth"))
    rec_val = Recording(MultiLabelEvaluator("scores", "truth", channel_names=["a", "b", "c"], threshold=[0.4, 0.5, 0.6]))
    batches = _batches(3, False)
    val = {"validation": [{"name": f"v{i}", "X": batches[0]["X"][i].flip(1).contiguous(),
                           "y": batches[0]["y"][i].flip(1).contiguous()} for i in range(2)]}

    def scoring_function(log):
        return log["multilabel_eval"]["summary_stats"]['mean', :, 'dice'].mean()
    logs = []
    loop = TrainLoop(scoring_interval=1, scoring_function=scoring_function)
    loop.run(model, HybridBinaryLogisticDiceLoss(pos_weight=[1, 2, 3]), opt, StandardPredict(), iter(batches), DEV,
             3, log_fn=logs.append, training_evaluators=[ScheduledEvaluation(rec, "multilabel_eval")],
             validation_evaluators=[ScheduledEvaluation(rec_val, "validation_eval", cohorts=["validation"], interval=2)],
             validation_subjects=val, label_transform=None, evaluation_images={"scores": "y_pred", "truth": "y"})
    assert len(logs) == 3 and len(rec.calls) == 3 and loop.stop_reason == "max_iterations"
    # the validation cohort, every second iteration: the same check on its own thresholds and names
    assert ["validation_eval" in log for log in logs] == [True, False, True] and len(rec_val.calls) == 2
    for log, call in zip((logs[0], logs[2]), rec_val.calls):
        df = log["validation_eval"]["validation"]["subject_stats"]
        assert list(df["subject"]) == ["v0"] * 3 + ["v1"] * 3 and list(df["label"]) == ["a", "b", "c"] * 2
        for i, (name, y_pred, y) in enumerate(call):
            assert name == f"v{i}"
            for c, (tp, fp, fn) in enumerate(torch_counts(y_pred, y, [0.4, 0.5, 0.6])):
                assert _same(np.float32(df["dice"][3 * i + c]),
                             np.float32(reference_stats(int(tp), int(fp), int(fn), y[0].numel())['dice'].item())), (i, c)
    scores = []
    for it, (log, call) in enumerate(zip(logs, rec.calls)):
        assert [name for name, _, _ in call] == ["a", "b"]
        dice = torch.zeros(2, 3)
        for i, (_, y_pred, y) in enumerate(call):
            for c, (tp, fp, fn) in enumerate(torch_counts(y_pred, y, [0.5] * 3)):
                dice[i, c] = reference_stats(int(tp), int(fp), int(fn), y[0].numel())['dice'].item()
        summary = log["multilabel_eval"]["summary_stats"]
        assert _same(summary['mean', :, 'dice'], dice.mean(0)), it
        assert _same(np.float32(log["model_score"]), np.float32(dice.mean(0).mean().item())), it
        assert {"loss", "dice_loss", "logistic_loss"} <= set(log)
        scores.append(log["model_score"])
    assert not torch.equal(rec.calls[0][0][1], rec.calls[2][0][1])          # the model moved between the iterations
    assert loop.max_score == max(scores) and loop.max_score_iteration == scores.index(max(scores))


def test_train_loop_with_a_label_transform_is_unchanged():
    """the softmax set-up -- a label_transform, SegmentationEvaluator on 'y_pred_eval' / 'y_eval' -- logs the counts of
    label_counts on the same subjects, which are those of torch.argmax on the CPU"""
    torch.manual_seed(0)
    model = ModularUNet(2, 2, [8, 16], 2).to(DEV)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    rec = Recording(SegmentationEvaluator("y_pred_eval", "y_eval"),
                    extra=lambda subjects: label_counts(subjects, "y_pred_eval", "y_eval", [1]))
    logs = []
    TrainLoop().run(model, HybridLogisticDiceLoss(), opt, StandardPredict(), iter(_batches(2, True)), DEV, 3,
                    log_fn=logs.append, training_evaluators=[ScheduledEvaluation(rec, "segmentation_eval")],
                    label_transform=_msseg2_chain(), label_values={"lesion": 1})
    assert len(logs) == 3 and len(rec.calls) == 3
    for log, call, (counts, sizes) in zip(logs, rec.calls, rec.extras):
        df = log["segmentation_eval"]["subject_stats"]
        assert list(df["subject"]) == ["a", "b"] and list(df["label"]) == ["lesion", "lesion"]
        for i, (_, y_pred, y) in enumerate(call):
            pred, target = y_pred.argmax(0) == 1, y.argmax(0) == 1
            cpu = [(pred & target).sum().item(), (pred & ~target).sum().item(), (~pred & target).sum().item()]
            assert [int(v) for v in counts[i, 0]] == cpu and int(sizes[i]) == 16 ** 3
            ref = reference_stats(*cpu, 16 ** 3)
            for k in ('target_volume', 'prediction_volume', 'TP', 'FP', 'TN', 'FN', 'dice', 'precision', 'recall'):
                assert _same(np.float32(df[k][i]), np.float32(ref[k].item())), (i, k)
