"""Host side of scheduled evaluation (evaluators.LabeledTensor, prediction.EvaluationPlan, trainer.ScheduledEvaluation
and TrainLoop's evaluation hooks).  No GPU: the evaluators here are test doubles, and the evaluation
label maps are never materialised."""
import math
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import GOLDEN
from segmentation_pipeline_amd import augmentation as A
from segmentation_pipeline_amd import preprocessing as P
from segmentation_pipeline_amd._lib import M355Error
from segmentation_pipeline_amd.evaluators import LabeledTensor, LabelMap, ScoreLabelMap
from segmentation_pipeline_amd.prediction import EvaluationPlan, StandardPredict, add_evaluation_labels
from segmentation_pipeline_amd.trainer import ScheduledEvaluation, TrainLoop

SUMMARY = ('mean', 'median', 'mode', 'std', 'min', 'max')


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "evaluation.npz")))


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------------------------------------ LabeledTensor
def test_labeled_tensor_summary_stats_bit_exact(fx):
    lt = LabeledTensor(["a", "b", "c"], [["x", "y"], ["p", "q", "r"], ["u", "v"]])
    lt.data[:] = torch.from_numpy(fx["lt.data"])
    assert _same(lt.compute_summary_stats(list(SUMMARY)).data, fx["lt.summary"])
    assert _same(lt["x", "q"], fx["lt.getitem_x_q"])
    assert _same(lt[["y", "x"], :, "v"], fx["lt.getitem_list"])
    with pytest.raises(NotImplementedError):
        lt[..., "u"]


@pytest.mark.parametrize("case", ["seg", "seg_default", "seg_single", "lme", "ise"])
def test_summary_of_reference_subject_tables_bit_exact(fx, case):
    """the reference's subject tables in, the reference's summary tables out (a single subject: std is nan)"""
    cols = [str(c) for c in fx[f"{case}.df_columns"]]
    lead = 2 if cols[1] == "label" else 1
    stats = cols[lead:]
    names = [str(n) for n in fx[f"{case}.names"]]
    keys = [names]
    if lead == 2:
        keys.append(list(dict.fromkeys(str(v) for v in fx[f"{case}.df.label"])))
    keys.append(stats)
    lt = LabeledTensor(["subject", "label", "stat"][:lead] + ["stat"] if lead == 2 else ["subject", "stat"], keys)
    values = np.stack([fx[f"{case}.df.{s}"] for s in stats], axis=-1).astype(np.float32)
    lt.data[:] = torch.from_numpy(values.reshape(lt.data.shape))
    summary = lt.compute_summary_stats([str(k) for k in fx[f"{case}.summary_keys0"]])
    assert _same(summary.data, fx[f"{case}.summary"])


def test_to_dataframe_and_to_dict_layout():
    lt = LabeledTensor(["subject", "label", "stat"], [["s0", "s1", "s0"], ["a", "b"], ["dice", "TP"]])
    lt.data[:] = torch.arange(12, dtype=torch.float32).view(3, 2, 2)
    df = lt.to_dataframe()
    assert list(df.columns) == ["subject", "label", "dice", "TP"]
    assert list(df["subject"]) == ["s0", "s0", "s1", "s1", "s0", "s0"]
    # a name given twice addresses its last position, in reading and writing
    assert list(df["dice"]) == [8.0, 10.0, 4.0, 6.0, 8.0, 10.0]
    d = lt.to_dict()
    assert d["s1"]["b"]["TP"] == 7.0 and d["s0"]["a"]["dice"] == 8.0
    with pytest.raises(ValueError):
        LabeledTensor(["a"], [["x"], ["y"]])


# ------------------------------------------------------------------------------------------------ inverse chains
def _dmri_chain(hbt):
    common_1 = A.Compose([
        P.ReplaceNan(),
        P.CropOrPad((96, 88, 24), padding_mode='minimum', mask_name='whole_roi_union'),
        P.CustomRemapLabels(remapping=[("right_whole", 2, 1)], masking_method="Right", include=["whole_roi"]),
        P.CustomRemapLabels(remapping=[("right_head", 4, 1), ("right_body", 5, 2), ("right_tail", 6, 3)],
                            masking_method="Right", include=["hbt_roi"])])
    augment = A.Compose([A.RandomFlip(axes=(0,), p=0.5), A.RandomGamma(p=0.3)])
    common_2 = A.Compose([
        A.RescaleIntensity((-1., 1.), (0.5, 99.5)),
        P.ConcatenateImages(image_names=["mean_dwi", "md", "fa"], image_channels=[1, 1, 1], new_image_name="X"),
        P.RenameProperty(old_name="hbt_roi" if hbt else "whole_roi", new_name="y"),
        P.CustomOneHot(include=["y"])])
    return A.Compose([common_1, augment, common_2])


def _msseg2_chain():
    common_1 = A.Compose([P.SetDataType(torch.float), P.EnforceConsistentAffine(source_image_name='flair_time01'),
                          P.TargetResample(target_spacing=1, tolerance=0.11), P.CropToMask('brain_mask'),
                          P.MinSizePad(96)])
    common_2 = A.Compose([
        A.RescaleIntensity((-1, 1.), (0.05, 99.5)),
        P.ConcatenateImages(image_names=["flair_time01", "flair_time02"], image_channels=[1, 1], new_image_name="X"),
        P.RenameProperty(old_name='ground_truth', new_name='y'),
        P.CustomOneHot(include="y")])
    return A.Compose([common_1, common_2, P.ImageFromLabels(new_image_name="patch_probability",
                                                            label_weights=[('brain_mask', 'brain', 1),
                                                                           ('y', 'lesion', 100)])])


def test_inverse_of_dmri_hippo_whole_roi_chain():
    plan = EvaluationPlan(_dmri_chain(hbt=False))
    assert plan.source_name == "whole_roi" and plan.half == (0, 1) and plan.mask_name is None
    assert plan.tables(2) == ([0, 1], [0, 2])
    assert plan.label_values({"left_whole": 1, "right_whole": 1}) == {"left_whole": 1, "right_whole": 2}


def test_inverse_of_dmri_hippo_hbt_chain():
    plan = EvaluationPlan(_dmri_chain(hbt=True))
    assert plan.source_name == "hbt_roi" and plan.half == (0, 1)
    assert plan.tables(4) == ([0, 1, 2, 3], [0, 4, 5, 6])
    lv = {"left_head": 1, "left_body": 2, "left_tail": 3, "right_head": 1, "right_body": 2, "right_tail": 3}
    assert plan.label_values(lv) == {"left_head": 1, "left_body": 2, "left_tail": 3, "right_head": 4,
                                     "right_body": 5, "right_tail": 6}


def test_inverse_of_msseg2_chain():
    plan = EvaluationPlan(_msseg2_chain())
    assert plan.source_name == "ground_truth" and plan.half is None and plan.mask_name is None
    assert plan.tables(2) == ([0, 1], [0, 1])
    assert plan.label_values({"lesion": 1}) == {"lesion": 1}


def test_inverse_with_dict_remap_and_map_mask():
    chain = A.Compose([P.CustomRemapLabels({3: 1, 1: 3}, masking_method="brain", include="lab"),
                       P.RenameProperty("lab", "y"), P.CustomOneHot()])
    plan = EvaluationPlan(chain)
    assert plan.mask_name == "brain" and plan.half is None
    assert plan.tables(4) == ([0, 1, 2, 3], [0, 3, 2, 1])


def test_gated_label_transforms_are_refused():
    gated = A.Compose([P.CustomRemapLabels({2: 1}, p=0.5), P.CustomOneHot()])
    with pytest.raises(M355Error, match="probability gate"):
        EvaluationPlan(gated)
    one_of = A.Compose([A.OneOf([P.CustomRemapLabels({2: 1}), A.RandomGamma()]), P.CustomOneHot()])
    with pytest.raises(M355Error, match="OneOf"):
        EvaluationPlan(one_of)
    gated_compose = A.Compose([A.Compose([P.RenameProperty("a", "y")], p=0.9), P.CustomOneHot()])
    with pytest.raises(M355Error):
        EvaluationPlan(gated_compose)
    with pytest.raises(M355Error, match="CustomOneHot"):
        EvaluationPlan(A.Compose([P.RenameProperty("a", "y")]))


def test_add_evaluation_labels_is_lazy_and_names_follow_a_batch():
    batch = {"y_pred": torch.zeros(2, 2, 4, 4, 4), "y": torch.zeros(2, 2, 4, 4, 4), "name": ["a", "b"]}
    subjects = add_evaluation_labels(batch, _dmri_chain(False), {"left_whole": 1, "right_whole": 1})
    assert [s["name"] for s in subjects] == ["a", "b"]
    for s in subjects:
        assert isinstance(s["y_pred_eval"], ScoreLabelMap) and s["y_pred_eval"].pending
        assert s["y_pred_eval"]["label_values"] == {"left_whole": 1, "right_whole": 2}
        assert s["y_eval"].role == "target"


# ------------------------------------------------------------------------------------------------ scheduling
class Recorder:
    """a CPU test double of an evaluator: records the subject names it saw, returns a summary table whose mean dice
    comes from `dice(iteration)`"""

    def __init__(self, dice=None):
        self.calls, self.dice, self.iteration = [], dice, 0

    def __call__(self, subjects):
        self.calls.append([s["name"] for s in subjects])
        assert all("y_pred_eval" in s for s in subjects)
        t = LabeledTensor(["summary_stat", "label", "stat"], [["mean"], ["left_whole", "right_whole"], ["dice"]])
        if self.dice is not None:
            t.data[0, :, 0] = torch.tensor(self.dice[len(self.calls) - 1])
        return {"subject_stats": None, "summary_stats": t}


def _setup(n_batches=8):
    torch.manual_seed(0)
    model = nn.Sequential(nn.Conv3d(3, 2, 3, padding=1), nn.Softmax(dim=1))
    opt = torch.optim.SGD(model.parameters(), lr=0.1)

    def criterion(y_pred, y):
        return {"loss": ((y_pred - y) ** 2).mean()}
    g = torch.Generator().manual_seed(1)
    batches = [{"X": torch.randn(2, 3, 4, 4, 4, generator=g),
                "y": nn.functional.one_hot(torch.randint(0, 2, (2, 4, 4, 4), generator=g), 2).permute(0, 4, 1, 2, 3).float(),
                "name": [f"t{i}a", f"t{i}b"]} for i in range(n_batches)]
    val = {"cbbrain_validation": [{"name": f"v{i}", "X": torch.randn(3, 4, 4, 4, generator=g),
                                   "y": torch.zeros(2, 4, 4, 4)} for i in range(3)],
           "ab300_validation": [{"name": "w0", "X": torch.randn(3, 4, 4, 4, generator=g), "y": torch.zeros(2, 4, 4, 4)}]}
    return model, opt, criterion, batches, val


def test_scheduled_evaluation_arguments():
    with pytest.raises(AssertionError):
        ScheduledEvaluation(Recorder(), "x", cohorts=["a"], subjects=["s"])
    s = ScheduledEvaluation(Recorder(), "x", cohorts=["a"], interval=5)
    assert (s.log_name, s.cohorts, s.subjects, s.interval) == ("x", ["a"], None, 5)


def test_intervals_cohorts_subjects_and_log_structure():
    model, opt, criterion, batches, val = _setup()
    train_rec, coh_rec, subj_rec = Recorder(), Recorder(), Recorder()
    logs = []
    loop = TrainLoop()
    loop.run(model, criterion, opt, StandardPredict(), iter(batches), torch.device("cpu"), 7, log_fn=logs.append,
             training_evaluators=[ScheduledEvaluation(train_rec, "train_eval", interval=3)],
             validation_evaluators=[ScheduledEvaluation(coh_rec, "seg", cohorts=["cbbrain_validation", "ab300_validation"],
                                                        interval=2),
                                    ScheduledEvaluation(subj_rec, "named", subjects=["w0", "v1"], interval=4)],
             validation_subjects=val, label_transform=_dmri_chain(False), label_values={"left_whole": 1, "right_whole": 1})
    assert len(logs) == 7
    assert train_rec.calls == [["t0a", "t0b"], ["t3a", "t3b"], ["t6a", "t6b"]]
    assert coh_rec.calls == [["v0", "v1", "v2"], ["w0"]] * 4
    assert subj_rec.calls == [["w0", "v1"]] * 2
    for i, log in enumerate(logs):
        assert ("train_eval" in log) == (i % 3 == 0)
        assert ("seg" in log) == (i % 2 == 0)
        assert ("named" in log) == (i % 4 == 0)
        if i % 2 == 0:
            assert set(log["seg"]) == {"cbbrain_validation", "ab300_validation"}
            assert set(log["seg"]["ab300_validation"]) == {"subject_stats", "summary_stats"}
        if i % 4 == 0:
            assert set(log["named"]) == {"subject_stats", "summary_stats"}


def test_dmri_hippo_scoring_function_drives_best_iteration():
    # the production scoring function (research/dmri_hippo/configs/main_config.py), verbatim
    def scoring_function(evaluation_dict):
        seg_eval_cbbrain = evaluation_dict['segmentation_eval']['cbbrain_validation']["summary_stats"]
        cbbrain_dice = seg_eval_cbbrain['mean', :, 'dice']
        cbbrain_dice = cbbrain_dice.mean()
        score = cbbrain_dice
        return score

    model, opt, criterion, batches, val = _setup()
    dice = [(0.1, 0.2), (0.5, 0.6), (0.4, 0.9), (0.3, 0.3), (0.2, 0.2), (0.1, 0.1)]
    rec = Recorder(dice)
    saved = []
    loop = TrainLoop(scoring_interval=2, scoring_function=scoring_function, max_iterations_with_no_improvement=4,
                     save_fn=lambda kind, it: saved.append((kind, it)))
    logs = []
    loop.run(model, criterion, opt, StandardPredict(), iter(batches), torch.device("cpu"), 8, log_fn=logs.append,
             validation_evaluators=[ScheduledEvaluation(rec, "segmentation_eval", cohorts=["cbbrain_validation"],
                                                        interval=2)],
             validation_subjects=val, label_transform=_dmri_chain(False),
             label_values={"left_whole": 1, "right_whole": 1})
    # scores at iterations 0, 2, 4, 6: 0.15, 0.55, 0.65, 0.3 -> best at 4
    assert [round(l["model_score"], 6) for l in logs if "model_score" in l] == [0.15, 0.55, 0.65, 0.3]
    assert loop.max_score_iteration == 4 and math.isclose(loop.max_score, 0.65, rel_tol=1e-6)
    assert [s for s in saved if s[0] == "best_checkpoints/"] == [("best_checkpoints/", 0), ("best_checkpoints/", 2),
                                                                 ("best_checkpoints/", 4)]


def test_run_without_evaluators_is_unchanged():
    runs = []
    for extra in ({}, {"training_evaluators": (), "validation_evaluators": ()}):
        model, opt, criterion, batches, _ = _setup()
        logs = []
        TrainLoop().run(model, criterion, opt, StandardPredict(), iter(batches), torch.device("cpu"), 4,
                        log_fn=logs.append, **extra)
        runs.append(logs)
    for a, b in zip(*runs):
        assert set(a) == {"loss"} == set(b)
        assert torch.equal(a["loss"], b["loss"])


def test_label_map_holder():
    m = LabelMap(torch.zeros(1, 2, 2, 2), {"a": 1})
    assert m["label_values"] == {"a": 1} and m.data.shape == (1, 2, 2, 2) and "label_values" in m
