"""Thresholded multi-label evaluation: what can be checked without a GPU -- the binding and its descriptor, the argument
checks of m355_eval_multilabel (no launches), MultiLabelEvaluator's interface and TrainLoop's label_transform=None."""
import ctypes
import inspect

import pytest
import torch

from segmentation_pipeline_amd import _lib, evaluators, ops
from segmentation_pipeline_amd.evaluators import MultiLabelEvaluator, SegmentationEvaluator

P = ctypes.c_void_p


def test_symbol_and_descriptor():
    assert "m355_eval_multilabel" in _lib.SIGNATURES and _lib.lib().m355_eval_multilabel is not None
    D = _lib.EvalMultilabelDesc
    assert [f[0] for f in D._fields_] == ["scores", "target", "S", "target_dtype"]
    assert (D.scores.offset, D.target.offset, D.S.offset, D.target_dtype.offset) == (0, 8, 16, 24)
    assert ctypes.sizeof(D) == 32
    assert "MultiLabelEvaluator" in evaluators.__all__


def _call(descs=None, n=1, dev=P(64), sd=_lib.EV_F32, C=2, thr=True, counts=P(64), scores=64, target=64, S=8,
          tdt=_lib.EV_BOOL):
    L = _lib.lib()
    if descs is None:
        descs = (_lib.EvalMultilabelDesc * max(n, 1))()
        for d in descs:
            d.scores, d.target, d.S, d.target_dtype = scores, target, S, tdt
    t = (ctypes.c_float * 64)(*([0.5] * 64)) if thr else None
    return L.m355_eval_multilabel(descs, n, dev, sd, C, t, counts, None), L.m355_last_error()


def test_argument_checks_reject_before_any_launch():
    rc, msg = _call(C=0)
    assert rc == -2 and b"eval_multilabel: 0 channels (1 .. 64)" in msg
    rc, msg = _call(C=65)
    assert rc == -2 and b"eval_multilabel: 65 channels" in msg
    rc, msg = _call(target=None)
    assert rc == -1 and b"eval_multilabel: subject 0: null target" in msg
    rc, msg = _call(n=0)
    assert rc == -1 and b"eval_multilabel: 0 subjects" in msg
    rc, msg = _call(scores=None)
    assert rc == -1 and b"null scores" in msg
    for kw in (dict(dev=None), dict(counts=None), dict(thr=False)):
        rc, msg = _call(**kw)
        assert rc == -1 and b"eval_multilabel: null pointer" in msg, kw
    rc, msg = _call(sd=_lib.EV_I32)
    assert rc == -1 and b"score type" in msg
    rc, msg = _call(S=0)
    assert rc == -1 and b"0 voxels" in msg
    rc, msg = _call(tdt=9)
    assert rc == -1 and b"target element type 9" in msg
    rc, msg = _call(tdt=-1)
    assert rc == -1


def test_ops_wrapper_errors():
    s = torch.zeros(2, 3, 3, 3)
    with pytest.raises(_lib.M355Error, match="one target per subject"):
        ops.eval_multilabel([], [])
    with pytest.raises(_lib.M355Error, match="one target per subject"):
        ops.eval_multilabel([s], [s, s])
    with pytest.raises(_lib.M355Error, match="3 thresholds for 2 channels"):
        ops.eval_multilabel([s], [s], [0.1, 0.2, 0.3])
    with pytest.raises(_lib.M355Error, match=r"65 channels \(1 .. 64\)"):
        ops.eval_multilabel([torch.zeros(65, 2, 2, 2)], [torch.zeros(65, 2, 2, 2)])
    with pytest.raises(_lib.M355Error, match="element type torch.int32"):
        ops.eval_multilabel([s.int()], [s])
    with pytest.raises(_lib.M355Error, match="expected a device tensor"):
        ops.eval_multilabel([s], [s])


def test_evaluator_defaults_and_repr():
    sig = inspect.signature(MultiLabelEvaluator.__init__)
    seg = inspect.signature(SegmentationEvaluator.__init__)
    assert list(sig.parameters)[1:] == ["prediction_name", "target_name", "channel_names", "threshold", "stats_to_output",
                                        "summary_stats_to_output"]
    assert sig.parameters["channel_names"].default is None and sig.parameters["threshold"].default == 0.5
    assert sig.parameters["stats_to_output"].default == seg.parameters["stats_to_output"].default
    assert sig.parameters["summary_stats_to_output"].default == ('mean', 'std', 'min', 'max')
    ev = MultiLabelEvaluator("scores", "truth", threshold=[0.5, 0.25])
    assert isinstance(ev, evaluators.Evaluator)
    assert repr(ev) == ("MultiLabelEvaluator(prediction_name='scores', target_name='truth', channel_names=None, "
                        "threshold=[0.5, 0.25], stats_to_output=('target_volume', 'prediction_volume', 'TP', 'FP', 'TN', "
                        "'FN', 'dice', 'precision', 'recall'), summary_stats_to_output=('mean', 'std', 'min', 'max'))")


def test_default_channel_names():
    assert MultiLabelEvaluator("a", "b")._channel_names(1) == ["0"]
    assert MultiLabelEvaluator("a", "b")._channel_names(5) == ["0", "1", "2", "3", "4"]
    assert MultiLabelEvaluator("a", "b", channel_names=("lesion", "edema"))._channel_names(2) == ["lesion", "edema"]
    with pytest.raises(_lib.M355Error, match="2 channel names .* for 3 channels"):
        MultiLabelEvaluator("a", "b", channel_names=("lesion", "edema"))._channel_names(3)


def test_train_loop_without_a_label_transform_builds_plain_subjects():
    """label_transform=None: the batch is split into subjects (names included), the evaluation images are attached and no
    label maps are added -- on the parent this died with an AttributeError in _label_steps"""
    from segmentation_pipeline_amd.trainer import ScheduledEvaluation, TrainLoop
    seen = []

    def evaluator(subjects):
        seen.append(subjects)
        return {"n": len(subjects)}
    batch = {"y_pred": torch.rand(2, 3, 4, 4, 4, requires_grad=True), "y": torch.ones(2, 3, 4, 4, 4),
             "X": torch.zeros(2, 1, 4, 4, 4), "name": ["a", "b"]}
    out = TrainLoop()._training_evaluations([ScheduledEvaluation(evaluator, "multi")], batch, None, None,
                                            {"scores": "y_pred", "truth": "y"})
    assert out == {"multi": {"n": 2}}
    (subjects,) = seen
    assert [s["name"] for s in subjects] == ["a", "b"]
    for i, s in enumerate(subjects):
        assert "y_pred_eval" not in s and "y_eval" not in s
        assert isinstance(s["scores"], evaluators.ScalarImage) and not s["scores"].data.requires_grad
        assert torch.equal(s["scores"].data, batch["y_pred"][i].detach()) and torch.equal(s["truth"].data, batch["y"][i])
        assert s["scores"].data.shape == (3, 4, 4, 4)
    # validation subjects: predicted, images attached, no label maps

    class Predictor:
        def predict(self, model, device, batch):
            return dict(batch, y_pred=batch["X"].repeat(1, 3, 1, 1, 1) + 1)
    val = {"cohort": [{"name": "v0", "X": torch.zeros(1, 4, 4, 4), "y": torch.ones(3, 4, 4, 4)}]}
    out = TrainLoop()._validation_evaluations([ScheduledEvaluation(evaluator, "multi", cohorts=["cohort"])], None,
                                              torch.device("cpu"), Predictor(), val, None, None,
                                              {"scores": "y_pred", "truth": "y"})
    assert out == {"multi": {"cohort": {"n": 1}}}
    (subject,) = seen[-1]
    assert subject["name"] == "v0" and "y_pred_eval" not in subject and "y_eval" not in subject
    assert torch.equal(subject["scores"].data, torch.ones(3, 4, 4, 4)) and torch.equal(subject["truth"].data, val["cohort"][0]["y"])
    # without names the subjects are numbered
    del batch["name"]
    TrainLoop()._training_evaluations([ScheduledEvaluation(evaluator, "multi")], batch, None, None, None)
    assert [s["name"] for s in seen[-1]] == ["0", "1"]
