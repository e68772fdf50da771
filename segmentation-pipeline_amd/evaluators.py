"""The reference's evaluators (evaluators/segmentation_evaluator.py, label_map_evaluator.py,
instance_segmentation_evaluator.py, labeled_tensor.py) with their counts taken on the device, and lesion-wise detection
statistics (the per-subject numbers of the reference's InstanceSegmentationEvaluator,
evaluators/instance_segmentation_evaluator.py) with the labelling and the overlap table on the device.  ContourImageEvaluator
(evaluators/contour_image_evaluator.py) and FindInterestingSlice (transforms/find_interesting_slice.py) take their
per-slice counts, ranks and slice mosaics on the device and draw on the host.

The overlap table of N target and M predicted components is a dense int64 [N + 1, M + 1] histogram (component 0 is
the background of either map), built by one pass of m355_label_histogram over the two label maps.  It is refused
above MAX_OVERLAP_ENTRIES entries.  The detection test and every statistic derived from the table run on the host in
float32, the dtype of the reference's table (so N == 0 or M == 0 gives the same nan results).
"""
import ctypes
import io
import itertools
import random
import warnings
from collections.abc import Mapping
from typing import Callable, Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from ._lib import M355Error, check
from .post_processing import _DTYPE_CODE, _OP_COPY, _OP_POSITIVE, _ccl, _connectivity, _device_volume, _histogram, _to_i32

__all__ = ["overlap_histogram", "msseg_detection_test", "instance_segmentation_stats", "MAX_OVERLAP_ENTRIES", "STAT_NAMES",
           "LabeledTensor", "LabelMap", "Evaluator", "SegmentationEvaluator", "MultiLabelEvaluator", "CalibrationEvaluator",
           "calibration_stats", "LabelMapEvaluator",
           "InstanceSegmentationEvaluator", "label_counts", "ScalarImage", "find_interesting_slices",
           "FindInterestingSlice", "ContourImageEvaluator", "render_contours", "SurfaceDistanceEvaluator",
           "surface_distances", "SURFACE_STAT_NAMES", "ImageRegionEvaluator", "IMAGE_REGION_STAT_NAMES"]

MAX_OVERLAP_ENTRIES = 1 << 26   # (N + 1) * (M + 1): 512 MiB of int64 counts

STAT_NAMES = ('target_components', 'predicted_components', 'target_detections', 'predicted_detections',
              'detection_recall', 'detection_precision', 'detection_f1', 'target_volume', 'prediction_volume',
              'TP', 'FP', 'TN', 'FN', 'dice', 'jaccard', 'precision', 'recall')


def _overlap(t32, p32, n_target, n_pred):
    entries = (n_target + 1) * (n_pred + 1)
    if entries > MAX_OVERLAP_ENTRIES:
        raise M355Error(f"overlap table of {n_target} target x {n_pred} predicted components has {entries} entries, "
                        f"more than MAX_OVERLAP_ENTRIES = {MAX_OVERLAP_ENTRIES}")
    return _histogram(t32, 0, entries, b=p32, bstride=n_pred + 1).view(n_target + 1, n_pred + 1)


def overlap_histogram(target_components, pred_components):
    """int64 [N + 1, M + 1] table: entry [i, j] counts the voxels of target component i and predicted component j
    (0 = background).  Inputs are label maps 0..N and 0..M of one shape; N and M are their maxima.  Numpy inputs
    give a numpy table, tensors a tensor on the GPU."""
    t, back = _device_volume(target_components)
    p, _ = _device_volume(pred_components)
    if t.shape != p.shape:
        raise M355Error(f"label maps of different shapes {tuple(t.shape)} and {tuple(p.shape)}")
    t32, p32 = _to_i32(t, _OP_COPY), _to_i32(p, _OP_COPY)
    _, (tmin, n_target) = _histogram(t32, 0, 1, minmax=True)
    _, (pmin, n_pred) = _histogram(p32, 0, 1, minmax=True)
    if min(tmin, pmin) < 0:
        raise M355Error("component labels must be >= 0")
    return back(_overlap(t32, p32, n_target, n_pred))


def _detects(row, row_total, col_total, min_recall, contribution_threshold, min_precision):
    """True / False for one target instance (row of the table), or None when the contributions never reach the
    threshold (the reference then records nothing for it)."""
    overlap = row[1:].sum()
    if overlap / row_total < min_recall:
        return False
    covered = 0.0
    for j in torch.argsort(row[1:], descending=True) + 1:
        if row[j] / col_total[j] < min_precision:
            return False
        covered = covered + row[j] / overlap
        if covered >= contribution_threshold:
            return True
    return None


def msseg_detection_test(overlap_histogram, min_recall=0.1, contribution_threshold=0.65, min_precision=0.3):
    """MSSEG (2016, 2021) lesion detection test on an (N + 1, M + 1) overlap table: a bool tensor, one entry per
    target instance 1..N.  A target is missed when the predictions cover less than min_recall of it; otherwise the
    predictions overlapping it, largest overlap first, must each reach min_precision until their share of the covered
    voxels reaches contribution_threshold.  Runs on the host in float32."""
    h = torch.as_tensor(overlap_histogram).detach().cpu().to(torch.float32)
    row_totals, col_totals = h.sum(dim=1), h.sum(dim=0)
    verdicts = (_detects(h[i], row_totals[i], col_totals, min_recall, contribution_threshold, min_precision)
                for i in range(1, h.shape[0]))
    return torch.tensor([v for v in verdicts if v is not None])


def _item(v):
    return v.item() if isinstance(v, torch.Tensor) else v


def instance_segmentation_stats(pred, target, connectivity=2, detection_test=msseg_detection_test,
                                detection_test_params=None):
    """The 17 per-subject statistics of InstanceSegmentationEvaluator for one prediction / target pair (3-D label maps,
    or [1, D, H, W] tensors as the evaluator's subjects hold): components of (map > 0) are labelled on the device,
    their overlap table is built there and the detection test runs on the host.  Returns {stat name: number}."""
    params = {} if detection_test_params is None else detection_test_params
    conn = _connectivity(connectivity)
    pred = pred[0] if pred.ndim == 4 else pred
    target = target[0] if target.ndim == 4 else target
    p, _ = _device_volume(pred)
    t, _ = _device_volume(target)
    if t.shape != p.shape:
        raise M355Error(f"prediction {tuple(p.shape)} and target {tuple(t.shape)} differ in shape")
    p_labels, M = _ccl(_to_i32(p, _OP_POSITIVE), conn)
    t_labels, N = _ccl(_to_i32(t, _OP_POSITIVE), conn)
    h = _overlap(t_labels, p_labels, N, M).cpu().to(torch.float32)

    hits_t = detection_test(h, **params)
    hits_p = detection_test(h.T, **params)
    recall_det = hits_t.sum() / N
    precision_det = hits_p.sum() / M
    TP, FP, TN, FN = h[1:, 1:].sum(), h[0, 1:].sum(), h[0, 0].sum(), h[1:, 0].sum()
    stats = {
        'target_components': N, 'predicted_components': M,
        'target_detections': hits_t.sum(), 'predicted_detections': hits_p.sum(),
        'detection_recall': recall_det, 'detection_precision': precision_det,
        'detection_f1': 2 * (recall_det * precision_det) / (recall_det + precision_det),
        'target_volume': TP + FN, 'prediction_volume': TP + FP,
        'TP': TP, 'FP': FP, 'TN': TN, 'FN': FN,
        'dice': 2 * TP / (2 * TP + FP + FN), 'jaccard': TP / (TP + FP + FN),
        'precision': TP / (TP + FP), 'recall': TP / (TP + FN),
    }
    return {k: _item(stats[k]) for k in STAT_NAMES}


# ---------------------------------------------------------------------------------------------- labelled tables
def _listify(key):
    if isinstance(key, (list, tuple)):
        return list(key)
    return [key]


class LabeledTensor:
    """A float32 host tensor whose dimensions are addressed by name (labeled_tensor.py, reference).  Keys: a string
    (looked up in its dimension; a name given twice in a dimension addresses its last position), a list of keys, an
    int or a slice, per dimension.  Ellipsis is refused."""

    def __init__(self, dim_names: Sequence[str], dim_keys: Sequence[Sequence[str]]):
        if len(dim_names) != len(dim_keys):
            raise ValueError(f"The number of dimension names ({len(dim_names)}) "
                             f"does not match the number of dimension keys ({len(dim_keys)}")
        self.dim_names = dim_names
        self.dim_keys = dim_keys
        self.dim_key_map = [dict((k, i) for i, k in enumerate(keys)) for keys in dim_keys]
        self.data = torch.zeros([len(keys) for keys in dim_keys])

    def parse_key(self, key):
        parts = _listify(key)
        if any(k is Ellipsis for k in parts):
            raise NotImplementedError("Elipsis indexing is not supported for LabeledTensors")
        out = []
        for k, lookup in zip(parts, self.dim_key_map):
            if isinstance(k, str):
                k = lookup[k]
            elif isinstance(k, (list, tuple)):
                k = [lookup[e] if isinstance(e, str) else e for e in k]
            out.append(k)
        return tuple(out) + tuple(parts[len(out):])

    def __getitem__(self, key) -> torch.Tensor:
        return self.data[self.parse_key(key)]

    def __setitem__(self, key, value):
        self.data[self.parse_key(key)] = value

    def to_dataframe(self):
        """one row per combination of the leading dimensions' keys, one column per key of the last dimension"""
        import pandas as pd
        lead, last = self.dim_names[:-1], self.dim_keys[-1]
        columns = {name: [] for name in lead}
        for k in last:
            columns[k] = []
        for combo in itertools.product(*self.dim_keys[:-1]):
            for name, k in zip(lead, combo):
                columns[name].append(k)
            for k, v in zip(last, self[combo].tolist()):
                columns[k].append(v)
        return pd.DataFrame(columns)

    def to_dict(self):
        out = {}
        for combo in itertools.product(*self.dim_keys):
            node = out
            for k in combo[:-1]:
                node = node.setdefault(k, {})
            node[combo[-1]] = self[combo].item()
        return _fill_nested(self.dim_keys, out)

    def compute_summary_stats(self, summary_stats_to_output):
        funcs = LabeledTensor.get_summary_stat_funcs()
        out = LabeledTensor(dim_names=["summary_stat", *self.dim_names[1:]],
                            dim_keys=[summary_stats_to_output, *self.dim_keys[1:]])
        for combo in itertools.product(*self.dim_keys[1:]):
            column = self[(slice(None), *combo)]
            for name in summary_stats_to_output:
                out[(name, *combo)] = funcs[name](column).item()
        return out

    @staticmethod
    def fix_tensor(x):
        """the finite values of x, or [0.] when there are none"""
        finite = x[x.isfinite()]
        return finite if finite.shape[0] else torch.tensor([0.])

    @staticmethod
    def get_summary_stat_funcs(dim: int = 0):
        fix = LabeledTensor.fix_tensor
        return {
            'mean': lambda x: torch.mean(fix(x), dim=dim),
            'median': lambda x: torch.median(fix(x), dim=dim).values,
            'mode': lambda x: torch.mode(fix(x), dim=dim).values,
            'std': lambda x: torch.std(fix(x), dim=dim),
            'min': lambda x: torch.min(fix(x), dim=dim).values,
            'max': lambda x: torch.max(fix(x), dim=dim).values,
        }


def _fill_nested(dim_keys, filled):
    """to_dict's layout: every key of every level present (the reference builds the nest first, then fills it)"""
    def build(level):
        if level == len(dim_keys):
            return 0
        return {k: build(level + 1) for k in dim_keys[level]}

    def merge(skeleton, values):
        for k, v in values.items():
            if isinstance(v, dict):
                merge(skeleton[k], v)
            else:
                skeleton[k] = v
        return skeleton
    return merge(build(0), filled)


# ---------------------------------------------------------------------------------------------- subjects
class LabelMap(dict):
    """The part of a torchio LabelMap the evaluators read: `.data` ([1, D, H, W]) and item access to attributes such
    as 'label_values'.  A real tio.LabelMap works in its place."""

    def __init__(self, data=None, label_values=None, **attributes):
        super().__init__(attributes)
        if data is not None:
            self['data'] = data
        if label_values is not None:
            self['label_values'] = dict(label_values)

    @property
    def data(self):
        return self['data']


class ScoreLabelMap(LabelMap):
    """A label map that is the argmax of model scores through a channel -> label value table (prediction.
    add_evaluation_labels).  Its `.data` (int64 [1, D, H, W]) is computed on first access; an evaluator given such
    maps counts straight from the scores instead (ops.eval_scores), without writing them."""

    def __init__(self, source, role, label_values=None):
        super().__init__(None, label_values)
        self.source, self.role = source, role

    @property
    def data(self):
        if 'data' not in self:
            self.source.materialise()
        return self['data']

    @property
    def pending(self):
        return 'data' not in self


class Evaluator:
    def __call__(self, subjects) -> dict:
        raise NotImplementedError()

    def __repr__(self):
        args = ", ".join(f"{k}={v!r}" for k, v in vars(self).items() if not k.startswith("_"))
        return f"{type(self).__name__}({args})"


def _fused_sources(subjects, pred_name, target_name):
    """the ScoreLabelMap sources when every prediction (and target) can be counted straight from scores, else None"""
    preds = [s[pred_name] for s in subjects]
    if not all(isinstance(p, ScoreLabelMap) and p.pending and p.role == "pred" for p in preds):
        return None
    sources = [p.source for p in preds]
    if any(src.plan is not sources[0].plan for src in sources):
        return None
    if target_name is None:
        return sources, None
    targets = [s[target_name] for s in subjects]
    own = [isinstance(t, ScoreLabelMap) and t.pending and t.role == "target" and t.source is src
           for t, src in zip(targets, sources)]
    if all(own):
        return sources, "own"
    if any(own):
        return None
    return sources, [t.data for t in targets]


def label_counts(subjects, pred_name, target_name, values):
    """int64 numpy [n, L, 3] (TP, FP, FN) per subject and label value, and the voxel count of each subject: one launch
    (ops.eval_scores when the predictions are unwritten ScoreLabelMaps, ops.eval_confusion otherwise), one copy back."""
    uniq = list(dict.fromkeys(int(v) for v in values))
    fused = _fused_sources(subjects, pred_name, target_name)
    if fused is not None:
        sources, tmode = fused
        plan = sources[0].plan
        targets = None
        if tmode == "own":
            targets = [src.target for src in sources]
        elif tmode is not None:
            targets = tmode
        counts, _, _ = ops.eval_scores([src.scores for src in sources], plan.tables(sources[0].scores.shape[0]), uniq, targets=targets,
                                       masks=[src.mask for src in sources] if plan.mask_name is not None else None,
                                       half=plan.half, one_hot_targets=tmode == "own")
        sizes = [src.scores[0].numel() for src in sources]
    else:
        preds = [s[pred_name].data for s in subjects]
        targets = [s[target_name].data for s in subjects] if target_name is not None else [None] * len(preds)
        dev = next((t.device for t in preds if t.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())
        counts = ops.eval_confusion([p.to(dev) for p in preds], [None if t is None else t.to(dev) for t in targets], uniq)
        sizes = [p.numel() for p in preds]
    counts = counts.cpu().numpy()
    pos = {v: i for i, v in enumerate(uniq)}
    return counts[:, [pos[int(v)] for v in values], :], np.asarray(sizes, dtype=np.int64)


def _subject_table(subjects, stats_to_output, second_keys):
    subject_names = [subject['name'] for subject in subjects]
    return LabeledTensor(dim_names=['subject', 'label', 'stat'], dim_keys=[subject_names, second_keys, stats_to_output])


def _finish(subject_stats, summary_stats_to_output):
    return {'subject_stats': subject_stats.to_dataframe(),
            'summary_stats': subject_stats.compute_summary_stats(summary_stats_to_output)}


class SegmentationEvaluator(Evaluator):
    """Overlap statistics of a predicted against a target label map per subject and label (segmentation_evaluator.py,
    reference): 'target_volume', 'prediction_volume', 'TP', 'FP', 'TN', 'FN', 'dice', 'jaccard', 'precision',
    'recall', and their summary stats over the subjects.  The counts come from one device launch; the statistics are
    the reference's float32 expressions on them (0 / 0 is nan, x / 0 inf)."""

    def __init__(self, prediction_label_map_name: str, target_label_map_name: str,
                 stats_to_output: Sequence[str] = ('target_volume', 'prediction_volume',
                                                   'TP', 'FP', 'TN', 'FN', 'dice', 'precision', 'recall'),
                 summary_stats_to_output: Sequence[str] = ('mean', 'std', 'min', 'max')):
        self.prediction_label_map_name = prediction_label_map_name
        self.target_label_map_name = target_label_map_name
        self.stats_to_output = stats_to_output
        self.summary_stats_to_output = summary_stats_to_output

    @staticmethod
    def _stats(tp, fp, fn, size):
        TP, FP, FN = (torch.tensor([v], dtype=torch.int64).float() for v in (tp, fp, fn))
        TN = torch.tensor([size - tp - fp - fn], dtype=torch.int64).float()
        return {'target_volume': TP + FN, 'prediction_volume': TP + FP, 'TP': TP, 'FP': FP, 'TN': TN, 'FN': FN,
                'dice': 2 * TP / (2 * TP + FP + FN), 'jaccard': TP / (TP + FP + FN),
                'precision': TP / (TP + FP), 'recall': TP / (TP + FN)}

    def __call__(self, subjects):
        label_values = subjects[0][self.prediction_label_map_name]['label_values']
        table = _subject_table(subjects, self.stats_to_output, list(label_values.keys()))
        counts, sizes = label_counts(subjects, self.prediction_label_map_name, self.target_label_map_name,
                                     list(label_values.values()))
        for i, subject in enumerate(subjects):
            for l, label_name in enumerate(label_values):
                tp, fp, fn = (int(v) for v in counts[i, l])
                stats = self._stats(tp, fp, fn, int(sizes[i]))
                for stat_name in self.stats_to_output:
                    table[subject['name'], label_name, stat_name] = stats[stat_name].item()
        return _finish(table, self.summary_stats_to_output)


class MultiLabelEvaluator(Evaluator):
    """SegmentationEvaluator's statistics for a sigmoid head: per subject and channel, `scores > threshold` against
    `target != 0`, every channel a binary problem of its own (a voxel may carry several labels or none).
    subject[prediction_name] / subject[target_name]: images with `.data` (ScalarImage, LabelMap) or bare tensors
    [C, W, H, D]; scores float32 / bfloat16 / float16, targets of any evaluation element type.  `threshold`: a float or
    one per channel.  The label keys are `channel_names` (default "0" .. "C-1"), 'size' of the statistics is the voxels
    of one channel.  One ops.eval_multilabel launch for all subjects and one copy back; the output has the layout of
    SegmentationEvaluator's, so the same scoring functions read it."""

    def __init__(self, prediction_name: str, target_name: str, channel_names: Optional[Sequence[str]] = None,
                 threshold=0.5,
                 stats_to_output: Sequence[str] = ('target_volume', 'prediction_volume',
                                                   'TP', 'FP', 'TN', 'FN', 'dice', 'precision', 'recall'),
                 summary_stats_to_output: Sequence[str] = ('mean', 'std', 'min', 'max')):
        self.prediction_name = prediction_name
        self.target_name = target_name
        self.channel_names = channel_names
        self.threshold = threshold
        self.stats_to_output = stats_to_output
        self.summary_stats_to_output = summary_stats_to_output

    @staticmethod
    def _data(image):
        return image if torch.is_tensor(image) else image.data

    def _channel_names(self, channels):
        if self.channel_names is None:
            return [str(c) for c in range(channels)]
        if len(self.channel_names) != channels:
            raise M355Error(f"{len(self.channel_names)} channel names {list(self.channel_names)} for {channels} channels")
        return list(self.channel_names)

    def __call__(self, subjects):
        scores = [self._data(s[self.prediction_name]) for s in subjects]
        targets = [self._data(s[self.target_name]) for s in subjects]
        dev = next((t.device for t in scores if t.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())
        names = self._channel_names(scores[0].shape[0])
        table = _subject_table(subjects, self.stats_to_output, names)
        counts = ops.eval_multilabel([s.to(dev) for s in scores], [t.to(dev) for t in targets], self.threshold).cpu().numpy()
        for i, subject in enumerate(subjects):
            size = scores[i][0].numel()
            for c, name in enumerate(names):
                tp, fp, fn = (int(v) for v in counts[i, c])
                stats = SegmentationEvaluator._stats(tp, fp, fn, size)
                for stat_name in self.stats_to_output:
                    table[subject['name'], name, stat_name] = stats[stat_name].item()
        return _finish(table, self.summary_stats_to_output)


def calibration_stats(table, bins_total=None):
    """ece, mce, confidence, accuracy and the per-bin (count, accuracy, confidence) of one reliability table: `table`
    int [B, 3] of (count, hits, conf_sum in 2^-32 fixed point), Python fp64 from the integers.  ece = sum_b (n_b / n)
    |acc_b - conf_b| over the non-empty bins, mce the largest gap; an empty table gives NaN."""
    rows = [(int(c), int(h), int(f)) for c, h, f in table]
    n = sum(c for c, _, _ in rows)
    per_bin = [(c, h / c, f / 4294967296.0 / c) if c else (0, float('nan'), float('nan')) for c, h, f in rows]
    if n == 0:
        nan = float('nan')
        return {'ece': nan, 'mce': nan, 'confidence': nan, 'accuracy': nan}, per_bin
    gaps = [(c, abs(a - q)) for c, a, q in per_bin if c]
    return {'ece': sum(c / n * g for c, g in gaps), 'mce': max(g for _, g in gaps),
            'confidence': sum(f for _, _, f in rows) / 4294967296.0 / n, 'accuracy': sum(h for _, h, _ in rows) / n}, per_bin


class CalibrationEvaluator(Evaluator):
    """Can the probabilities be trusted?  Per subject: expected and maximum calibration error ('ece', 'mce'), mean
    'confidence' and 'accuracy', Brier score and negative log-likelihood ('brier', 'nll'), and the reliability table.
    subject[prediction_name]: probabilities [C, W, H, D] (an image with `.data` or a bare tensor; float32 / bfloat16 /
    float16); subject[target_name]: a one-hot or soft map of the same shape, or a map of channel indices ([W, H, D] or
    [1, W, H, D], an integer type).  kind 'categorical' (softmax head): the label keys are 'top' (the top-label table:
    confidence = the largest probability, hit = it is the target's class) followed by `channel_names` (default "0" ..
    "C-1"), whose rows hold the classwise statistics (confidence = p_c, hit = the target is positive in c); 'binary'
    (sigmoid head): the channel rows only, every channel a problem of its own.  'brier' and 'nll' are the subject's sums
    over all channels divided by its valid voxels (binary: by its valid (voxel, channel) pairs) and stand in every row
    of the subject.  A subject with no valid voxel gets NaN.  One ops.eval_calibration call and one copy back; the
    statistics are Python fp64 on the integers.  The output has SegmentationEvaluator's layout ('subject_stats',
    'summary_stats') and also 'reliability': a LabeledTensor [subject, label, bin, {count, accuracy, confidence}]
    (float64; empty bins NaN)."""

    def __init__(self, prediction_name: str, target_name: str, channel_names: Optional[Sequence[str]] = None,
                 bins: int = 15, kind: str = 'categorical',
                 stats_to_output: Sequence[str] = ('ece', 'mce', 'brier', 'nll', 'confidence', 'accuracy'),
                 summary_stats_to_output: Sequence[str] = ('mean', 'std', 'min', 'max')):
        if kind not in ('categorical', 'binary'):
            raise ValueError(f"kind must be 'categorical' or 'binary', not {kind!r}")
        self.prediction_name = prediction_name
        self.target_name = target_name
        self.channel_names = channel_names
        self.bins = bins
        self.kind = kind
        self.stats_to_output = stats_to_output
        self.summary_stats_to_output = summary_stats_to_output

    _data = staticmethod(MultiLabelEvaluator._data)
    _channel_names = MultiLabelEvaluator._channel_names

    def __call__(self, subjects):
        scores = [self._data(s[self.prediction_name]) for s in subjects]
        targets = [self._data(s[self.target_name]) for s in subjects]
        dev = next((t.device for t in scores if t.is_cuda), None)
        if dev is None and torch.cuda.is_available():      # (without a device the op itself refuses host tensors)
            dev = torch.device("cuda", torch.cuda.current_device())
        channels, n = scores[0].shape[0], len(subjects)
        names = (['top'] if self.kind == 'categorical' else []) + self._channel_names(channels)
        table = _subject_table(subjects, self.stats_to_output, names)
        reliability = LabeledTensor(dim_names=['subject', 'label', 'bin', 'stat'],
                                    dim_keys=[[s['name'] for s in subjects], names, [str(b) for b in range(self.bins)],
                                              ['count', 'accuracy', 'confidence']])
        reliability.data = reliability.data.double()
        device_counts = ops.eval_calibration([s.to(dev) for s in scores], [t.to(dev) for t in targets], self.bins, self.kind)
        counts = ops.CalibrationCounts.unpack(device_counts.packed.cpu(), n, channels, self.bins, self.kind)
        top, classwise = counts.top.numpy(), counts.classwise.numpy()
        for i, subject in enumerate(subjects):
            tables = ([top[i]] if self.kind == 'categorical' else []) + [classwise[i, c] for c in range(channels)]
            valid = int(top[i, :, 0].sum()) if self.kind == 'categorical' else int(classwise[i, :, :, 0].sum())
            sums = {'brier': counts.brier[i].item() / valid, 'nll': counts.nll[i].item() / valid} if valid else \
                {'brier': float('nan'), 'nll': float('nan')}
            for l, name in enumerate(names):
                stats, per_bin = calibration_stats(tables[l])
                stats.update(sums)
                for stat_name in self.stats_to_output:
                    table[subject['name'], name, stat_name] = stats[stat_name]
                reliability.data[i, l] = torch.tensor(per_bin, dtype=torch.float64)
        return dict(_finish(table, self.summary_stats_to_output), reliability=reliability)


CURVE_STATS = ('error', 'absolute_error', 'squared_error', 'percent_diff')


class LabelMapEvaluator(Evaluator):
    """Volume of every label per subject (label_map_evaluator.py, reference), and with `curve_params` (label name ->
    polynomial coefficients, highest power first) and `curve_attribute` (a subject key, e.g. 'age') the deviation from
    the curve: 'error', 'absolute_error', 'squared_error', 'percent_diff'.  Volumes come from one device launch."""

    def __init__(self, label_map_name: str, curve_params: Optional[Dict[str, np.ndarray]] = None,
                 curve_attribute: Optional[str] = None, stats_to_output: Sequence[str] = ('volume',),
                 summary_stats_to_output: Sequence[str] = ('mean', 'std', 'min', 'max')):
        self.label_map_name = label_map_name
        self.curve_params = curve_params
        self.curve_attribute = curve_attribute
        self.stats_to_output = stats_to_output
        self.summary_stats_to_output = summary_stats_to_output
        if any(stat in CURVE_STATS for stat in stats_to_output):
            if curve_params is None:
                raise ValueError("curve_params must be provided")
            if curve_attribute is None:
                raise ValueError("curve_attribute must be provided")
        self.poly_func = None
        if curve_params is not None and curve_attribute is not None:
            self.poly_func = {label: np.poly1d(param) for label, param in curve_params.items()}

    def __call__(self, subjects):
        label_values = subjects[0][self.label_map_name]['label_values']
        table = _subject_table(subjects, self.stats_to_output, list(label_values.keys()))
        counts, _ = label_counts(subjects, self.label_map_name, None, list(label_values.values()))
        for i, subject in enumerate(subjects):
            for l, label_name in enumerate(label_values):
                volume = torch.tensor([int(counts[i, l, 0] + counts[i, l, 1])], dtype=torch.int64)
                stats = {'volume': volume}
                if self.poly_func is not None:
                    expected = self.poly_func[label_name](subject[self.curve_attribute])
                    error = volume - expected
                    stats.update({'error': error, 'absolute_error': abs(error), 'squared_error': error ** 2,
                                  'percent_diff': (error / expected) * 100})
                for stat_name in self.stats_to_output:
                    table[subject['name'], label_name, stat_name] = stats[stat_name].item()
        return _finish(table, self.summary_stats_to_output)


IMAGE_REGION_STAT_NAMES = ops.REGION_STATS + ('volume',)


def _device_tensors(tensors):
    """the tensors on one device: that of the first device tensor among them, else the current device when there is one
    (host tensors are then uploaded); without any device they stay where they are and the op refuses them"""
    dev = next((t.device for t in tensors if t.is_cuda), None)
    if dev is None and torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    return list(tensors) if dev is None else [t.to(dev) for t in tensors]


class ImageRegionEvaluator(Evaluator):
    """Summary statistics of images inside the mask of every label per subject (image_region_evaluator.py, reference,
    which declares the table and stops): a ['subject', 'label', 'image_name', 'stat'] table with 'mean', 'std'
    (unbiased), 'median' (torch.median's lower middle value), 'min', 'max' of the image's values where
    `label map == label value`, the channels of an image pooled, and 'volume', the voxels of the label (the same for
    every image).  An absent label has volume 0 and NaN statistics; a one-voxel label has std NaN.  Label names and
    values come from subjects[0][label_map_name]['label_values'].  The images are read as they are: an intensity
    normalisation applied before the evaluation is not inverted.  One ops.region_stats call for all subjects, labels
    and images, and one device -> host copy."""

    def __init__(self, label_map_name: str, image_names: Sequence[str], stats_to_output: Sequence[str] = None,
                 summary_stats_to_output: Sequence[str] = None):
        self.label_map_name = label_map_name
        self.image_names = image_names
        self.stats_to_output = IMAGE_REGION_STAT_NAMES if stats_to_output is None else stats_to_output
        self.summary_stats_to_output = ('mean', 'std', 'min', 'max') if summary_stats_to_output is None \
            else summary_stats_to_output
        unknown = [s for s in self.stats_to_output if s not in IMAGE_REGION_STAT_NAMES]
        if unknown:
            raise M355Error(f"unknown image region stats {unknown} (known: {', '.join(IMAGE_REGION_STAT_NAMES)})")

    def __call__(self, subjects):
        label_values = subjects[0][self.label_map_name]['label_values']
        label_names = list(label_values.keys())
        image_names = list(self.image_names)
        subject_stats = LabeledTensor(dim_names=['subject', 'label', 'image_name', 'stat'],
                                      dim_keys=[[subject['name'] for subject in subjects], label_names, image_names,
                                                list(self.stats_to_output)])
        labels, images = [], []
        for subject in subjects:
            tensors = _device_tensors([subject[self.label_map_name].data] + [subject[name].data for name in image_names])
            labels.append(tensors[0])
            images.append(tensors[1:])
        need_median = 'median' in self.stats_to_output
        res = ops.region_stats(labels, images, [int(v) for v in label_values.values()], median=need_median)
        L = len(label_names)
        for j, stat_name in enumerate(self.stats_to_output):
            if stat_name == 'volume':
                subject_stats.data[..., j] = res.count[:, :L, None].float()
            else:
                subject_stats.data[..., j] = res.stats[:, :L, :, ops.REGION_STATS.index(stat_name)]
        return _finish(subject_stats, self.summary_stats_to_output)


class InstanceSegmentationEvaluator(Evaluator):
    """Lesion-wise detection and overlap statistics per subject (instance_segmentation_evaluator.py, reference), from
    `instance_segmentation_stats` (components and overlap table on the device); a ['subject', 'stat'] table."""

    def __init__(self, prediction_label_map_name: str, target_label_map_name: str,
                 stats_to_output: Sequence[str] = STAT_NAMES,
                 summary_stats_to_output: Sequence[str] = ('mean', 'std', 'min', 'max', 'median', 'mode'),
                 connectivity: int = 2, detection_test: Callable = msseg_detection_test,
                 detection_test_params: Optional[Dict] = None):
        self.prediction_label_map_name = prediction_label_map_name
        self.target_label_map_name = target_label_map_name
        self.stats_to_output = stats_to_output
        self.summary_stats_to_output = summary_stats_to_output
        self.connectivity = connectivity
        self.detection_test = detection_test
        self.detection_test_params = {} if detection_test_params is None else detection_test_params

    def __call__(self, subjects):
        table = LabeledTensor(dim_names=['subject', 'stat'],
                              dim_keys=[[s['name'] for s in subjects], self.stats_to_output])
        for subject in subjects:
            stats = instance_segmentation_stats(subject[self.prediction_label_map_name].data,
                                                subject[self.target_label_map_name].data, self.connectivity,
                                                self.detection_test, self.detection_test_params)
            for stat_name in self.stats_to_output:
                table[subject['name'], stat_name] = stats[stat_name]
        return _finish(table, self.summary_stats_to_output)


# ---------------------------------------------------------------------------------------------- surface distances
SURFACE_STAT_NAMES = ('hd', 'hd95', 'assd', 'asd_pred_to_target', 'asd_target_to_pred', 'nsd', 'pred_surface',
                      'target_surface')
_SURFACE_DEVICE_STATS = 6   # the first six are taken on the device; the two surface sizes are the counts themselves


def _volume3(data):
    """a label map's data ([1, W, H, D] or [W, H, D]; numpy or tensor) as a contiguous integer device volume [W, H, D]"""
    if getattr(data, "ndim", 0) == 4:
        if data.shape[0] != 1:
            raise M355Error(f"surface distances: a label map of shape {tuple(data.shape)}; expected [1, W, H, D]")
        data = data[0]
    return _device_volume(data)[0]


def _to_i32_unchecked(t, status):
    """_to_i32 without the read-back: `status` (a device int32 slot) is left for the caller to look at"""
    out = torch.empty(t.shape, dtype=torch.int32, device=t.device)
    check(_lib.lib().m355_label_convert_in(ops._p(t), _DTYPE_CODE[t.dtype], _OP_COPY, ops._p(out), t.numel(),
                                           ops._p(status), ops._stream()), "label_convert_in")
    return out


def _surface_table(pairs, values, spacings, percentile, tolerance):
    """float64 numpy [n, L, 8] in the order of SURFACE_STAT_NAMES for the (prediction, target) volumes `pairs`, the int
    label values `values` and one spacing triple per subject.  Two passes over the subjects, so device memory holds one
    subject's volumes at a time: the first only counts the border voxels (one copy to the host sizes the pooled gather
    buffer exactly), the second converts and masks again -- both cheap next to the transforms -- and fills the buffer.
    At most two device -> host copies, whatever n and L."""
    n, L = len(pairs), len(values)
    if not 0.0 <= float(percentile) <= 100.0:
        raise M355Error(f"percentile {percentile!r} (0 .. 100)")
    for i, (p, t) in enumerate(pairs):
        if p.shape != t.shape or p.device != t.device:
            raise M355Error(f"surface distances: subject {i}: prediction {tuple(p.shape)} on {p.device}, target "
                            f"{tuple(t.shape)} on {t.device}")
    dev = pairs[0][0].device
    out = np.full((n, L, len(SURFACE_STAT_NAMES)), np.nan)
    with torch.cuda.device(dev):
        head = torch.zeros(2 * n * L + 2 * n, dtype=torch.int32, device=dev)   # border counts [n, L, 2], cast flags [n, 2]
        max_vox = max(p.numel() for p, _ in pairs)
        borders = torch.empty((2, max_vox), dtype=torch.uint8, device=dev)

        def masks(l, counts):
            """the borders of label l in the current subject's two int32 volumes, into the scratch; counts: two int32 slots"""
            made = []
            for side, x in enumerate(converted):
                b = borders[side, :x.numel()].view(x.shape)
                ops.surface_mask(x, values[l], border=b, count=counts[side:side + 1])
                made.append(b)
            return made

        for i, (p, t) in enumerate(pairs):
            at = 2 * n * L + 2 * i
            converted = [_to_i32_unchecked(p, head[at:at + 1]), _to_i32_unchecked(t, head[at + 1:at + 2])]
            for l in range(L):
                masks(l, head[2 * (i * L + l):2 * (i * L + l) + 2])
        host = head.cpu().numpy()                                             # copy 1
        if host[2 * n * L:].any():
            raise M355Error("label values must fit int32")
        counts = host[:2 * n * L].reshape(n, L, 2).astype(np.int64)
        out[:, :, 6:] = counts
        todo = [(i, l) for i in range(n) for l in range(L) if counts[i, l].min() > 0]
        if not todo:
            return out
        offsets, total = {}, 0
        for i, l in todo:
            offsets[(i, l)] = total
            total += int(counts[i, l].sum())
        pool = torch.empty(total, dtype=torch.float32, device=dev)
        cursors = torch.zeros(2 * len(todo), dtype=torch.int32, device=dev)
        junk = torch.zeros(2, dtype=torch.int32, device=dev)
        table = torch.empty((len(todo), _SURFACE_DEVICE_STATS), dtype=torch.float64, device=dev)
        d2 = torch.empty(max_vox, dtype=torch.float32, device=dev)
        workspace = None
        last = -1
        for k, (i, l) in enumerate(todo):
            if i != last:
                p, t = pairs[i]
                converted = [_to_i32_unchecked(p, junk[0:1]), _to_i32_unchecked(t, junk[1:2])]
                size3 = (ctypes.c_int32 * 3)(*p.shape)
                workspace = torch.empty(max(int(_lib.lib().m355_edt_workspace(size3)), 16), dtype=torch.uint8, device=dev)
                last = i
            border_p, border_t = masks(l, junk)
            n_p, n_t = int(counts[i, l, 0]), int(counts[i, l, 1])
            a = pool[offsets[(i, l)]:offsets[(i, l)] + n_p]
            b = pool[offsets[(i, l)] + n_p:offsets[(i, l)] + n_p + n_t]
            dist = d2[:p.numel()].view(p.shape)
            ops.edt_sq(border_t, spacings[i], out=dist, workspace=workspace)
            ops.surface_gather(border_p, dist, a, cursors[2 * k:2 * k + 1])
            ops.edt_sq(border_p, spacings[i], out=dist, workspace=workspace)
            ops.surface_gather(border_t, dist, b, cursors[2 * k + 1:2 * k + 2])
            # the gather order is not specified: every sum below runs over a sorted segment, so the bits repeat
            mean_a = torch.sort(a).values.double().sum() / n_p
            mean_b = torch.sort(b).values.double().sum() / n_t
            both = torch.sort(pool[offsets[(i, l)]:offsets[(i, l)] + n_p + n_t]).values.double()
            rank = float(percentile) / 100.0 * (n_p + n_t - 1)
            lo = min(int(np.floor(rank)), n_p + n_t - 1)
            hi = min(lo + 1, n_p + n_t - 1)
            table[k] = torch.stack([both[-1], both[lo] + (both[hi] - both[lo]) * (rank - lo), (mean_a + mean_b) / 2,
                                    mean_a, mean_b, (both <= float(tolerance)).sum().double() / (n_p + n_t)])
        table = table.cpu().numpy()                                           # copy 2
    for k, (i, l) in enumerate(todo):
        out[i, l, :_SURFACE_DEVICE_STATS] = table[k]
    return out


def _image_spacing(image, override):
    if override is not None:
        return ops._spacing3(override)
    spacing = getattr(image, "spacing", None)
    if spacing is None and isinstance(image, Mapping) and "spacing" in image:
        spacing = image["spacing"]
    return (1.0, 1.0, 1.0) if spacing is None else ops._spacing3(spacing)


def surface_distances(pred, target, label_values, spacing=(1, 1, 1), percentile=95, tolerance=1.0):
    """Surface distances of one prediction / target pair of label maps ([W, H, D] or [1, W, H, D]; numpy or tensors) for
    every entry of `label_values` ({label name: value}): {label name: {stat: float}} with the eight statistics of
    SURFACE_STAT_NAMES, defined under SurfaceDistanceEvaluator.  The functional form of that evaluator for one subject:
    the same launches and the same two copies."""
    p, t = _volume3(pred), _volume3(target)
    table = _surface_table([(p, t.to(p.device))], [int(v) for v in label_values.values()], [ops._spacing3(spacing)],
                           percentile, tolerance)
    return {name: {stat: float(table[0, l, s]) for s, stat in enumerate(SURFACE_STAT_NAMES)}
            for l, name in enumerate(label_values)}


class SurfaceDistanceEvaluator(Evaluator):
    """Boundary statistics of a predicted against a target label map per subject and label, in SegmentationEvaluator's
    output layout (so ScheduledEvaluation, the loggers and the scoring functions read it unchanged).  With dP and dT the
    borders of `pred == value` and `target == value` -- the voxels of the label that lie on a face of the volume or have
    a six-neighbour outside the label: mask ^ binary_erosion(mask), border_value 0 -- and the multisets
    A = {d(p, dT) : p in dP}, B = {d(t, dP) : t in dT} of Euclidean distances in units of `spacing` (the medpy
    conventions):
      'hd'                  max(A u B), the Hausdorff distance
      'hd95'                numpy.percentile(A + B, percentile), linear interpolation (the key keeps its name for any
                            percentile)
      'asd_pred_to_target'  mean(A);  'asd_target_to_pred'  mean(B)
      'assd'                the mean of those two means
      'nsd'                 (#{a <= tolerance} + #{b <= tolerance}) / (|A| + |B|): a surface Dice over border VOXELS, not
                            the area-weighted one of the surface-distance literature
      'pred_surface'        |A|;  'target_surface'  |B|
    When either border is empty (the label is absent from a map) every distance statistic and 'nsd' is nan.

    `spacing`: the constructor's argument, else the prediction image's `.spacing` (torchio), else its 'spacing' key, else
    1.  Label names and values come from subjects[0][prediction_label_map_name]['label_values']; predictions are read
    through `.data`, so a pending ScoreLabelMap writes itself.  Distances are fp32 (exact squares for unit spacing,
    correctly rounded roots), the order statistics and fp64 means are taken on the device over sorted segments:
    results repeat bit for bit.  Two device -> host copies per call whatever the number of subjects and labels: the
    border counts, then the table."""

    def __init__(self, prediction_label_map_name: str, target_label_map_name: str, spacing=None, percentile=95,
                 tolerance=1.0, stats_to_output: Sequence[str] = ('hd', 'hd95', 'assd'),
                 summary_stats_to_output: Sequence[str] = ('mean', 'std', 'min', 'max')):
        unknown = [s for s in stats_to_output if s not in SURFACE_STAT_NAMES]
        if unknown:
            raise M355Error(f"unknown surface distance stats {unknown} (known: {', '.join(SURFACE_STAT_NAMES)})")
        self.prediction_label_map_name = prediction_label_map_name
        self.target_label_map_name = target_label_map_name
        self.spacing = spacing
        self.percentile = percentile
        self.tolerance = tolerance
        self.stats_to_output = stats_to_output
        self.summary_stats_to_output = summary_stats_to_output

    def __call__(self, subjects):
        label_values = subjects[0][self.prediction_label_map_name]['label_values']
        table = _subject_table(subjects, self.stats_to_output, list(label_values.keys()))
        pairs, spacings = [], []
        for subject in subjects:
            image = subject[self.prediction_label_map_name]
            p = _volume3(image.data)
            pairs.append((p, _volume3(subject[self.target_label_map_name].data).to(p.device)))
            spacings.append(_image_spacing(image, self.spacing))
        stats = _surface_table(pairs, [int(v) for v in label_values.values()], spacings, self.percentile, self.tolerance)
        for i, subject in enumerate(subjects):
            for l, label_name in enumerate(label_values):
                for stat_name in self.stats_to_output:
                    table[subject['name'], label_name, stat_name] = stats[i, l, SURFACE_STAT_NAMES.index(stat_name)]
        return _finish(table, self.summary_stats_to_output)


# ---------------------------------------------------------------------------------------------- contour images
class ScalarImage(dict):
    """The part of a torchio ScalarImage ContourImageEvaluator reads: `.data` ([C, W, H, D])."""

    def __init__(self, data=None, **attributes):
        super().__init__(attributes)
        if data is not None:
            self['data'] = data

    @property
    def data(self):
        return self['data']


PLANES = ops.PLANES


class _RankCall:
    """The device results of one find_interesting_slices call (ops.slice_rank) shared by its holders: ids and ranked
    counts laid out as the count table, and the number of non-empty slices per (holder, plane) segment."""

    def __init__(self, ids, ranked, nums, segments):
        self.ids, self.ranked, self.nums, self.segments = ids, ranked, nums, segments
        dev = ids.device
        self._offsets = torch.tensor([o for o, _ in segments], dtype=torch.int64, device=dev)
        self._lens = torch.tensor([n for _, n in segments], dtype=torch.int64, device=dev)
        self._host_nums = None
        self._picks = {}

    def host_nums(self):
        if self._host_nums is None:
            self._host_nums = self.nums.cpu().tolist()
        return self._host_nums

    def pick(self, slice_id):
        """int64 device [segments, 2]: get_slice_property of the ids and of the counts at rank `slice_id`, for every
        segment at once (no synchronisation)"""
        if slice_id not in self._picks:
            num = self.nums.to(torch.int64)
            at = self._offsets + torch.clamp(torch.clamp(num - 1, max=slice_id), min=0)
            middle = self._lens // 2
            empty = num == 0
            self._picks[slice_id] = torch.stack([torch.where(empty, middle, self.ids[at].to(torch.int64)),
                                                 torch.where(empty, middle, self.ranked[at].to(torch.int64))], dim=1)
        return self._picks[slice_id]


class _RankedPlanes(Mapping):
    """{'Saggital' | 'Coronal' | 'Axial': ranked device tensor} as the reference's FindInterestingSlice stores it: a
    read-only mapping, so copies, `dict(x)` and iteration all go through `__getitem__`.  The tensors' lengths (the
    slices with foreground) are known on the device only: the first item access copies the lengths of the whole call
    to the host, once.  ContourImageEvaluator reads the padded tables instead."""

    def __init__(self, call, table, first_segment):
        self.call, self.table, self.first_segment = call, table, first_segment

    def __getitem__(self, plane):
        if plane not in PLANES:
            raise KeyError(plane)
        seg = self.first_segment + PLANES.index(plane)
        off, _ = self.call.segments[seg]
        return self.table[off:off + self.call.host_nums()[seg]]

    def __iter__(self):
        return iter(PLANES)

    def __len__(self):
        return len(PLANES)


def _is_one_hot(image):
    return "one_hot" in image and bool(image['one_hot'])


def find_interesting_slices(label_maps):
    """FindInterestingSlice for every holder of `label_maps` (anything with `.data` [C, W, H, D] and item access) in one
    ops.slice_counts and one ops.slice_rank launch: sets image['interesting_slice_ids'] and
    image['interesting_slice_counts'], dicts keyed 'Saggital', 'Coronal', 'Axial' of int32 device tensors -- the
    slices holding foreground (`data[0] != 0`, or argmax over the channels != 0 when image['one_hot']) by voxel
    count descending, and those counts.  Equal counts are ordered by ascending slice id (the reference leaves their
    order to an unstable sort).  Returns the holders."""
    label_maps = list(label_maps)
    if not label_maps:
        return label_maps
    datas = [image.data for image in label_maps]
    dev = next((t.device for t in datas if t.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())
    one_hot = [_is_one_hot(image) for image in label_maps]
    volumes = []
    for i, (t, oh) in enumerate(zip(datas, one_hot)):
        if t.dim() != 4:
            raise ValueError(f"label map {i}: data of shape {tuple(t.shape)}; expected [C, W, H, D]")
        volumes.append((t if oh else t[0]).to(dev))
    counts, layout = ops.slice_counts(volumes, one_hot)
    segments = []
    for off, size3 in layout:
        for dim in size3:
            segments.append((off, dim))
            off += dim
    call = _RankCall(*ops.slice_rank(counts, segments), segments)
    for i, image in enumerate(label_maps):
        image['interesting_slice_ids'] = _RankedPlanes(call, call.ids, 3 * i)
        image['interesting_slice_counts'] = _RankedPlanes(call, call.ranked, 3 * i)
    return label_maps


class FindInterestingSlice:
    """transforms/find_interesting_slice.py of the reference as a callable: FindInterestingSlice()(image) annotates a
    label map holder, FindInterestingSlice()(subject) every label map of a subject dict.  The reference takes the
    subject's `tio.LabelMap`s; here a label map is an evaluators.LabelMap, or any other holder with a tensor `.data`
    and item access that is not a scalar image: not an evaluators.ScalarImage, and when it has a 'type' (every torchio
    image does) that type is 'label'."""

    def __init__(self, **kwargs):
        self.kwargs = kwargs

    @staticmethod
    def _is_label_map(value):
        if isinstance(value, LabelMap):
            return True
        if isinstance(value, ScalarImage) or not isinstance(value, Mapping) or not hasattr(value, "__setitem__"):
            return False
        if not torch.is_tensor(getattr(value, "data", None)):
            return False
        return value.get("type", "label") == "label"

    def __call__(self, image_or_subject):
        if torch.is_tensor(getattr(image_or_subject, "data", None)):
            find_interesting_slices([image_or_subject])
        else:
            find_interesting_slices([v for v in image_or_subject.values() if self._is_label_map(v)])
        return image_or_subject


def render_contours(img, y, y_pred, label_values, scale=0.1, line_width=1.5, legend=False):
    """The drawing of contour_image_evaluator.py:136-172 (reference), call for call: `img` a 2-D array, `y` / `y_pred`
    {label name: bool mask} or None.  Targets are contoured at level 0.5, solid; predictions at 0.95, dashed; colours
    by label id.  Returns a PIL.Image.  matplotlib's backend is whatever the process has chosen."""
    import matplotlib
    import matplotlib.pyplot as plt
    from PIL import Image

    H, W = img.shape
    fig = plt.figure(figsize=tuple(np.array((W, H)) * scale))
    plt.imshow(img, cmap="gray",)
    X_grid, Y_grid = np.meshgrid(np.linspace(0, W - 1, W), np.linspace(0, H - 1, H))
    options = dict(linewidths=line_width, alpha=1.)
    cmap = [None, "r", "g", "b", "y", "c", "m"]
    for name in ("Accent", "Dark2", "Set1", "Set2", "tab20"):
        cmap += list(matplotlib.colormaps[name].colors)
    contours = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if y is not None:
            for label_name, label_id in label_values.items():
                contour = plt.contour(X_grid, Y_grid, y[label_name], levels=[0.5], colors=cmap[label_id:label_id + 1],
                                      **options)
                contours.append(contour)
                if legend:
                    plt.legend([contour.legend_elements()[0][0] for contour in contours], label_values.items(), ncol=3,
                               bbox_to_anchor=(0.5, 0), loc='upper center', fancybox=True)
        if y_pred is not None:
            for label_name, label_id in label_values.items():
                plt.contour(X_grid, Y_grid, y_pred[label_name], levels=[0.95], linestyles="dashed",
                            colors=cmap[label_id:label_id + 1], **options)
    plt.tick_params(which='both', bottom=False, top=False, left=False, labelbottom=False, labelleft=False)
    buf = io.BytesIO()
    fig.savefig(buf, bbox_inches="tight", pad_inches=0.0, facecolor="black")
    buf.seek(0)
    pil_image = Image.open(buf)
    plt.close(fig)
    return pil_image


class ContourImageEvaluator(Evaluator):
    """A slice of every subject's image tiled into one picture, the target's labels contoured solid and the
    prediction's dashed (contour_image_evaluator.py, reference); a PIL.Image, or {subject name: PIL.Image} with
    `split_subjects`.  `plane`: 'Axial', 'Coronal', 'Saggital', 'random' (random.randint per call) or 'interesting'
    (with `interesting_slice`: the plane whose slice at rank `slice_id` holds most foreground in the first subject).
    With `interesting_slice`, `slice_id` is a rank among the slices by foreground voxels (find_interesting_slices).

    The volumes stay on the device: per call the chosen ranks come back in one copy (with `interesting_slice` only)
    and the finished mosaics -- image, target labels, prediction labels -- in another (ops.slice_mosaic)."""

    def __init__(self, plane: str, image_name: str, prediction_label_map_name: str, target_label_map_name: str,
                 slice_id: int, legend: bool, ncol: int, scale: float = 0.1, line_width: float = 1.5,
                 interesting_slice: bool = False, split_subjects: bool = False):
        self.plane = plane
        self.image_name = image_name
        self.prediction_label_map_name = prediction_label_map_name
        self.target_label_map_name = target_label_map_name
        self.slice_id = slice_id
        self.legend = legend
        self.ncol = ncol
        self.scale = scale
        self.line_width = line_width
        self.interesting_slice = interesting_slice
        self.split_subjects = split_subjects

    def _ranked_image(self, subject):
        if self.target_label_map_name in subject:
            return subject[self.target_label_map_name]
        return subject[self.prediction_label_map_name]

    def get_slice_id(self, subject, plane):
        if not self.interesting_slice:
            return self.slice_id, plane
        image = self._ranked_image(subject)
        if 'interesting_slice_ids' not in image:
            image = FindInterestingSlice()(image)
        interesting_slice_ids = image['interesting_slice_ids']
        interesting_slice_counts = image['interesting_slice_counts']
        if plane.lower() == 'interesting':
            count = -1
            for check_plane in ("Axial", "Coronal", "Saggital"):
                new_count = self.get_slice_property(image, interesting_slice_counts, self.slice_id, check_plane)
                if new_count > count:
                    plane = check_plane
                    count = new_count
        return self.get_slice_property(image, interesting_slice_ids, self.slice_id, plane), plane

    def get_slice_property(self, image, slice_property, slice_id, plane):
        _, W, H, D = image.data.shape
        dim = {'Axial': D, 'Coronal': H, 'Saggital': W}[plane]

        if slice_property[plane].shape[0] == 0:
            return dim // 2
        if slice_id >= slice_property[plane].shape[0]:
            return slice_property[plane][-1]
        return slice_property[plane][slice_id]

    def _resolve(self, subjects, plane):
        """[(slice id, plane)] per subject, as get_slice_id gives them subject by subject (the first subject settles
        an 'interesting' plane for all), with one copy from the device for all of them"""
        if not self.interesting_slice:
            return [(self.slice_id, plane)] * len(subjects)
        images = [self._ranked_image(subject) for subject in subjects]
        find_interesting_slices([image for image in images if 'interesting_slice_ids' not in image])
        ours = [isinstance(image['interesting_slice_ids'], _RankedPlanes) for image in images]
        calls = list({id(image['interesting_slice_ids'].call): image['interesting_slice_ids'].call
                      for image, own in zip(images, ours) if own}.values())
        rows, base = {}, 0
        if calls:
            picked = torch.cat([call.pick(self.slice_id) for call in calls]).cpu().tolist()
            for call in calls:
                rows[id(call)] = picked[base:base + len(call.segments)]
                base += len(call.segments)
        out = []
        for subject, image, own in zip(subjects, images, ours):
            if not own:   # ranks another FindInterestingSlice stored: the reference's own path
                slice_id, plane = self.get_slice_id(subject, plane)
                out.append((int(slice_id), plane))
                continue
            ranked = image['interesting_slice_ids']
            by_plane = dict(zip(PLANES, rows[id(ranked.call)][ranked.first_segment:ranked.first_segment + 3]))
            if plane.lower() == 'interesting':
                count = -1
                for check_plane in ("Axial", "Coronal", "Saggital"):
                    if by_plane[check_plane][1] > count:
                        plane, count = check_plane, by_plane[check_plane][1]
            out.append((by_plane[plane][0], plane))
        return out

    def _mosaics(self, subjects, resolved, names, impute_shape):
        """the make_grid mosaics of `names` [(image name, pad value)] as host arrays: one launch, one copy"""
        datas = [subject[name].data for name, _ in names for subject in subjects if name in subject]
        dev = next((t.device for t in datas if t.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())
        specs = []
        for name, pad in names:
            tiles = [(subject[name].data[0].to(dev) if name in subject else None, plane, slice_id)
                     for subject, (slice_id, plane) in zip(subjects, resolved)]
            specs.append((tiles, self.ncol, pad, impute_shape))
        outs, buf = ops.slice_mosaic(specs)
        host = buf.cpu()
        arrays = []
        for out in outs:
            start = out.data_ptr() - buf.data_ptr()
            arrays.append(host[start:start + out.numel() * out.element_size()].view(out.dtype).view(out.shape))
        return arrays

    def __call__(self, subjects):
        if not self.split_subjects:
            return self.get_image(subjects)
        return {subject['name']: self.get_image([subject]) for subject in subjects}

    def get_image(self, subjects):
        out_pred = self.prediction_label_map_name is not None and self.prediction_label_map_name in subjects[0]
        out_target = self.target_label_map_name is not None and self.target_label_map_name in subjects[0]
        if out_pred:
            label_values = subjects[0][self.prediction_label_map_name]['label_values']
        if out_target:
            label_values = subjects[0][self.target_label_map_name]['label_values']

        if self.plane.lower() == 'random':
            plane = ("Axial", "Coronal", "Saggital")[random.randint(0, 2)]
        else:
            plane = self.plane

        resolved = self._resolve(subjects, plane)
        plane = resolved[0][1]
        resolved = [(slice_id, plane) for slice_id, _ in resolved]
        impute_shape = ops.slice_shape(subjects[0][self.image_name].data.shape[1:], plane)

        names = [(self.image_name, -1)]
        if out_target:
            names.append((self.target_label_map_name, 0))
        if out_pred:
            names.append((self.prediction_label_map_name, 0))
        arrays = self._mosaics(subjects, resolved, names, impute_shape)
        img, y, y_pred = arrays[0].numpy(), None, None
        if out_target:
            y = {label_name: (arrays[1] == label_value).numpy() for label_name, label_value in label_values.items()}
        if out_pred:
            y_pred = {label_name: (arrays[-1] == label_value).numpy() for label_name, label_value in label_values.items()}
        return render_contours(img, y, y_pred, label_values if (out_target or out_pred) else {}, self.scale,
                               self.line_width, self.legend)
