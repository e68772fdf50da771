"""Lesion-wise detection statistics (the per-subject numbers of the reference's InstanceSegmentationEvaluator,
evaluators/instance_segmentation_evaluator.py) with the labelling and the overlap table on the device.

The overlap table of N target and M predicted components is a dense int64 [N + 1, M + 1] histogram (component 0 is
the background of either map), built by one pass of m355_label_histogram over the two label maps.  It is refused
above MAX_OVERLAP_ENTRIES entries.  The detection test and every statistic derived from the table run on the host in
float32, the dtype of the reference's table (so N == 0 or M == 0 gives the same nan results).
"""
import torch

from ._lib import M355Error
from .post_processing import _OP_COPY, _OP_POSITIVE, _ccl, _connectivity, _device_volume, _histogram, _to_i32

__all__ = ["overlap_histogram", "msseg_detection_test", "instance_segmentation_stats", "MAX_OVERLAP_ENTRIES", "STAT_NAMES"]

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
