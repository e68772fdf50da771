"""HybridTopKDiceLoss: Dice plus a cross-entropy over the hardest k % of the voxels only, on a device radix select.

The compound loss nnU-Net ships for sparse targets (`DC_and_topk_loss`).  The per-voxel cross-entropy
`e = -sum_c w_c t_c log p_c` is averaged over the `top_k` fraction of the voxels OF THE WHOLE BATCH with the largest `e`:
online hard-example mining.  Once a patch is 99.9 % confidently right background, the sum of those tiny terms still
dominates a plain cross-entropy; a focal factor only shrinks them; top-k removes them from the loss, and from the
gradient, altogether.  The Dice term is HybridLogisticDiceLoss's, `square_dice` included.

    k = max(1, floor(N * S * top_k))
    logistic_loss = (1 / (C * k)) * sum of the k largest e          (top_k = 1: HybridLogisticDiceLoss's logistic_loss)
    loss = (1 - dice_weight) * logistic_loss + dice_weight * dice_loss

The k-th largest value is found by a three-pass radix select, not a sort; voxels that tie with it share what is left of
k instead of being drawn, so the result and its gradient are deterministic.

With `from_logits=True` the input is the logits of a model with hypothesis_class=nn.Identity and the log-softmax is taken
inside the loss.  That is the recommended mode: the hardest voxels are by definition those saturated on the wrong class,
where a softmax head's own backward multiplies their gradient by p = 0.

`set_top_k(fraction)` changes the fraction between steps (the usual schedule anneals it from 1.0 to 0.1).  k lives in a
device scalar per input shape that the kernels read, filled in place without a synchronisation, so a step captured by
trainer.GraphedTrainStep follows the schedule on its next replay.

Same dict shape as the other criteria: {'loss', 'dice_loss', 'logistic_loss', 'topk_threshold'}; the threshold (the k-th
largest e, detached) is for the loggers; the gradient flows through 'loss' only.
"""
import math

import torch

from .. import ops
from ._device_weights import DeviceWeightsCriterion


def _checked_fraction(top_k):
    if isinstance(top_k, bool) or not isinstance(top_k, (int, float)) or not (math.isfinite(top_k) and 0 < top_k <= 1):
        raise ValueError(f"top_k = {top_k}: expected a fraction in (0, 1]")
    return float(top_k)


class HybridTopKDiceLoss(DeviceWeightsCriterion):
    def __init__(self, top_k=0.1, dice_weight=0.5, logistic_class_weights=None, square_dice=True, from_logits=False):
        super().__init__()
        self.top_k = _checked_fraction(top_k)
        self.dice_weight = dice_weight
        self.logistic_class_weights = logistic_class_weights
        self.square_dice = square_dice
        self.from_logits = from_logits
        self._counts = {}    # (N, S, device) -> 0-dim int64 device tensor holding k; its address stays

    def set_top_k(self, fraction):
        """Change the fraction between steps: every k already on a device is filled in place (no synchronisation)."""
        self.top_k = _checked_fraction(fraction)
        for (N, S, _), held in self._held_counts().items():
            held.fill_(ops.topk_count(N, S, self.top_k))

    def _held_counts(self):
        held = self.__dict__.get("_counts")
        if not isinstance(held, dict):
            held = self._counts = {}
        return held

    def _count(self, N, S, device):
        held = self._held_counts()
        key = (N, S, device)
        if key not in held:
            held[key] = torch.tensor(ops.topk_count(N, S, self.top_k), dtype=torch.int64, device=device)
        return held[key]

    def __getstate__(self):   # pickled losses hold no device tensor
        state = super().__getstate__()
        state["_counts"] = {}
        return state

    def forward(self, prediction, target):
        channels = prediction.shape[1] if prediction.dim() >= 2 else 0
        N = prediction.shape[0] if prediction.dim() >= 2 else 0
        S = prediction.numel() // max(1, N * channels)
        loss, dice_loss, logistic_loss, threshold = ops.topk_logistic_dice_loss(
            prediction, target, self._count(N, S, prediction.device), self.dice_weight,
            self._device_weights("logistic_class_weights", channels, prediction.device), self.square_dice,
            self.from_logits)
        return {'loss': loss, 'dice_loss': dice_loss, 'logistic_loss': logistic_loss, 'topk_threshold': threshold.detach()}
