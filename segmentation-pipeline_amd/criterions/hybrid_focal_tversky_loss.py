"""HybridFocalTverskyLoss: a Tversky overlap term plus a focal cross-entropy, on fused HIP reduction kernels.

For targets that fill a small fraction of the volume.  The overlap term is the Tversky index
`TP / (TP + alpha FP + beta FN)`, which weighs a false positive (alpha) and a false negative (beta) separately -- beta >
alpha buys recall -- and `tversky_power` e raises `1 - TI` to a power (e = 0.75: the focal Tversky loss of Abraham & Khan;
e = 1: plain Tversky).  The log term `t * (1 - p)^gamma * log p` is the cross-entropy with the focal factor, which fades
on voxels the model already classifies correctly; `focal_gamma` is 0 (no factor) or >= 1.  `tversky_class_weights` weigh
the Tversky terms per channel (a zero drops one, such as the background), `logistic_class_weights` the log terms.

With the defaults (alpha = beta = 0.5, e = 1, gamma = 0) it is HybridLogisticDiceLoss(square_dice=False).

With `from_logits=True` the input is the logits of a model with hypothesis_class=nn.Identity; the log-softmax over the
channels is taken inside the loss and the gradient with respect to the logits directly.  It stays alive at a voxel that
is saturated on the wrong class, where a softmax's own backward multiplies by p = 0, and the head's backward pass over
the volume is gone.

The log term is the positive half `t log p` only, as in HybridLogisticDiceLoss: among softmax channels the other
channels' positive halves pay for a false positive.  On sigmoid channels, which do not compete, nothing does:
HybridBinaryLogisticDiceLoss remains the criterion with both halves.

Same dict shape as the other criteria: {'loss', 'tversky_loss', 'focal_loss'}; the gradient flows through 'loss' only.
"""
import math

from .. import ops
from ._device_weights import DeviceWeightsCriterion


class HybridFocalTverskyLoss(DeviceWeightsCriterion):
    def __init__(self, tversky_weight=0.5, alpha=0.5, beta=0.5, tversky_power=1.0, focal_gamma=0.0,
                 logistic_class_weights=None, tversky_class_weights=None, from_logits=False):
        super().__init__()
        for name, v in (("alpha", alpha), ("beta", beta)):
            if not (math.isfinite(v) and v >= 0):
                raise ValueError(f"{name} = {v}: expected a finite value >= 0")
        if not (math.isfinite(tversky_power) and tversky_power > 0):
            raise ValueError(f"tversky_power = {tversky_power}: expected a finite value > 0")
        if not (math.isfinite(focal_gamma) and (focal_gamma == 0 or focal_gamma >= 1)):
            # (1 - p)^(gamma - 1) in the gradient is infinite at p = 1 for a gamma between 0 and 1
            raise ValueError(f"focal_gamma = {focal_gamma}: expected 0 or a finite value >= 1")
        self.tversky_weight = tversky_weight
        self.alpha = alpha
        self.beta = beta
        self.tversky_power = tversky_power
        self.focal_gamma = focal_gamma
        self.logistic_class_weights = logistic_class_weights
        self.tversky_class_weights = tversky_class_weights
        self.from_logits = from_logits

    def forward(self, prediction, target):
        channels = prediction.shape[1] if prediction.dim() >= 2 else 0
        loss, tversky_loss, focal_loss = ops.focal_tversky_loss(
            prediction, target, self.tversky_weight, self.alpha, self.beta, self.tversky_power, self.focal_gamma,
            self._device_weights("logistic_class_weights", channels, prediction.device),
            self._device_weights("tversky_class_weights", channels, prediction.device), self.from_logits)
        return {'loss': loss, 'tversky_loss': tversky_loss, 'focal_loss': focal_loss}
