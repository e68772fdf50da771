"""HybridBinaryLogisticDiceLoss: binary cross-entropy + Dice for sigmoid heads, on fused HIP reduction kernels.

The counterpart of HybridLogisticDiceLoss for models whose channels do not compete (hypothesis_class=nn.Sigmoid: one-channel
masks, multi-label structures).  Its log term is the whole binary cross-entropy, `pos_weight * t * log p + (1 - t) *
log(1 - p)` per channel, so a confident false positive is paid for in the log term too, and `pos_weight` weights the rare
positive class per channel.  With `from_logits=True` the input is the logits of a model with hypothesis_class=nn.Identity
and the gradient is taken with respect to them directly: it stays alive at a saturated voxel, where a sigmoid's own
backward multiplies by p (1 - p) = 0.

Same dict of three scalars as HybridLogisticDiceLoss; the gradient flows through 'loss' only.
"""
from .. import ops
from ._device_weights import DeviceWeightsCriterion


class HybridBinaryLogisticDiceLoss(DeviceWeightsCriterion):
    def __init__(self, dice_weight=0.5, logistic_class_weights=None, pos_weight=None, square_dice=True, from_logits=False):
        super().__init__()
        self.dice_weight = dice_weight
        self.logistic_class_weights = logistic_class_weights
        self.pos_weight = pos_weight
        self.square_dice = square_dice
        self.from_logits = from_logits

    def forward(self, prediction, target):
        channels = prediction.shape[1] if prediction.dim() >= 2 else 0
        loss, dice_loss, logistic_loss = ops.binary_logistic_dice_loss(
            prediction, target, self.dice_weight, self._device_weights("logistic_class_weights", channels, prediction.device),
            self._device_weights("pos_weight", channels, prediction.device), self.square_dice, self.from_logits)
        return {'loss': loss, 'dice_loss': dice_loss, 'logistic_loss': logistic_loss}
