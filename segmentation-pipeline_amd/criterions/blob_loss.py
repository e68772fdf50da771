"""BlobLoss: any criterion of this package plus the lesion-wise (blob) Dice of Kofler et al., "blob loss: instance
imbalance aware loss functions for semantic segmentation", on device connected components.

Every other criterion here (Dice + CE, BCE + Dice, focal Tversky, top-k CE, boundary) is a sum over voxels: one
2000-voxel lesion outweighs forty 50-voxel lesions, and the small ones are those the detection metrics count.  The blob
term evaluates the Dice of HybridLogisticDiceLoss once per connected component of the target, with the other components of
its (n, c) plane masked out of prediction and target, and averages over the components: every lesion has the same vote
whatever its size.

The label map of a step exists only on the device, so the components are found there, every step: `ops.blob_dice_loss`
labels all planes with a non-zero weight in one labelling, reduces the prediction per component in one pass with integer
sums and has a closed-form backward.  Nothing is read on the host, so trainer.GraphedTrainStep captures it.

    loss = global_weight * criterion(prediction, target)['loss'] + blob_weight * blob

The defaults global_weight = 2, blob_weight = 1 are the paper's alpha and beta.  Both are device scalars (registered
buffers): `set_weights` fills them in place without a synchronisation, so a warm-up schedule is one line between steps
and a captured step picks the new value up on its next replay.

`blob_class_weights=None` weighs every channel 1, except channel 0 (the background) 0 when there is more than one
channel, BoundaryLoss's convention.  A voxel is a member when target > 0.5, which serves the soft 'area' targets of
DeepSupervisionLoss; compose as DeepSupervisionLoss(BlobLoss(inner)): a tuple prediction is not this wrapper's business.
The prediction must hold probabilities (a softmax or sigmoid head): a value outside [0, 1] or not finite in a weighted
channel gives a NaN blob term, which the fused optimizers skip like any non-finite step.  A wrapped criterion with
from_logits=True, at any depth, is therefore refused at construction (ValueError): use a softmax or sigmoid head with
from_logits=False, or keep the logits criterion outside this wrapper -- DeepSupervisionLoss forwards either kind.  The
blob term is Dice only; a per-blob log term is not part of it.  (A coarse cell of exactly 0.5 is no member here and in
BoundaryLoss, and foreground in LovaszLoss: DESIGN §4.30.)

The result is `criterion`'s dict with 'loss' replaced by the total and 'blob_loss', 'global_loss' (detached), 'blob_count'
(a device int32: the number of components; -1 if the labelling gave up, with a NaN term), 'blob_weight' and
'global_weight' added; the gradient flows through 'loss' only.
"""
import math

import torch

from .. import ops
from .._lib import M355Error
from ._device_weights import DeviceWeightsCriterion, require_probabilities


class BlobLoss(DeviceWeightsCriterion):
    def __init__(self, criterion, blob_weight=1.0, global_weight=2.0, blob_class_weights=None, square_dice=True,
                 connectivity=3):
        super().__init__()
        for name, v in (("blob_weight", blob_weight), ("global_weight", global_weight)):
            if not math.isfinite(v):
                raise ValueError(f"{name} = {v}: expected a finite value")
        if blob_class_weights is not None:
            if isinstance(blob_class_weights, torch.Tensor):
                if blob_class_weights.dim() != 1:
                    raise ValueError(f"blob_class_weights of shape {tuple(blob_class_weights.shape)}: expected [C]")
                blob_class_weights = blob_class_weights.tolist()
            blob_class_weights = tuple(float(v) for v in blob_class_weights)
            if not blob_class_weights or any(not (math.isfinite(v) and v >= 0) for v in blob_class_weights):
                raise ValueError(f"blob_class_weights = {blob_class_weights}: expected finite values >= 0")
            if not sum(blob_class_weights) > 0:
                raise ValueError(f"blob_class_weights = {blob_class_weights}: at least one channel needs a positive weight")
        require_probabilities(self, criterion)
        if connectivity not in (1, 2, 3):
            raise ValueError(f"connectivity = {connectivity!r}: expected 1, 2 or 3 (6, 18 or 26 neighbours)")
        self.criterion = criterion
        self.blob_class_weights = blob_class_weights
        self.square_dice = bool(square_dice)
        self.connectivity = int(connectivity)
        self.register_buffer("global_weight", torch.tensor(float(global_weight), dtype=torch.float32))
        self.register_buffer("blob_weight", torch.tensor(float(blob_weight), dtype=torch.float32))

    def set_weights(self, global_=None, blob=None):
        """Fill the mixing weights in place (no synchronisation; the buffers keep their addresses)."""
        for buf, v in ((self.global_weight, global_), (self.blob_weight, blob)):
            if v is not None:
                if not math.isfinite(v):
                    raise ValueError(f"weight {v}: expected a finite value")
                buf.fill_(float(v))

    def _class_weights(self, channels, device):
        """-> (the weights as host floats, as an fp32 device tensor [channels] uploaded once per (values, device))"""
        values = self.blob_class_weights
        if values is None:
            values = ops.blob_default_class_weights(channels)
        return values, self._device_weights("blob_class_weights", channels, device, given=values)

    def __getstate__(self):   # pickled losses hold no device tensor: the buffers go to the host too
        state = super().__getstate__()
        state["_buffers"] = {k: v.cpu() for k, v in self._buffers.items()}
        return state

    def forward(self, prediction, target):
        if not torch.is_tensor(prediction):
            raise M355Error("BlobLoss takes one prediction tensor; for the tuple of a deep-supervision model compose "
                            "DeepSupervisionLoss(BlobLoss(criterion))")
        if prediction.dim() != 5 or prediction.shape != target.shape:
            raise M355Error(f"prediction {tuple(prediction.shape)} and target {tuple(target.shape)}: expected one shape "
                            f"[N, C, D, H, W]")
        N, channels = prediction.shape[0], prediction.shape[1]
        values, weights = self._class_weights(channels, prediction.device)
        if self.global_weight.device != prediction.device:
            # (once: the buffers follow the first prediction, like the class weights; their addresses stay from then on)
            self.global_weight = self.global_weight.to(prediction.device)
            self.blob_weight = self.blob_weight.to(prediction.device)
        d = dict(self.criterion(prediction, target))
        blob, count = ops.blob_dice_loss(prediction, target.detach(), weights, self.square_dice, self.connectivity,
                                         planes=[w != 0.0 for w in values] * N)
        inner = d['loss']
        d['loss'] = self.global_weight * inner + self.blob_weight * blob
        d['blob_loss'] = blob.detach()
        d['global_loss'] = inner.detach()
        d['blob_count'] = count
        d['blob_weight'] = self.blob_weight.clone()
        d['global_weight'] = self.global_weight.clone()
        return d
