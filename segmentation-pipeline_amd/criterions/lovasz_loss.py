"""LovaszLoss: the Lovasz-softmax loss of Berman et al., "The Lovasz-Softmax loss: a tractable surrogate for the
optimization of the intersection-over-union measure in neural networks" (CVPR 2018), alone or added to any criterion of
this package.

The evaluators score a model by hard Dice / Jaccard per label; the other criteria here are sums over voxels and optimise
that only indirectly.  The Lovasz extension of the Jaccard loss is its convex surrogate: per channel, the errors
e = |foreground - p| of all voxels are sorted, and the loss is their dot product with the increments of the Jaccard loss
along the sorted order.  It treats every channel as a binary problem, so it serves a softmax and a sigmoid head alike.

The step's target exists only on the device, so the sort runs there: `ops.lovasz_loss` is a key pass, a segmented radix
sort, a scan pass and a one-launch backward.  Elements with equal errors share the mean of their
subgradients, so neither the loss nor the gradient depends on how a sort breaks ties.  Nothing is read on the host, so
trainer.GraphedTrainStep captures it.

    loss = regional_weight * criterion(prediction, target)['loss'] + lovasz_weight * lovasz

With `criterion=None` the loss is `lovasz_weight * lovasz`.  The two mixing weights are device scalars (registered
buffers): `set_weights` fills them in place without a synchronisation -- train on Dice + CE, then fade the Lovasz term
in -- and a captured step picks the new value up on its next replay.

classes='present' (Berman's default) averages the channels that have a foreground voxel, 'all' every channel;
per_image=True takes the mean per image first; `lovasz_class_weights` weighs the channels (None: all ones).  A voxel is
foreground when target >= 0.5, which serves the soft 'area' targets of DeepSupervisionLoss (a coarse cell of exactly 0.5
is foreground here and outside in BoundaryLoss and BlobLoss, which take target > 0.5: DESIGN §4.30); compose as
DeepSupervisionLoss(LovaszLoss(inner)): a tuple prediction is not this wrapper's business.  The prediction must hold
probabilities: a NaN or a value outside [0, 1] gives a NaN loss.  A wrapped criterion with from_logits=True, at any depth,
is therefore refused at construction (ValueError): use a softmax or sigmoid head with from_logits=False, or keep the
logits criterion outside this wrapper -- DeepSupervisionLoss forwards either kind.

The result is `criterion`'s dict (or an empty one) with 'loss' replaced by the total and 'lovasz_loss', 'regional_loss'
(detached), 'lovasz_weight' and 'regional_weight' added; the gradient flows through 'loss' only.
"""
import math

import torch

from .. import ops
from .._lib import M355Error
from ._device_weights import DeviceWeightsCriterion, require_probabilities


class LovaszLoss(DeviceWeightsCriterion):
    def __init__(self, criterion=None, lovasz_weight=1.0, regional_weight=1.0, classes='present', per_image=False,
                 lovasz_class_weights=None):
        super().__init__()
        for name, v in (("lovasz_weight", lovasz_weight), ("regional_weight", regional_weight)):
            if not math.isfinite(v):
                raise ValueError(f"{name} = {v}: expected a finite value")
        require_probabilities(self, criterion)
        if classes not in ops.LOVASZ_CLASSES:
            raise ValueError(f"classes = {classes!r}: expected 'present' or 'all'")
        if lovasz_class_weights is not None:
            if isinstance(lovasz_class_weights, torch.Tensor):
                if lovasz_class_weights.dim() != 1:
                    raise ValueError(f"lovasz_class_weights of shape {tuple(lovasz_class_weights.shape)}: expected [C]")
                lovasz_class_weights = lovasz_class_weights.tolist()
            lovasz_class_weights = tuple(float(v) for v in lovasz_class_weights)
            if not lovasz_class_weights or any(not (math.isfinite(v) and v >= 0) for v in lovasz_class_weights):
                raise ValueError(f"lovasz_class_weights = {lovasz_class_weights}: expected finite values >= 0")
        self.criterion = criterion
        self.classes = classes
        self.per_image = bool(per_image)
        self.lovasz_class_weights = lovasz_class_weights
        self.register_buffer("regional_weight", torch.tensor(float(regional_weight), dtype=torch.float32))
        self.register_buffer("lovasz_weight", torch.tensor(float(lovasz_weight), dtype=torch.float32))

    def set_weights(self, regional=None, lovasz=None):
        """Fill the mixing weights in place (no synchronisation; the buffers keep their addresses)."""
        for buf, v in ((self.regional_weight, regional), (self.lovasz_weight, lovasz)):
            if v is not None:
                if not math.isfinite(v):
                    raise ValueError(f"weight {v}: expected a finite value")
                buf.fill_(float(v))

    def __getstate__(self):   # pickled losses hold no device tensor: the buffers go to the host too
        state = super().__getstate__()
        state["_buffers"] = {k: v.cpu() for k, v in self._buffers.items()}
        return state

    def forward(self, prediction, target):
        if not torch.is_tensor(prediction):
            raise M355Error("LovaszLoss takes one prediction tensor; for the tuple of a deep-supervision model compose "
                            "DeepSupervisionLoss(LovaszLoss(criterion))")
        if prediction.dim() < 3 or prediction.shape != target.shape:
            raise M355Error(f"prediction {tuple(prediction.shape)} and target {tuple(target.shape)}: expected one shape "
                            f"[N, C, ...]")
        weights = self._device_weights("lovasz_class_weights", prediction.shape[1], prediction.device)
        if self.regional_weight.device != prediction.device:
            # (once: the buffers follow the first prediction, like the class weights; their addresses stay from then on)
            self.regional_weight = self.regional_weight.to(prediction.device)
            self.lovasz_weight = self.lovasz_weight.to(prediction.device)
        lovasz = ops.lovasz_loss(prediction, target.detach(), self.classes, self.per_image, weights)
        if self.criterion is None:
            d = {}
            regional = torch.zeros((), dtype=torch.float32, device=prediction.device)
            d['loss'] = self.lovasz_weight * lovasz
        else:
            d = dict(self.criterion(prediction, target))
            regional = d['loss']
            d['loss'] = self.regional_weight * regional + self.lovasz_weight * lovasz
        d['lovasz_loss'] = lovasz.detach()
        d['regional_loss'] = regional.detach()
        d['lovasz_weight'] = self.lovasz_weight.clone()
        d['regional_weight'] = self.regional_weight.clone()
        return d
