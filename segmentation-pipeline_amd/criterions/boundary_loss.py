"""BoundaryLoss: any criterion of this package plus the boundary loss of Kervadec et al., "Boundary loss for highly
unbalanced segmentation" (MIDL 2019), on a device distance transform.

The regional criteria here (Dice + CE, BCE + Dice, focal Tversky) are sums over voxels that do not see WHERE an error is;
the boundary term is `mean(p * phi)` with `phi` the signed distance map of the target -- negative inside the structure,
positive outside, growing with the distance from its border -- so a false positive far from the structure costs more
than one next to it.  `phi` follows the published implementation (`one_hot2dist`): +d(nearest inside voxel) outside,
-(d(nearest outside voxel) - 1) inside, 0 everywhere for a channel without a boundary in the patch.

The label map of a step exists only on the device (the augmentations and the sampler run there), so `phi` is computed
there, every step: `ops.signed_distance` transforms all (n, c) planes with a non-zero weight in three launches, one
transform per plane, and `ops.boundary_loss` is one pass over (p, phi) with fp64 sums.  Nothing is read
on the host, so trainer.GraphedTrainStep captures it.

    loss = regional_weight * criterion(prediction, target)['loss'] + boundary_weight * boundary

The two mixing weights are device scalars (registered buffers): `set_weights` fills them in place without a
synchronisation, so both published schedules are one line between steps -- "rebalance": set_weights(1 - a, a);
"increase": set_weights(boundary=a) with a growing -- and a captured step picks the new value up on its next replay.

`boundary_class_weights=None` weighs every channel 1, except channel 0 (the background) 0 when there is more than one
channel, the published default.  A voxel is inside when target > 0.5, which serves the soft 'area' targets of
DeepSupervisionLoss (a coarse cell of exactly 0.5 is outside here and in BlobLoss, foreground in LovaszLoss: DESIGN §4.30);
compose as DeepSupervisionLoss(BoundaryLoss(inner)): a tuple prediction is not this wrapper's business.

The prediction must hold probabilities (a softmax or sigmoid head): on logits `mean(p * phi)` is unbounded.  A wrapped
criterion with from_logits=True, at any depth, is therefore refused at construction (ValueError): use a softmax or
sigmoid head with from_logits=False, or keep the logits criterion outside this wrapper -- DeepSupervisionLoss forwards
either kind.

The result is `criterion`'s dict with 'loss' replaced by the total and 'boundary_loss', 'regional_loss' (detached),
'boundary_weight' and 'regional_weight' added; the gradient flows through 'loss' only.
"""
import math

import torch

from .. import ops
from .._lib import M355Error
from ._device_weights import DeviceWeightsCriterion, require_probabilities


class BoundaryLoss(DeviceWeightsCriterion):
    def __init__(self, criterion, boundary_weight=0.01, regional_weight=1.0, boundary_class_weights=None,
                 spacing=(1., 1., 1.)):
        super().__init__()
        for name, v in (("boundary_weight", boundary_weight), ("regional_weight", regional_weight)):
            if not math.isfinite(v):
                raise ValueError(f"{name} = {v}: expected a finite value")
        if boundary_class_weights is not None:
            if isinstance(boundary_class_weights, torch.Tensor):
                if boundary_class_weights.dim() != 1:
                    raise ValueError(f"boundary_class_weights of shape {tuple(boundary_class_weights.shape)}: expected [C]")
                boundary_class_weights = boundary_class_weights.tolist()
            boundary_class_weights = tuple(float(v) for v in boundary_class_weights)
            if not boundary_class_weights or any(not (math.isfinite(v) and v >= 0) for v in boundary_class_weights):
                raise ValueError(f"boundary_class_weights = {boundary_class_weights}: expected finite values >= 0")
            if not sum(boundary_class_weights) > 0:
                raise ValueError(f"boundary_class_weights = {boundary_class_weights}: at least one channel needs a "
                                 f"positive weight")
        require_probabilities(self, criterion)
        spacing = ops._spacing3(spacing)
        if any(not (math.isfinite(s) and s > 0) for s in spacing):
            raise ValueError(f"spacing = {spacing}: expected finite values > 0")
        self.criterion = criterion
        self.boundary_class_weights = boundary_class_weights
        self.spacing = spacing
        self.register_buffer("regional_weight", torch.tensor(float(regional_weight), dtype=torch.float32))
        self.register_buffer("boundary_weight", torch.tensor(float(boundary_weight), dtype=torch.float32))

    def set_weights(self, regional=None, boundary=None):
        """Fill the mixing weights in place (no synchronisation; the buffers keep their addresses)."""
        for buf, v in ((self.regional_weight, regional), (self.boundary_weight, boundary)):
            if v is not None:
                if not math.isfinite(v):
                    raise ValueError(f"weight {v}: expected a finite value")
                buf.fill_(float(v))

    def _class_weights(self, channels, device):
        """-> (the weights as host floats, as an fp32 device tensor [channels] uploaded once per (values, device))"""
        values = self.boundary_class_weights
        if values is None:
            values = (0.0,) + (1.0,) * (channels - 1) if channels > 1 else (1.0,)
        return values, self._device_weights("boundary_class_weights", channels, device, given=values)

    def __getstate__(self):   # pickled losses hold no device tensor: the buffers go to the host too
        state = super().__getstate__()
        state["_buffers"] = {k: v.cpu() for k, v in self._buffers.items()}
        return state

    def forward(self, prediction, target):
        if not torch.is_tensor(prediction):
            raise M355Error("BoundaryLoss takes one prediction tensor; for the tuple of a deep-supervision model compose "
                            "DeepSupervisionLoss(BoundaryLoss(criterion))")
        if prediction.dim() != 5 or prediction.shape != target.shape:
            raise M355Error(f"prediction {tuple(prediction.shape)} and target {tuple(target.shape)}: expected one shape "
                            f"[N, C, D, H, W]")
        N, channels = prediction.shape[0], prediction.shape[1]
        values, weights = self._class_weights(channels, prediction.device)
        if self.regional_weight.device != prediction.device:
            # (once: the buffers follow the first prediction, like the class weights; their addresses stay from then on)
            self.regional_weight = self.regional_weight.to(prediction.device)
            self.boundary_weight = self.boundary_weight.to(prediction.device)
        d = dict(self.criterion(prediction, target))
        phi = ops.signed_distance(target.detach().contiguous(), self.spacing, [w != 0.0 for w in values] * N)
        boundary = ops.boundary_loss(prediction, phi, weights)
        regional = d['loss']
        d['loss'] = self.regional_weight * regional + self.boundary_weight * boundary
        d['boundary_loss'] = boundary.detach()
        d['regional_loss'] = regional.detach()
        d['boundary_weight'] = self.boundary_weight.clone()
        d['regional_weight'] = self.regional_weight.clone()
        return d
