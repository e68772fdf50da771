"""DeepSupervisionLoss: any criterion of this package applied at every level of a deep-supervision model.

`models.DeepSupervisionUNet` returns, in training mode, the tuple (y_pred, aux_1, ..., aux_k): the full-resolution
prediction and those of the decoder levels at 1/2, 1/4, ... of its size.  This wrapper scales the target down once
(`ops.target_pyramid`: one launch for all k levels), applies `criterion` to every (prediction, target) pair and returns
the weighted sum

    loss = w_0 l_0 + w_1 l_1 + ... + w_k l_k,        w_j = 2^-j / sum_i 2^-i  by default (nnU-Net's weights),

accumulated left to right on device scalars: nothing is read on the host, so trainer.GraphedTrainStep can capture it.

`target_mode='area'` gives a coarse cell the mean of its voxels -- a target smaller than the cell stays visible as
fractional mass, and every criterion here takes soft targets; `'nearest'` is nnU-Net's choice, the voxel at the cell's
origin.  A tensor prediction (eval mode, validation, a model without auxiliary heads) goes to `criterion` unchanged.

The result is the dict of level 0 -- `dice_loss`, `logistic_loss`, ... keep meaning what loggers expect -- with 'loss'
replaced by the total and 'loss_level{j}' (detached) added for every level that was evaluated; a level with weight 0 is not.
"""
import torch
from torch import nn

from .. import ops
from .._lib import M355Error


def default_weights(levels):
    """w_j = 2^-j / sum_i 2^-i for j = 0..levels - 1 (4/7, 2/7, 1/7 for three)"""
    total = sum(2.0 ** -i for i in range(levels))
    return [2.0 ** -j / total for j in range(levels)]


class DeepSupervisionLoss(nn.Module):
    def __init__(self, criterion, weights=None, target_mode='area'):
        super().__init__()
        if target_mode not in ops.PYRAMID_MODES:
            raise ValueError(f"target_mode = {target_mode!r}: expected 'area' or 'nearest'")
        if weights is not None:
            weights = [float(w) for w in weights]
            if not weights or any(not w >= 0.0 or w == float("inf") for w in weights):
                raise ValueError(f"weights = {weights}: expected a sequence of finite, non-negative values")
            if not any(weights):
                raise ValueError(f"weights = {weights}: at least one level needs a positive weight")
        self.criterion = criterion
        self.weights = weights
        self.target_mode = target_mode

    def forward(self, prediction, target):
        if torch.is_tensor(prediction):
            return self.criterion(prediction, target)
        predictions = list(prediction)
        k = len(predictions) - 1
        if self.weights is None:
            weights = default_weights(k + 1)
        elif len(self.weights) != k + 1:
            raise ValueError(f"{len(self.weights)} weights for {k + 1} prediction levels")
        else:
            weights = self.weights
        targets = [target] + (ops.target_pyramid(target, k, self.target_mode) if k else [])
        for j, (p, t) in enumerate(zip(predictions, targets)):
            if tuple(p.shape) != tuple(t.shape):
                raise M355Error(f"level {j}: prediction {tuple(p.shape)} and target {tuple(t.shape)} differ "
                                f"(the target of level j is the target at 1/2^j of its size)")
        out, total, per_level = None, None, {}
        for j, w in enumerate(weights):
            if w == 0.0:
                continue
            d = self.criterion(predictions[j], targets[j])
            if out is None:
                out = dict(d)          # level 0's, unless its weight is 0: then the finest evaluated level's
            term = w * d['loss']
            total = term if total is None else total + term
            per_level[f'loss_level{j}'] = d['loss'].detach()
        out['loss'] = total
        out.update(per_level)
        return out
