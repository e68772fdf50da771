"""Drop-in for `segmentation_pipeline.criterions` (reference criterions/__init__.py:1)."""
from .hybrid_logistic_dice_loss import HybridLogisticDiceLoss
from .hybrid_binary_logistic_dice_loss import HybridBinaryLogisticDiceLoss
from .hybrid_focal_tversky_loss import HybridFocalTverskyLoss
from .hybrid_topk_dice_loss import HybridTopKDiceLoss
from .deep_supervision_loss import DeepSupervisionLoss
from .boundary_loss import BoundaryLoss
from .blob_loss import BlobLoss
from .lovasz_loss import LovaszLoss
