"""Per-channel weights of a criterion on the device, uploaded once.

The reference builds the weight tensor every call (hybrid_logistic_dice_loss.py:23-25); from a Python list that is a
blocking host-to-device copy per step (~0.8 ms of a 12 ms step).  Here a list or tuple is uploaded once per (values, device)
and held in `_uploaded`: attribute name -> (values, device, tensor).  A pickled criterion holds no device tensor, as the
reference's does not.  `_uploaded` is looked up in the instance's `__dict__` and made on first use, so an instance restored
from a pickle of an earlier layout (no `_uploaded`, or `_uploaded = None`) uploads on its first call like a new one.
"""
import torch
from torch import nn

from .._lib import M355Error


def require_probabilities(wrapper, criterion):
    """BoundaryLoss, BlobLoss and LovaszLoss hand the prediction they are given to a term of their own that needs
    probabilities; a wrapped criterion with from_logits=True -- at any depth of `.criterion` -- says the prediction holds
    logits, on which the boundary term is an unbounded `mean(logit * phi)` and the blob and Lovasz terms are NaN.  Refused
    where the nest is built (a ValueError), not found in a loss curve."""
    inner, seen = criterion, set()
    while inner is not None and id(inner) not in seen:
        seen.add(id(inner))
        if getattr(inner, "from_logits", False):
            raise ValueError(
                f"{type(wrapper).__name__} around {type(inner).__name__}(from_logits=True): the "
                f"{type(wrapper).__name__} term takes probabilities, not logits.  Give the model a softmax or sigmoid "
                f"head and the criterion from_logits=False, or keep the logits criterion outside "
                f"{type(wrapper).__name__} (DeepSupervisionLoss forwards either kind)")
        inner = getattr(inner, "criterion", None)


class DeviceWeightsCriterion(nn.Module):
    def __init__(self):
        super().__init__()
        self._uploaded = {}

    def _device_weights(self, name, channels, device, given=None):
        """self.<name> -- a list, tuple, tensor or None; or `given` in its place -- as an fp32 device tensor [channels], or
        None.  channels=None: the length is not checked here."""
        if given is None:
            given = getattr(self, name)
        if given is None:
            return None
        if isinstance(given, torch.Tensor):
            if channels is not None and (given.dim() != 1 or given.numel() != channels):
                raise M355Error(f"{name} of shape {tuple(given.shape)} for {channels} channels")
            return given.to(device=device, dtype=torch.float32)
        values = tuple(float(v) for v in given)
        if channels is not None and len(values) != channels:
            raise M355Error(f"{name} of {len(values)} values for {channels} channels")
        cache = self.__dict__.get("_uploaded")
        if not isinstance(cache, dict):
            cache = self._uploaded = {}
        held = cache.get(name)
        if held is None or held[0] != values or held[1] != device:
            held = cache[name] = (values, device, torch.tensor(values, dtype=torch.float32, device=device))
        return held[2]

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_uploaded"] = {}
        return state
