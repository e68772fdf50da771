"""What the criteria's reference modules (binary_loss_ref, focal_tversky_ref) share: the per-channel weight vector of the
torch formulas and the plumbing of the raw C-ABI wrappers."""
import ctypes as C

import torch

from segmentation_pipeline_amd import _lib


def _per_channel(w, C_, like):
    if w is None:
        return torch.ones(C_, dtype=like.dtype)
    return torch.as_tensor(w, dtype=like.dtype)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc} {_lib.lib().m355_last_error().decode()}")


def _dev(w):
    return None if w is None else torch.tensor(w, dtype=torch.float32, device="cuda")
