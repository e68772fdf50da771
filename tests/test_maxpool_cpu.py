"""nn.MaxPool3d(2, 2) as downsample_class: what can be checked without a GPU -- the geometry validation of
models/modular_unet.py:_run_downsample, the bindings, and the argument checks of the library (no launches)."""
import ctypes

import pytest
from torch import nn

from segmentation_pipeline_amd import _lib
from segmentation_pipeline_amd.models.modular_unet import _run_downsample

SYMBOLS = ["m355_maxpool3d_2x_fwd", "m355_maxpool3d_2x_bwd", "m355_maxpool3d_2x_fwd_h16", "m355_maxpool3d_2x_bwd_h16"]
P = ctypes.c_void_p


def test_supported_geometry_validates_without_a_tensor():
    assert _run_downsample(nn.MaxPool3d(2), None) is None
    assert _run_downsample(nn.MaxPool3d(kernel_size=2, stride=2), None) is None
    assert _run_downsample(nn.MaxPool3d((2, 2, 2), (2, 2, 2)), None) is None


@pytest.mark.parametrize("module", [
    nn.MaxPool3d(3, 2, 1), nn.MaxPool3d(2, 1), nn.MaxPool3d(2, 2, ceil_mode=True), nn.MaxPool3d(2, 2, dilation=2),
    nn.MaxPool3d(2, 2, return_indices=True), nn.MaxPool3d((2, 2, 1), (2, 2, 1))],
    ids=["k3s2p1", "k2s1", "ceil_mode", "dilation2", "return_indices", "anisotropic"])
def test_other_geometries_are_refused(module):
    with pytest.raises(NotImplementedError, match=r"only MaxPool3d\(kernel_size=2, stride=2\) has a HIP kernel"):
        _run_downsample(module, None)


def test_symbols_are_bound():
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert getattr(_lib.lib(), s) is not None


def test_argument_checks_reject_before_any_launch():
    L = _lib.lib()
    a = P(64)
    rc = L.m355_maxpool3d_2x_fwd(a, a, a, 1, 1, 3, 4, 4, 0, 0, None)
    assert rc == -2 and b"odd" in L.m355_last_error() and b"maxpool3d_2x_fwd" in L.m355_last_error()
    rc = L.m355_maxpool3d_2x_fwd(None, a, a, 1, 1, 4, 4, 4, 0, 0, None)
    assert rc == -1 and b"null" in L.m355_last_error()
    assert L.m355_maxpool3d_2x_fwd(a, a, None, 1, 0, 4, 4, 4, 0, 0, None) == -1
    # backward: the route is not optional there
    rc = L.m355_maxpool3d_2x_bwd(a, None, None, a, 1, 1, 4, 4, 4, 0, 0, 0, None)
    assert rc == -1 and b"null" in L.m355_last_error()
    assert L.m355_maxpool3d_2x_bwd(a, a, None, a, 1, 1, 4, 4, 5, 0, 0, 0, None) == -2
    # c8: null, odd, compute mode, 16-byte alignment of the c8 tensors and 8-byte alignment of the route items
    assert L.m355_maxpool3d_2x_fwd_h16(None, a, None, 1, 8, 4, 4, 4, 0, 0, _lib.COMPUTE_BF16, None) == -1
    rc = L.m355_maxpool3d_2x_fwd_h16(a, a, None, 1, 8, 4, 6, 3, 0, 0, _lib.COMPUTE_BF16, None)
    assert rc == -2 and b"odd" in L.m355_last_error()
    rc = L.m355_maxpool3d_2x_fwd_h16(a, a, None, 1, 8, 4, 4, 4, 0, 0, 0, None)
    assert rc == -1 and b"compute" in L.m355_last_error()
    rc = L.m355_maxpool3d_2x_fwd_h16(P(72), a, None, 1, 8, 4, 4, 4, 0, 0, _lib.COMPUTE_F16, None)
    assert rc == -1 and b"aligned" in L.m355_last_error()
    assert L.m355_maxpool3d_2x_fwd_h16(a, a, P(68), 1, 8, 4, 4, 4, 0, 0, _lib.COMPUTE_F16, None) == -1
    assert L.m355_maxpool3d_2x_bwd_h16(a, None, None, a, 1, 8, 4, 4, 4, 0, 0, 0, _lib.COMPUTE_BF16, None) == -1
    assert L.m355_maxpool3d_2x_bwd_h16(a, a, None, a, 1, 8, 4, 4, 4, 0, 0, 0, 7, None) == -1
    rc = L.m355_maxpool3d_2x_bwd_h16(a, a, P(8), a, 1, 8, 4, 4, 4, 0, 0, 0, _lib.COMPUTE_BF16, None)
    assert rc == -1 and b"aligned" in L.m355_last_error()
    assert L.m355_maxpool3d_2x_bwd_h16(a, a, None, a, 1, 8, 2, 2, 7, 0, 0, 0, _lib.COMPUTE_BF16, None) == -2
