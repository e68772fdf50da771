"""m355_norm_act_bwd_pool (the normalisation backward that sums the skip gradient and the un-pooled gradient inside its two
passes) checks its arguments like the entry points it replaces.  Pure host code, no GPU: dummy non-null pointers, every call
stops at its argument checks and nothing is launched."""
import ctypes as C

from segmentation_pipeline_amd import _lib

EINVALID, EUNSUPPORTED, EWORKSPACE = -1, -2, -4


def call(d, D, H, W, ws_bytes, x=4096, dskip=4096, dpool=4096, mean=4096, rstd=4096, dx=4096, ws=4096):
    p = lambda v: C.c_void_p(v) if v else None
    g = C.c_void_p(4096)
    return _lib.lib().m355_norm_act_bwd_pool(C.byref(d), p(x), p(dskip), 0, p(dpool), 0, D, H, W, p(mean), p(rstd), g, g, p(dx),
                                             g, g, 1, p(ws), ws_bytes, None)


def test_pool_backward_argument_checks():
    L = _lib.lib()
    d = _lib.NormDesc(2, 16, 4 * 6 * 8, 8, 2, 1e-5, 0.01, 0, 0, 0)
    need = L.m355_norm_workspace(C.byref(d))
    for missing in ("x", "dpool", "mean", "rstd", "dx", "ws"):
        assert call(d, 4, 6, 8, need, **{missing: 0}) == EINVALID and b"null" in L.m355_last_error(), missing
    assert call(d, 4, 6, 6, need) == EINVALID and b"D*H*W" in L.m355_last_error()
    assert call(d, 0, 6, 8, need) == EINVALID
    odd = _lib.NormDesc(2, 16, 3 * 6 * 8, 8, 2, 1e-5, 0.01, 0, 0, 0)
    big = L.m355_norm_workspace(C.byref(odd))
    for dims in ((3, 6, 8), (6, 3, 8), (6, 8, 3)):
        assert call(odd, *dims, big) == EUNSUPPORTED and b"odd" in L.m355_last_error(), dims
    bad = _lib.NormDesc(1, 30, 64, 8, 0, 1e-5, 0.0, 0, 0, 0)
    assert call(bad, 4, 4, 4, 1 << 30) == EINVALID and b"divisible" in L.m355_last_error()
    assert L.m355_norm_act_bwd_pool(None, *([None] * 2), 0, None, 0, 4, 4, 4, *([None] * 7), 1, None, 0, None) == EINVALID


def test_pool_backward_workspace_is_the_norm_workspace():
    """one byte less than m355_norm_workspace is refused, whatever y_batch_stride says (the entry does not use it); a null
    dskip is the pool gradient alone and passes the pointer check"""
    L = _lib.lib()
    for case in ((2, 16, 8, (4, 6, 8)), (2, 16, 0, (4, 6, 6)), (1, 32, 32, (32, 32, 32)), (1, 8, 8, (2, 2, 2))):
        N, Cc, groups, (D, H, W) = case
        d = _lib.NormDesc(N, Cc, D * H * W, groups, 2, 1e-5, 0.01, 0, 12345, 0)
        need = L.m355_norm_workspace(C.byref(d))
        assert call(d, D, H, W, need - 1) == EWORKSPACE and b"workspace" in L.m355_last_error(), case
        assert call(d, D, H, W, need - 1, dskip=0) == EWORKSPACE, case
