"""The fp32 normalisation backward behind a fused AvgPool3d(2, 2) (m355_norm_act_bwd_pool) forms skip gradient + un-pooled
gradient inside its two passes.  Its results must have the BITS of the two-step form it replaces, m355_avgpool3d_2x_bwd[_add]
into a dense tensor followed by m355_norm_act_bwd: same expression per element, same chunks, same accumulation order per
thread, whichever load path the pointers allow.  Kernel level on the raw entry points, then one backward of a small U-Net
with the switch on and off."""
import ctypes as C
from functools import partial

import pytest
import torch
from torch import nn

from raw_ops import _p
from segmentation_pipeline_amd import ops
from segmentation_pipeline_amd._lib import NormDesc
from segmentation_pipeline_amd.models import ModularUNet

pytestmark = pytest.mark.gpu

LEAKY, GELU = 2, 4
N, CC = 2, 16


def offset_copy(t, floats):
    """a dense copy of t whose base pointer sits `floats` floats behind an aligned address"""
    buf = torch.empty(t.numel() + floats, dtype=t.dtype, device=t.device)
    v = buf[floats:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * floats) % 16
    return v


def fused(hip, x, dskip, dskip_bs, dpool, mean, rstd, gamma, beta, groups, act, dx):
    _, _, D, H, W = x.shape
    d = NormDesc(N, CC, D * H * W, groups, act, 1e-5, 0.01, 0, 0, 0)
    dg, db = hip.empty(CC), hip.empty(CC)
    ws = hip._ws("norm_workspace", d)
    hip._chk(hip.fn("norm_act_bwd_pool")(C.byref(d), _p(x), _p(dskip), dskip_bs, _p(dpool), 0, D, H, W, _p(mean), _p(rstd),
                                         _p(gamma), _p(beta), _p(dx), _p(dg), _p(db), 1, _p(ws), ws.numel(), hip._stream()),
             "norm_act_bwd_pool")
    return dx, dg, db


# what is offset by one float: nothing | x and dx (the two-step form runs its scalar kernels too) | the skip gradient (the
# two-step form keeps its vector kernels on the dense sum: the fused pass must keep their element-to-thread mapping)
@pytest.mark.parametrize("skip,misaligned", [(s, m) for s in ("dense", "slice", "absent") for m in ("none", "x", "dskip")
                                             if (s, m) != ("absent", "dskip")])
@pytest.mark.parametrize("spatial", [(4, 6, 8), (4, 6, 6)])
@pytest.mark.parametrize("groups,act", [(8, LEAKY), (0, GELU)])
def test_pool_backward_has_the_bits_of_the_two_step_form(hip, spatial, skip, misaligned, groups, act):
    g = torch.Generator().manual_seed(7)
    shape = (N, CC) + spatial
    x = torch.randn(shape, generator=g).cuda()
    dpool = torch.randn((N, CC) + tuple(v // 2 for v in spatial), generator=g).cuda()
    gamma, beta = (torch.rand(CC, generator=g) + 0.5).cuda(), torch.randn(CC, generator=g).cuda()
    mean, rstd, _, _ = hip.norm_stats(x, groups)
    dskip, dskip_bs = None, 0
    if skip == "dense":
        dskip = torch.randn(shape, generator=g).cuda()
    elif skip == "slice":   # a channel slice of a wider gradient, as the decoder's concat gradient hands it over
        wide = torch.randn((N, 40) + spatial, generator=g).cuda()
        if misaligned == "dskip":
            wide = offset_copy(wide, 1)
        dskip, dskip_bs = wide[:, 8:8 + CC], wide.stride(0)
    if skip == "dense" and misaligned == "dskip":
        dskip = offset_copy(dskip, 1)
    if misaligned == "x":
        x = offset_copy(x, 1)
    dx = torch.empty_like(x) if misaligned != "x" else offset_copy(torch.empty_like(x), 1)

    # the two-step form: the sum into a dense tensor, then the usual backward
    dense_skip = None if dskip is None else dskip.contiguous()
    tot = hip.avgpool_bwd(dpool, shape) if dskip is None else hip.avgpool_bwd_add(dpool, dense_skip, shape)
    d = NormDesc(N, CC, x[0, 0].numel(), groups, act, 1e-5, 0.01, 0, 0, 0)
    ref_dx = torch.empty_like(x) if misaligned != "x" else offset_copy(torch.empty_like(x), 1)
    ref_dg, ref_db = hip.empty(CC), hip.empty(CC)
    ws = hip._ws("norm_workspace", d)
    hip._chk(hip.fn("norm_act_bwd")(C.byref(d), _p(x), _p(tot), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(ref_dx), _p(ref_dg),
                                    _p(ref_db), 1, _p(ws), ws.numel(), hip._stream()), "norm_act_bwd")

    got_dx, got_dg, got_db = fused(hip, x, dskip, dskip_bs, dpool, mean, rstd, gamma, beta, groups, act, dx)
    torch.cuda.synchronize()
    assert torch.isfinite(got_dx).all()
    assert torch.equal(got_dx, ref_dx), (got_dx - ref_dx).abs().max().item()
    assert torch.equal(got_dg, ref_dg) and torch.equal(got_db, ref_db)


def test_pool_backward_across_chunks_and_blocks(hip):
    """more than one chunk of the first pass per channel (16384 elements) and more than one block row of the second: 32^3,
    GroupNorm(8), a sliced skip gradient; two calls give the same bits"""
    g = torch.Generator().manual_seed(11)
    spatial = (32, 32, 32)
    shape = (N, CC) + spatial
    x = torch.randn(shape, generator=g).cuda()
    dpool = torch.randn((N, CC, 16, 16, 16), generator=g).cuda()
    wide = torch.randn((N, 24) + spatial, generator=g).cuda()
    dskip = wide[:, 4:4 + CC]
    gamma, beta = (torch.rand(CC, generator=g) + 0.5).cuda(), torch.randn(CC, generator=g).cuda()
    mean, rstd, _, _ = hip.norm_stats(x, 8)
    tot = hip.avgpool_bwd_add(dpool, dskip.contiguous(), shape)
    ref = hip.norm_act_bwd(x, tot, mean, rstd, gamma, beta, 8, LEAKY)
    a = fused(hip, x, dskip, wide.stride(0), dpool, mean, rstd, gamma, beta, 8, LEAKY, torch.empty_like(x))
    b = fused(hip, x, dskip, wide.stride(0), dpool, mean, rstd, gamma, beta, 8, LEAKY, torch.empty_like(x))
    torch.cuda.synchronize()
    for got, again, want in zip(a, b, ref):
        assert torch.equal(got, want) and torch.equal(got, again)


GN8 = {'normalization_class': partial(nn.GroupNorm, 8)}
CONVT = dict(upsample_class=nn.ConvTranspose3d, upsample_params={'kernel_size': 2, 'stride': 2})


def one_backward(build, monkeypatch, fuse):
    monkeypatch.setattr(ops, "FUSE_POOL_BWD", fuse)
    ops.fused_bwd_counts["pool"] = 0
    torch.manual_seed(0)
    model = build().cuda().train()
    x = torch.randn((2, 4, 16, 16, 32), generator=torch.Generator().manual_seed(3)).cuda()
    model(x).square().mean().backward()
    torch.cuda.synchronize()
    return {k: v.grad.clone() for k, v in model.named_parameters()}, ops.fused_bwd_counts["pool"]


def test_model_gradients_are_unchanged_and_every_pooled_block_is_fused(monkeypatch):
    """ModularUNet on three levels: the two encoder blocks in front of a pool take the fused backward; every parameter
    gradient has the bits of the run with the switch off"""
    build = lambda: ModularUNet(4, 3, [8, 16, 32], 3, block_params=dict(GN8), **CONVT)
    off, n_off = one_backward(build, monkeypatch, False)
    on, n_on = one_backward(build, monkeypatch, True)
    assert (n_off, n_on) == (0, 2)
    assert all(torch.isfinite(v).all() for v in on.values())
    for k in off:
        assert torch.equal(on[k], off[k]), k


def test_residual_blocks_keep_the_two_step_form(monkeypatch):
    """a block with a residual branch adds it inside its last pass and pools separately: nothing to fuse, nothing changes"""
    build = lambda: ModularUNet(4, 3, [8, 16, 32], 3, block_params=dict(GN8, residual=True), **CONVT)
    off, n_off = one_backward(build, monkeypatch, False)
    on, n_on = one_backward(build, monkeypatch, True)
    assert (n_off, n_on) == (0, 0)
    for k in off:
        assert torch.equal(on[k], off[k]), k
