"""The slot harness of raw_ops (Slot: a tensor embedded in a canary-filled concat buffer) checked on the CPU oracle.

The GPU suite (test_strided_slots_gpu.py) relies on two things that can be validated without a device: the harness
sees what it claims to see (stray writes, unwritten elements, modified inputs, a wrong stride), and the C oracle honours
batch strides -- run on slots it gives the very bits of its dense call.
"""
import pytest
import torch

from raw_ops import Slot


def rnd(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


LAYOUTS = [dict(c_pre=4, c_post=4, lead=0), dict(c_pre=1, c_post=2, lead=0), dict(c_pre=3, c_post=1, lead=1),
           dict(c_pre=0, c_post=1, lead=2, extra=3)]


def test_slot_layout_and_canaries():
    x = rnd(2, 3, 3, 5, 7, seed=1)
    s = Slot("cpu", None, c_pre=3, c_post=2, lead=1, extra=5, data=x)
    S = 3 * 5 * 7
    assert s.bs == (3 + 3 + 2) * S + 5 and s.unit == S
    assert s.ptr == s.ibuf.data_ptr() + 4 * s.off and s.misalign() == (4 * (1 + 3 * S)) % 16
    assert s.off >= S + 1 + 3 * S and s.off - 1 - 3 * S >= 64 and (s.off - 1 - 3 * S) % 16 == 0   # front guard
    assert s.ibuf.numel() - (s.off + s.bs + 3 * S + 2 * S + 5) >= max(S, 64)                       # tail guard
    assert torch.equal(s.result(), x) and s.result().is_contiguous()
    s.assert_guards_intact()
    s.assert_unchanged()
    # everything outside the slot is the canary, bit for bit
    assert int((s.ibuf == s.canary).sum()) == s.ibuf.numel() - x.numel()
    assert torch.isnan(s.ibuf.view(torch.float32)[0])
    # 16-bit slots in units of channel blocks
    for dt in (torch.bfloat16, torch.float16):
        h = Slot("cpu", (2, 2, 10, 8), c_pre=1, c_post=1, dtype=dt)
        assert h.bs == 4 * 80 and h.misalign() == 0 and torch.isnan(h.view().float()).all()
        h.assert_untouched()
        with pytest.raises(AssertionError):
            h.assert_fully_written()


def test_slot_detects_stray_writes_missing_writes_and_modified_inputs():
    S = 2 * 3 * 5
    for where in ("front", "between", "post", "tail"):
        o = Slot("cpu", (2, 2, 2, 3, 5), c_pre=1, c_post=1, lead=1)
        o.view().fill_(1.0)
        o.check_output()
        flat = o.ibuf.view(torch.float32)
        at = {"front": o.off - 1, "between": o.off + 2 * S + S + 3, "post": o.off + 2 * S, "tail": o.off + o.bs + 3 * S}[where]
        flat[at] = 0.0
        with pytest.raises(AssertionError, match="outside the slot"):
            o.assert_guards_intact()
    o = Slot("cpu", (2, 2, 2, 3, 5))
    o.view().fill_(1.0)
    o.view()[1, 1, 1, 2, 4] = float("nan")                    # an ordinary NaN is a value, not the canary
    o.assert_fully_written()
    o.ibuf[o.off + o.bs + 2 * S - 1] = o.canary                # the last element of sample 1 left unwritten
    with pytest.raises(AssertionError, match="never written"):
        o.assert_fully_written()
    i = Slot("cpu", None, data=rnd(1, 2, 2, 3, 5))
    i.view()[0, 0, 0, 0, 0] += 1.0
    with pytest.raises(AssertionError, match="modified"):
        i.assert_unchanged()
    r = Slot("cpu", (1, 2, 2, 3, 5))
    r.assert_untouched()
    r.view()[0, 1, 0, 0, 0] = 0.0
    with pytest.raises(AssertionError, match="rejected"):
        r.assert_untouched()


def _same(slot, dense, what):
    got = slot.check_output(what)
    assert torch.equal(got, dense), f"{what}: the oracle on slots differs from its dense call"


@pytest.mark.parametrize("lay", LAYOUTS, ids=lambda l: "-".join(f"{k}{v}" for k, v in l.items()))
def test_oracle_on_slots_matches_dense_conv(oracle, lay):
    lay2 = dict(lay, c_pre=lay["c_post"], c_post=lay["c_pre"] + 1)      # input and output strides differ
    for (N, ci, co, D, H, W, k, s, p) in [(2, 3, 5, 3, 5, 7, 3, 1, 1), (2, 2, 3, 4, 6, 6, 4, 2, 1), (1, 4, 2, 3, 3, 5, 3, 1, 1)]:
        x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(co, ci, k, k, k, seed=2) * 0.2, rnd(co, seed=3)
        y = oracle.conv3d_fwd(x, w, b, None, s, p)
        add, dy = rnd(*y.shape, seed=4), rnd(*y.shape, seed=5)
        xs, ads = oracle.slot(x, **lay), oracle.slot(add, **lay2)
        out = oracle.conv3d_fwd(xs, w, b, ads, s, p, out=oracle.slot(y.shape, **lay2))
        _same(out, oracle.conv3d_fwd(x, w, b, add, s, p), "conv3d_fwd")
        xs.assert_unchanged()
        ads.assert_unchanged()
        dys = oracle.slot(dy, **lay2)
        _same(oracle.conv3d_bwd_data(dys, w, x.shape, s, p, out=oracle.slot(x.shape, **lay)),
              oracle.conv3d_bwd_data(dy, w, x.shape, s, p), "conv3d_bwd_data")
        dw, db = oracle.conv3d_bwd_weight(xs, dys, k, s, p)
        dw0, db0 = oracle.conv3d_bwd_weight(x, dy, k, s, p)
        assert torch.equal(dw, dw0) and torch.equal(db, db0)
        dys.assert_unchanged()
    st = oracle.conv3d_fwd_stats(oracle.slot(x, **lay), w, b, 1, out=oracle.slot(y.shape, **lay2))
    st0 = oracle.conv3d_fwd_stats(x, w, b, 1)
    _same(st[0], st0[0], "conv3d_fwd_stats")
    assert torch.equal(st[1], st0[1]) and torch.equal(st[2], st0[2])


@pytest.mark.parametrize("lay", LAYOUTS, ids=lambda l: "-".join(f"{k}{v}" for k, v in l.items()))
def test_oracle_on_slots_matches_dense_conv_transpose(oracle, lay):
    lay2 = dict(lay, c_pre=lay["c_post"], c_post=lay["c_pre"] + 1)
    for (N, ci, co, D, H, W, k, s, p, op) in [(2, 3, 5, 2, 3, 5, 2, 2, 0, 0), (2, 2, 3, 3, 3, 3, 3, 2, 1, 1), (1, 4, 4, 2, 2, 3, 4, 2, 1, 0)]:
        x, w, b = rnd(N, ci, D, H, W, seed=1), rnd(ci, co, k, k, k, seed=2) * 0.3, rnd(co, seed=3)
        y = oracle.convt_fwd(x, w, b, s, p, op)
        dy = rnd(*y.shape, seed=5)
        xs, dys = oracle.slot(x, **lay), oracle.slot(dy, **lay2)
        _same(oracle.convt_fwd(xs, w, b, s, p, op, out=oracle.slot(y.shape, **lay2)), y, "convt_fwd")
        _same(oracle.convt_bwd_data(dys, w, x.shape, s, p, op, out=oracle.slot(x.shape, **lay)),
              oracle.convt_bwd_data(dy, w, x.shape, s, p, op), "convt_bwd_data")
        dw, db = oracle.convt_bwd_weight(xs, dys, k, s, p, op)
        dw0, db0 = oracle.convt_bwd_weight(x, dy, k, s, p, op)
        assert torch.equal(dw, dw0) and torch.equal(db, db0)
        xs.assert_unchanged()
        dys.assert_unchanged()


@pytest.mark.parametrize("lay", LAYOUTS, ids=lambda l: "-".join(f"{k}{v}" for k, v in l.items()))
def test_oracle_on_slots_matches_dense_norm_pool_upsample(oracle, lay):
    lay2 = dict(lay, c_pre=lay["c_post"], c_post=lay["c_pre"] + 1)
    lay3 = dict(lay, c_pre=2, c_post=3)
    for (N, Cc, D, H, W, groups, act) in [(2, 4, 3, 5, 7, 2, 1), (2, 3, 2, 4, 6, 0, 2), (1, 6, 2, 2, 4, 3, 0)]:
        x, gamma, beta = rnd(N, Cc, D, H, W, seed=1) * 1.7 + 0.3, rnd(Cc, seed=2), rnd(Cc, seed=3)
        add, dy = rnd(N, Cc, D, H, W, seed=4), rnd(N, Cc, D, H, W, seed=7)
        running = None if groups else (rnd(Cc, seed=5) * 0.1, torch.rand(Cc) + 0.5)
        xs = oracle.slot(x, **lay)
        st, st0 = oracle.norm_stats(xs, groups, running=running), oracle.norm_stats(x, groups, running=running)
        assert all(a is None and b is None or torch.equal(a, b) for a, b in zip(st, st0))
        mean, rstd = st0[:2]
        ads = oracle.slot(add, **lay3)
        _same(oracle.norm_act_fwd(xs, mean, rstd, gamma, beta, groups, act, ads, out=oracle.slot(x.shape, **lay2)),
              oracle.norm_act_fwd(x, mean, rstd, gamma, beta, groups, act, add), "norm_act_fwd")
        dys = oracle.slot(dy, **lay2)
        dx, dg, db = oracle.norm_act_bwd(xs, dys, mean, rstd, gamma, beta, groups, act, out=oracle.slot(x.shape, **lay))
        dx0, dg0, db0 = oracle.norm_act_bwd(x, dy, mean, rstd, gamma, beta, groups, act)
        _same(dx, dx0, "norm_act_bwd")
        assert torch.equal(dg, dg0) and torch.equal(db, db0)
        for s in (xs, ads, dys):
            s.assert_unchanged()
    for shape in [(2, 3, 2, 4, 6), (2, 2, 4, 2, 10), (1, 5, 2, 2, 2)]:
        x = rnd(*shape, seed=1)
        y = oracle.avgpool_fwd(x)
        dy = rnd(*y.shape, seed=2)
        xs, dys, ads = oracle.slot(x, **lay), oracle.slot(dy, **lay2), oracle.slot(x * 0.5, **lay3)
        _same(oracle.avgpool_fwd(xs, out=oracle.slot(y.shape, **lay2)), y, "avgpool_fwd")
        _same(oracle.avgpool_bwd(dys, x.shape, out=oracle.slot(x.shape, **lay)), oracle.avgpool_bwd(dy, x.shape), "avgpool_bwd")
        _same(oracle.avgpool_bwd_add(dys, ads, x.shape, out=oracle.slot(x.shape, **lay)),
              oracle.avgpool_bwd_add(dy, x * 0.5, x.shape), "avgpool_bwd_add")
        up = oracle.upsample_fwd(x)
        _same(oracle.upsample_fwd(xs, out=oracle.slot(up.shape, **lay2)), up, "upsample_fwd")
        dup = rnd(*up.shape, seed=3)
        _same(oracle.upsample_bwd(oracle.slot(dup, **lay2), x.shape, out=oracle.slot(x.shape, **lay)),
              oracle.upsample_bwd(dup, x.shape), "upsample_bwd")
        s2d = oracle.space_to_depth(x)
        _same(oracle.space_to_depth(xs, out=oracle.slot(s2d.shape, **lay2)), s2d, "space_to_depth")
        _same(oracle.depth_to_space(oracle.slot(s2d, **lay2), out=oracle.slot(x.shape, **lay)), x, "depth_to_space")
        _same(oracle.copy_channels(xs, out=oracle.slot(x.shape, **lay3)), x, "copy_channels")
        for s in (xs, dys, ads):
            s.assert_unchanged()


def test_wrong_stride_is_caught(oracle):
    """A stride that is off by one channel, or by one element, but stays inside the guarded buffer: sample 1 lands in
    the foreign channels around the slot.  The harness must see both the stray writes and the hole they leave."""
    N, ci, co, D, H, W = 2, 3, 4, 3, 5, 7
    S = D * H * W
    x, w = rnd(N, ci, D, H, W, seed=1), rnd(co, ci, 3, 3, 3, seed=2) * 0.2
    y0 = oracle.conv3d_fwd(x, w)
    for delta in (-S, S, -1, 1):
        out = oracle.slot(y0.shape, c_pre=2, c_post=2)
        out.bs_arg = out.bs + delta
        oracle.conv3d_fwd(x, w, out=out)
        with pytest.raises(AssertionError, match="outside the slot"):
            out.assert_guards_intact()
        with pytest.raises(AssertionError, match="never written"):
            out.assert_fully_written()
        assert torch.equal(out.result()[0], y0[0])       # (sample 0 does not depend on the stride)
    # a wrong INPUT stride: reads run into the canary, the result turns NaN
    xs = oracle.slot(x, c_pre=2, c_post=2)
    xs.bs_arg = xs.bs + 1
    y = oracle.conv3d_fwd(xs, w)
    assert torch.isfinite(y[0]).all() and torch.isnan(y[1]).any()
    # norm + activation reading add with y's stride (add's buffer is the wider one, so the reads stay inside it)
    Cc = 4
    xn, add = rnd(N, Cc, D, H, W, seed=3), rnd(N, Cc, D, H, W, seed=4)
    mean, rstd = oracle.norm_stats(xn, 2)[:2]
    ads, out = oracle.slot(add, c_pre=1, c_post=3), oracle.slot(xn.shape, c_pre=2, c_post=1)
    ads.bs_arg = out.bs
    got = oracle.norm_act_fwd(xn, mean, rstd, None, None, 2, 1, ads, out=out).result()
    ref = oracle.norm_act_fwd(xn, mean, rstd, None, None, 2, 1, add)
    assert torch.equal(got[0], ref[0]) and not torch.equal(got[1], ref[1])
