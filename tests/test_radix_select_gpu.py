"""The radix select of csrc/radix_select.hpp through its three users, on the bins where a pick can go
wrong: the first and last bin of a lane's run of 32, of a thread's 8 or 4, and of the histogram.

The inputs are built from uint32 keys: one digit of the three (11 / 11 / 10 bits at shifts 21 / 10 / 0) takes a list of
edge values while the other two are held fixed, and the floats are the inverse key transform in numpy.  Every answer is
an element of the input, so every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import topk_loss_ref as T
from segmentation_pipeline_amd import _lib, ops
from segmentation_pipeline_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _order_stats(x, ks, fracs):
    """m355_aug_order_stats of two ranks, called as in test_augmentation_gpu._order_stats"""
    L = _lib.lib()
    t = torch.from_numpy(np.ascontiguousarray(x.reshape(1, 1, 1, -1))).to(DEV)
    out = torch.empty(len(ks), dtype=torch.float64, device=DEV)
    ws = torch.empty(int(L.m355_aug_workspace()), dtype=torch.uint8, device=DEV)
    _lib.check(L.m355_aug_order_stats(_p(t), 1, (C.c_int32 * 3)(1, 1, x.size), None, 0, len(ks),
                                      (C.c_int64 * 2)(*ks), (C.c_double * 2)(*fracs), _p(out), _p(ws), ws.numel(),
                                      _stream()), "order_stats")
    return out.cpu().numpy()

SHIFT = (21, 10, 0)
FIXED = (1531, 777, 333)        # the digits that are held: a positive float of ordinary size
# digit 0 restricted to finite floats: 0 .. 3 and 2044 .. 2047 are the infinities and the NaNs
EDGES = {0: [4, 31, 32, 33, 63, 64, 1023, 1024, 2015, 2016, 2043],
         1: [0, 1, 31, 32, 33, 63, 64, 1023, 1024, 2015, 2016, 2046, 2047],
         # the list of digit 1 capped at 1023, and the last lane's run of the 1024-bin histogram
         2: [0, 1, 31, 32, 33, 63, 64, 991, 992, 1022, 1023]}


def key2f(keys):
    """the floats whose order-preserving keys are `keys`: the inverse of f2key"""
    keys = np.asarray(keys, dtype=np.uint32)
    bits = np.where(keys & np.uint32(0x80000000), keys & np.uint32(0x7fffffff), ~keys)
    return bits.astype(np.uint32).view(np.float32)


def _case(p):
    digits = EDGES[p] + [EDGES[p][2], EDGES[p][-1]]          # two of the values twice
    keys = []
    for d in digits:
        dg = list(FIXED)
        dg[p] = d
        keys.append(sum(v << s for v, s in zip(dg, SHIFT)))
    x = key2f(keys)
    x = x[np.random.default_rng(100 + p).permutation(x.size)]
    assert np.isfinite(x).all() and 13 <= x.size <= 15
    assert np.unique(x).size == x.size - 2
    return x


CASES = {p: _case(p) for p in (0, 1, 2)}


@pytest.mark.parametrize("p", [0, 1, 2])
def test_aug_order_stats_every_rank(p):
    """m355_aug_order_stats at fraction 0: rank k is np.sort(x)[k] for every k.  Two ranks a call; 0 and n - 1 are never
    asked together, which would take the min / max shortcut instead of the select."""
    x = CASES[p]
    n, s = x.size, np.sort(x)
    for k in range(0, n, 2):
        k2 = k + 1 if k + 1 < n else 1
        got = _order_stats(x, [k, k2], [0.0, 0.0])
        assert got[0] == s[k] and got[1] == s[k2], (p, k, k2, got, s[k], s[k2])


@pytest.mark.parametrize("p", [0, 1, 2])
def test_region_stats_median_of_every_prefix(p):
    """ops.region_stats: the median of the region holding the first m values is np.sort(x[:m])[(m - 1) // 2] for every
    m; the rows 'all' (label != 0, the same voxels) and 'whole' (all n values) with it"""
    x = CASES[p]
    n = x.size
    img = torch.from_numpy(x.reshape(1, 1, 1, n)).to(DEV)
    labs = []
    for m in range(1, n + 1):
        lab = torch.zeros((1, 1, n), dtype=torch.uint8)
        lab[..., :m] = 1
        labs.append(lab.to(DEV))
    res = ops.region_stats(labs, [[img]] * n, [1])
    med = res.stats[:, :, 0, 2].numpy()                      # [subject, (region 1, all, whole)]
    whole = np.sort(x)[(n - 1) // 2]
    for m in range(1, n + 1):
        want = np.sort(x[:m])[(m - 1) // 2]
        assert med[m - 1, 0] == want and med[m - 1, 1] == want and med[m - 1, 2] == whole, (p, m, med[m - 1], want, whole)
        assert int(res.count[m - 1, 0]) == m


@pytest.fixture(scope="module")
def topk_inputs():
    """N = 2, C = 3, S = 5 * 7 * 9 probabilities; a quarter of the voxels predict 1 / 3 for every class: their e tie"""
    g = torch.Generator().manual_seed(7)
    N, Cn, S = 2, 3, 5 * 7 * 9
    p = torch.softmax(2 * torch.randn((N, Cn, S), generator=g), dim=1)
    tie = (torch.randperm(N * S, generator=g) < N * S // 4).reshape(N, 1, S)
    p = torch.where(tie, torch.full_like(p, 1.0 / 3.0), p)
    t = torch.zeros(N, Cn, S).scatter_(1, torch.randint(0, Cn, (N, 1, S), generator=g), 1.0)
    return p.reshape(N, Cn, 5, 7, 9).cuda(), t.reshape(N, Cn, 5, 7, 9).cuda(), N * S


@pytest.mark.parametrize("device_k", [False, True], ids=["host_k", "device_k"])
def test_topk_threshold_is_the_kth_largest_bit_for_bit(topk_inputs, device_k):
    """the threshold of m355_topk_loss_fwd is torch.topk(e, k).values[-1] on the e the forward wrote, for k at both ends
    and in the middle (inside the tie for some of them), as a host number and as a device scalar.
    (test_topk_loss_gpu.py compares the threshold with torch's fp32 cross-entropy within 2 ulp; this is the select alone.)"""
    x, t, M = topk_inputs
    seen_tie = False
    for k in (1, 2, M // 2, M - 1, M):
        kw = dict(k_device=torch.tensor(k, dtype=torch.int64, device=DEV)) if device_k else dict(k=k)
        out3, sums, e, state = T.raw_fwd(x, t, **kw)
        tau, r, k_state = T.state_fields(state)
        want = torch.topk(e, k).values[-1]
        assert k_state == k
        assert state[:1].view(torch.int32).item() == want.view(torch.int32).item(), (k, tau, want.item())
        n_gt, n_eq = int((e > want).sum()), int((e == want).sum())
        assert n_gt < k <= n_gt + n_eq
        assert r == torch.tensor((k - n_gt) / n_eq, dtype=torch.float32).item(), (k, r, n_gt, n_eq)
        seen_tie |= n_eq > 1
    assert seen_tie
