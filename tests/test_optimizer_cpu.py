"""segmentation_pipeline_amd.optim without a GPU: the fp64 reference is pinned to torch itself, the library's block plan and
argument checks are pure host code, and the optimizers refuse what they do not implement when they are built."""
import ctypes as C
import math

import pytest
import torch

import optim_ref as R
from segmentation_pipeline_amd import _lib, optim

L = _lib.lib()
CAP = L.m355_optim_capacity()


def plan(counts):
    T = len(counts)
    arr = (C.c_int64 * T)(*counts)
    blk0, nblk = (C.c_int64 * T)(), (C.c_int64 * T)()
    chunk, ws = C.c_int32(), C.c_size_t()
    assert L.m355_optim_plan(arr, T, C.byref(chunk), blk0, nblk, C.byref(ws)) == 0, L.m355_last_error()
    return chunk.value, list(blk0), list(nblk), ws.value


CHUNK = plan([1])[0]


# ------------------------------------------------------------------------------------------------ reference vs torch
@pytest.mark.parametrize("case", R.option_grid(), ids=lambda c: c[0])
def test_reference_is_torch_in_fp64(case):
    """RefOptimizer and torch.optim + clip_grad_norm_ + PolynomialLR + lerp evaluate the same expressions: in fp64 they agree
    to 1e-12 relative over 6 steps"""
    _, rule, hypers, extras = case
    specs, params, grads = R.tensor_set(64, seed=3)
    ref, rec = R.run_reference(rule, specs, params, grads, hypers, extras)
    ex = R.resolve_extras(extras)
    tr = R.torch_stack(rule, R.build_groups(specs, params, hypers, torch.float64), [R.split_groups(specs, g) for g in grads],
                       **ex)

    def close(a, b, what):
        assert a.dtype == b.dtype == torch.float64
        err = (a - b).abs().max().item()
        assert err <= 1e-12 * max(b.abs().max().item(), 1e-300), f"{what}: {err}"

    for gi in range(2):
        for i, p in enumerate(ref.groups[gi]["params"]):
            close(p, tr["params"][gi][i], f"param {gi}/{i}")
            for k, v in tr["state"][gi][i].items():
                close(ref.state[gi][i][k], v, f"{k} {gi}/{i}")
            if ref.ema is not None:
                close(ref.ema[gi][i], tr["ema"][gi][i], f"ema {gi}/{i}")
    for step in range(R.STEPS):
        for gi in range(2):
            assert rec[step]["lr"][gi] == pytest.approx(tr["lr"][step][gi], rel=1e-12)
        if "max_grad_norm" in ex:
            assert rec[step]["norm"] == pytest.approx(tr["norm"][step], rel=1e-12)


def test_clip_engages_on_some_steps_only():
    """the tensor set of the GPU tests: the clip must be active on some of its steps and idle on others"""
    specs, params, grads = R.tensor_set(CHUNK, seed=R.GPU_SEED)
    _, rec = R.run_reference("sgd", specs, params, grads, (dict(lr=0.1), dict(lr=0.1)), {"max_grad_norm": None})
    coefs = [r["clip"] for r in rec]
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), coefs


# ------------------------------------------------------------------------------------------------ block plan
@pytest.mark.parametrize("counts", [[1], [0, 5], [CHUNK - 1, CHUNK, CHUNK + 1], [2 * CHUNK + 7, 3], [5] * CAP, [5] * (CAP + 1)],
                         ids=["one", "zero", "around-chunk", "two-chunks", "cap", "cap+1"])
def test_block_plan(counts):
    chunk, blk0, nblk, ws = plan(counts)
    assert chunk == CHUNK > 0
    at = 0
    for n, b0, nb in zip(counts, blk0, nblk):
        assert b0 == at, "block ranges are contiguous and disjoint"
        assert nb == (n + chunk - 1) // chunk, "every element lies in exactly one block of `chunk` elements"
        assert (nb - 1) * chunk < n <= nb * chunk if n else nb == 0
        at += nb
    assert ws >= 8 * at and ws >= 8, "one fp64 partial per block"


def test_capacity():
    assert 1 <= CAP and CAP * 56 + 1024 <= 4096, "the table travels in the kernel arguments"
    assert _lib.OPTIM_MAX_GROUPS >= 2


# ------------------------------------------------------------------------------------------------ argument validation
def _desc(rule=_lib.OPTIM_SGD, groups=1, clip=0, max_norm=0.0, total_steps=0, power=0.9, ema_decay=-1.0, **group):
    d = _lib.OptimDesc()
    d.rule, d.groups, d.clip, d.max_norm, d.total_steps, d.power, d.ema_decay = rule, groups, clip, max_norm, total_steps, \
        power, ema_decay
    for g in range(min(max(groups, 0), _lib.OPTIM_MAX_GROUPS)):
        q = d.group[g]
        q.lr, q.beta1, q.beta2, q.eps = 0.1, 0.9, 0.999, 1e-8
        for k, v in group.items():
            setattr(q, k, v)
    return d


def _tensors(count=1, **over):
    arr = (_lib.OptimTensor * max(count, 1))()
    for i in range(count):
        e = arr[i]
        e.param, e.grad, e.state1, e.state2, e.ema, e.n, e.blk0, e.group = 64, 128, 192, 256, 320, 5, i, 0
    for k, v in over.items():
        setattr(arr[0], k, v)
    return arr


P = C.c_void_p


def _fails(rc, name):
    assert rc == -1, rc
    assert name.encode() in L.m355_last_error(), L.m355_last_error()


def test_plan_validation():
    chunk, ws = C.c_int32(), C.c_size_t()
    one, out = (C.c_int64 * 1)(-3), (C.c_int64 * 1)()
    _fails(L.m355_optim_plan(one, 1, C.byref(chunk), out, out, C.byref(ws)), "optim_plan")
    _fails(L.m355_optim_plan(None, 1, C.byref(chunk), out, out, C.byref(ws)), "optim_plan")
    _fails(L.m355_optim_plan(one, -1, C.byref(chunk), out, out, C.byref(ws)), "optim_plan")
    _fails(L.m355_optim_plan(one, 1, None, out, out, C.byref(ws)), "optim_plan")


@pytest.mark.parametrize("what", ["null-table", "too-many", "none", "negative-count", "null-grad", "blk0", "null-workspace",
                                  "small-workspace"])
def test_norm_validation(what):
    t, n, ws, nbytes = _tensors(2), 2, P(4096), 4096
    if what == "null-table":
        t = None
    elif what == "too-many":
        t, n = _tensors(CAP + 1), CAP + 1
    elif what == "none":
        n = 0
    elif what == "negative-count":
        t = _tensors(2, n=-1)
    elif what == "null-grad":
        t = _tensors(2, grad=None)
    elif what == "blk0":
        t[1].blk0 = 5
    elif what == "null-workspace":
        ws = None
    elif what == "small-workspace":
        nbytes = 8
    _fails(L.m355_optim_norm(t, n, ws, nbytes, None), "optim_norm")


@pytest.mark.parametrize("what", ["null-desc", "rule", "groups", "null-state", "nslots", "workspace", "max-norm", "lr-nan",
                                  "lr-negative", "wd", "momentum", "nesterov", "beta", "eps", "ema", "power", "total-steps"])
def test_prepare_validation(what):
    d, nslots, ws, nbytes, state = _desc(), 4, P(4096), 4096, P(8192)
    if what == "null-desc":
        d = None
    elif what == "rule":
        d = _desc(rule=3)
    elif what == "groups":
        d = _desc(groups=_lib.OPTIM_MAX_GROUPS + 1)
    elif what == "null-state":
        state = None
    elif what == "nslots":
        nslots = -1
    elif what == "workspace":
        d, nbytes = _desc(clip=1, max_norm=1.0), 16
    elif what == "max-norm":
        d = _desc(clip=1, max_norm=math.inf)
    elif what == "lr-nan":
        d = _desc(lr=math.nan)
    elif what == "lr-negative":
        d = _desc(lr=-0.1)
    elif what == "wd":
        d = _desc(weight_decay=-1.0)
    elif what == "momentum":
        d = _desc(momentum=math.inf)
    elif what == "nesterov":
        d = _desc(nesterov=1, momentum=0.0)
    elif what == "beta":
        d = _desc(rule=_lib.OPTIM_ADAM, beta2=1.0)
    elif what == "eps":
        d = _desc(rule=_lib.OPTIM_ADAMW, eps=-1e-8)
    elif what == "ema":
        d = _desc(ema_decay=1.0)
    elif what == "power":
        d = _desc(total_steps=4, power=math.nan)
    elif what == "total-steps":
        d = _desc(total_steps=-4)
    _fails(L.m355_optim_prepare(C.byref(d) if d is not None else None, nslots, ws, nbytes, None, None, state, None),
           "optim_prepare")


@pytest.mark.parametrize("what", ["null-desc", "hyper", "null-table", "too-many", "negative-count", "null-param",
                                  "null-momentum", "null-exp-avg-sq", "null-ema", "group", "misaligned", "null-state"])
def test_update_validation(what):
    d, t, n, state = _desc(momentum=0.9), _tensors(2), 2, P(8192)
    if what == "null-desc":
        d = None
    elif what == "hyper":
        d = _desc(momentum=-0.5)
    elif what == "null-table":
        t = None
    elif what == "too-many":
        t, n = _tensors(CAP + 1), CAP + 1
    elif what == "negative-count":
        t = _tensors(2, n=-7)
    elif what == "null-param":
        t = _tensors(2, param=None)
    elif what == "null-momentum":
        t = _tensors(2, state1=None)
    elif what == "null-exp-avg-sq":
        d, t = _desc(rule=_lib.OPTIM_ADAM), _tensors(2, state2=None)
    elif what == "null-ema":
        d, t = _desc(ema_decay=0.9), _tensors(2, ema=None)
    elif what == "group":
        t = _tensors(2, group=1)
    elif what == "misaligned":
        t = _tensors(2, param=66)
    elif what == "null-state":
        state = None
    _fails(L.m355_optim_update(C.byref(d) if d is not None else None, t, n, state, None), "optim_update")


# ------------------------------------------------------------------------------------------------ the Python classes
def fake_params(*sizes):
    """parameters "on the device" without one: fake tensors carry device and layout, which is all construction looks at"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        return [torch.nn.Parameter(torch.empty(n, device="cuda")) for n in sizes]


@pytest.mark.parametrize("cls", [optim.FusedSGD, optim.FusedAdam])
def test_constructor_refusals(cls):
    kw = {"lr": 0.1}
    for flag in ("maximize", "differentiable") + (("amsgrad",) if cls is optim.FusedAdam else ()):
        with pytest.raises(NotImplementedError, match=flag):
            cls(fake_params(4), **kw, **{flag: True})
    with pytest.raises(ValueError, match="float32"):
        cls([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))], **kw)
    with pytest.raises(ValueError, match="HIP device"):
        cls([torch.nn.Parameter(torch.zeros(4))], **kw)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        strided = torch.nn.Parameter(torch.empty(4, 6, device="cuda").t())
        f64 = torch.nn.Parameter(torch.empty(4, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="contiguous"):
        cls([strided], **kw)
    with pytest.raises(ValueError, match="float32"):
        cls([f64], **kw)
    with pytest.raises(ValueError):
        cls(fake_params(4), **kw, max_grad_norm=-1.0)
    with pytest.raises(ValueError):
        cls(fake_params(4), **kw, ema_decay=1.0)
    with pytest.raises(NotImplementedError, match="maximize"):
        cls([{"params": fake_params(4), "maximize": True}], **kw)


@pytest.mark.parametrize("total_steps", [0, -3, 2.5])
def test_poly_lr_refuses(total_steps):
    with pytest.raises(ValueError, match="total_steps"):
        optim.PolyLR(total_steps)


def test_poly_lr_closed_form():
    s = optim.PolyLR(8, power=0.9)
    assert s.lr_at(0.1, 0) == 0.1 and s.lr_at(0.1, 8) == 0.0 == s.lr_at(0.1, 11)
    assert s.lr_at(0.1, 3) == pytest.approx(0.1 * (1 - 3 / 8) ** 0.9, rel=1e-15)


def test_state_dict_of_a_fresh_optimizer_has_torchs_keys():
    cpu = [torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(3))]
    for ours, theirs in ((optim.FusedSGD(fake_params(4, 3), lr=0.1, momentum=0.9, ema_decay=0.99, schedule=optim.PolyLR(8)),
                          torch.optim.SGD(cpu, lr=0.1, momentum=0.9)),
                         (optim.FusedAdam(fake_params(4, 3), lr=0.1), torch.optim.Adam(cpu, lr=0.1)),
                         (optim.FusedAdam(fake_params(4, 3), lr=0.1, decoupled_weight_decay=True),
                          torch.optim.AdamW(cpu, lr=0.1))):
        a, b = ours.state_dict(), theirs.state_dict()
        assert set(b) <= set(a) and a["state"] == b["state"] == {}
        assert len(a["param_groups"]) == len(b["param_groups"]) == 1
        assert set(a["param_groups"][0]) == set(b["param_groups"][0])
        assert a["param_groups"][0]["params"] == b["param_groups"][0]["params"] == [0, 1]
        theirs.load_state_dict(a)   # the extra key is ignored
        assert a["m355_optim"]["step"] == 0
        assert ours._step_supports_amp_scaling


def test_load_refuses_disagreeing_steps():
    theirs = torch.optim.Adam([torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(3))], lr=0.1)
    p, q = theirs.param_groups[0]["params"]
    p.grad, q.grad = torch.ones(4), torch.ones(3)
    theirs.step()
    q.grad = None
    theirs.step()
    sd = theirs.state_dict()
    assert float(sd["state"][0]["step"]) == 2 and float(sd["state"][1]["step"]) == 1
    with pytest.raises(ValueError, match="one step counter"):
        optim.FusedAdam(fake_params(4, 3), lr=0.1).load_state_dict(sd)
