"""FusedSGD / FusedAdam on the device against the fp64 reference of tests/optim_ref.py.

Tolerance of the trajectories (measured, not fixed): torch's own fp32 optimizer stack on the CPU on the same inputs is the
yardstick, e_torch = max |torch32 - ref64| per tensor, and the device must stay within 4 * e_torch + 2^-24 * max |ref64|.
The lines starting with `optimizer_accuracy` are what profiles/optimizer_accuracy.txt records."""
import copy
import ctypes as C

import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

PAD, CANARY = 8, 1234.5


def _lib_consts():
    from segmentation_pipeline_amd import _lib
    L = _lib.lib()
    chunk, ws = C.c_int32(), C.c_size_t()
    one, out = (C.c_int64 * 1)(1), (C.c_int64 * 1)()
    assert L.m355_optim_plan(one, 1, C.byref(chunk), out, out, C.byref(ws)) == 0
    return chunk.value, L.m355_optim_capacity()


CHUNK, CAP = _lib_consts()
_sets = {}


def tensor_set(many=None):
    """one seeded tensor set per kind, shared by the tests and never modified"""
    if many not in _sets:
        _sets[many] = R.tensor_set(CHUNK, seed=R.GPU_SEED, many=many)
    return _sets[many]


class Slot:
    """a float32 tensor of n elements inside a buffer of canaries, `off` elements past a 16-byte boundary"""

    def __init__(self, values, off=0):
        n = values.numel()
        self.buf = torch.full((n + 2 * PAD + 4,), CANARY, device="cuda")
        self.lo, self.hi = PAD + off, PAD + off + n
        self.view = self.buf[self.lo:self.hi]
        self.view.copy_(values.float())
        assert self.view.data_ptr() % 16 == 4 * off

    def intact(self):
        return bool((self.buf[:self.lo] == CANARY).all()) and bool((self.buf[self.hi:] == CANARY).all())


def make_fused(rule, specs, params, hypers, extras, guard_state=False):
    """-> (optimizer, parameter slots, gradient slots, state slots); parameters in the order of split_groups"""
    from segmentation_pipeline_amd import optim
    pslots = [Slot(p, s["p_off"]) for s, p in zip(specs, params)]
    gslots = [Slot(torch.zeros(s["n"]), s["g_off"]) if s["has_grad"] else None for s in specs]
    ps = [torch.nn.Parameter(sl.view) for sl in pslots]
    for p, sl in zip(ps, pslots):
        assert p.data_ptr() == sl.view.data_ptr()
    groups = [dict(h, params=g) for h, g in zip(hypers, R.split_groups(specs, ps))]
    ex = R.resolve_extras(extras)
    kw = dict(max_grad_norm=ex.get("max_grad_norm"), ema_decay=ex.get("ema_decay"),
              schedule=optim.PolyLR(ex["total_steps"]) if "total_steps" in ex else None)
    if rule == "sgd":
        opt = optim.FusedSGD(groups, lr=hypers[0]["lr"], **kw)
    else:
        opt = optim.FusedAdam(groups, lr=hypers[0]["lr"], decoupled_weight_decay=rule == "adamw", **kw)
    sslots = []
    if guard_state:   # optimizer state and EMA in guarded buffers, alignments mixed as well
        for i, (p, s) in enumerate(zip(ps, specs)):
            keys = ("exp_avg", "exp_avg_sq") if rule != "sgd" else (("momentum_buffer",) if hypers[0].get("momentum") else ())
            for k in keys:
                sl = Slot(torch.zeros(s["n"]), (i + len(k)) % 2)
                opt.state[p][k] = sl.view
                sslots.append(sl)
            if p in opt._ema:
                sl = Slot(p.detach().cpu(), i % 2)
                opt._ema[p] = sl.view
                sslots.append(sl)
    for p, g in zip(ps, gslots):
        if g is not None:
            p.grad = g.view
    return opt, ps, pslots, gslots, sslots


def load_grads(gslots, grads, scale=1.0):
    for sl, g in zip(gslots, grads):
        if sl is not None:
            sl.view.copy_((g * scale).float())


def everything(opt, ps):
    """every tensor a step may write, as clones"""
    out = [p.detach().clone() for p in ps]
    for p in ps:
        out += [v.clone() for v in opt.state.get(p, {}).values() if torch.is_tensor(v)]
    if opt.ema_decay is not None:
        out += [e.clone() for e in opt.ema_parameters()]
    return out


def same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def compare(tag, opt, ps, specs, ref, tr, worst):
    """the pass condition of the module docstring for parameters, state and EMA of every tensor"""
    ref_p, tr_p = [p for g in ref.groups for p in g["params"]], [p for g in tr["params"] for p in g]
    ref_s, tr_s = [s for g in ref.state for s in g], [s for g in tr["state"] for s in g]
    ref_e = [e for g in ref.ema for e in g] if ref.ema is not None else None
    tr_e = [e for g in tr["ema"] for e in g] if tr["ema"] is not None else None
    order = [i for g in (0, 1) for i, s in enumerate(specs) if s["group"] == g]   # split_groups order -> spec index
    fails = []

    def one(what, got, r64, t32):
        e_gpu = (got.detach().cpu().double() - r64).abs().max().item()
        e_torch = (t32.double() - r64).abs().max().item()
        bound = 4 * e_torch + 2.0 ** -24 * r64.abs().max().item()
        print(f"optimizer_accuracy {tag} {what}: max err {e_gpu:.3e}  torch fp32 on the CPU {e_torch:.3e}  bound {bound:.3e}")
        worst[0] = max(worst[0], e_gpu / bound if bound > 0 else (0.0 if e_gpu == 0 else float("inf")))
        if not e_gpu <= bound:
            fails.append((what, e_gpu, bound))

    emas = opt.ema_parameters() if opt.ema_decay is not None else None
    flat_ps = [p for g in opt.param_groups for p in g["params"]]
    for k, p in enumerate(flat_ps):
        n = specs[order[k]]["n"]
        one(f"param[{n}]", p, ref_p[k], tr_p[k])
        for key, v in ref_s[k].items():
            one(f"{key}[{n}]", opt.state[p][key], v, tr_s[k][key])
        if emas is not None:
            one(f"ema[{n}]", emas[k], ref_e[k], tr_e[k])
    assert not fails, fails


def run_case(case, many=None, guard_state=False):
    name, rule, hypers, extras = case
    specs, params, grads = tensor_set(many)
    ref, rec = R.run_reference(rule, specs, params, grads, hypers, extras)
    ex = R.resolve_extras(extras)
    tr = R.torch_stack(rule, R.build_groups(specs, params, hypers, torch.float32),
                       [R.split_groups(specs, [None if g is None else g.float() for g in gg]) for gg in grads], **ex)
    opt, ps, pslots, gslots, sslots = make_fused(rule, specs, params, hypers, extras, guard_state)
    for step, g in enumerate(grads):
        load_grads(gslots, g)
        opt.step()
        lr = opt.lr_now.cpu().double()
        for gi in range(2):
            assert abs(lr[gi].item() - rec[step]["lr"][gi]) <= 2.0 ** -23 * rec[step]["lr"][gi], (step, gi)
        if "max_grad_norm" in ex:
            assert abs(opt.grad_norm.item() - rec[step]["norm"]) <= 2.0 ** -23 * rec[step]["norm"], step
            assert abs(opt.clip_coef.item() - rec[step]["clip"]) <= 2.0 ** -23
        assert int(opt.skipped) == 0 and int(opt.step_count) == step + 1
    worst = [0.0]
    tag = name + ("" if many is None else f" x{many}") + (" guarded" if guard_state else "")
    compare(tag, opt, ps, specs, ref, tr, worst)
    print(f"optimizer_accuracy {tag}: worst err / bound {worst[0]:.3f}")
    for sl in pslots + [g for g in gslots if g is not None] + sslots:
        assert sl.intact(), "a guard canary was overwritten"
    # the parameter without a gradient and every gradient are untouched
    for s, p, sl, p0 in zip(specs, ps, pslots, params):
        if not s["has_grad"]:
            assert torch.equal(sl.view.cpu(), p0.float())
    for sl, g in zip(gslots, grads[-1]):
        if sl is not None:
            assert torch.equal(sl.view.cpu(), g.float()), "gradients are read, never written"
    return opt, ps


CASES = R.option_grid()
FULL = {c[0]: c for c in CASES}


# ------------------------------------------------------------------------------------------------ trajectories
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_trajectory(case):
    run_case(case)


@pytest.mark.parametrize("name", ["sgd-nesterov-wd-all", "adamw-wd-all"])
def test_trajectory_with_more_tensors_than_one_table(name):
    run_case(FULL[name], many=CAP + 1)


@pytest.mark.parametrize("name", ["sgd-nesterov-wd-all", "sgd-momentum", "adam-wd-all", "adamw-wd-all"])
def test_guard_canaries_around_state_and_ema(name):
    """optimizer state and EMA live in guarded, partly misaligned buffers as well (zero momentum buffers installed up front:
    with dampening 0 the first step then gives buf = 0 * momentum + g = g, as torch does with a loaded buffer)"""
    run_case(FULL[name], guard_state=True)


# ------------------------------------------------------------------------------------------------ norm
def test_norm_is_exact_to_an_ulp_and_repeats_bit_for_bit():
    specs, params, grads = tensor_set()
    name, rule, hypers, extras = FULL["sgd-plain-clip"]
    hypers = tuple(dict(h, lr=0.0) for h in hypers)
    opt, ps, pslots, gslots, _ = make_fused(rule, specs, params, hypers, extras)
    for g in grads[:3]:
        load_grads(gslots, g)
        want = sum(float((x ** 2).sum()) for x in g if x is not None) ** 0.5
        opt.step()
        a = opt.grad_norm.clone()
        opt.step()
        b = opt.grad_norm.clone()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        rel = abs(a.item() - want) / want
        print(f"optimizer_accuracy norm: {a.item():.9g} vs fp64 {want:.17g}  rel {rel:.3e}")
        assert rel <= 2.0 ** -23


# ------------------------------------------------------------------------------------------------ skip
@pytest.mark.parametrize("name", ["sgd-nesterov-wd-all", "adam-wd-all", "adamw-wd-all"])
def test_skip_leaves_every_bit(name):
    specs, params, grads = tensor_set()
    _, rule, hypers, extras = FULL[name]
    opt, ps, pslots, gslots, _ = make_fused(rule, specs, params, hypers, extras)
    load_grads(gslots, grads[0])
    opt.step()
    before, t = everything(opt, ps), int(opt.step_count)
    # an external flag
    load_grads(gslots, grads[1])
    opt.found_inf = torch.ones((), device="cuda")
    opt.step()
    assert int(opt.skipped) == 1 and int(opt.step_count) == t and same_bits(before, everything(opt, ps))
    # one inf in one gradient, clipping on, no flag
    del opt.found_inf
    gslots[5].view[17] = float("inf")
    opt.step()
    assert int(opt.skipped) == 1 and int(opt.step_count) == t and same_bits(before, everything(opt, ps))
    gslots[5].view[17] = float("nan")
    opt.step()
    assert int(opt.skipped) == 1 and int(opt.step_count) == t and same_bits(before, everything(opt, ps))
    # a lowered flag applies the step
    load_grads(gslots, grads[1])
    opt.found_inf = torch.zeros((), device="cuda")
    opt.step()
    assert int(opt.skipped) == 0 and int(opt.step_count) == t + 1 and not same_bits(before, everything(opt, ps))


@pytest.mark.parametrize("name", ["sgd-nesterov-wd-all", "adamw-wd-all", "adam"])
def test_grad_scale_is_removed_exactly(name):
    specs, params, grads = tensor_set()
    _, rule, hypers, extras = FULL[name]
    a, ps_a, _, gs_a, _ = make_fused(rule, specs, params, hypers, extras)
    b, ps_b, _, gs_b, _ = make_fused(rule, specs, params, hypers, extras)
    b.grad_scale = torch.tensor(8.0, device="cuda")
    for g in grads[:3]:
        load_grads(gs_a, g)
        load_grads(gs_b, g, scale=8.0)
        a.step()
        b.step()
    assert same_bits(everything(a, ps_a), everything(b, ps_b))
    if "max_grad_norm" in extras:
        assert torch.equal(a.grad_norm, b.grad_norm) and torch.equal(a.clip_coef, b.clip_coef)


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("name", ["sgd-nesterov-wd-all", "adamw-wd-all"])
def test_two_optimizers_agree_bit_for_bit(name):
    specs, params, grads = tensor_set()
    _, rule, hypers, extras = FULL[name]
    runs = []
    for _ in range(2):
        opt, ps, _, gslots, _ = make_fused(rule, specs, params, hypers, extras)
        for g in grads[:3]:
            load_grads(gslots, g)
            opt.step()
        runs.append(everything(opt, ps) + [opt.grad_norm.clone(), opt.lr_now.clone()])
    assert same_bits(*runs)


# ------------------------------------------------------------------------------------------------ checkpoints
def _plain_params(specs, params):
    return [torch.nn.Parameter(p.float().cuda()) for p in params]


def _within(tag, got, r64, t32):
    e_gpu = (got.detach().cpu().double() - r64).abs().max().item()
    e_torch = (t32.double() - r64).abs().max().item()
    bound = 4 * e_torch + 2.0 ** -24 * r64.abs().max().item()
    print(f"optimizer_accuracy {tag}: max err {e_gpu:.3e}  torch fp32 on the CPU {e_torch:.3e}  bound {bound:.3e}")
    assert e_gpu <= bound, tag


@pytest.mark.parametrize("direction", ["torch-adam-to-fused", "fused-sgd-to-torch"])
def test_checkpoints_interchange_with_torch(direction):
    from segmentation_pipeline_amd import optim
    specs, params, grads = tensor_set()
    rule = "adam" if direction == "torch-adam-to-fused" else "sgd"
    h = dict(lr=0.01, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05) if rule == "adam" else \
        dict(lr=0.05, momentum=0.9, weight_decay=0.01)
    live = [i for i, s in enumerate(specs) if s["has_grad"]]
    sp = [dict(specs[i], group=0) for i in live]
    p64, g64 = [params[i] for i in live], [[g[i] for i in live] for g in grads[:4]]
    ref, _ = R.run_reference(rule, sp, p64, g64, (h, h), {})
    tr = R.torch_stack(rule, R.build_groups(sp, p64, (h, h), torch.float32)[:1], [[[g.float() for g in gg]] for gg in g64])
    tcls = torch.optim.Adam if rule == "adam" else torch.optim.SGD
    fcls = optim.FusedAdam if rule == "adam" else optim.FusedSGD
    first_cls, second_cls = (tcls, fcls) if direction == "torch-adam-to-fused" else (fcls, tcls)
    pa = _plain_params(sp, p64)
    first = first_cls(pa, **h)

    def steps(opt, ps, gs):
        for gg in gs:
            for p, g in zip(ps, gg):
                p.grad = g.float().cuda()
            opt.step()

    steps(first, pa, g64[:2])
    sd = copy.deepcopy(first.state_dict())   # (a state_dict refers to the live state tensors, and loading does not copy them)
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    second = second_cls(pb, **h)
    second.load_state_dict(sd)
    steps(first, pa, g64[2:])
    steps(second, pb, g64[2:])
    for k, (a, b) in enumerate(zip(pa, pb)):
        _within(f"{direction} original param[{sp[k]['n']}]", a, ref.groups[0]["params"][k], tr["params"][0][k])
        _within(f"{direction} loaded param[{sp[k]['n']}]", b, ref.groups[0]["params"][k], tr["params"][0][k])
    fused = second if direction == "torch-adam-to-fused" else first
    assert int(fused.step_count) == 4
    if rule == "adam":
        sd2 = fused.state_dict()
        assert all(float(st["step"]) == 4.0 and st["step"].dtype == torch.float32 and st["step"].dim() == 0
                   for st in sd2["state"].values())


def test_ema_and_schedule_position_survive_a_checkpoint():
    from segmentation_pipeline_amd import optim
    specs, params, grads = tensor_set(many=5)
    mk = lambda: optim.FusedSGD([torch.nn.Parameter(p.float().cuda()) for p in params], lr=0.1, momentum=0.9, ema_decay=0.9,
                                schedule=optim.PolyLR(8))
    a, b = mk(), mk()

    def step(opt, g):
        for p, x in zip(opt.param_groups[0]["params"], g):
            p.grad = x.float().cuda()
        opt.step()

    step(a, grads[0])
    step(a, grads[1])
    with torch.no_grad():
        for p, q in zip(a.param_groups[0]["params"], b.param_groups[0]["params"]):
            q.copy_(p)
    b.load_state_dict(copy.deepcopy(a.state_dict()))
    step(a, grads[2])
    step(b, grads[2])
    assert int(b.step_count) == 3 and torch.equal(a.lr_now, b.lr_now) and float(b.lr_now[0]) < 0.1
    assert same_bits(everything(a, a.param_groups[0]["params"]), everything(b, b.param_groups[0]["params"]))


# ------------------------------------------------------------------------------------------------ versions, packed weights
def _tiny():
    from segmentation_pipeline_amd.models import ModularUNet
    return ModularUNet(1, 2, [8, 16], 2)


def _batches(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        x = torch.randn((1, 1, 16, 16, 16), generator=g)
        lab = torch.randint(0, 2, (1, 16, 16, 16), generator=g)
        out.append({"X": x.cuda(), "y": torch.nn.functional.one_hot(lab, 2).permute(0, 4, 1, 2, 3).float().contiguous().cuda()})
    return out


def _fresh_copy(model):
    m = _tiny().cuda()
    m.load_state_dict(model.state_dict())
    return m.eval()


def test_versions_advance_and_no_stale_packed_weight_is_used():
    from segmentation_pipeline_amd import optim
    from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss
    torch.manual_seed(0)
    model = _tiny().cuda().train()
    opt = optim.FusedSGD(model.parameters(), lr=0.05, momentum=0.9, ema_decay=0.5)
    b = _batches(1)[0]
    crit = HybridLogisticDiceLoss()
    for _ in range(2):
        opt.zero_grad()
        crit(model(b["X"]), b["y"])["loss"].backward()
        versions = [p._version for p in model.parameters()]
        opt.step()
        assert all(p._version > v for p, v in zip(model.parameters(), versions) if p.grad is not None)
    model.eval()
    with torch.no_grad():
        after_step = model(b["X"])
        assert torch.equal(after_step, _fresh_copy(model)(b["X"]))
        raw = [p.detach().clone() for p in model.parameters()]
        with opt.ema_weights():
            assert all(torch.equal(p, e) for p, e in zip(model.parameters(), opt.ema_parameters()))
            inside = model(b["X"])
            assert torch.equal(inside, _fresh_copy(model)(b["X"]))
            assert not torch.equal(inside, after_step)
        assert all(torch.equal(p, r) for p, r in zip(model.parameters(), raw))
        assert torch.equal(model(b["X"]), after_step)


# ------------------------------------------------------------------------------------------------ through the trainer
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_graphed_train_step_advances_the_schedule_on_replay(mode):
    """3 eager warm-up calls, one capture, two replays: losses bit-identical to the eager loop, and the learning rate the
    replayed steps used follows PolyLR -- no optimizer that keeps its learning rate on the host can do that"""
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd import optim
    from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss
    from segmentation_pipeline_amd.trainer import GraphedTrainStep
    torch.manual_seed(0)
    m_e = _tiny().cuda().train()
    m_g = copy.deepcopy(m_e)
    crit = HybridLogisticDiceLoss()
    sched = optim.PolyLR(8)
    mk = lambda m: optim.FusedSGD(m.parameters(), lr=0.01, momentum=0.99, nesterov=True, max_grad_norm=12, ema_decay=0.99,
                                  schedule=optim.PolyLR(8))
    with sp.precision(mode):
        opt_e, opt_g = mk(m_e), mk(m_g)
        step = GraphedTrainStep(m_g, crit, opt_g, warmup=3)
        losses_e, losses_g, lrs = [], [], []
        for b in _batches(6):
            opt_e.zero_grad(set_to_none=True)
            ld = crit(m_e(b["X"]), b["y"])
            ld["loss"].backward()
            opt_e.step()
            losses_e.append(ld["loss"].detach().clone())
            losses_g.append(step(b)["loss"])
            lrs.append(float(opt_g.lr_now[0]))
            assert torch.equal(opt_e.lr_now, opt_g.lr_now) and torch.equal(opt_e.grad_norm, opt_g.grad_norm)
    assert next(iter(step._graphs.values()))["graph"] is not None
    assert torch.equal(torch.stack(losses_e), torch.stack(losses_g))
    for t, lr in enumerate(lrs):
        want = sched.lr_at(0.01, t)
        assert abs(lr - want) <= 2.0 ** -23 * want, (t, lr, want)
    assert lrs[3] > lrs[4] > lrs[5], "the replayed steps must train at decreasing rates"
    assert int(opt_g.step_count) == 6
    for (k, a), (_, b) in zip(m_e.state_dict().items(), m_g.state_dict().items()):
        assert torch.equal(a, b), k
    assert same_bits(opt_e.ema_parameters(), opt_g.ema_parameters())


def test_fp16_train_step_takes_the_device_side_skip_path():
    import segmentation_pipeline_amd as sp
    from segmentation_pipeline_amd import optim
    from segmentation_pipeline_amd.criterions import HybridLogisticDiceLoss
    from segmentation_pipeline_amd.prediction import StandardPredict
    from segmentation_pipeline_amd.trainer import train_step
    torch.manual_seed(0)
    model = _tiny().cuda()
    opt = optim.FusedAdam(model.parameters(), lr=1e-3)
    before = [p.detach().clone() for p in model.parameters()]
    with sp.precision("fp16"):
        ld, _ = train_step(model, HybridLogisticDiceLoss(), opt, StandardPredict(image_names=["X", "y"]), _batches(1)[0],
                           torch.device("cuda"))
    assert "found_inf" in ld and "skipped_step" not in ld
    assert float(ld["found_inf"]) == 0.0 and int(opt.skipped) == 0 and int(opt.step_count) == 1
    assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), before))
