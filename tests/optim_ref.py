"""Reference for segmentation_pipeline_amd.optim: an fp64 restatement of torch.optim.SGD / Adam / AdamW with gradient
clipping by global norm, the closed form of PolynomialLR and a weight EMA on plain tensors (RefOptimizer), the torch stack it
is pinned to (torch_stack: torch.optim + clip_grad_norm_ + lr_scheduler.PolynomialLR + lerp), and the tensor sets and
option grids of the tests."""
import itertools
import math

import torch

RULES = ("sgd", "adam", "adamw")
STEPS = 6


class RefOptimizer:
    """groups: [{"params": [tensor, ...], **hyper}]; step(grads) with grads[group][i] a tensor or None.  Works in the dtype
    of the parameters it is given (fp64 as the reference); parameters are updated in place."""

    def __init__(self, rule, groups, max_grad_norm=None, ema_decay=None, total_steps=None, power=0.9):
        assert rule in RULES
        self.rule, self.groups = rule, groups
        self.max_grad_norm, self.ema_decay, self.total_steps, self.power = max_grad_norm, ema_decay, total_steps, power
        self.t = 0
        self.state = [[{} for _ in g["params"]] for g in groups]
        self.ema = [[p.clone() for p in g["params"]] for g in groups] if ema_decay is not None else None
        self.grad_norm = self.clip_coef = None
        self.lr_now = [g["lr"] for g in groups]
        self.skipped = False

    def lr_at(self, lr0, t):
        if self.total_steps is None:
            return lr0
        return lr0 * (1.0 - min(t, self.total_steps) / self.total_steps) ** self.power

    def step(self, grads, found_inf=False, grad_scale=None):
        inv = 1.0 if grad_scale is None else 1.0 / grad_scale
        coef = 1.0
        self.skipped = bool(found_inf)
        if self.max_grad_norm is not None:
            total = sum(float((g.double() ** 2).sum()) for gg in grads for g in gg if g is not None)
            self.grad_norm = math.sqrt(total) * inv
            coef = min(1.0, self.max_grad_norm / (self.grad_norm + 1e-6))
            self.skipped = self.skipped or not math.isfinite(self.grad_norm)
        self.clip_coef = coef
        self.lr_now = [self.lr_at(g["lr"], self.t) for g in self.groups]
        if self.skipped:
            return
        t1 = self.t + 1
        for gi, group in enumerate(self.groups):
            lr, wd = self.lr_now[gi], group.get("weight_decay", 0.0)
            for i, p in enumerate(group["params"]):
                if grads[gi][i] is None:
                    continue
                g = grads[gi][i].to(p.dtype) * (coef * inv)
                st = self.state[gi][i]
                if self.rule == "sgd":
                    mom, damp = group.get("momentum", 0.0), group.get("dampening", 0.0)
                    if wd != 0:
                        g = g + wd * p
                    if mom != 0:
                        st["momentum_buffer"] = g.clone() if "momentum_buffer" not in st else \
                            mom * st["momentum_buffer"] + (1 - damp) * g
                        g = g + mom * st["momentum_buffer"] if group.get("nesterov") else st["momentum_buffer"]
                    p -= lr * g
                else:
                    b1, b2 = group.get("betas", (0.9, 0.999))
                    eps = group.get("eps", 1e-8)
                    if self.rule == "adamw":
                        p *= 1 - lr * wd
                    elif wd != 0:
                        g = g + wd * p
                    if "exp_avg" not in st:
                        st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                    st["exp_avg"] = st["exp_avg"] + (1 - b1) * (g - st["exp_avg"])
                    st["exp_avg_sq"] = b2 * st["exp_avg_sq"] + (1 - b2) * g * g
                    bc1, bc2 = 1 - b1 ** t1, 1 - b2 ** t1
                    denom = st["exp_avg_sq"].sqrt() / math.sqrt(bc2) + eps
                    p -= (lr / bc1) * st["exp_avg"] / denom
                if self.ema is not None:
                    d = self.ema_decay
                    self.ema[gi][i] = d * self.ema[gi][i] + (1 - d) * p
        self.t = t1


def torch_stack(rule, groups, grads_per_step, max_grad_norm=None, ema_decay=None, total_steps=None, power=0.9):
    """The composition the fused step stands in for, on the CPU in the dtype of the given parameters:
    -> dict(params, state, ema, lr, norm): per group lists after the last step, lr / norm per step."""
    params = [[torch.nn.Parameter(p.clone()) for p in g["params"]] for g in groups]
    tgroups = [dict({k: v for k, v in g.items() if k != "params"}, params=ps) for g, ps in zip(groups, params)]
    cls = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "adamw": torch.optim.AdamW}[rule]
    opt = cls(tgroups, lr=groups[0]["lr"])
    sched = None if total_steps is None else torch.optim.lr_scheduler.PolynomialLR(opt, total_iters=total_steps, power=power)
    ema = [[p.detach().clone() for p in ps] for ps in params] if ema_decay is not None else None
    lrs, norms = [], []
    flat = [p for ps in params for p in ps]
    for grads in grads_per_step:
        for ps, gg in zip(params, grads):
            for p, g in zip(ps, gg):
                p.grad = None if g is None else g.to(p.dtype).clone()
        if max_grad_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(flat, max_grad_norm)))
        lrs.append([g["lr"] for g in opt.param_groups])
        opt.step()
        if sched is not None:
            sched.step()
        if ema is not None:
            with torch.no_grad():
                for ps, es in zip(params, ema):
                    for p, e, in zip(ps, es):
                        if p.grad is not None:
                            e.lerp_(p, 1 - ema_decay)
    keys = {"sgd": ("momentum_buffer",), "adam": ("exp_avg", "exp_avg_sq"), "adamw": ("exp_avg", "exp_avg_sq")}[rule]
    state = [[{k: opt.state[p][k] for k in keys if k in opt.state.get(p, {}) and opt.state[p][k] is not None} for p in ps]
             for ps in params]
    return {"params": [[p.detach() for p in ps] for ps in params], "state": state, "ema": ema, "lr": lrs, "norm": norms}


# ------------------------------------------------------------------------------------------------ option grids
def option_grid():
    """(id, rule, hyper-parameters of group 0 and 1, extras): every rule with and without each option"""
    out = []
    sgd = [("plain", {}), ("momentum", {"momentum": 0.9}), ("dampening", {"momentum": 0.9, "dampening": 0.25}),
           ("nesterov", {"momentum": 0.99, "nesterov": True})]
    extras = [("", {}), ("clip", {"max_grad_norm": None}), ("poly", {"total_steps": 8}), ("ema", {"ema_decay": 0.9}),
              ("all", {"max_grad_norm": None, "total_steps": 8, "ema_decay": 0.9})]
    for (hn, h), wd, (en, e) in itertools.product(sgd, (False, True), extras):
        if wd and en not in ("", "all"):
            continue   # (weight decay does not interact with the extras: one pairing with none and one with all)
        g0 = dict(h, lr=0.05, weight_decay=0.01 if wd else 0.0)
        g1 = dict(h, lr=0.02, weight_decay=0.0)
        out.append((f"sgd-{hn}{'-wd' if wd else ''}{'-' + en if en else ''}", "sgd", (g0, g1), dict(e)))
    for rule, wd, (en, e) in itertools.product(("adam", "adamw"), (False, True), extras):
        if wd and en not in ("", "all"):
            continue
        g0 = dict(lr=0.01, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05 if wd else 0.0)
        g1 = dict(lr=0.004, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.0)
        out.append((f"{rule}{'-wd' if wd else ''}{'-' + en if en else ''}", rule, (g0, g1), dict(e)))
    return out


# ------------------------------------------------------------------------------------------------ tensor sets
def tensor_set(chunk, seed=0, many=None):
    """-> (specs, params64, grads64): specs[i] = dict(n, group, p_off, g_off, has_grad) with offsets in elements into the
    16-byte-aligned storage (1 = a view starting 4 bytes in); params64 / grads64[step] are flat lists in spec order (a
    gradient None where has_grad is False).  many = T: T tensors of 5 elements instead (more than one table launch).
    The gradients are seeded normals scaled so that the global norm lies above CLIP_NORM on some steps and below it on
    others (checked on the reference by the tests)."""
    gen = torch.Generator().manual_seed(seed)
    if many is not None:
        specs = [dict(n=5, group=i % 2, p_off=0, g_off=0, has_grad=True) for i in range(many)]
    else:
        sizes = [1, 3, 4, 5, 255, 257, chunk - 1, chunk + 1, 2 * chunk + 7]
        specs = [dict(n=n, group=i % 2, p_off=0, g_off=0, has_grad=True) for i, n in enumerate(sizes)]
        specs.append(dict(n=261, group=0, p_off=1, g_off=0, has_grad=True))    # parameter 4 bytes into its storage
        specs.append(dict(n=262, group=1, p_off=0, g_off=1, has_grad=True))    # ... and the other way round
        specs.append(dict(n=chunk + 9, group=1, p_off=1, g_off=1, has_grad=True))   # both, the same way: scalar head + vector body
        specs.append(dict(n=7, group=0, p_off=0, g_off=0, has_grad=False))
    params = [torch.randn(s["n"], generator=gen, dtype=torch.float64) for s in specs]
    total = sum(s["n"] for s in specs if s["has_grad"])
    grads = []
    for step in range(STEPS):
        scale = GRAD_SCALES[step] * CLIP_NORM / math.sqrt(total)
        grads.append([torch.randn(s["n"], generator=gen, dtype=torch.float64).mul_(scale).float().double()
                      if s["has_grad"] else None for s in specs])
    params = [p.float().double() for p in params]   # (exactly representable in fp32: every side starts from the same values)
    return specs, params, grads


CLIP_NORM = 12.0
GPU_SEED = 11   # the seed of the tensor sets the GPU tests run on
GRAD_SCALES = (0.5, 2.0, 0.8, 1.5, 3.0, 0.6)   # expected global norm / CLIP_NORM per step


def split_groups(specs, flat):
    return [[t for s, t in zip(specs, flat) if s["group"] == g] for g in (0, 1)]


def build_groups(specs, params, hypers, dtype):
    return [dict(h, params=[p.to(dtype).clone() for p in ps]) for h, ps in zip(hypers, split_groups(specs, params))]


def resolve_extras(extras):
    e = dict(extras)
    if "max_grad_norm" in e:
        e["max_grad_norm"] = CLIP_NORM
    return e


def run_reference(rule, specs, params, grads, hypers, extras):
    """RefOptimizer in fp64 over all steps -> (ref, per-step records)"""
    ref = RefOptimizer(rule, build_groups(specs, params, hypers, torch.float64), **resolve_extras(extras))
    rec = []
    for g in grads:
        ref.step(split_groups(specs, g))
        rec.append(dict(norm=ref.grad_norm, clip=ref.clip_coef, lr=list(ref.lr_now)))
    return ref, rec
