"""FusedSGD / FusedAdam: the optimizer step on the library's own kernels (csrc/optimizer.hip).

One norm pass (only with `max_grad_norm`) and one update pass over all parameters do what a training scheme otherwise
composes from `clip_grad_norm_`, a `torch.optim` optimizer, an `lr_scheduler` and a `_foreach_lerp_` for the weight EMA.
The step counter, the current learning rates, the clip coefficient and the decision to skip a step are DEVICE data: the
kernels compute them, `step()` never synchronises with the host, and a step captured by trainer.GraphedTrainStep advances
its learning-rate schedule on every replay.  There is no fallback: without the library `step()` raises.
"""
import ctypes as C
import math
from contextlib import contextmanager
from typing import List

import torch

from . import _lib

__all__ = ["PolyLR", "FusedSGD", "FusedAdam"]


class PolyLR:
    """lr_t = lr0 * (1 - min(t, total_steps) / total_steps) ** power, t = 0 on the first step: the closed form of
    torch.optim.lr_scheduler.PolynomialLR.  `param_groups[i]["lr"]` stays lr0; the current rate is `opt.lr_now`."""

    def __init__(self, total_steps: int, power: float = 0.9):
        if int(total_steps) != total_steps or total_steps <= 0:
            raise ValueError(f"PolyLR: total_steps must be a positive integer, got {total_steps!r}")
        if not math.isfinite(power) or power < 0:
            raise ValueError(f"PolyLR: power must be finite and >= 0, got {power!r}")
        self.total_steps, self.power = int(total_steps), float(power)

    def lr_at(self, lr0: float, t: int) -> float:
        return lr0 * (1.0 - min(t, self.total_steps) / self.total_steps) ** self.power

    def __repr__(self):
        return f"PolyLR(total_steps={self.total_steps}, power={self.power})"


_EXTRA = "m355_optim"   # state_dict key of what torch's optimizers have no place for (they ignore it)


def _stream():
    from . import ops
    return ops._stream()


class _Fused(torch.optim.Optimizer):
    _rule = None

    def __init__(self, params, defaults, max_grad_norm, ema_decay, schedule):
        if max_grad_norm is not None and not (math.isfinite(max_grad_norm) and max_grad_norm > 0):
            raise ValueError(f"max_grad_norm must be finite and positive, got {max_grad_norm!r}")
        if ema_decay is not None and not (0.0 <= ema_decay < 1.0):
            raise ValueError(f"ema_decay must lie in [0, 1), got {ema_decay!r}")
        if schedule is not None and not isinstance(schedule, PolyLR):
            raise TypeError("schedule must be None or an optim.PolyLR")
        self.max_grad_norm, self.ema_decay, self.schedule = max_grad_norm, ema_decay, schedule
        self._device = None
        self._ema = {}          # parameter -> shadow
        self._record = None     # the state record (int32 words), allocated on first use
        self._t_loaded = 0      # step counter to put into a record that does not exist yet
        self._workspace = None
        self._cache = None
        super().__init__(params, defaults)
        self._step_supports_amp_scaling = True   # the GradScaler protocol: found_inf / grad_scale are read on the device

    # ------------------------------------------------------------------ construction
    def _check_group(self, group):
        for k in ("amsgrad", "maximize", "differentiable"):
            if group.get(k):
                raise NotImplementedError(f"{type(self).__name__}: {k}=True is not supported")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        self._check_group(group)
        if len(self.param_groups) > _lib.OPTIM_MAX_GROUPS:
            raise ValueError(f"{type(self).__name__}: at most {_lib.OPTIM_MAX_GROUPS} parameter groups")
        for p in group["params"]:
            if p.dtype != torch.float32:
                raise ValueError(f"{type(self).__name__}: parameters must be float32, got {p.dtype}")
            if not p.is_cuda:
                raise ValueError(f"{type(self).__name__}: parameters must live on a HIP device, got {p.device} "
                                 "(there is no CPU fallback)")
            if not p.is_contiguous():
                raise ValueError(f"{type(self).__name__}: parameters must be contiguous")
            if self._device is None:
                self._device = p.device
            elif p.device != self._device:
                raise ValueError(f"{type(self).__name__}: parameters on {self._device} and {p.device}")
            if p.grad is not None and p.grad.is_sparse:
                raise NotImplementedError(f"{type(self).__name__}: sparse gradients are not supported")
            if self.ema_decay is not None:
                self._ema[p] = p.detach().clone()
        self._cache = None

    # ------------------------------------------------------------------ device state
    def _rec(self):
        if self._record is None:
            self._record = torch.zeros(_lib.OPTIM_STATE_WORDS, dtype=torch.int32, device=self._device)
            if self._t_loaded:
                self._record[_lib.OPTIM_ST_T] = self._t_loaded
        return self._record

    def _word(self, i, dtype):
        w = self._rec()[i]
        return w if dtype == torch.int32 else w.view(dtype)

    @property
    def grad_norm(self):
        """0-dim float32: the global gradient norm of the last step (what clip_grad_norm_ returns); NaN without clipping"""
        return self._word(_lib.OPTIM_ST_NORM, torch.float32)

    @property
    def clip_coef(self):
        return self._word(_lib.OPTIM_ST_CLIP, torch.float32)

    @property
    def lr_now(self):
        """float32 [number of groups]: the learning rates the last step used"""
        return self._rec()[_lib.OPTIM_ST_LR:_lib.OPTIM_ST_LR + len(self.param_groups)].view(torch.float32)

    @property
    def step_count(self):
        """0-dim int32: steps applied so far (skipped ones do not count)"""
        return self._word(_lib.OPTIM_ST_T, torch.int32)

    @property
    def skipped(self):
        """0-dim int32: 1 when the last step was skipped (found_inf, or a non-finite gradient norm with clipping)"""
        return self._word(_lib.OPTIM_ST_SKIP, torch.int32)

    # ------------------------------------------------------------------ EMA
    def ema_parameters(self) -> List[torch.Tensor]:
        """the shadow tensors in parameter order"""
        if self.ema_decay is None:
            raise RuntimeError("this optimizer keeps no EMA (ema_decay=None)")
        return [self._ema[p] for g in self.param_groups for p in g["params"]]

    @contextmanager
    def ema_weights(self):
        """the parameters hold the EMA weights inside the block (in-place copies: versions advance, packed forms refresh)"""
        shadows = self.ema_parameters()
        params = [p for g in self.param_groups for p in g["params"]]
        with torch.no_grad():
            saved = [p.detach().clone() for p in params]
            torch._foreach_copy_(params, shadows)
        try:
            yield self
        finally:
            with torch.no_grad():
                torch._foreach_copy_(params, saved)

    # ------------------------------------------------------------------ the step
    def _group_desc(self, group, q):
        raise NotImplementedError

    def _state_of(self, p, group):
        """-> (state1, state2, first)"""
        raise NotImplementedError

    def _hyper_key(self):
        raise NotImplementedError

    def _desc(self):
        d = _lib.OptimDesc()
        d.rule, d.groups = self._rule, len(self.param_groups)
        d.clip = 0 if self.max_grad_norm is None else 1
        d.max_norm = float(self.max_grad_norm or 0.0)
        d.total_steps = self.schedule.total_steps if self.schedule else 0
        d.power = self.schedule.power if self.schedule else 0.0
        d.ema_decay = -1.0 if self.ema_decay is None else float(self.ema_decay)
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            q = d.group[gi]
            q.lr, q.weight_decay = float(group["lr"]), float(group["weight_decay"])
            self._group_desc(group, q)
        return d

    def _build(self, items, ptrs, hyper):
        L = _lib.lib()
        T = len(items)
        for p, g, _ in items:
            if g.is_sparse:
                raise NotImplementedError(f"{type(self).__name__}: sparse gradients are not supported")
            if g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous():
                raise ValueError(f"{type(self).__name__}: gradients must be contiguous float32 tensors on the parameter's device")
        counts = (C.c_int64 * T)(*[p.numel() for p, _, _ in items])
        blk0, nblk = (C.c_int64 * T)(), (C.c_int64 * T)()
        chunk, ws_bytes = C.c_int32(), C.c_size_t()
        _lib.check(L.m355_optim_plan(counts, T, C.byref(chunk), blk0, nblk, C.byref(ws_bytes)), "optim_plan")
        arr = (_lib.OptimTensor * T)()
        firsts = []
        for i, (p, g, gi) in enumerate(items):
            s1, s2, first = self._state_of(p, self.param_groups[gi])
            ema = self._ema.get(p)
            e = arr[i]
            e.param, e.grad = p.data_ptr(), g.data_ptr()
            e.state1 = s1.data_ptr() if s1 is not None else None
            e.state2 = s2.data_ptr() if s2 is not None else None
            e.ema = ema.data_ptr() if ema is not None else None
            e.n, e.blk0, e.group, e.first = counts[i], blk0[i], gi, int(first)
            firsts.append(first)
        cap = int(L.m355_optim_capacity())
        size = C.sizeof(_lib.OptimTensor)
        launches = [(C.c_void_p(C.addressof(arr) + i * size), min(cap, T - i)) for i in range(0, T, cap)]
        if self._workspace is None or self._workspace.numel() < ws_bytes.value:
            self._workspace = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=self._device)
        touched = [p for p, _, _ in items] + [self._ema[p] for p, _, _ in items if p in self._ema]
        return {"ptrs": ptrs, "hyper": hyper, "arr": arr, "launches": launches, "nslots": int(blk0[T - 1] + nblk[T - 1]),
                "desc": self._desc(), "touched": touched, "volatile": any(firsts)}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        items = [(p, p.grad, gi) for gi, group in enumerate(self.param_groups) for p in group["params"]
                 if p.grad is not None and p.numel()]
        if not items:
            return loss
        L = _lib.lib()
        ptrs = [t.data_ptr() for p, g, _ in items for t in (p, g)]
        hyper = self._hyper_key()
        c = self._cache
        if c is None or c["ptrs"] != ptrs or c["hyper"] != hyper:
            c = self._build(items, ptrs, hyper)
            self._cache = None if c["volatile"] else c   # (`first` entries describe this step only)
        found_inf, grad_scale = getattr(self, "found_inf", None), getattr(self, "grad_scale", None)
        for t in (found_inf, grad_scale):
            if t is not None and (t.dtype != torch.float32 or t.device != self._device or t.numel() != 1):
                raise ValueError("found_inf / grad_scale must be one-element float32 tensors on the parameters' device")
        rec, ws = self._rec(), self._workspace
        idx = self._device.index
        if idx is not None and idx != torch.cuda.current_device():
            with torch.cuda.device(idx):
                self._launch(L, c, rec, ws, found_inf, grad_scale)
        else:
            self._launch(L, c, rec, ws, found_inf, grad_scale)
        # the kernels wrote through raw pointers: the packed-weight caches (ops._packed_weight, components._derived_weight)
        # key on `_version`
        torch.autograd.graph.increment_version(c["touched"])
        return loss

    @staticmethod
    def _launch(L, c, rec, ws, found_inf, grad_scale):
        st = _stream()
        desc = C.byref(c["desc"])
        wp, wb, rp = C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(rec.data_ptr())
        if c["desc"].clip:
            for ptr, n in c["launches"]:
                _lib.check(L.m355_optim_norm(ptr, n, wp, wb, st), "optim_norm")
        _lib.check(L.m355_optim_prepare(desc, c["nslots"], wp, wb,
                                        None if found_inf is None else C.c_void_p(found_inf.data_ptr()),
                                        None if grad_scale is None else C.c_void_p(grad_scale.data_ptr()), rp, st),
                   "optim_prepare")
        for ptr, n in c["launches"]:
            _lib.check(L.m355_optim_update(desc, ptr, n, rp, st), "optim_update")

    # ------------------------------------------------------------------ checkpoints (torch's layout)
    def _steps(self) -> int:
        return int(self._record[_lib.OPTIM_ST_T].item()) if self._record is not None else self._t_loaded

    def _set_steps(self, t: int):
        self._t_loaded = int(t)
        if self._record is not None:
            self._record[_lib.OPTIM_ST_T] = int(t)

    def state_dict(self):
        sd = super().state_dict()
        t = self._steps()   # (reads the device counter: may synchronise)
        params = [p for g in self.param_groups for p in g["params"]]
        sd[_EXTRA] = {"step": t, "ema": None if self.ema_decay is None else [self._ema[p] for p in params],
                      "schedule": None if self.schedule is None else {"total_steps": self.schedule.total_steps,
                                                                      "power": self.schedule.power}}
        return sd

    def load_state_dict(self, state_dict):
        extra = state_dict.get(_EXTRA)
        super().load_state_dict({k: v for k, v in state_dict.items() if k != _EXTRA})
        for group in self.param_groups:
            self._check_group(group)
        self._cache = None
        if extra is not None:
            self._set_steps(extra["step"])
            if extra.get("ema") is not None and self.ema_decay is not None:
                params = [p for g in self.param_groups for p in g["params"]]
                with torch.no_grad():
                    for p, e in zip(params, extra["ema"]):
                        self._ema[p].copy_(e)


class FusedSGD(_Fused):
    """torch.optim.SGD (weight decay, momentum, dampening, Nesterov) with gradient clipping by global norm, a polynomial
    learning-rate schedule and an EMA of the weights in the same two passes.  `state_dict()` has torch.optim.SGD's layout.
    The momentum buffer starts at zero and the step that first sees a parameter's gradient sets it to that gradient."""
    _rule = _lib.OPTIM_SGD

    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, max_grad_norm=None,
                 ema_decay=None, schedule=None, maximize=False, differentiable=False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=None, differentiable=differentiable, fused=None)
        super().__init__(params, defaults, max_grad_norm, ema_decay, schedule)

    def _group_desc(self, group, q):
        q.momentum, q.dampening, q.nesterov = float(group["momentum"]), float(group["dampening"]), int(bool(group["nesterov"]))

    def _hyper_key(self):
        return [(g["lr"], g["weight_decay"], g["momentum"], g["dampening"], g["nesterov"]) for g in self.param_groups]

    def _state_of(self, p, group):
        if group["momentum"] == 0:
            return None, None, False
        st = self.state[p]
        buf = st.get("momentum_buffer")
        first = buf is None
        if first:
            buf = st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return buf, None, first


class FusedAdam(_Fused):
    """torch.optim.Adam, or AdamW with decoupled_weight_decay=True, with the same extras as FusedSGD.  One step counter for
    all parameters, kept on the device; `state_dict()` has torch.optim.Adam's layout (`step` per parameter, all equal)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, decoupled_weight_decay=False,
                 max_grad_norm=None, ema_decay=None, schedule=None, amsgrad=False, maximize=False, differentiable=False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self._rule = _lib.OPTIM_ADAMW if decoupled_weight_decay else _lib.OPTIM_ADAM
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=None, capturable=False, differentiable=differentiable, fused=None,
                        decoupled_weight_decay=bool(decoupled_weight_decay))
        super().__init__(params, defaults, max_grad_norm, ema_decay, schedule)

    def _check_group(self, group):
        super()._check_group(group)
        want = self._rule == _lib.OPTIM_ADAMW
        if bool(group.get("decoupled_weight_decay", want)) != want:
            raise ValueError("FusedAdam: decoupled_weight_decay must be the same for every parameter group")

    def _group_desc(self, group, q):
        q.beta1, q.beta2, q.eps = float(group["betas"][0]), float(group["betas"][1]), float(group["eps"])

    def _hyper_key(self):
        return [(g["lr"], g["weight_decay"], tuple(g["betas"]), g["eps"]) for g in self.param_groups]

    def _state_of(self, p, group):
        st = self.state[p]
        if "exp_avg" not in st:
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st["exp_avg"], st["exp_avg_sq"], False

    def state_dict(self):
        sd = super().state_dict()
        t = sd[_EXTRA]["step"]
        # (torch packs the live per-parameter dicts: copy before adding the key)
        sd["state"] = {k: dict(st, step=torch.tensor(float(t), dtype=torch.float32)) for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        steps = {float(st["step"]) for st in state_dict["state"].values() if "step" in st}
        if len(steps) > 1:
            raise ValueError(f"FusedAdam keeps one step counter for all parameters; the checkpoint holds {sorted(steps)}")
        super().load_state_dict(state_dict)
        for st in self.state.values():
            st.pop("step", None)
        if steps:
            self._set_steps(int(steps.pop()))
