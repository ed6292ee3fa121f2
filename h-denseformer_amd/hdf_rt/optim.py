"""Flat optimizers over the module's flat parameter buffer: the three optimizers trainer.py:793-840 builds (Adam, AdamW,
SGD with Nesterov momentum), each one kernel per step (hdf_optim_step) and numerically torch's own fp32 step, over the
reference's two parameter groups (L2 / decoupled weight decay on ndim>1 non-bias tensors, none on the rest).

They are torch.optim.Optimizer subclasses, so torch.optim.lr_scheduler.*, torch.amp.GradScaler and the trainer's
`optimizer.param_groups[0]['lr']` logging work on them.  Under a GradScaler the gradient is unscaled, and a step with
non-finite gradients skipped, INSIDE the kernel: step() never synchronises with the device."""
import copy

import torch
from torch.optim.lr_scheduler import LRScheduler

from ._lib import HdfError, check, lib, ptr, stream_ptr

ADAM, ADAMW, SGD = 0, 1, 2          # HDF_OPTIM_* of include/hdf.h
_STATE_WORDS = 8                    # HDF_OPTIM_STATE_WORDS


def _no_decay(name, p):
    """trainer.py:812-817, the rule weight_decay_mask() encodes per element"""
    return p.ndim == 1 or name.endswith(".bias")


class FlatOptimizer(torch.optim.Optimizer):
    """Common base.  param_groups are the reference's two, in its order: the decay group, then the no-decay group with
    weight_decay 0.0.  The kernel picks the group of an element from the model's weight_decay_mask() byte and takes `lr`
    and `weight_decay` from each group; the other hyper-parameters must agree between the groups.

    GradScaler finds _step_supports_amp_scaling, sets `self.grad_scale` / `self.found_inf` (device tensors) around its call
    of step() and leaves the unscaling and the skip to the kernel.

    The groups are fixed (add_param_group refuses).  state_dict() is NOT torch's format: the state is held per flat
    buffer, not per parameter, so there is no 'params' index list and torch's state-dict hooks are not run; it loads into
    the same class over a net of the same geometry only."""
    _step_supports_amp_scaling = True
    _rule = None
    _state_names = ()

    def __init__(self, model, defaults):
        self.model = model
        decay, no_decay = [], []
        for name, p in model.named_parameters():
            (no_decay if _no_decay(name, p) else decay).append(p)
        super().__init__([{"params": decay}, {"params": no_decay, "weight_decay": 0.0}], defaults)
        self._state_for = None
        self._calls = 0

    def add_param_group(self, param_group):
        # (the base constructor adds the two groups through here)
        if len(self.param_groups) >= 2:
            raise ValueError(f"{type(self).__name__} works on the model's flat buffer with exactly two parameter groups "
                             f"(decay, no decay): a group cannot be added")
        super().add_param_group(param_group)

    def _state(self):
        # the list the last forward verified: no second walk over the 1 420 parameters per step (1.5 ms of host time)
        flat = self.model.flat_parameters(self.model.checked_parameters())
        if self._state_for is None or self._state_for.data_ptr() != flat.data_ptr():
            # a new flat buffer (module moved / re-flattened): the state restarts, and so does the bias correction
            for name in self._state_names:
                setattr(self, name, torch.zeros_like(flat))
            self.mask = self.model.weight_decay_mask()
            # word 0: the steps taken, counted on the device (a skipped step does not count); the rest is the kernel's
            self._step_state = torch.zeros(_STATE_WORDS, dtype=torch.int32, device=flat.device)
            self._state_for = flat
            self._calls = 0
        return flat

    @property
    def step_counter(self):
        """int32 device tensor of one element: the steps taken (what the bias correction uses)"""
        self._state()
        return self._step_state[:1]

    @property
    def step_count(self):
        """step() calls since the state last restarted, counted on the host: equal to step_counter unless a GradScaler
        skipped steps.  Assigning sets both (0 restarts the bias correction)."""
        return self._calls

    @step_count.setter
    def step_count(self, value):
        self._calls = int(value)
        if self._state_for is not None:
            self._step_state[:1].fill_(int(value))

    def zero_grad(self, set_to_none=True):
        for p in self.model.checked_parameters():
            p.grad = None

    def _rule_args(self, group):
        """(beta1 or momentum, beta2, eps, nesterov) of the kernel call"""
        raise NotImplementedError

    def _amp_scalar(self, name, flat):
        t = getattr(self, name, None)
        if t is None:
            return None
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.numel() == 1 and t.device == flat.device):
            raise HdfError(f"{type(self).__name__}.{name} must be one fp32 value on {flat.device} (torch.amp.GradScaler "
                           f"sets it so)")
        return t

    @torch.no_grad()
    def step(self, grad_scale=1.0):
        """One update from the flat gradient buffer.  grad_scale: a host-side multiplier on the gradient (not the
        GradScaler's scale: that one arrives as the device tensor self.grad_scale and divides)."""
        flat = self._state()
        g = self.model.flat_grads()
        g0, g1 = self.param_groups
        args = self._rule_args(g0)
        if args != self._rule_args(g1):
            raise HdfError(f"{type(self).__name__}: the two parameter groups may differ in lr and weight_decay only")
        s = [getattr(self, n) for n in self._state_names] + [None]
        self._calls += 1
        check(lib().hdf_optim_step(self._rule, ptr(flat), ptr(g), ptr(s[0]), ptr(s[1]), ptr(self.mask), flat.numel(),
                                   g0["lr"], g1["lr"], g0["weight_decay"], g1["weight_decay"], *args, grad_scale,
                                   ptr(self._amp_scalar("grad_scale", flat)), ptr(self._amp_scalar("found_inf", flat)),
                                   ptr(self._step_state), stream_ptr()), "hdf_optim_step")

    # ---- resuming: the flat state buffers, the device step counter and the groups' hyper-parameters
    def state_dict(self):
        self._state()
        state = {n: getattr(self, n).clone() for n in self._state_names}
        state["step"] = self._step_state[:1].clone()
        return {"optimizer": type(self).__name__, "state": state,
                "param_groups": [{k: copy.deepcopy(v) for k, v in g.items() if k != "params"}
                                 for g in self.param_groups]}

    def load_state_dict(self, state_dict):
        if state_dict.get("optimizer") != type(self).__name__:
            raise ValueError(f"state of {state_dict.get('optimizer')!r} loaded into {type(self).__name__}")
        if len(state_dict["param_groups"]) != len(self.param_groups):
            raise ValueError("state_dict has a different number of parameter groups")
        flat = self._state()
        with torch.no_grad():
            for n in self._state_names:
                src = state_dict["state"][n]
                if src.shape != flat.shape:
                    raise ValueError(f"{n}: {tuple(src.shape)} saved, the model's flat buffer is {tuple(flat.shape)}")
                getattr(self, n).copy_(src)
            self._step_state[:1].copy_(state_dict["state"]["step"])
        self._calls = int(state_dict["state"]["step"])
        for g, saved in zip(self.param_groups, state_dict["param_groups"]):
            g.update(copy.deepcopy(saved))


class FlatAdam(FlatOptimizer):
    """torch.optim.Adam: L2 weight decay added to the gradient"""
    _rule = ADAM
    _state_names = ("exp_avg", "exp_avg_sq")

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4):
        super().__init__(model, {"lr": lr, "betas": betas, "eps": eps, "weight_decay": weight_decay})

    def _rule_args(self, group):
        return group["betas"][0], group["betas"][1], group["eps"], 0


class FlatAdamW(FlatAdam):
    """torch.optim.AdamW: decoupled weight decay, p *= 1 - lr*weight_decay before the moment update"""
    _rule = ADAMW

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


class FlatSGD(FlatOptimizer):
    """torch.optim.SGD with L2 weight decay, a momentum buffer (dampening 0, initialised to the first gradient) and,
    by default as in trainer.py:832, Nesterov momentum"""
    _rule = SGD
    _state_names = ("momentum_buffer",)

    def __init__(self, model, lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4):
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum above 0")
        super().__init__(model, {"lr": lr, "momentum": momentum, "nesterov": nesterov, "weight_decay": weight_decay})

    def _rule_args(self, group):
        return group["momentum"], 0.0, 0.0, int(bool(group["nesterov"]))


def build_optimizer(name, net, lr, weight_decay, momentum=0.9):
    """trainer.py:_get_optimizer on the flat path: the same hyper-parameters per (case-insensitive) name.  An unknown name
    raises (the reference returns None and fails later)."""
    low = name.lower()
    if low == "sgd":
        return FlatSGD(net, lr=lr, momentum=momentum, nesterov=True, weight_decay=weight_decay)
    if low == "adamw":
        return FlatAdamW(net, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    if low == "adam":
        return FlatAdam(net, lr=lr, weight_decay=weight_decay)
    raise ValueError(f"unknown optimizer {name!r}: one of 'SGD', 'AdamW', 'Adam'")


class PolyLR(LRScheduler):
    """The reference's default schedule ('poly_lr', trainer.py:1020-1031) against the current LRScheduler constructor:
    lr = base_lr * (1 - (epoch - ck_epoch) / (max_epochs - ck_epoch)) ** exponent, frozen once epoch > max_epochs."""

    def __init__(self, optimizer, max_epochs, ck_epoch=0, exponent=0.9, last_epoch=-1):
        self.max_epochs = max_epochs
        self.ck_epoch = ck_epoch
        self.exponent = exponent
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        if self.last_epoch > self.max_epochs:
            return [group["lr"] for group in self.optimizer.param_groups]
        factor = (1 - (self.last_epoch - self.ck_epoch) / (self.max_epochs - self.ck_epoch)) ** self.exponent
        return [base_lr * factor for base_lr in self.base_lrs]
