"""Fused optimizers: drop-ins for ``torch.optim.Adamax`` as the reference driver uses it
(/root/reference/dss2_run.py:91-92 ``getattr(optim, 'Adamax')(model.parameters(), lr=3e-3)``, stepped
at :143) and for the names a user puts into that line instead -- Adam, AdamW, RMSprop, SGD -- as ONE HIP
launch over all parameter tensors instead of ~6 ATen launches per tensor: every class here is a rule of the one
multi-tensor kernel behind ``dss2_optim_step*`` (include/dss2_hip.h).  State keys match torch's, so
optimizer checkpoints (``optimizer_state_dict`` in dss2_run.py:240-247) load either way.  ``lr`` may be a
0-dim fp32 device tensor: the launches then read it, so a recorded step (graphs.GraphedStep / PlannedStep)
follows a ``torch.optim.lr_scheduler`` (the schedulers fill a tensor ``lr`` in place).  ``clip_grad_norm_``
is ``torch.nn.utils.clip_grad_norm_`` in two launches that a recorded step carries.  No CPU fallback."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def _refuse(name, **kw):
    for k, v in kw.items():
        if v:
            raise ValueError(f"{name}: {k}={v!r} is not supported (the fused kernels are torch's single-tensor rule, minimizing)")


class _FusedOptimizer(torch.optim.Optimizer):
    """Tables, flat-bucket detection and step count shared by the fused optimizers.  A subclass names its rule's state slots
    (``_slots``) and fills the launch's hyper-parameters (``_hyper``)."""
    _HIDE_FRESH = True       # export no state for a parameter that has not been stepped (what torch's class would hold)
    _EXPORT_STEP = True      # (torch.optim.SGD keeps no step count)

    def __init__(self, params, defaults, capturable: bool = False):
        lr = defaults["lr"]
        if torch.is_tensor(lr):
            if lr.numel() != 1 or lr.dtype != torch.float32:
                raise ValueError("a tensor lr must be one fp32 element (the launches read it on the device)")
        elif lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        super().__init__(params, defaults)
        self.capturable = bool(capturable)
        self._table = {}
        self._flat_table = {}
        self.table_builds = 0      # diagnostics: how often the descriptor table had to be rebuilt

    # ---- what a rule defines
    def _slots(self, group):
        """State keys of the kernel's slots s0, s1, s2 (None: the rule does not use the slot)."""
        raise NotImplementedError

    def _hyper(self, group) -> "_lib.OptimHyper":
        raise NotImplementedError

    def _loaded_step(self, ps) -> float:
        known = [self.state[p]["step"] for p in ps if "step" in self.state[p]]
        return float(known[0]) if known else 0.0

    def _with_lr(self, group, h):
        lr = group["lr"]
        if torch.is_tensor(lr):
            h.lr, h.lr_dev = 0.0, lr.data_ptr()
        else:
            h.lr, h.lr_dev = float(lr), None
        return h

    def load_state_dict(self, state_dict):
        lrs = [g["lr"] for g in self.param_groups]
        super().load_state_dict(state_dict)
        self._table = {}           # the state tensors were replaced
        self._flat_table = {}
        for g, lr in zip(self.param_groups, lrs):
            g.pop("_step", None)   # re-derived from the loaded per-parameter steps
            if torch.is_tensor(lr):            # recorded launches read THIS tensor: keep it, take the loaded value
                with torch.no_grad():
                    lr.fill_(float(g["lr"]))
                g["lr"] = lr

    def state_dict(self):
        sd = super().state_dict()
        for g in sd["param_groups"]:
            g.pop("_step", None)   # internal: torch's format keeps the count per parameter (state[...]["step"])
        # Internally every parameter of a group shares ONE step tensor.  Exported as is, pickle / deepcopy would keep the
        # aliasing, and torch.optim.Adamax loading such a checkpoint would advance the shared tensor once per PARAMETER
        # per iteration (wrong bias correction).  torch's format is one independent tensor per parameter: export clones.
        state = {}
        for k, st in sd["state"].items():
            st = dict(st)
            step = st.get("step")
            if self._HIDE_FRESH and (step is None or float(step) == 0.0):
                continue           # created by init_state(), not stepped yet: torch's class holds nothing
            if not self._EXPORT_STEP:
                st.pop("step", None)
                if not st:
                    continue
            elif torch.is_tensor(step):
                st["step"] = step.detach().clone()
            state[k] = st
        sd["state"] = state
        return sd

    def _new_state(self, gi, keys, p, st) -> None:
        for k in keys:
            if k not in st:
                st[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
                self._table.pop(gi, None)
                self._flat_table.pop(gi, None)

    @torch.no_grad()
    def init_state(self) -> None:
        """Create the optimizer state of every parameter now (normally done lazily by the first step).  Needed before
        capturing ``step()`` into a hipGraph without warm-up steps: state created INSIDE a capture would be re-zeroed by
        every replay."""
        for gi, group in enumerate(self.param_groups):
            ps = list(group["params"])
            if not ps:
                continue
            if group.get("_step") is None:
                first = self._loaded_step(ps)
                group["_step"] = (torch.tensor(first, dtype=torch.float32, device=ps[0].device) if self.capturable else torch.tensor(first))
            keys = [k for k in self._slots(group) if k is not None]
            for p in ps:
                st = self.state[p]
                self._new_state(gi, keys, p, st)
                st["step"] = group["_step"]

    def _step_flat(self, gi, group, ps, shared, step, dev) -> bool:
        """ONE launch for all tensors when every gradient is a contiguous view of one flat bucket (what the backward of
        this library hands to autograd): the descriptor table lives on the device and holds the gradients' offsets inside
        the bucket, which do not change from step to step; only the bucket's address travels with the launch."""
        g0 = ps[0].grad
        base = g0.untyped_storage().data_ptr()
        for p in ps:
            g = p.grad
            if not g.is_contiguous() or g.dtype != torch.float32 or g.untyped_storage().data_ptr() != base:
                return False
        offs = tuple(p.grad.storage_offset() for p in ps)
        key = (tuple(p.data_ptr() for p in ps), offs)
        cached = self._flat_table.get(gi)
        if cached is None or cached[0] != key:
            if torch.cuda.is_current_stream_capturing():
                return False      # (a table upload cannot be captured: the by-value path below serves this step)
            import numpy as np
            slots = self._slots(group)
            arr = np.zeros(len(ps), dtype=np.dtype(_lib.OptimFlatDesc))
            for i, p in enumerate(ps):
                stp = self.state[p]
                arr[i] = (p.data_ptr(), offs[i]) + tuple(stp[k].data_ptr() if k is not None else 0 for k in slots) + (p.numel(),)
            tab = torch.from_numpy(arr.view(np.uint8)).to(dev)
            cached = self._flat_table[gi] = (key, tab, max(p.numel() for p in ps),
                                             torch.zeros(1, dtype=torch.int32, device=dev))
            self.table_builds += 1
        _, tab, max_n, counter = cached
        step_dev = shared.data_ptr() if self.capturable else None
        _lib.check(_lib.lib().dss2_optim_step_flat(tab.data_ptr(), len(ps), max_n, base, C.byref(self._hyper(group)), int(step),
                                                   step_dev, counter.data_ptr(), _lib.stream_ptr(dev)), "dss2_optim_step_flat")
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi in range(len(self.param_groups)):
            self._step_group(gi)
        return loss

    @torch.no_grad()
    def step_group(self, gi: int) -> None:
        """Step ONE parameter group (parallel.step_overlapped: the groups follow the chunks of the gradient bucket)."""
        self._step_group(gi)

    def _step_group(self, gi: int) -> None:
        group = self.param_groups[gi]
        ps = [p for p in group["params"] if p.grad is not None]
        if not ps:
            return
        dev = ps[0].device
        for p in ps:
            if not p.is_cuda or p.dtype != torch.float32:
                raise RuntimeError(f"{type(self).__name__} needs fp32 GPU parameters (there is no CPU fallback)")
        lr = group["lr"]
        if torch.is_tensor(lr) and (lr.device != dev or lr.dtype != torch.float32 or lr.numel() != 1):
            raise RuntimeError(f"{type(self).__name__}: a tensor lr must be one fp32 element on the parameters' device ({dev})")
        # one step tensor shared by every parameter of the group (torch keeps one per parameter with the same value):
        # advanced ONCE per step -- on the host, or by the kernel itself when capturable
        shared = group.get("_step")
        if shared is None:
            first = self._loaded_step(ps)
            shared = group["_step"] = (torch.tensor(first, dtype=torch.float32, device=dev) if self.capturable
                                       else torch.tensor(first))
        keys = [k for k in self._slots(group) if k is not None]
        for p in ps:
            st = self.state[p]
            if keys and keys[-1] not in st:
                self._new_state(gi, keys, p, st)
            if st.get("step") is not shared:
                st["step"] = shared
        if not self.capturable:
            shared += 1.0
            step = int(shared)
        if self._step_flat(gi, group, ps, shared, step if not self.capturable else 0, dev):
            return
        grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in ps]
        # host-side descriptor table, passed to the kernels BY VALUE (no device copy to keep alive, capture-safe);
        # parameter and state addresses are written once, the gradient addresses every step (the flat gradient
        # buckets of the backward move)
        cached = self._table.get(gi)
        pkey = tuple(p.data_ptr() for p in ps)
        if cached is None or cached[1] != pkey:
            tab = (_lib.OptimDesc * len(ps))()
            for d, p in zip(tab, ps):
                stp = self.state[p]
                d.param, d.n = p.data_ptr(), p.numel()
                for name, k in zip(("s0", "s1", "s2"), self._slots(group)):
                    setattr(d, name, stp[k].data_ptr() if k is not None else None)
            cached = self._table[gi] = (tab, pkey)
            self.table_builds += 1
        tab = cached[0]
        for d, g in zip(tab, grads):
            d.grad = g.data_ptr()
        st = _lib.stream_ptr(dev)
        if self.capturable:
            _lib.check(_lib.lib().dss2_optim_step_dev(C.addressof(tab), len(ps), C.byref(self._hyper(group)), shared.data_ptr(), st),
                       "dss2_optim_step_dev")
        else:
            _lib.check(_lib.lib().dss2_optim_step(C.addressof(tab), len(ps), C.byref(self._hyper(group)), step, st), "dss2_optim_step")


class FusedAdamax(_FusedOptimizer):
    """``torch.optim.Adamax`` (state: step, exp_avg, exp_inf), the reference driver's optimizer."""
    _HIDE_FRESH = False      # (its checkpoints keep the zero state of init_state(), as they always have)

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable: bool = False):
        """capturable=True (as in torch's optimizers): the step count lives on the device, so ``step()`` may be captured
        into a hipGraph together with forward + loss + backward (graphs.GraphedStep) and every replay advances it."""
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), capturable)

    def _slots(self, group):
        return ("exp_avg", "exp_inf", None)

    def _hyper(self, group):
        b1, b2 = group["betas"]
        return self._with_lr(group, _lib.OptimHyper(rule=_lib.OPT_ADAMAX, beta1=float(b1), beta2=float(b2), eps=float(group["eps"]),
                                                    weight_decay=float(group["weight_decay"])))


class FusedAdam(_FusedOptimizer):
    """``torch.optim.Adam`` (state: step, exp_avg, exp_avg_sq, max_exp_avg_sq with amsgrad)."""
    _DECOUPLED = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, capturable: bool = False,
                 maximize=False, foreach=None, fused=None, differentiable=False):
        _refuse(type(self).__name__, maximize=maximize, foreach=foreach, fused=fused, differentiable=differentiable)
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad)), capturable)

    def _slots(self, group):
        return ("exp_avg", "exp_avg_sq", "max_exp_avg_sq" if group["amsgrad"] else None)

    def _hyper(self, group):
        b1, b2 = (float(b) for b in group["betas"])
        flags = (_lib.OPT_AMSGRAD if group["amsgrad"] else 0) | (_lib.OPT_DECOUPLED_WD if self._DECOUPLED else 0)
        return self._with_lr(group, _lib.OptimHyper(rule=_lib.OPT_ADAM, flags=flags, beta1=b1, beta2=b2, omb1=1 - b1, omb2=1 - b2,
                                                    eps=float(group["eps"]), weight_decay=float(group["weight_decay"])))


class FusedAdamW(FusedAdam):
    """``torch.optim.AdamW``: Adam with the decoupled weight decay ``p *= 1 - lr * weight_decay``."""
    _DECOUPLED = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, capturable: bool = False,
                 maximize=False, foreach=None, fused=None, differentiable=False):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, capturable=capturable, maximize=maximize, foreach=foreach,
                         fused=fused, differentiable=differentiable)


class FusedRMSprop(_FusedOptimizer):
    """``torch.optim.RMSprop`` (state: step, square_avg, momentum_buffer with momentum, grad_avg when centered)."""

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False, *, capturable: bool = False,
                 maximize=False, foreach=None, fused=None, differentiable=False):
        _refuse("FusedRMSprop", maximize=maximize, foreach=foreach, fused=fused, differentiable=differentiable)
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= momentum:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if not 0.0 <= alpha:
            raise ValueError(f"Invalid alpha value: {alpha}")
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum, centered=bool(centered)),
                         capturable)

    def _slots(self, group):
        return ("square_avg", "momentum_buffer" if group["momentum"] > 0 else None, "grad_avg" if group["centered"] else None)

    def _hyper(self, group):
        a, mu = float(group["alpha"]), float(group["momentum"])
        flags = (_lib.OPT_MOMENTUM if mu > 0 else 0) | (_lib.OPT_CENTERED if group["centered"] else 0)
        return self._with_lr(group, _lib.OptimHyper(rule=_lib.OPT_RMSPROP, flags=flags, beta2=a, omb2=1 - a, eps=float(group["eps"]),
                                                    weight_decay=float(group["weight_decay"]), momentum=mu))


class FusedSGD(_FusedOptimizer):
    """``torch.optim.SGD`` (state: momentum_buffer with momentum; no step count in its checkpoints -- the kernels keep one of
    their own, because the first step's buffer is the gradient itself)."""
    _EXPORT_STEP = False

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, capturable: bool = False,
                 maximize=False, foreach=None, fused=None, differentiable=False):
        _refuse("FusedSGD", maximize=maximize, foreach=foreach, fused=fused, differentiable=differentiable)
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=bool(nesterov)),
                         capturable)

    def _slots(self, group):
        return ("momentum_buffer" if group["momentum"] != 0 else None, None, None)

    def _loaded_step(self, ps) -> float:
        # a loaded momentum buffer has been stepped (how often does not matter: only the first step differs)
        return 1.0 if any("momentum_buffer" in self.state[p] for p in ps) else 0.0

    def _hyper(self, group):
        mu = float(group["momentum"])
        flags = (_lib.OPT_MOMENTUM if mu != 0 else 0) | (_lib.OPT_NESTEROV if group["nesterov"] else 0)
        return self._with_lr(group, _lib.OptimHyper(rule=_lib.OPT_SGD, flags=flags, weight_decay=float(group["weight_decay"]), momentum=mu,
                                                    omdamp=1 - float(group["dampening"])))


_CLIP_TABLES = {}      # flat-bucket tables of clip_grad_norm_: {(device, offsets, sizes): device table}


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm: float) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_(parameters, max_norm)`` (2-norm, ``error_if_nonfinite=False``) in two launches of this
    library, so a recorded step carries it: fp64 partial sums of squares per workgroup, then every workgroup re-adds them in
    order, forms ``coef = min(1, max_norm / (norm + 1e-6))`` and scales its share of the gradients in place.  Deterministic (no
    float atomics), nothing is read back: the fp32 norm is returned as a device tensor."""
    if torch.is_tensor(parameters):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.zeros(())
    dev = grads[0].device
    for g in grads:
        if not g.is_cuda or g.dtype != torch.float32 or g.device != dev or not g.is_contiguous():
            raise RuntimeError("clip_grad_norm_ needs contiguous fp32 gradients on one GPU (there is no CPU fallback)")
    total = sum(g.numel() for g in grads)
    base = grads[0].untyped_storage().data_ptr()
    tab = None
    if all(g.untyped_storage().data_ptr() == base for g in grads):      # views of one flat bucket: a device table of offsets
        key = (dev, tuple(g.storage_offset() for g in grads), tuple(g.numel() for g in grads))
        tab = _CLIP_TABLES.get(key)
        if tab is None and not torch.cuda.is_current_stream_capturing():      # (an upload cannot be captured: by value then)
            tab = _CLIP_TABLES[key] = torch.tensor([key[1], key[2]], dtype=torch.int64).t().contiguous().to(dev)
    chunks = 1 if tab is not None else -(-len(grads) // _lib.OPTIM_GRAD_CHUNK)
    if chunks > _lib.OPTIM_MAX_PARTIALS:
        raise RuntimeError(f"clip_grad_norm_: {len(grads)} separate gradient tensors are more than {_lib.OPTIM_MAX_PARTIALS} launches carry")
    n_wg = max(1, min(-(-total // 4096), _lib.OPTIM_MAX_PARTIALS // chunks))
    partials = torch.empty(_lib.OPTIM_MAX_PARTIALS, dtype=torch.float64, device=dev)
    norm = torch.empty((), dtype=torch.float32, device=dev)
    if tab is not None:
        host, flat, gbase = None, tab.data_ptr(), base
    else:
        descs = (_lib.GradDesc * len(grads))()
        for d, g in zip(descs, grads):
            d.grad, d.n = g.data_ptr(), g.numel()
        host, flat, gbase = C.addressof(descs), None, None
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    _lib.check(L.dss2_grad_sqsum_partials(host, flat, gbase, len(grads), n_wg, partials.data_ptr(), st), "dss2_grad_sqsum_partials")
    _lib.check(L.dss2_grad_clip_scale(host, flat, gbase, len(grads), n_wg, partials.data_ptr(), float(max_norm), norm.data_ptr(), st),
               "dss2_grad_clip_scale")
    return norm
