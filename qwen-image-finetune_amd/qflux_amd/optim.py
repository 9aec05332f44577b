"""The fused optimizers as torch.optim.Optimizer classes, for the reference's unmodified loop.

BaseTrainer.configure_optimizers (base_trainer.py:884-916) builds `cls(lora_layers, **init_args)` from the YAML's class_path; with
`class_path: qflux_amd.optim.Adam8bit` (or AdamW, Adam, AdamW8bit, Prodigy, SGD, Adafactor, CAME, Lion, Lion8bit, PagedLion8bit, Muon, AdamWScheduleFree, RAdam, NAdam, Adamax, AdEMAMix, AdEMAMix8bit, ScaledAdamW) that optimizer is one of the classes below and
`optimizer.step()` is the family's ONE fused launch over the flat LoRA buffers instead of a foreach over every adapter view.  Each
class takes the constructor keywords of the class it stands in for and holds the same state object, steps it with the same kernel
and writes the same optimizer.bin as QwenLoraTrainStep(optimizer=...) (trainer/optim_state.py): files are interchangeable between
the two ways of driving the model and with the original packages'.

`params` must be exactly the adapter parameters of ONE model: a plain list, or torch's list of group dicts whose union is that set,
each parameter in exactly one group.  AdamW, Adam, Adam8bit, AdamW8bit, SGD, Lion, Lion8bit, PagedLion8bit, RAdam, NAdam, Adamax, AdEMAMix and AdEMAMix8bit step several groups
in their one launch (the *_grouped kernels of include/qfx.h; one group launches the ungrouped kernel, as ever); ScaledAdamW takes
groups too, which may differ in lr and weight_decay only (they become per-tensor fields of its pair table); Prodigy, Adafactor, CAME,
Muon and AdamWScheduleFree refuse a second group.  loraplus_param_groups builds the two LoRA+ groups.  The loop has clipped already
(accelerator.clip_grad_norm_, base_trainer.py:449-455), so step() launches without the fused clip; lr, betas, eps, weight_decay and
the family's own fields are read from every param_groups[k] at every step (schedulers write there).  step() never synchronises
with the host.  add_param_group is refused after the first step.
"""
from __future__ import annotations

import torch

from .trainer import optim_state as OS
from .trainer.optim_config import optimizer_kwargs_from_config

__all__ = ["AdamW", "Adam", "Adam8bit", "AdamW8bit", "Prodigy", "SGD", "Adafactor", "CAME", "Lion", "Lion8bit", "PagedLion8bit", "Muon", "AdamWScheduleFree",
           "RAdam", "NAdam", "Adamax", "AdEMAMix", "AdEMAMix8bit", "ScaledAdamW", "loraplus_param_groups"]


def _find_store(param_groups):
    """The LoraStore whose adapter parameters are exactly the union of the groups, each in exactly one group; ValueError naming the
    offending group and the first offender otherwise."""
    store, have = None, {}
    for k, group in enumerate(param_groups):
        for i, p in enumerate(group["params"]):
            where = f"parameter {i} (shape {tuple(p.shape)})" + (f" of parameter group {k}" if len(param_groups) > 1 else "")
            ref = getattr(p, "_lora_store", None)
            st = ref() if ref is not None else None
            if st is None:
                raise ValueError(f"{where} is not an adapter parameter of a qflux_amd model")
            if store is not None and st is not store:
                raise ValueError(f"{where} belongs to another model than parameter 0: one optimizer steps one model's adapters")
            if id(p) in have:
                raise ValueError(f"{where} is in parameter group {have[id(p)]} already: every adapter parameter belongs to exactly one group")
            store, have[id(p)] = st, k
    if store is None:
        raise ValueError("no parameters")
    for n, p in store.params():
        if id(p) not in have:
            raise ValueError(f"adapter parameter {n!r} of the model is missing" + (f" from all {len(param_groups)} parameter groups"
                             if len(param_groups) > 1 else "") + ": stepping a subset of the adapter set is not supported")
    return store


def _as_groups(params):
    """torch's reading of `params`: a list of group dicts as it is, anything else one group."""
    params = list(params)
    return params if params and isinstance(params[0], dict) else [{"params": params}]


def loraplus_param_groups(model, lr, loraplus_lr_ratio, weight_decay=0.0, b_weight_decay=None):
    """The two LoRA+ parameter groups (Hayou et al. 2024) of `model`'s adapters, ready for any class here that takes groups: group 0 =
    every lora_A with `lr` and `weight_decay`, group 1 = every lora_B with lr * loraplus_lr_ratio and b_weight_decay (None: the same
    weight_decay; 0.0 is the common "no decay on lora_B").  Modelled on peft.optimizers.create_loraplus_optimizer and kohya's
    loraplus_lr_ratio; peft's own grouping (it also splits embeddings and the decay / no-decay names) is not verified against the
    package, which is not a dependency."""
    if not loraplus_lr_ratio > 0:
        raise ValueError(f"loraplus_lr_ratio must be positive, not {loraplus_lr_ratio}")
    named = [(n, p) for n, p in model.named_parameters() if "lora_" in n]
    a, b = [p for n, p in named if "lora_A" in n], [p for n, p in named if "lora_B" in n]
    if not a or not b or len(a) + len(b) != len(named):
        raise ValueError(f"loraplus_param_groups: {len(a)} lora_A and {len(b)} lora_B parameters among {len(named)} adapter parameters")
    return [{"params": a, "lr": lr, "weight_decay": weight_decay},
            {"params": b, "lr": lr * loraplus_lr_ratio, "weight_decay": weight_decay if b_weight_decay is None else b_weight_decay}]


class _FlatOptimizer(torch.optim.Optimizer):
    _PATH = None       # the class path optimizer_kwargs_from_config knows this class by

    def __init__(self, params, _own_args=None, **init_args):
        """init_args: the stood-in class's keywords, mapped (and refused) as the YAML's are; _own_args: optimizer_args beyond them."""
        kw = optimizer_kwargs_from_config(self._PATH, init_args)
        _, self.family, self._cls, wd, self._args = OS.resolve_family(kw["optimizer"], kw.get("weight_decay"),
                                                                      dict(kw.get("optimizer_args") or {}, **(_own_args or {})) or None)
        # the family's own group fields (SGD's momentum, Prodigy's init_args) are visible in the group, as in the package's
        own = {n: v for n, v in self._args.items() if n in self._cls.save(None, [], 0, self._args)[0]}
        params = _as_groups(params)
        _find_store(params)              # before torch's own checks: an overlap is named with its group
        self._cls.check_groups(len(params))
        super().__init__(params, dict(dict(lr=kw["lr"], betas=kw.get("betas", (0.9, 0.999)), eps=kw.get("eps", 1e-8), weight_decay=wd), **own))
        self._raw_store = _find_store(self.param_groups)
        self._opt_state = None
        self._step_count_fused = 0

    def add_param_group(self, param_group):
        if getattr(self, "_step_count_fused", 0) or getattr(self, "_opt_state", None) is not None:
            raise RuntimeError("add_param_group after the first step (or a loaded state): the fused step's group map and state belong "
                               "to the groups the optimizer was built with; build a new optimizer and load this one's state_dict")
        super().add_param_group(param_group)
        if hasattr(self, "_raw_store"):      # after the constructor: the groups must still be one model's adapter set
            self._cls.check_groups(len(self.param_groups))
            _find_store(self.param_groups)

    def _store(self):
        """The model's store through its `lora_store` property: packed on the model's current device, gradient views attached (the
        set-to-none zero_grad drops them; accelerator.prepare() / .to() move the module)."""
        return getattr(self._raw_store.model, "lora_store", self._raw_store)

    def _group(self):
        g = self.param_groups[0]
        for n in self._args:
            if n in g:
                self._args[n] = g[n]
        return g

    def _members(self, st):
        """One tuple of store-entry indices per group, in the group's parameter order; None with one group."""
        if len(self.param_groups) == 1:
            return None
        at = {id(p): i for i, (_, p, _, _) in enumerate(st.entries)}
        return tuple(tuple(at[id(p)] for p in g["params"]) for g in self.param_groups)

    def _rows(self):
        return self.param_groups if len(self.param_groups) > 1 else None

    def _ensure_state(self, st):
        self._opt_state = OS.ensure_state(self._cls, self._opt_state, st, self._args, self._members(st))
        return self._opt_state

    @torch.no_grad()
    def step(self, closure=None):
        if self._opt_state is not None and not self._opt_state.train_mode:
            raise RuntimeError(self._opt_state.EVAL_STEP)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g, st = self._group(), self._store()
        st.ensure_grads()
        self._ensure_state(st)
        self._step_count_fused += 1
        rows = self._rows()
        self._opt_state.step(st, g["lr"], g["betas"], g["eps"], g["weight_decay"], self._step_count_fused, None, 0.0, 1.0, self._args,
                             **({"groups": rows} if rows else {}))
        return loss

    def state_dict(self):
        g, st = self._group(), self._store()
        return OS.state_dict(self._cls, self._opt_state, st, self._step_count_fused, self._args, g["lr"], g["betas"], g["eps"],
                             g["weight_decay"], groups=self._rows(), members=self._members(st))

    def load_state_dict(self, state_dict):
        g, st = self._group(), self._store()
        hyper = {n: g[n] for n in ("lr", "betas", "eps", "weight_decay")}
        self._opt_state, self._step_count_fused = OS.load_state_dict(self._cls, st, state_dict, self._args, hyper, groups=self._rows(),
                                                                     members=self._members(st))
        g.update(hyper)
        g.update({n: v for n, v in self._args.items() if n in g})


class AdamW(_FlatOptimizer):
    """torch.optim.AdamW (fp32 moments, decoupled weight decay)."""
    _PATH = "qflux_amd.optim.AdamW"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None):
        if amsgrad or maximize or differentiable:
            raise NotImplementedError("amsgrad / maximize / differentiable are not implemented by the fused AdamW step")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


class Adam(_FlatOptimizer):
    """torch.optim.Adam with weight_decay 0 (its L2 decay is not implemented: QwenLoraTrainStep(optimizer="adam"))."""
    _PATH = "qflux_amd.optim.Adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None):
        if amsgrad or maximize or differentiable:
            raise NotImplementedError("amsgrad / maximize / differentiable are not implemented by the fused Adam step")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


class Adam8bit(_FlatOptimizer):
    """bitsandbytes.optim.Adam8bit: blockwise 8-bit moments in bitsandbytes' state layout (trainer/adam8bit.py).  blocksize (256 or
    2048) is this class's own keyword; a file brings its own."""
    _PATH = "qflux_amd.optim.Adam8bit"
    _WD = 0.0

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=None, amsgrad=False, optim_bits=32, args=None,
                 min_8bit_size=4096, percentile_clipping=100, block_wise=True, is_paged=False, *, blocksize=256):
        if args is not None:
            raise NotImplementedError("bitsandbytes' `args` override object is not supported")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=self._WD if weight_decay is None else weight_decay,
                         amsgrad=amsgrad, optim_bits=optim_bits, min_8bit_size=min_8bit_size, percentile_clipping=percentile_clipping,
                         block_wise=block_wise, is_paged=is_paged, _own_args={"blocksize": blocksize})


class AdamW8bit(Adam8bit):
    """bitsandbytes.optim.AdamW8bit: Adam8bit with weight_decay 1e-2 by default."""
    _PATH = "qflux_amd.optim.AdamW8bit"
    _WD = 1e-2


class Prodigy(_FlatOptimizer):
    """prodigyopt.Prodigy (decoupled weight decay only)."""
    _PATH = "qflux_amd.optim.Prodigy"

    def __init__(self, params, lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0, decouple=True, use_bias_correction=False,
                 safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf"), fsdp_in_use=False, slice_p=1):
        if fsdp_in_use or slice_p != 1:
            raise NotImplementedError("fsdp_in_use / slice_p are not implemented by the fused Prodigy step")
        super().__init__(params, lr=lr, betas=betas, beta3=beta3, eps=eps, weight_decay=weight_decay, decouple=decouple,
                         use_bias_correction=use_bias_correction, safeguard_warmup=safeguard_warmup, d0=d0, d_coef=d_coef,
                         growth_rate=growth_rate)


class SGD(_FlatOptimizer):
    """torch.optim.SGD (momentum, dampening, Nesterov, L2 weight decay)."""
    _PATH = "qflux_amd.optim.SGD"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None):
        if differentiable:
            raise NotImplementedError("differentiable is not implemented by the fused SGD step")
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                         maximize=maximize)


class Adafactor(_FlatOptimizer):
    """transformers.optimization.Adafactor (factored second moments, update clipping, relative step / parameter scaling)."""
    _PATH = "qflux_amd.optim.Adafactor"

    def __init__(self, params, lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, weight_decay=0.0,
                 scale_parameter=True, relative_step=True, warmup_init=False):
        super().__init__(params, lr=lr, eps=eps, clip_threshold=clip_threshold, decay_rate=decay_rate, beta1=beta1,
                         weight_decay=weight_decay, scale_parameter=scale_parameter, relative_step=relative_step, warmup_init=warmup_init)


class CAME(_FlatOptimizer):
    """came_pytorch.CAME (Adafactor's factored second moments, a full first moment rescaled by a factored estimate of its
    instability).  betas is the package's triple, eps its pair; lr is required and > 0."""
    _PATH = "qflux_amd.optim.CAME"

    def __init__(self, params, lr=None, eps=(1e-30, 1e-16), clip_threshold=1.0, betas=(0.9, 0.999, 0.9999), weight_decay=0.0):
        super().__init__(params, lr=lr, eps=eps, clip_threshold=clip_threshold, betas=betas, weight_decay=weight_decay)


class Lion(_FlatOptimizer):
    """lion_pytorch.Lion (one fp32 moment, sign update, decoupled weight decay before the update).  use_triton only says where the
    package runs the same arithmetic; decoupled_weight_decay=True and the cautious variant are not implemented."""
    _PATH = "lion_pytorch.Lion"        # mapped as the class it stands in for: its own path is not a name optimizer_kwargs_from_config knows

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0, cautious_factor=1.0, use_triton=False,
                 decoupled_weight_decay=False):
        super().__init__(params, lr=lr, betas=betas, weight_decay=weight_decay, cautious_factor=cautious_factor, use_triton=use_triton,
                         decoupled_weight_decay=decoupled_weight_decay)


class Lion8bit(_FlatOptimizer):
    """bitsandbytes.optim.Lion8bit: the moment in blockwise 8-bit codes, bitsandbytes' one-state layout (trainer/adam8bit.py).
    blocksize (256 or 2048) is this class's own keyword; a file brings its own."""
    _PATH = "qflux_amd.optim.Lion8bit"

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0, optim_bits=32, args=None, min_8bit_size=4096,
                 percentile_clipping=100, block_wise=True, is_paged=False, *, blocksize=256):
        if args is not None:
            raise NotImplementedError("bitsandbytes' `args` override object is not supported")
        super().__init__(params, lr=lr, betas=betas, weight_decay=weight_decay, optim_bits=optim_bits, min_8bit_size=min_8bit_size,
                         percentile_clipping=percentile_clipping, block_wise=block_wise, is_paged=is_paged,
                         _own_args={"blocksize": blocksize})


class PagedLion8bit(Lion8bit):
    """bitsandbytes.optim.PagedLion8bit: paged memory only moves the state, the step is Lion8bit's."""
    _PATH = "qflux_amd.optim.PagedLion8bit"


class Muon(_FlatOptimizer):
    """torch.optim.Muon (momentum, Newton-Schulz orthogonalisation of every adapter matrix's update in bf16, decoupled weight decay,
    the learning rate adjusted per matrix shape).  eps is Muon's own: the floor of the update's Frobenius norm."""
    _PATH = "qflux_amd.optim.Muon"

    def __init__(self, params, lr=1e-3, weight_decay=0.1, momentum=0.95, nesterov=True, ns_coefficients=(3.4445, -4.7750, 2.0315),
                 eps=1e-7, ns_steps=5, adjust_lr_fn=None):
        if not 0.0 <= lr:
            raise ValueError(f"Learning rate should be >= 0 but is: {lr}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"weight decay should be >= 0 but is: {weight_decay}")
        super().__init__(params, lr=lr, weight_decay=weight_decay, momentum=momentum, nesterov=nesterov, ns_coefficients=ns_coefficients,
                         eps=eps, ns_steps=ns_steps, adjust_lr_fn=adjust_lr_fn)


class RAdam(_FlatOptimizer):
    """torch.optim.RAdam (variance rectification: Adam without the second moment until rho_t > 5; L2 or decoupled weight decay)."""
    _PATH = "qflux_amd.optim.RAdam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, decoupled_weight_decay=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=decoupled_weight_decay,
                         maximize=maximize, capturable=capturable, differentiable=differentiable)


class NAdam(_FlatOptimizer):
    """torch.optim.NAdam (Adam with the Nesterov momentum schedule mu_t; L2 or decoupled weight decay)."""
    _PATH = "qflux_amd.optim.NAdam"

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, momentum_decay=4e-3, decoupled_weight_decay=False,
                 *, foreach=None, maximize=False, capturable=False, differentiable=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, momentum_decay=momentum_decay,
                         decoupled_weight_decay=decoupled_weight_decay, maximize=maximize, capturable=capturable,
                         differentiable=differentiable)


class Adamax(_FlatOptimizer):
    """torch.optim.Adamax (Adam under the infinity norm: exp_inf = max(beta2 exp_inf, |g| + eps); L2 weight decay)."""
    _PATH = "qflux_amd.optim.Adamax"

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, foreach=None, *, maximize=False,
                 differentiable=False, capturable=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=maximize, capturable=capturable,
                         differentiable=differentiable)


class AdEMAMix(_FlatOptimizer):
    """bitsandbytes.optim.AdEMAMix (Adam plus a slow gradient average that enters the update with weight alpha; fp32 states).  betas
    is the triple (beta1, beta2, beta3); t_alpha / t_beta3: the lengths in steps of the warm-ups of alpha and beta3, None = none."""
    _PATH = "qflux_amd.optim.AdEMAMix"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999, 0.9999), alpha=5.0, t_alpha=None, t_beta3=None, eps=1e-8, weight_decay=1e-2,
                 optim_bits=32, min_8bit_size=4096, is_paged=False):
        super().__init__(params, lr=lr, betas=betas, alpha=alpha, t_alpha=t_alpha, t_beta3=t_beta3, eps=eps, weight_decay=weight_decay,
                         optim_bits=optim_bits, min_8bit_size=min_8bit_size, is_paged=is_paged)


class AdEMAMix8bit(_FlatOptimizer):
    """bitsandbytes.optim.AdEMAMix8bit: the three states in blockwise 8-bit codes, both averages in one two-plane state1
    (trainer/optim_state.py).  blocksize (256 or 2048) is this class's own keyword; a file brings its own."""
    _PATH = "qflux_amd.optim.AdEMAMix8bit"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999, 0.9999), alpha=5.0, t_alpha=None, t_beta3=None, eps=1e-8, weight_decay=1e-2,
                 min_8bit_size=4096, is_paged=False, *, blocksize=256):
        super().__init__(params, lr=lr, betas=betas, alpha=alpha, t_alpha=t_alpha, t_beta3=t_beta3, eps=eps, weight_decay=weight_decay,
                         min_8bit_size=min_8bit_size, is_paged=is_paged, _own_args={"blocksize": blocksize})


class ScaledAdamW(_FlatOptimizer):
    """Riemannian-preconditioned AdamW for LoRA pairs (Zhang & Pilanci, "Riemannian Preconditioned LoRA", ICML 2024): the gradient
    of lora_A is multiplied by (B^T B + reg I)^-1, that of lora_B by (A A^T + reg I)^-1, then AdamW -- one launch, one workgroup
    per pair (include/qfx.h: qfx_scaled_adamw_step, whose listing is the specification; the authors' package was not at hand).
    `params` must be the adapter set of one model, as for Muon: the pairs are found through the model's flat store.  Groups may
    differ in lr and weight_decay (loraplus_param_groups), not in betas or eps.  precondition=False is plain AdamW per tensor.
    `skipped` (a device int32 after the first step) counts the pairs the last step left untouched."""
    _PATH = "qflux_amd.optim.ScaledAdamW"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, reg=1e-6, precondition=True):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, reg=reg, precondition=precondition)

    @property
    def skipped(self):
        return None if self._opt_state is None else self._opt_state.skipped


class AdamWScheduleFree(_FlatOptimizer):
    """schedulefree.AdamWScheduleFree (no first moment, no schedule: the adapter weights are the gradient point y in train mode and
    the averaged x in eval mode).  As with the package, call .train() before training and .eval() before validating or saving the
    weights; step() in eval mode raises.  foreach only says how the package loops over its tensors."""
    _PATH = "qflux_amd.optim.AdamWScheduleFree"

    def __init__(self, params, lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, warmup_steps=0, r=0.0, weight_lr_power=2.0,
                 foreach=True):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, warmup_steps=warmup_steps, r=r,
                         weight_lr_power=weight_lr_power, foreach=foreach)

    def _swap(self, train):
        g, st = self._group(), self._store()
        self._ensure_state(st).swap(st, g["betas"][0], train)

    @torch.no_grad()
    def eval(self):
        """y -> x in place (one launch over the flat buffer); nothing happens in eval mode already."""
        self._swap(False)

    @torch.no_grad()
    def train(self):
        """x -> y in place; nothing happens in train mode already."""
        self._swap(True)
