"""Exponential moving averages of the adapter weights (diffusers.training_utils.EMAModel, every diffusers training script's
--use_ema) over the flat LoRA buffer.

get_decay restates EMAModel.get_decay; EmaState holds up to four flat fp32 shadow buffers of one LoraStore and plugs into the train
steps (QwenLoraTrainStep(ema_decay=...): updated behind every optimizer step in ONE launch, swapped into the parameter buffer for
eval() / sampling / the _ema weight files, saved as ema.bin); EMAModel is the class of that name for the reference's own loop, next
to the optimizer classes of qflux_amd.optim.  The update is EMAModel.step's `s.sub_(one_minus_decay * (s - p))` with its three fp32
roundings (include/qfx.h, qfx_ema_update); swapping a shadow in exchanges the two buffers bit for bit (qfx_ema_swap), so the trained
weights come back exactly.  diffusers is not a dependency: the semantics are restated from the published class and are not pinned
against the package.
"""
from __future__ import annotations

import torch

from . import ops

__all__ = ["get_decay", "EmaState", "EMAModel", "check_config", "ensure_state"]

MAX_SHADOWS = ops.EMA_MAX_SHADOWS
ARG_DEFAULTS = dict(min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3)
KEYS = ("decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power", "shadow_params")
EVAL_STEP = ("optimizer step in eval form: the adapter weights hold EMA shadow {k}, not the trained weights the gradient belongs "
             "to; call train() first")
EVAL_GRAD = ("forward_backward in eval form: the adapter weights hold EMA shadow {k}, a gradient taken there would train the wrong "
             "weights; call train() first")


def get_decay(optimization_step, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3):
    """EMAModel.get_decay in Python floats: the decay of the optimization_step-th update (counted from 1)."""
    step = max(0, optimization_step - update_after_step - 1)
    if step <= 0:
        return 0.0
    cur = 1 - (1 + step / inv_gamma) ** -power if use_ema_warmup else (1 + step) / (10 + step)
    return max(min(cur, decay), min_decay)


def check_config(ema_decay, ema_args=None):
    """The train steps' ema_decay / ema_args -> (tuple of 1..4 decays, the EMAModel keywords with defaults filled in), or
    (None, None) for ema_decay=None."""
    if ema_decay is None:
        if ema_args:
            raise ValueError("ema_args without ema_decay")
        return None, None
    decays = (float(ema_decay),) if isinstance(ema_decay, (int, float)) else tuple(float(d) for d in ema_decay)
    if not 1 <= len(decays) <= MAX_SHADOWS:
        raise ValueError(f"ema_decay: 1..{MAX_SHADOWS} decays, not {len(decays)}")
    for d in decays:
        if not 0.0 <= d <= 1.0:
            raise ValueError(f"ema_decay must lie in [0, 1], not {d}")
    unknown = set(ema_args or {}) - set(ARG_DEFAULTS)
    if unknown:
        raise ValueError(f"ema_args: unknown {sorted(unknown)}; the EMAModel keywords are {sorted(ARG_DEFAULTS)}")
    args = dict(ARG_DEFAULTS, **(ema_args or {}))
    if not 0.0 <= args["min_decay"] <= 1.0:
        raise ValueError(f"ema_args: min_decay must lie in [0, 1], not {args['min_decay']}")
    return decays, args


def _layout_key(store):
    return (tuple((off, k) for _, _, off, k in store.entries), str(store.pflat.device))


def ensure_state(state, store, decays, args):
    """The EmaState for the store's current layout: fresh shadows (copies of the weights, no update counted) when there is none yet
    or the adapter set changed, as optim_state.ensure_state does for optimizer state."""
    if state is None or state.key != _layout_key(store):
        state = EmaState(store, decays, **args)
    return state


class EmaState:
    """Up to four flat fp32 shadows of store.pflat, created as copies of it; optimization_step counts update() calls; `active` is the
    shadow currently swapped into the parameter buffer (None: the parameter buffer holds the trained weights).  While shadow k is
    swapped in, its buffer holds the trained weights."""

    def __init__(self, store, decays, **ema_args):
        self.decays, self.args = check_config(decays, ema_args)
        self.key = _layout_key(store)
        self.shadows = [store.pflat.detach().clone() for _ in self.decays]
        self.optimization_step = 0
        self.active = None

    def _index(self, k):
        if not (isinstance(k, int) and 0 <= k < len(self.shadows)):
            raise ValueError(f"EMA shadow {k!r}: this state has shadows 0..{len(self.shadows) - 1}")
        return k

    def decay_at(self, step):
        return [get_decay(step, d, **self.args) for d in self.decays]

    def update(self, store):
        """One more optimizer step happened: every shadow moves towards store.pflat at its decay for this step, in one launch on
        the current stream."""
        if self.active is not None:
            raise RuntimeError(EVAL_STEP.format(k=self.active))
        self.optimization_step += 1
        ops.ema_update(store.pflat, self.shadows, [1 - d for d in self.decay_at(self.optimization_step)])

    def swap_in(self, store, k=0):
        """Shadow k into the parameter buffer (one launch; the shadow swapped in before, if any, goes out first)."""
        k = self._index(k)
        if self.active == k:
            return
        self.swap_out(store)
        ops.ema_swap(store.pflat, self.shadows[k])
        self.active = k

    def swap_out(self, store):
        """The trained weights back into the parameter buffer, bit for bit; nothing happens when no shadow is in."""
        if self.active is not None:
            ops.ema_swap(store.pflat, self.shadows[self.active])
            self.active = None

    def buffers(self):
        return [(f"ema{k}", t) for k, t in enumerate(self.shadows)]

    @staticmethod
    def names(decays):
        return [f"ema{k}" for k in range(len(decays))]

    def _values(self, store, k):
        """Shadow k's values wherever they are now."""
        return store.pflat if self.active == k else self.shadows[k]

    def state_dict(self, store):
        """One dict per shadow in EMAModel.state_dict()'s layout; shadow_params: one CPU tensor per adapter parameter in
        named_parameters() order, shaped like the parameter."""
        out = []
        for k, d in enumerate(self.decays):
            flat = self._values(store, k).detach()
            out.append(dict(decay=d, min_decay=self.args["min_decay"], optimization_step=self.optimization_step,
                            update_after_step=self.args["update_after_step"], use_ema_warmup=self.args["use_ema_warmup"],
                            inv_gamma=self.args["inv_gamma"], power=self.args["power"],
                            shadow_params=[flat[off:off + n].view(p.shape).cpu().clone() for _, p, off, n in store.entries]))
        return out

    def load_state_dict(self, store, sd):
        """The file's shadows, update count and settings (shadow k's decay from sd[k], the shared keywords from sd[0]) replace this
        state's; the number of shadows and every parameter's shape must match."""
        sd = list(sd)
        if len(sd) != len(self.shadows):
            raise ValueError(f"EMA state with {len(sd)} shadows for a step configured with {len(self.shadows)}")
        for k, e in enumerate(sd):
            missing = set(KEYS) - set(e)
            if missing:
                raise ValueError(f"EMA state of shadow {k} lacks {sorted(missing)}")
            if len(e["shadow_params"]) != len(store.entries):
                raise ValueError(f"EMA state of shadow {k} has {len(e['shadow_params'])} tensors, {len(store.entries)} adapter parameters")
            for i, (t, (_, p, _, _)) in enumerate(zip(e["shadow_params"], store.entries)):
                if tuple(t.shape) != tuple(p.shape):
                    raise ValueError(f"EMA state of shadow {k}: tensor {i} has shape {tuple(t.shape)}, {tuple(p.shape)} expected")
        decays, args = check_config([e["decay"] for e in sd], {n: sd[0][n] for n in ARG_DEFAULTS})
        for k, e in enumerate(sd):
            flat = self._values(store, k)
            for t, (_, _, off, n) in zip(e["shadow_params"], store.entries):
                flat[off:off + n].copy_(t.reshape(-1).to(device=flat.device, dtype=torch.float32))
        self.decays, self.args, self.optimization_step = decays, args, int(sd[0]["optimization_step"])


class EMAModel:
    """diffusers.training_utils.EMAModel for the reference's loop: `ema = EMAModel(lora_layers, decay=...)`, `ema.step(lora_layers)`
    behind every optimizer.step(), `ema.store(...)` / `ema.copy_to(...)` / `ema.restore(...)` around validation.  When the
    parameters are the adapter parameters of ONE qflux_amd model (the views of its flat LoRA buffer), each of step, copy_to, store
    and restore is one flat launch or copy and the parameters argument of the methods is not read again; otherwise every tensor is
    stepped by the plain torch expression, in the same rounding order.  foreach only says how the package loops over its tensors;
    model_cls / model_config (save_pretrained) are kept and not used."""

    def __init__(self, parameters, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3,
                 foreach=False, model_cls=None, model_config=None):
        from .optim import _find_store
        parameters = list(parameters)
        (decay,), self._args = check_config(decay, dict(min_decay=min_decay, update_after_step=update_after_step,
                                                        use_ema_warmup=use_ema_warmup, inv_gamma=inv_gamma, power=power))
        self.decay, self.cur_decay_value, self.foreach, self.model_cls, self.model_config = decay, None, foreach, model_cls, model_config
        self.temp_stored_params = None
        try:
            self._raw_store = _find_store([{"params": parameters}])
        except ValueError:
            self._raw_store = None
        if self._raw_store is not None:
            self._state = EmaState(self._store(), (decay,), **self._args)
        else:
            self._state = None
            self._step = 0
            self._shadow = [p.detach().clone() for p in parameters]

    def _store(self):
        return getattr(self._raw_store.model, "lora_store", self._raw_store)

    def _flat(self):
        """(store, state) of the flat path, the state re-keyed to the store's layout."""
        st = self._store()
        self._state = ensure_state(self._state, st, (self.decay,), self._args)
        return st, self._state

    min_decay = property(lambda self: self._args["min_decay"])
    update_after_step = property(lambda self: self._args["update_after_step"])
    use_ema_warmup = property(lambda self: self._args["use_ema_warmup"])
    inv_gamma = property(lambda self: self._args["inv_gamma"])
    power = property(lambda self: self._args["power"])

    @property
    def optimization_step(self):
        return self._step if self._state is None else self._state.optimization_step

    @property
    def shadow_params(self):
        if self._state is None:
            return self._shadow
        st, state = self._flat()
        return [state.shadows[0][off:off + n].view(p.shape) for _, p, off, n in st.entries]

    def get_decay(self, optimization_step):
        return get_decay(optimization_step, self.decay, **self._args)

    @torch.no_grad()
    def step(self, parameters=None):
        if self._state is not None:
            st, state = self._flat()
            state.update(st)
            self.cur_decay_value = state.decay_at(state.optimization_step)[0]
            return
        parameters = list(parameters)
        self._step += 1
        self.cur_decay_value = self.get_decay(self._step)
        one_minus_decay = 1 - self.cur_decay_value
        for s, p in zip(self._shadow, parameters):
            if p.requires_grad:
                s.sub_(one_minus_decay * (s - p))
            else:
                s.copy_(p)

    @torch.no_grad()
    def copy_to(self, parameters=None):
        """The averaged weights into the parameters."""
        if self._state is not None:
            st, state = self._flat()
            st.pflat.copy_(state.shadows[0])
            return
        for s, p in zip(self._shadow, list(parameters)):
            p.data.copy_(s.to(p.device).data)

    @torch.no_grad()
    def store(self, parameters=None):
        """Keep a copy of the current parameters for restore()."""
        if self._state is not None:
            self.temp_stored_params = self._store().pflat.detach().clone()
        else:
            self.temp_stored_params = [p.detach().cpu().clone() for p in parameters]

    @torch.no_grad()
    def restore(self, parameters=None):
        if self.temp_stored_params is None:
            raise RuntimeError("This ExponentialMovingAverage has no `store()`ed weights to `restore()`")
        if self._state is not None:
            self._store().pflat.copy_(self.temp_stored_params)
        else:
            for c, p in zip(self.temp_stored_params, list(parameters)):
                p.data.copy_(c.data)
        self.temp_stored_params = None

    def to(self, device=None, dtype=None, non_blocking=False):
        """Plain tensors move like the package's (dtype: floating-point shadows only); the flat shadow lives with the model's flat
        buffer in fp32 and follows it by itself."""
        if self._state is None:
            self._shadow = [s.to(device=device, dtype=dtype, non_blocking=non_blocking) if s.is_floating_point()
                            else s.to(device=device, non_blocking=non_blocking) for s in self._shadow]
        return self

    def state_dict(self):
        if self._state is not None:
            st, state = self._flat()
            return state.state_dict(st)[0]
        return dict(decay=self.decay, min_decay=self.min_decay, optimization_step=self._step, update_after_step=self.update_after_step,
                    use_ema_warmup=self.use_ema_warmup, inv_gamma=self.inv_gamma, power=self.power, shadow_params=self._shadow)

    def load_state_dict(self, state_dict):
        if self._state is not None:
            st, state = self._flat()
            state.load_state_dict(st, [state_dict])
            self.decay, self._args = state.decays[0], state.args
            return
        missing = set(KEYS) - set(state_dict)
        if missing:
            raise ValueError(f"EMA state lacks {sorted(missing)}")
        shadow = list(state_dict["shadow_params"])
        if len(shadow) != len(self._shadow) or any(a.shape != b.shape for a, b in zip(shadow, self._shadow)):
            raise ValueError("shadow_params do not match this EMAModel's parameters")
        (self.decay,), self._args = check_config(state_dict["decay"], {n: state_dict[n] for n in ARG_DEFAULTS})
        self._step = int(state_dict["optimization_step"])
        self._shadow = [t.detach().clone().to(s.device) for t, s in zip(shadow, self._shadow)]
