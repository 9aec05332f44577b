"""The reference's YAML `optimizer: {class_path, init_args}` -> keyword arguments of the train steps (and of the torch.optim classes
in qflux_amd.optim): optimizer_kwargs_from_config.  Depends on the state classes only; which init_args become optimizer_args is read
from their DEFAULTS."""
from __future__ import annotations

from . import optim_state as OS

# class path -> the optimizer= family; a pair is (with state_bits=8, with state_bits=32).  The qflux_amd.optim classes map to the family
# each of them runs whatever state_bits says; qflux_amd.optim.Lion and torch.optim.SGD are deliberately absent
_ADAM8, _ADAMW8, _LION8 = ("adam8bit_blockwise", "adam8bit"), ("adamw8bit_blockwise", "adamw"), ("lion8bit_blockwise", "lion")
_ADEMAMIX8 = ("ademamix8bit_blockwise", "ademamix")
_FAMILY = {
    "torch.optim.AdamW": "adamw", "bitsandbytes.optim.AdamW": "adamw", "qflux_amd.optim.AdamW": "adamw",
    "torch.optim.Adam": "adam", "bitsandbytes.optim.Adam": "adam", "qflux_amd.optim.Adam": "adam",
    "bitsandbytes.optim.Adam8bit": _ADAM8, "bitsandbytes.optim.PagedAdam8bit": _ADAM8, "qflux_amd.optim.Adam8bit": _ADAM8[0],
    "bitsandbytes.optim.AdamW8bit": _ADAMW8, "bitsandbytes.optim.PagedAdamW8bit": _ADAMW8, "qflux_amd.optim.AdamW8bit": _ADAMW8[0],
    "lion_pytorch.Lion": "lion", "bitsandbytes.optim.Lion": "lion", "bitsandbytes.optim.Lion32bit": "lion",
    "bitsandbytes.optim.Lion8bit": _LION8, "bitsandbytes.optim.PagedLion8bit": _LION8,
    "qflux_amd.optim.Lion8bit": _LION8[0], "qflux_amd.optim.PagedLion8bit": _LION8[0],
    "prodigyopt.Prodigy": "prodigy", "qflux_amd.optim.Prodigy": "prodigy", "qflux_amd.optim.SGD": "sgd",
    "transformers.optimization.Adafactor": "adafactor", "transformers.Adafactor": "adafactor", "qflux_amd.optim.Adafactor": "adafactor",
    "came_pytorch.CAME": "came", "came_pytorch.CAME.CAME": "came", "qflux_amd.optim.CAME": "came",
    "torch.optim.Muon": "muon", "qflux_amd.optim.Muon": "muon",
    "schedulefree.AdamWScheduleFree": "adamw_schedulefree", "qflux_amd.optim.AdamWScheduleFree": "adamw_schedulefree",
    "torch.optim.RAdam": "radam", "qflux_amd.optim.RAdam": "radam", "torch.optim.NAdam": "nadam", "qflux_amd.optim.NAdam": "nadam",
    "torch.optim.Adamax": "adamax", "qflux_amd.optim.Adamax": "adamax",
    "bitsandbytes.optim.AdEMAMix": "ademamix", "bitsandbytes.optim.AdEMAMix32bit": "ademamix",
    "bitsandbytes.optim.PagedAdEMAMix": "ademamix", "bitsandbytes.optim.PagedAdEMAMix32bit": "ademamix",
    "qflux_amd.optim.AdEMAMix": "ademamix",
    "bitsandbytes.optim.AdEMAMix8bit": _ADEMAMIX8, "bitsandbytes.optim.PagedAdEMAMix8bit": _ADEMAMIX8,
    "qflux_amd.optim.AdEMAMix8bit": _ADEMAMIX8[0],
    "qflux_amd.optim.ScaledAdamW": "scaled_adamw",
}
# the lr of torch.optim.RAdam / NAdam / Adamax when the config gives none
_ADAMX_LR = {"radam": 1e-3, "nadam": 2e-3, "adamax": 2e-3}
# init_args of the 8-bit bnb classes the blockwise step refuses: name -> (the one value it accepts, what any other value asks for)
_REFUSED_8BIT = {"percentile_clipping": (100, "percentile clipping"), "max_unorm": (0.0, "update-norm clipping (max_unorm)"),
                 "block_wise": (True, "non-blockwise 8-bit state"), "skip_zeros": (False, "skip_zeros"), "amsgrad": (False, "amsgrad")}


def _take(a: dict, cls) -> dict:
    """The init_args that are optimizer_args of the family (the names its state class owns in DEFAULTS), moved out of `a`."""
    return {k: a.pop(k) for k in list(a) if k in cls.DEFAULTS}


def optimizer_kwargs_from_config(class_path: str, init_args: dict | None = None, state_bits: int = 32) -> dict:
    """The reference's YAML `optimizer: {class_path, init_args}` (BaseTrainer.configure_optimizers, base_trainer.py:884-909) ->
    keyword arguments of QwenLoraTrainStep / FluxKontextTrainStep.
        torch.optim.AdamW                      -> optimizer="adamw"   (lr, betas, eps, weight_decay)
        bitsandbytes.optim.Adam8bit / Adam     -> optimizer="adam8bit": Adam with FP32 moments (see resolve_family; 8-bit states buy nothing
        bitsandbytes.optim.AdamW8bit / AdamW   -> optimizer="adamw"     next to 288 GB of HBM)
        prodigyopt.Prodigy                     -> optimizer="prodigy" + optimizer_args
    state_bits=8 maps the four 8-bit bnb classes (Adam8bit, PagedAdam8bit, AdamW8bit, PagedAdamW8bit) to the blockwise 8-bit optimizer
    with bnb's state layout instead: "adam8bit_blockwise" (weight decay default 0) / "adamw8bit_blockwise" (default 1e-2), min_8bit_size
    honoured; percentile_clipping != 100, max_unorm != 0, block_wise=False, skip_zeros=True and amsgrad=True are refused; is_paged only
    moves memory (same math).  state_bits=32 is the mapping above.
    The torch.optim classes of qflux_amd.optim (the drop-in loop's optimizers) map to the family each of them runs, whatever state_bits
    says: AdamW -> "adamw", Adam -> "adam", Adam8bit / AdamW8bit -> "adam8bit_blockwise" / "adamw8bit_blockwise" (the class is named for
    its state), Prodigy -> "prodigy", SGD -> "sgd" + optimizer_args (momentum, dampening, nesterov; maximize is refused).
    torch.optim.SGD itself is not mapped.
        transformers.optimization.Adafactor / transformers.Adafactor / qflux_amd.optim.Adafactor -> optimizer="adafactor" + optimizer_args
    (eps pair, clip_threshold, decay_rate, beta1, scale_parameter, relative_step, warmup_init); lr is None with relative_step (the
    package's default) and the package's refusals apply: lr with relative_step, warmup_init without it, no lr without it.
        lion_pytorch.Lion / bitsandbytes.optim.Lion / Lion32bit -> optimizer="lion" (lr, betas, weight_decay;
    betas left out = the class's (0.9, 0.99), weight decay default 0); lion_pytorch's use_triton and decoupled_weight_decay=False are
    accepted (where the arithmetic runs; the plain decoupled form), decoupled_weight_decay=True and cautious_factor != 1 are refused.
        bitsandbytes.optim.Lion8bit / PagedLion8bit -> "lion" (fp32 moment) with state_bits=32, "lion8bit_blockwise" (bnb's one-state
    8-bit layout, min_8bit_size honoured) with state_bits=8 -- the Adam8bit rule, with the same init_args refused;
    qflux_amd.optim.Lion8bit / PagedLion8bit always map to the blockwise form.  The path qflux_amd.optim.Lion itself is NOT mapped
    here and keeps raising (tests/test_optim_classes_cpu.py pins that refusal): the class exists and steps "lion", a config for the
    fused train step names lion_pytorch.Lion, whose keywords it takes.
        torch.optim.Muon / qflux_amd.optim.Muon -> optimizer="muon" + optimizer_args (momentum, nesterov, ns_coefficients, eps,
    ns_steps, adjust_lr_fn); weight decay left out is the class's 0.1; ns_steps >= 100 and an unknown adjust_lr_fn are refused with
    torch's messages.
        schedulefree.AdamWScheduleFree / qflux_amd.optim.AdamWScheduleFree -> optimizer="adamw_schedulefree" + optimizer_args
    (warmup_steps, r, weight_lr_power); lr and weight decay left out are the class's 0.0025 and 0; foreach is dropped.  Keep the
    reference's lr_scheduler at `constant`: the warm-up is the optimizer's own warmup_steps.
        came_pytorch.CAME / came_pytorch.CAME.CAME / qflux_amd.optim.CAME -> optimizer="came" + optimizer_args (eps pair,
    clip_threshold); betas is the package's triple (left out: (0.9, 0.999, 0.9999)); lr is required and > 0 (the package's assert),
    weight decay left out is 0; a betas that is no triple, an eps that is no pair, a beta outside [0, 1] and any other keyword are
    refused.
        torch.optim.RAdam / NAdam / Adamax and qflux_amd.optim.RAdam / NAdam / Adamax -> optimizer="radam" / "nadam" / "adamax" (lr,
    betas, eps, weight_decay; left out: the class's own lr 1e-3 / 2e-3 / 2e-3, weight decay 0) + optimizer_args
    (decoupled_weight_decay for RAdam and NAdam, momentum_decay for NAdam; none for Adamax); foreach is dropped; maximize,
    capturable and differentiable =True are refused, and so is every keyword the class itself does not take (amsgrad, fused, ...);
    torch's constructor checks apply with torch's messages (ValueError).
        bitsandbytes.optim.AdEMAMix / AdEMAMix32bit / PagedAdEMAMix / PagedAdEMAMix32bit and qflux_amd.optim.AdEMAMix ->
    optimizer="ademamix" (lr, betas -- the triple beta1, beta2, beta3 --, eps, weight_decay; left out: lr 1e-3, betas (0.9, 0.999,
    0.9999), weight decay 1e-2) + optimizer_args (alpha, t_alpha, t_beta3).  bitsandbytes.optim.AdEMAMix8bit / PagedAdEMAMix8bit ->
    "ademamix" (fp32 states) with state_bits=32, "ademamix8bit_blockwise" (bnb's 8-bit layout with a two-plane state1,
    min_8bit_size honoured) with state_bits=8 -- the Adam8bit rule; qflux_amd.optim.AdEMAMix8bit always maps to the blockwise form.
    is_paged and optim_bits are dropped; percentile_clipping != 100, max_unorm != 0, block_wise=False, skip_zeros=True and
    amsgrad=True are refused, and so is every other keyword; a betas that is no triple, a beta outside [0, 1), a negative lr, eps,
    weight_decay or alpha and a t_alpha / t_beta3 that is neither None nor > 0 raise ValueError.
        qflux_amd.optim.ScaledAdamW -> optimizer="scaled_adamw" (lr, betas, eps, weight_decay; left out: lr 1e-3, weight decay
    1e-2) + optimizer_args (reg, precondition); reg that is not finite and > 0, a precondition that is no bool and every other
    keyword are refused.  The authors' package of the method was not at hand, so no class path of theirs is mapped.
    Unknown classes raise: silently training with a different optimizer is worse than stopping."""
    if state_bits not in (8, 32):
        raise ValueError(f"state_bits must be 8 or 32, not {state_bits!r}")
    a = dict(init_args or {})
    fam = _FAMILY.get(class_path)
    if isinstance(fam, tuple):
        fam = fam[state_bits == 32]
    out = {}
    if fam in ("adafactor", "muon"):
        # eps is the family's own (Adafactor's pair, the floor of Muon's norm): one of its optimizer_args, read before the common
        # keywords below; neither class takes betas
        if "betas" in a:
            raise NotImplementedError(f"unsupported optimizer init_args for {class_path}: ['betas']")
        if fam == "adafactor":      # lr may be None (relative_step); the package's own refusals apply
            lr = a.pop("lr", None)
            out["lr"] = None if lr is None else float(lr)
            args = _take(a, OS.AdafactorState)
            if "eps" in args:
                args["eps"] = tuple(float(e) for e in args["eps"])
            OS.AdafactorState.validate(dict(OS.AdafactorState.DEFAULTS, **args), out["lr"])
        else:
            args = _take(a, OS.MuonState)
            OS.MuonState.validate(dict(OS.MuonState.DEFAULTS, **args))
            if "ns_coefficients" in args:
                args["ns_coefficients"] = tuple(float(c) for c in args["ns_coefficients"])
        out["optimizer_args"] = args
    elif fam == "came":
        # eps is the family's own pair, read before the common keywords below; betas is its triple and travels as betas
        args = _take(a, OS.CameState)
        if "eps" in args and isinstance(args["eps"], (tuple, list)):
            args["eps"] = tuple(float(e) for e in args["eps"])
        betas = tuple(float(b) for b in a["betas"]) if isinstance(a.get("betas"), (tuple, list)) else a.get("betas")
        OS.CameState.validate(dict(OS.CameState.DEFAULTS, **args), a.get("lr"), OS.CameState.BETAS if betas is None else betas)
        out["optimizer_args"] = args
    for k in ("lr", "eps", "weight_decay"):
        if k in a:
            out[k] = float(a.pop(k))
    if "betas" in a:
        out["betas"] = tuple(float(b) for b in a.pop("betas"))
    if fam is None:
        raise NotImplementedError(f"optimizer {class_path!r} has no fused counterpart (use the drop-in path with the torch optimizer)")
    out["optimizer"] = fam
    if fam in OS.ADEMAMIX:
        cls = OS.FAMILIES[fam][0]
        out.setdefault("lr", 1e-3)
        out.setdefault("weight_decay", 1e-2)
        out.setdefault("betas", cls.BETAS)
        for k, (ok, what) in _REFUSED_8BIT.items():
            if k in a and a.pop(k) != ok:
                raise NotImplementedError(f"{class_path}: {what} is not implemented by the fused AdEMAMix step ({k} must be {ok!r})")
        args = {k: a.pop(k) for k in list(a) if k in cls.OWN}
        OS.ops.ademamix_check(out["lr"], out["betas"], out.get("eps", 1e-8), out["weight_decay"], **dict(cls.OWN, **args))
        m8 = a.pop("min_8bit_size", None)      # a keyword of every bnb class; only the 8-bit state reads it
        if m8 is not None and fam.endswith("_blockwise"):
            args["min_8bit_size"] = int(m8)
        a.pop("is_paged", None)        # paged memory: where the state lives, not what is computed
        a.pop("optim_bits", None)      # the class name decides the state's width
        out["optimizer_args"] = args
        if a:      # before the common knobs below are dropped: none of them is a keyword of these classes
            raise NotImplementedError(f"unsupported optimizer init_args for {class_path}: {sorted(a)}")
    elif fam == "scaled_adamw":
        out.setdefault("lr", 1e-3)
        out.setdefault("weight_decay", 1e-2)
        args = _take(a, OS.ScaledAdamWState)
        full = dict(OS.ScaledAdamWState.DEFAULTS, **args)
        OS.ScaledAdamWState.validate(full)
        OS.ops.scaled_adamw_check(out["lr"], out.get("betas", (0.9, 0.999)), out.get("eps", 1e-8), full["reg"], full["precondition"])
        out["optimizer_args"] = args
        if a:      # before the common knobs below are dropped: none of them is a keyword of this class
            raise NotImplementedError(f"unsupported optimizer init_args for {class_path}: {sorted(a)}")
    elif fam.endswith("_blockwise"):
        out.setdefault("weight_decay", 0.01 if fam == "adamw8bit_blockwise" else 0.0)
        for k, (ok, what) in _REFUSED_8BIT.items():
            if k in a and a.pop(k) != ok:
                raise NotImplementedError(f"{class_path}: {what} is not implemented by the blockwise 8-bit step ({k} must be {ok!r})")
        if "min_8bit_size" in a:
            out["optimizer_args"] = {"min_8bit_size": int(a.pop("min_8bit_size"))}
        a.pop("is_paged", None)        # paged memory: where the state lives, not what is computed
        a.pop("optim_bits", None)      # the 8-bit classes pass 8 whatever this says
    elif fam in ("adam", "adam8bit"):
        out.setdefault("weight_decay", 0.0)
    elif fam == "lion":
        out.setdefault("weight_decay", 0.0)
        if a.pop("decoupled_weight_decay", False):
            raise NotImplementedError(f"{class_path}: decoupled_weight_decay=True (weight decay scaled by lr / the initial lr) is not implemented")
        if float(a.pop("cautious_factor", 1.0)) != 1.0:
            raise NotImplementedError(f"{class_path}: the cautious variant (cautious_factor != 1) is not implemented")
        a.pop("use_triton", None)      # where lion_pytorch runs the same arithmetic
    elif fam == "sgd":
        if a.pop("maximize", False):
            raise NotImplementedError(f"{class_path}: maximize=True is not implemented")
        out["optimizer_args"] = _take(a, OS.SgdState)
        a.pop("differentiable", None)
    elif fam == "adamw_schedulefree":
        out.setdefault("lr", 0.0025)
        out.setdefault("weight_decay", 0.0)
        out["optimizer_args"] = _take(a, OS.ScheduleFreeAdamWState)
        OS.ScheduleFreeAdamWState.validate(dict(OS.ScheduleFreeAdamWState.DEFAULTS, **out["optimizer_args"]))
    elif fam == "prodigy":
        out["optimizer_args"] = _take(a, OS.ProdigyState)
    elif fam in OS.ADAMX:
        cls = OS.ADAMX[fam]
        on = [k for k in cls.REFUSED if a.pop(k, False)]
        if on:
            raise NotImplementedError(f"{class_path}: {' / '.join(on)}=True is not implemented by the fused step")
        out.setdefault("lr", _ADAMX_LR[fam])
        out.setdefault("weight_decay", 0.0)
        args = _take(a, cls)
        cls.validate(dict(cls.DEFAULTS, **args))
        OS.ops.adamx_check(out["lr"], out.get("betas", (0.9, 0.999)), out.get("eps", 1e-8), out["weight_decay"])
        if cls.DEFAULTS:
            out["optimizer_args"] = args
        a.pop("foreach", None)         # how torch loops over its tensors
        if a:      # before the common knobs below are dropped: none of them is a keyword of these classes
            raise NotImplementedError(f"unsupported optimizer init_args for {class_path}: {sorted(a)}")
    for k in ("min_8bit_size", "percentile_clipping", "block_wise", "optim_bits", "is_paged", "amsgrad", "foreach", "fused"):
        a.pop(k, None)       # knobs of the 8-bit state / torch dispatch: no meaning for the fused fp32 step
    if a:
        raise NotImplementedError(f"unsupported optimizer init_args for {class_path}: {sorted(a)}")
    return out
