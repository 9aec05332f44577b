"""Device state of the fused optimizers over the flat LoRA buffers, one class per family: AdamWState (fp32 moments, torch.optim.AdamW's
file layout), ProdigyState (prodigyopt.Prodigy's), BlockwiseState (bitsandbytes' blockwise 8-bit), SgdState (torch.optim.SGD's),
AdafactorState (transformers.optimization.Adafactor's), CameState (came_pytorch.CAME's), LionState (lion_pytorch.Lion's), LionBlockwiseState (bitsandbytes'
Lion8bit), MuonState (torch.optim.Muon's), ScheduleFreeAdamWState (schedulefree.AdamWScheduleFree's), RAdamState / NAdamState /
AdamaxState (torch.optim.RAdam's / NAdam's / Adamax's), AdEMAMixState / AdEMAMixBlockwiseState (bitsandbytes' AdEMAMix / AdEMAMix8bit)
and ScaledAdamWState (Riemannian-preconditioned AdamW for LoRA pairs).
QwenLoraTrainStep and the torch.optim classes of qflux_amd.optim hold one of them and know only their common surface:
  cls(store, args)               zeroed state for the store's layout; re-created whenever cls.layout_key(store, args) changes
  LAYOUT_ARGS                    the optimizer_args that shape the buffers: broadcast_state agrees on them before the buffers
  cls.names(args) / buffers()    fixed, ordered (name, tensor) list that broadcast_state sends and check_replicas sums
  step(store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale, args)   the family's one step launch
  cls.save(state, entries, step, args) -> (extra param-group fields, per-parameter state); state may be None (no step yet)
  cls.load(store, sd, args) -> (state or None, highest per-parameter step the family reads, else 0)
  sync_host()                    after the buffers were received from another rank: host-side copies of device scalars follow them
  swap(store, beta1, train)      the parameter buffer between its train and eval form; a no-op for every family but the schedule-free
Parameter groups (torch.optim's second axis; LoRA+): `members` = one tuple of store-entry indices per group, in the group's parameter
order, each entry in exactly one group; None (or one group) is the single-group case and changes nothing.  The families with
GROUPED = True step several groups in their ONE launch (the *_grouped kernels of include/qfx.h): regroup() builds the one-byte map
from the layout to the group once per layout and grouping and keeps it with the state, step(..., groups=[row per group]) reads lr /
betas / eps / weight_decay (and the family's own fields) from each row.  Every other family refuses a second group.  The grouping is
part of layout_key; a change of the grouping alone rebuilds the map, not the moments (ensure_state)."""
from __future__ import annotations

import torch

from .. import ops
from .._lib import PRODIGY_STATE
from . import adam8bit as A8


def _out(t, off, k, shape=None):
    """CPU copy of one parameter's slice of a flat buffer (shaped like the parameter when given)."""
    t = t[off:off + k]
    return (t if shape is None else t.view(shape)).detach().cpu().clone()


class ParamGroupsNotImplemented(NotImplementedError, ValueError):
    """A second parameter group given to a family whose fused step has one.  Also a ValueError: that is what the constructors
    raised for any second group before the grouped kernels existed."""


def norm_members(members):
    """None for one group (the ungrouped kernels, today's keys and files), else a tuple of tuples of store-entry indices."""
    if members is None or len(members) <= 1:
        return None
    return tuple(tuple(int(i) for i in m) for m in members)


def _members_key(members):
    return () if members is None else (("groups", members),)


def members_assign(members, n_entries):
    """assign[i] = the group of store entry i; every entry must be in exactly one group."""
    assign = [None] * n_entries
    for k, m in enumerate(members):
        for i in m:
            if not 0 <= i < n_entries or assign[i] is not None:
                raise ValueError(f"parameter group {k}: store entry {i} is " + ("in more than one group" if 0 <= i < n_entries else "unknown"))
            assign[i] = k
    if None in assign:
        raise ValueError(f"store entry {assign.index(None)} is in no parameter group")
    return assign


def ensure_state(cls, state, store, args, members=None):
    """The state object for the store's current layout and the grouping: zeroed state when the layout changed (or there is none
    yet), the same moments with a rebuilt group map when only the grouping did."""
    if state is None or state.key != cls.layout_key(store, args, members):
        if state is None or state.base_key != cls.layout_key(store, args):
            state = cls(store, args)
        state.regroup(store, members)
    return state


class FlatState:
    LAYOUT_ARGS = ()
    DEFAULTS = {}               # the family's optimizer_args and their defaults; empty: the family takes none

    GROUPED = False             # the family's one launch reads per-group hyperparameters
    FAMILY = None               # how a refusal names the family

    def __init__(self, store, args):
        self.base_key = self.layout_key(store, args)
        self.members = self.group_map = None

    @property
    def key(self):
        return self.base_key + _members_key(self.members)

    def regroup(self, store, members):
        """Take the grouping `members` (None: one group): a refusal for a family without grouped kernels, else the one-byte map of
        the layout (build_group_map: range-checked on the host, uploaded once).  The moments stay as they are."""
        members = norm_members(members)
        if members is not None:
            self.check_groups(len(members))
            assign = members_assign(members, len(store.entries))
            self.group_map = self.build_group_map(store, assign, len(members))
        else:
            self.group_map = None
        self.members = members

    @classmethod
    def check_groups(cls, n_groups):
        if n_groups > 1 and not cls.GROUPED:
            raise ParamGroupsNotImplemented(f"{cls.FAMILY}: {n_groups} parameter groups -- the fused {cls.FAMILY} step runs over ONE group (its "
                                      "global estimates / per-matrix steps are defined per group in the original package; the grouped "
                                      "kernels cover AdamW / Adam, SGD, Lion, RAdam, NAdam, Adamax, AdEMAMix and the blockwise 8-bit families)")
        if n_groups > ops.MAX_PARAM_GROUPS:
            raise ValueError(f"{n_groups} parameter groups: the grouped kernels take at most {ops.MAX_PARAM_GROUPS}")

    def build_group_map(self, store, assign, n_groups):
        """fp32 families: the group of every 64-element tile of the flat buffers."""
        return ops.tile_group_map([(off, k) for _, _, off, k in store.entries], assign, n_groups, numel=store.pflat.numel(),
                                  device=store.pflat.device)

    @staticmethod
    def validate(args):
        pass

    @classmethod
    def check_rule_fields(cls, k, rule):
        """A param_groups rule of the train steps, before any store exists: a family refuses here the fields it cannot vary."""

    @classmethod
    def group_args(cls, sd, args):
        """The file's group; its fields named in DEFAULTS are copied into args, which are then validated."""
        g = sd["param_groups"][0]
        for n in cls.DEFAULTS:
            if n in g:
                args[n] = g[n]
        cls.validate(args)
        return g

    @staticmethod
    def file_entries(store, sd):
        """(i, p, off, k, e) for every entry of the store the file has per-parameter state e for."""
        for i, (_, p, off, k) in enumerate(store.entries):
            e = sd["state"].get(i)
            if e is not None:
                yield i, p, off, k, e

    @staticmethod
    def field(i, p, e, n, numel=None, shape=None):
        """e[n], which must exist and have `numel` elements or the shape `shape`."""
        if n not in e:
            raise ValueError(f"optimizer state of parameter {i} (shape {tuple(p.shape)}) has no {n!r}: {sorted(e)}")
        if numel is not None and e[n].numel() != numel:
            raise ValueError(f"optimizer state of parameter {i}: {n} has {e[n].numel()} elements, {numel} expected")
        if shape is not None and tuple(e[n].shape) != tuple(shape):
            raise ValueError(f"optimizer state of parameter {i}: {n} has shape {tuple(e[n].shape)}, {tuple(shape)} expected")
        return e[n]

    @classmethod
    def layout_key(cls, store, args, members=None):
        return cls._base_key(store, args) + _members_key(norm_members(members))

    @classmethod
    def _base_key(cls, store, args):
        return (tuple((off, k) for _, _, off, k in store.entries), str(store.pflat.device)) + tuple(int(args[n]) for n in cls.LAYOUT_ARGS)

    @classmethod
    def names(cls, args):
        """The buffer names of a state built with `args`: what a rank without state lists in their place."""
        return cls.NAMES

    def buffers(self):
        return [(n, getattr(self, n)) for n in self.NAMES]

    def sync_host(self):
        pass

    train_mode = True

    def swap(self, store, beta1, train):
        pass


class AdamWState(FlatState):
    """exp_avg / exp_avg_sq in fp32, indexed like pflat (also the "adam" / "adam8bit" aliases)."""
    NAMES = ("m", "v")
    GROUPED, FAMILY = True, "AdamW"

    def __init__(self, store, args):
        super().__init__(store, args)
        self.m = torch.zeros_like(store.pflat)
        self.v = torch.zeros_like(store.pflat)

    def step(self, store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale, args, groups=None):
        if groups is not None and len(groups) > 1:
            rows = [(r["lr"], r["betas"][0], r["betas"][1], r["eps"], r["weight_decay"]) for r in groups]
            return ops.adamw_step_grouped(store.pflat, store.gflat, self.m, self.v, self.group_map, rows, step, gnorm_sq=gnorm_sq,
                                          max_norm=max_norm, grad_scale=grad_scale)
        ops.adamw_step(store.pflat, store.gflat, self.m, self.v, lr, betas[0], betas[1], eps, weight_decay, step, gnorm_sq=gnorm_sq,
                       max_norm=max_norm, grad_scale=grad_scale)

    @classmethod
    def save(cls, state, entries, step, args):
        """torch.optim.AdamW's per-parameter {"step", "exp_avg", "exp_avg_sq"}."""
        if state is None:
            return {"amsgrad": False}, {}
        return {"amsgrad": False}, {i: {"step": torch.tensor(float(step)), "exp_avg": _out(state.m, off, k, p.shape),
                                        "exp_avg_sq": _out(state.v, off, k, p.shape)} for i, (_, p, off, k) in enumerate(entries)}

    @classmethod
    def load(cls, store, sd, args):
        state, step = cls(store, args), 0
        for i, p, off, k, e in cls.file_entries(store, sd):
            # a bitsandbytes-layout file (state1 / state2 / absmax / qmap) resumes with its moments dequantised
            ea, es = (e["exp_avg"], e["exp_avg_sq"]) if "exp_avg" in e else A8.bnb_moments(e)
            state.m[off:off + k].copy_(ea.reshape(-1).to(state.m.device))
            state.v[off:off + k].copy_(es.reshape(-1).to(state.v.device))
            step = max(step, int(float(e["step"])))
        return state, step


class ProdigyState(AdamWState):
    """AdamW's two moments plus s, p0 and the fp64 device scalars d, d_max, d_numerator, d_denom, d_hat, k (pstate)."""
    NAMES = ("m", "v", "ps", "p0", "pstate")
    GROUP = ("d", "d_max", "d_numerator", "d_denom", "d_hat", "k")
    GROUPED, FAMILY = False, "Prodigy"
    DEFAULTS = dict(beta3=None, decouple=True, use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0,
                    growth_rate=float("inf"))

    def __init__(self, store, args):
        super().__init__(store, args)
        self.ps = self.p0 = self.pstate = None     # created by the first step(), as prodigyopt does: p0 = the parameters at that call

    def _create(self, p0=None):
        self.ps = torch.zeros_like(self.m)
        self.p0 = torch.zeros_like(self.m) if p0 is None else p0.detach().clone()
        self.pstate = torch.zeros(PRODIGY_STATE, dtype=torch.float64, device=self.m.device)

    def buffers(self):
        if self.pstate is None:       # a state that is to receive rank src's buffers (broadcast_state)
            self._create()
        return super().buffers()

    def step(self, store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale, args):
        if self.pstate is None:
            self._create(store.pflat)
            ops.prodigy_init_state(self.pstate, args["d0"])
        ops.prodigy_step(store.pflat, store.gflat, self.m, self.v, self.ps, self.p0, self.pstate, lr=lr, betas=betas, eps=eps,
                         weight_decay=weight_decay, gnorm_sq=gnorm_sq, max_norm=max_norm, grad_scale=grad_scale, **args)

    @classmethod
    def save(cls, state, entries, step, args):
        """prodigyopt's layout: per parameter {"step", "s", "p0", "exp_avg", "exp_avg_sq"}; the group carries the init_args and
        d, d_max, d_numerator, d_denom, d_hat, k (d0 defaults before the first step)."""
        d0 = args["d0"]
        group = dict(args, d=d0, d_max=d0, d_numerator=0.0, d_denom=0.0, d_hat=d0, k=0)
        if state is None:
            return group, {}
        group.update(zip(cls.GROUP, state.pstate.cpu().tolist()))
        group["k"] = int(group["k"])
        return group, {i: {"step": group["k"], "s": _out(state.ps, off, k), "p0": _out(state.p0, off, k),
                           "exp_avg": _out(state.m, off, k, p.shape), "exp_avg_sq": _out(state.v, off, k, p.shape)}
                       for i, (_, p, off, k) in enumerate(entries)}

    @classmethod
    def load(cls, store, sd, args):
        """The step count is the group's k (QwenLoraTrainStep reads it), not the per-parameter one."""
        g = cls.group_args(sd, args)
        if not sd["state"]:
            return None, 0
        state = cls(store, args)
        state._create()
        for i, (_, p, off, k) in enumerate(store.entries):
            e = sd["state"][i]
            state.m[off:off + k].copy_(e["exp_avg"].reshape(-1)); state.v[off:off + k].copy_(e["exp_avg_sq"].reshape(-1))
            state.ps[off:off + k].copy_(e["s"].reshape(-1))
            if e["p0"].numel() == k:            # the package stores a 0-dim zero for an all-zero parameter
                state.p0[off:off + k].copy_(e["p0"].reshape(-1))
        state.pstate.copy_(torch.tensor([float(g[n]) for n in cls.GROUP] + [0.0] * (PRODIGY_STATE - len(cls.GROUP)), dtype=torch.float64))
        return state, 0


class _BlockwiseBase(FlatState):
    """bitsandbytes' blockwise 8-bit state of MOMENTS moments (adam8bit.py): per moment j the codes qj indexed like pflat, absmaxj per
    8-bit block and the code book qmapj (signed for the first moment), an fp32 moment (m32, v32) for the tensors below min_8bit_size,
    and the block table of the layout.  In a file the moments are state1 / state2."""
    LAYOUT_ARGS = ("blocksize", "min_8bit_size")
    DEFAULTS = dict(min_8bit_size=4096, blocksize=256)
    MOMENTS = 0
    F32 = ("m32", "v32")
    GROUPED = True

    @staticmethod
    def validate(args, optimizer="blockwise 8-bit state"):
        if args["blocksize"] not in A8.BLOCKSIZES or int(args["min_8bit_size"]) < 1:
            raise ValueError(f"{optimizer}: blocksize must be one of {A8.BLOCKSIZES} and min_8bit_size >= 1 ({args})")
        args["min_8bit_size"] = int(args["min_8bit_size"])

    def __init_subclass__(cls):
        r = range(1, cls.MOMENTS + 1)
        cls.F32 = _BlockwiseBase.F32[:cls.MOMENTS]
        cls.NAMES = tuple([f"q{j}" for j in r] + [f"absmax{j}" for j in r] + list(cls.F32) + [f"qmap{j}" for j in r])

    def __init__(self, store, args):
        super().__init__(store, args)
        dev = store.pflat.device
        self.layout = ops.adam8bit_block_table([(off, k) for _, _, off, k in store.entries], args["blocksize"], args["min_8bit_size"],
                                               device=dev)
        for j, f32 in enumerate(self.F32, 1):
            setattr(self, f"q{j}", torch.zeros(store.pflat.numel(), dtype=torch.uint8, device=dev))     # bnb's initial state: codes 0,
            setattr(self, f"absmax{j}", torch.zeros(max(1, self.layout.n_absmax), dtype=torch.float32, device=dev))     # absmax 0 (decodes to 0)
            setattr(self, f32, torch.zeros(max(1, self.layout.n_fp32), dtype=torch.float32, device=dev))
            setattr(self, f"qmap{j}", A8.dynamic_map(j == 1).to(dev))

    def build_group_map(self, store, assign, n_groups):
        """The group of every block-table entry (an entry never leaves its tensor)."""
        return ops.block_group_map(self.layout, assign, n_groups, device=store.pflat.device)

    def param_state(self, i, shape, step):
        """bnb's per-parameter state of entry i (CPU tensors)."""
        off, k, eight, a0, nb, s0 = self.layout.tensors[i]
        r = range(1, self.MOMENTS + 1)
        if not eight:
            return dict({"step": step}, **{f"state{j}": _out(getattr(self, self.F32[j - 1]), s0, k, shape) for j in r})
        e = dict({"step": step}, **{f"state{j}": _out(getattr(self, f"q{j}"), off, k, shape) for j in r})
        e.update({f"qmap{j}": getattr(self, f"qmap{j}").cpu().clone() for j in r})
        e.update({f"absmax{j}": _out(getattr(self, f"absmax{j}"), a0, nb) for j in r})
        return e

    def load_param_state(self, i, e):
        off, k, eight, a0, nb, s0 = self.layout.tensors[i]
        if (e["state1"].dtype == torch.uint8) != eight:
            raise ValueError(f"optimizer state of parameter {i} ({k} elements) is {'8-bit' if not eight else 'fp32'} in the file: it was "
                             f"saved with another min_8bit_size than {self.layout.min_8bit_size}")
        r = range(1, self.MOMENTS + 1)
        if not eight:
            for j in r:
                getattr(self, self.F32[j - 1])[s0:s0 + k].copy_(e[f"state{j}"].reshape(-1))
            return
        if any(e[f"absmax{j}"].numel() != nb for j in r):
            raise ValueError(f"optimizer state of parameter {i}: {e['absmax1'].numel()} absmax blocks, {nb} expected")
        for j in r:
            getattr(self, f"q{j}")[off:off + k].copy_(e[f"state{j}"].reshape(-1))
            getattr(self, f"absmax{j}")[a0:a0 + nb].copy_(e[f"absmax{j}"].reshape(-1))

    @classmethod
    def save(cls, state, entries, step, args):
        """bnb's Optimizer2State / Optimizer1State layout: per parameter {"step", "stateJ", "qmapJ", "absmaxJ"} (8-bit) or {"step",
        "stateJ"} (fp32 moments, numel < min_8bit_size); no group fields of its own."""
        if state is None or step == 0:
            return {}, {}
        return {}, {i: state.param_state(i, p.shape, step) for i, (_, p, _, _) in enumerate(entries)}

    @classmethod
    def load(cls, store, sd, args):
        """The block size is inferred from the file's absmax sizes, the code books are the file's."""
        bs, *qmaps = A8.file_layout(sd["state"], store.entries)
        if bs is not None:
            args["blocksize"] = bs
        state, step = cls(store, args), 0
        if qmaps[0] is not None:
            for j in range(1, cls.MOMENTS + 1):
                getattr(state, f"qmap{j}").copy_(qmaps[j - 1])
        for i, p, off, k, e in cls.file_entries(store, sd):
            state.load_param_state(i, e)
            step = max(step, int(float(e["step"])))
        return state, step


class BlockwiseState(_BlockwiseBase):
    """bitsandbytes' blockwise 8-bit Adam / AdamW: two moments (q1, q2, absmax1, absmax2, m32, v32, qmap1, qmap2)."""
    MOMENTS = 2
    FAMILY = "Adam8bit"

    def step(self, store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale, args, groups=None):
        if groups is not None and len(groups) > 1:
            rows = [(r["lr"], r["betas"][0], r["betas"][1], r["eps"], r["weight_decay"]) for r in groups]
            return ops.adam8bit_step_grouped(store.pflat, store.gflat, self.q1, self.q2, self.absmax1, self.absmax2, self.m32, self.v32,
                                             self.layout, self.qmap1, self.qmap2, self.group_map, rows, step, gnorm_sq=gnorm_sq,
                                             max_norm=max_norm, grad_scale=grad_scale)
        ops.adam8bit_step(store.pflat, store.gflat, self.q1, self.q2, self.absmax1, self.absmax2, self.m32, self.v32, self.layout,
                          self.qmap1, self.qmap2, lr, betas, eps, weight_decay, step, gnorm_sq=gnorm_sq, max_norm=max_norm,
                          grad_scale=grad_scale)


class SgdState(FlatState):
    """torch.optim.SGD: one momentum buffer indexed like pflat, only when momentum != 0.  `first` marks the step that creates the
    buffer (torch: buf = the decayed gradient, no dampening); a state that was loaded or received from another rank has stepped."""
    NAMES = ("buf",)
    DEFAULTS = dict(momentum=0.0, dampening=0.0, nesterov=False)
    GROUPED, FAMILY = True, "SGD"

    def __init__(self, store, args):
        super().__init__(store, args)
        self.buf = torch.zeros_like(store.pflat) if args["momentum"] != 0 else None
        self.first = True

    @classmethod
    def _base_key(cls, store, args):
        return super()._base_key(store, args) + (args["momentum"] != 0,)

    @classmethod
    def names(cls, args):
        return cls.NAMES if args["momentum"] != 0 else ()

    @staticmethod
    def validate(args):
        """torch.optim.SGD's constructor checks."""
        if args["momentum"] < 0.0:
            raise ValueError(f"Invalid momentum value: {args['momentum']}")
        if args["nesterov"] and (args["momentum"] <= 0 or args["dampening"] != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")

    def buffers(self):
        self.first = False            # listed for a broadcast or a replica check: the state of a run that has stepped
        return [("buf", self.buf)] if self.buf is not None else []

    def step(self, store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale, args, groups=None):
        if groups is not None and len(groups) > 1:
            rows = [(r["lr"], r.get("momentum", args["momentum"]), r.get("dampening", args["dampening"]), r["weight_decay"],
                     r.get("nesterov", args["nesterov"])) for r in groups]
            if self.buf is None and any(r[1] != 0 for r in rows):      # the state was shaped by a group without momentum
                self.buf = torch.zeros_like(store.pflat)
            ops.sgd_step_grouped(store.pflat, store.gflat, self.buf, self.group_map, rows, first=self.first, gnorm_sq=gnorm_sq,
                                 max_norm=max_norm, grad_scale=grad_scale)
        else:
            ops.sgd_step(store.pflat, store.gflat, self.buf, lr, args["momentum"], args["dampening"], weight_decay, args["nesterov"],
                         first=self.first, gnorm_sq=gnorm_sq, max_norm=max_norm, grad_scale=grad_scale)
        self.first = False

    @classmethod
    def save(cls, state, entries, step, args):
        """torch.optim.SGD's layout: per parameter {"momentum_buffer"} (no state without momentum or before the first step); the
        group carries momentum, dampening, nesterov, maximize."""
        group = dict(momentum=args["momentum"], dampening=args["dampening"], nesterov=args["nesterov"], maximize=False)
        if state is None or state.buf is None or state.first:
            return group, {}
        return group, {i: {"momentum_buffer": _out(state.buf, off, k, p.shape)} for i, (_, p, off, k) in enumerate(entries)}

    @classmethod
    def load(cls, store, sd, args):
        if sd["param_groups"][0].get("maximize", False):
            raise NotImplementedError("SGD with maximize=True")
        cls.group_args(sd, args)
        if not sd["state"] or args["momentum"] == 0:
            return None, 0
        state = cls(store, args)
        for i, p, off, k, e in cls.file_entries(store, sd):
            if e.get("momentum_buffer") is not None:
                state.buf[off:off + k].copy_(e["momentum_buffer"].reshape(-1))
        state.first = False
        return state, 0


class AdafactorState(FlatState):
    """transformers.optimization.Adafactor: factored second moments of every adapter matrix (one vector per row, one per column,
    packed in entry order), an elementwise one for tensors with fewer than two dimensions, the RMS of every tensor as of its last
    step, and exp_avg indexed like pflat when beta1 is given.  Zeros are the package's initial state.  `eps` is the package's pair
    (added to the squared gradient, floor of the parameter scale) and lives in the optimizer_args: the train step's own eps is unused."""
    NAMES = ("row", "col", "v", "rms", "m")
    FAMILY = "Adafactor"
    DEFAULTS = dict(eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, scale_parameter=True, relative_step=True,
                    warmup_init=False)

    def __init__(self, store, args):
        super().__init__(store, args)
        dev = store.pflat.device
        self.layout = ops.adafactor_table([(off, p.shape) for _, p, off, _ in store.entries], device=dev)
        z = lambda n: torch.zeros(max(1, n), dtype=torch.float32, device=dev)
        self.row, self.col, self.v, self.rms = z(self.layout.n_row), z(self.layout.n_col), z(self.layout.n_v), z(self.layout.n_tensors)
        self.m = torch.zeros_like(store.pflat) if args["beta1"] is not None else None

    @classmethod
    def _base_key(cls, store, args):
        return super()._base_key(store, args) + (tuple(tuple(p.shape) for _, p, _, _ in store.entries), args["beta1"] is not None)

    @classmethod
    def names(cls, args):
        return cls.NAMES if args["beta1"] is not None else cls.NAMES[:-1]

    @staticmethod
    def validate(args, lr=False):
        """The package's constructor checks; lr=False: the learning rate is not known here."""
        if args["warmup_init"] and not args["relative_step"]:
            raise ValueError("`warmup_init=True` requires `relative_step=True`")
        if lr is not False and lr is not None and args["relative_step"]:
            raise ValueError("Cannot combine manual `lr` and `relative_step=True` options")
        if lr is None and not args["relative_step"]:
            raise ValueError("Adafactor with relative_step=False needs a learning rate (lr=None)")
        eps = args["eps"]
        if not isinstance(eps, (tuple, list)) or len(eps) != 2:
            raise ValueError(f"Adafactor's eps is a pair (eps1, eps2), not {eps!r}")
        args["eps"] = (float(eps[0]), float(eps[1]))
        if not args["clip_threshold"] > 0:
            raise ValueError(f"Invalid clip_threshold value: {args['clip_threshold']}")
        if args["beta1"] is not None and not 0.0 <= args["beta1"] < 1.0:
            raise ValueError(f"Invalid beta1 value: {args['beta1']}")

    def buffers(self):
        return [(n, getattr(self, n)) for n in self.NAMES if getattr(self, n) is not None]

    def step(self, store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale, args):
        self.validate(args, lr)
        ops.adafactor_step(store.pflat, store.gflat, self.row, self.col, self.v, self.m, self.rms, self.layout, step, lr=lr,
                           weight_decay=weight_decay, gnorm_sq=gnorm_sq, max_norm=max_norm, grad_scale=grad_scale, **args)

    @classmethod
    def save(cls, state, entries, step, args):
        """transformers' layout: per parameter {"step", "RMS", "exp_avg_sq_row" [rows], "exp_avg_sq_col" [cols]} (two or more
        dimensions) or {"step", "RMS", "exp_avg_sq"} (fewer), plus "exp_avg" with beta1; the group carries the package's options."""
        group = {n: args[n] for n in cls.DEFAULTS}
        if state is None or step == 0:
            return group, {}
        per = {}
        for i, (_, p, off, k) in enumerate(entries):
            _, rows, cols, factored, r0, c0, v0 = state.layout.tensors[i]
            e = {"step": step, "RMS": state.rms[i].detach().cpu().clone()}
            if factored:
                e["exp_avg_sq_row"], e["exp_avg_sq_col"] = _out(state.row, r0, rows), _out(state.col, c0, cols)
            else:
                e["exp_avg_sq"] = _out(state.v, v0, k, p.shape)
            if state.m is not None:
                e["exp_avg"] = _out(state.m, off, k, p.shape)
            per[i] = e
        return group, per

    @classmethod
    def load(cls, store, sd, args):
        """Every statistic must have the shape the parameter implies; a file written without beta1 cannot resume a run with it."""
        cls.group_args(sd, args)
        if not sd["state"]:
            return None, 0
        state, step, rms = cls(store, args), 0, [0.0] * len(store.entries)
        for i, p, off, k, e in cls.file_entries(store, sd):
            _, rows, cols, factored, r0, c0, v0 = state.layout.tensors[i]
            want = {"exp_avg_sq_row": (rows,), "exp_avg_sq_col": (cols,)} if factored else {"exp_avg_sq": tuple(p.shape)}
            if state.m is not None:
                want["exp_avg"] = tuple(p.shape)
            for n, shape in want.items():
                cls.field(i, p, e, n, shape=shape)
            if factored:
                state.row[r0:r0 + rows].copy_(e["exp_avg_sq_row"]); state.col[c0:c0 + cols].copy_(e["exp_avg_sq_col"])
            else:
                state.v[v0:v0 + k].copy_(e["exp_avg_sq"].reshape(-1))
            if state.m is not None:
                state.m[off:off + k].copy_(e["exp_avg"].reshape(-1))
            rms[i] = float(e.get("RMS", 0.0))
            step = max(step, int(float(e["step"])))
        state.rms.copy_(torch.tensor(rms, dtype=torch.float32))
        return state, step


class CameState(FlatState):
    """came_pytorch.CAME: Adafactor's factored second moments of every adapter matrix (row, col), a second factored pair over the
    instability (rrow, rcol: exp_avg_res_row / exp_avg_res_col), an elementwise second moment (v) for 1-D tensors, the RMS of every
    tensor as of its last step (kept as the package keeps it; the update does not read it), and exp_avg (m) indexed like pflat.
    Zeros are the package's initial state.  `eps` is the package's pair (added to the squared gradient, to the instability) and
    lives in the optimizer_args: the train step's own eps is unused.  `betas` is the package's TRIPLE and travels where the other
    families' pair does (the train steps' betas=, the group's "betas"): default_betas("came")."""
    NAMES = ("row", "col", "rrow", "rcol", "v", "rms", "m")
    FAMILY = "CAME"
    DEFAULTS = dict(eps=(1e-30, 1e-16), clip_threshold=1.0)
    BETAS = (0.9, 0.999, 0.9999)
    # per-parameter keys of came_pytorch's state_dict, restated from the published source (came_pytorch/CAME.py, step()); NOT checked
    # against an installed package
    FACTORED_KEYS = ("step", "RMS", "exp_avg", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_res_row", "exp_avg_res_col")
    UNFACTORED_KEYS = ("step", "RMS", "exp_avg", "exp_avg_sq")

    def __init__(self, store, args):
        super().__init__(store, args)
        dev = store.pflat.device
        self.layout = ops.came_table([(off, p.shape) for _, p, off, _ in store.entries], device=dev)
        z = lambda n: torch.zeros(max(1, n), dtype=torch.float32, device=dev)
        self.row, self.col, self.rrow, self.rcol = z(self.layout.n_row), z(self.layout.n_col), z(self.layout.n_row), z(self.layout.n_col)
        self.v, self.rms = z(self.layout.n_v), z(self.layout.n_tensors)
        self.m = torch.zeros_like(store.pflat)

    @classmethod
    def _base_key(cls, store, args):
        return super()._base_key(store, args) + (tuple(tuple(p.shape) for _, p, _, _ in store.entries),)

    @staticmethod
    def validate(args, lr=False, betas=None):
        """The package's constructor checks; lr=False / betas=None: not known here."""
        eps = args["eps"]
        if not isinstance(eps, (tuple, list)) or len(eps) != 2:
            raise ValueError(f"CAME's eps is a pair (eps1, eps2), not {eps!r}")
        args["eps"] = (float(eps[0]), float(eps[1]))
        if not args["clip_threshold"] > 0:
            raise ValueError(f"Invalid clip_threshold value: {args['clip_threshold']}")
        if args["eps"][0] < 0 or args["eps"][1] < 0:
            raise ValueError(f"Invalid eps value: {args['eps']}")
        if lr is not False and (lr is None or not float(lr) > 0.0):        # the constructor's rule; a schedule may pass through 0 later
            raise ValueError(f"CAME needs a learning rate > 0, not {lr!r}")
        if betas is not None:
            ops.came_check(1.0, betas, args["eps"], args["clip_threshold"])

    def step(self, store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale, args):
        self.validate(args, betas=betas)
        ops.came_step(store.pflat, store.gflat, self.row, self.col, self.rrow, self.rcol, self.v, self.m, self.rms, self.layout, lr,
                      betas=betas, eps=args["eps"], clip_threshold=args["clip_threshold"], weight_decay=weight_decay, gnorm_sq=gnorm_sq,
                      max_norm=max_norm, grad_scale=grad_scale)

    @classmethod
    def save(cls, state, entries, step, args):
        """came_pytorch's layout: per parameter FACTORED_KEYS (two dimensions: exp_avg_sq_row / exp_avg_res_row [rows], exp_avg_sq_col
        / exp_avg_res_col [cols]) or UNFACTORED_KEYS (one); the group carries eps (the pair) and clip_threshold next to lr, betas (the
        triple) and weight_decay."""
        group = {n: args[n] for n in cls.DEFAULTS}
        if state is None or step == 0:
            return group, {}
        per = {}
        for i, (_, p, off, k) in enumerate(entries):
            _, rows, cols, factored, r0, c0, v0 = state.layout.tensors[i]
            e = {"step": step, "RMS": state.rms[i].detach().cpu().clone(), "exp_avg": _out(state.m, off, k, p.shape)}
            if factored:
                e["exp_avg_sq_row"], e["exp_avg_sq_col"] = _out(state.row, r0, rows), _out(state.col, c0, cols)
                e["exp_avg_res_row"], e["exp_avg_res_col"] = _out(state.rrow, r0, rows), _out(state.rcol, c0, cols)
            else:
                e["exp_avg_sq"] = _out(state.v, v0, k, p.shape)
            per[i] = e
        return group, per

    @classmethod
    def load(cls, store, sd, args):
        """Every statistic must have the shape the parameter implies."""
        cls.group_args(sd, args)
        if not sd["state"]:
            return None, 0
        state, step, rms = cls(store, args), 0, [0.0] * len(store.entries)
        for i, p, off, k, e in cls.file_entries(store, sd):
            _, rows, cols, factored, r0, c0, v0 = state.layout.tensors[i]
            want = {"exp_avg": tuple(p.shape)}
            if factored:
                want.update(exp_avg_sq_row=(rows,), exp_avg_sq_col=(cols,), exp_avg_res_row=(rows,), exp_avg_res_col=(cols,))
            else:
                want["exp_avg_sq"] = tuple(p.shape)
            for n, shape in want.items():
                cls.field(i, p, e, n, shape=shape)
            state.m[off:off + k].copy_(e["exp_avg"].reshape(-1))
            if factored:
                state.row[r0:r0 + rows].copy_(e["exp_avg_sq_row"]); state.col[c0:c0 + cols].copy_(e["exp_avg_sq_col"])
                state.rrow[r0:r0 + rows].copy_(e["exp_avg_res_row"]); state.rcol[c0:c0 + cols].copy_(e["exp_avg_res_col"])
            else:
                state.v[v0:v0 + k].copy_(e["exp_avg_sq"].reshape(-1))
            rms[i] = float(e.get("RMS", 0.0))
            step = max(step, int(float(e["step"])))
        state.rms.copy_(torch.tensor(rms, dtype=torch.float32))
        return state, step


class LionState(FlatState):
    """lion_pytorch.Lion / bitsandbytes.optim.Lion: the one moment exp_avg in fp32, indexed like pflat.  eps is unused."""
    NAMES = ("exp_avg",)
    GROUPED, FAMILY = True, "Lion"

    def __init__(self, store, args):
        super().__init__(store, args)
        self.exp_avg = torch.zeros_like(store.pflat)

    def step(self, store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale, args, groups=None):
        if groups is not None and len(groups) > 1:
            rows = [(r["lr"], r["betas"][0], r["betas"][1], r["weight_decay"]) for r in groups]
            return ops.lion_step_grouped(store.pflat, store.gflat, self.exp_avg, self.group_map, rows, gnorm_sq=gnorm_sq,
                                         max_norm=max_norm, grad_scale=grad_scale)
        ops.lion_step(store.pflat, store.gflat, self.exp_avg, lr, betas[0], betas[1], weight_decay, gnorm_sq=gnorm_sq, max_norm=max_norm,
                      grad_scale=grad_scale)

    @classmethod
    def save(cls, state, entries, step, args):
        """lion_pytorch's layout: per parameter {"exp_avg"} (no step count: it does not enter the arithmetic); lr, betas and
        weight_decay in the group.  A state exists from the first step or a loaded file on (a lion_pytorch file counts no steps)."""
        if state is None:
            return {}, {}
        return {}, {i: {"exp_avg": _out(state.exp_avg, off, k, p.shape)} for i, (_, p, off, k) in enumerate(entries)}

    @classmethod
    def load(cls, store, sd, args):
        """Either lion_pytorch's {"exp_avg"} or a bitsandbytes Lion file's {"step", "state1"} (fp32 as it is, 8-bit codes dequantised)."""
        if not sd["state"]:
            return None, 0
        state, step = cls(store, args), 0
        for i, p, off, k, e in cls.file_entries(store, sd):
            ea = e["exp_avg"] if "exp_avg" in e else A8.bnb_moment1(e)
            if ea.numel() != k:
                raise ValueError(f"optimizer state of parameter {i}: {ea.numel()} elements, {k} expected")
            state.exp_avg[off:off + k].copy_(ea.reshape(-1).float())
            step = max(step, int(float(e.get("step", 0))))
        return state, step


class LionBlockwiseState(_BlockwiseBase):
    """bitsandbytes.optim.Lion8bit / PagedLion8bit: ONE moment (q1, absmax1, m32, qmap1) over the same block table."""
    MOMENTS = 1
    FAMILY = "Lion8bit"

    def step(self, store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale, args, groups=None):
        if groups is not None and len(groups) > 1:
            rows = [(r["lr"], r["betas"][0], r["betas"][1], r["weight_decay"]) for r in groups]
            return ops.lion8bit_step_grouped(store.pflat, store.gflat, self.q1, self.absmax1, self.m32, self.layout, self.qmap1,
                                             self.group_map, rows, gnorm_sq=gnorm_sq, max_norm=max_norm, grad_scale=grad_scale)
        ops.lion8bit_step(store.pflat, store.gflat, self.q1, self.absmax1, self.m32, self.layout, self.qmap1, lr, betas, weight_decay,
                          gnorm_sq=gnorm_sq, max_norm=max_norm, grad_scale=grad_scale)


class MuonState(FlatState):
    """torch.optim.Muon: one fp32 momentum buffer indexed like pflat (zeros are the class's initial state), the per-matrix descriptor
    table of the layout (adjust_lr_fn shapes it: the lr ratio of every matrix is an entry) and the bf16 workspace the table asks for.
    `eps` is Muon's own (the floor of the Frobenius norm, 1e-7) and lives in the optimizer_args: the train step's Adam eps is unused,
    and so are betas.  `first` marks a state that has not stepped (torch keeps no state before the first step)."""
    NAMES = ("buf",)
    FAMILY = "Muon"
    DEFAULTS = dict(momentum=0.95, nesterov=True, ns_coefficients=(3.4445, -4.7750, 2.0315), eps=1e-7, ns_steps=5, adjust_lr_fn=None)

    def __init__(self, store, args):
        super().__init__(store, args)
        dev = store.pflat.device
        self.layout = ops.muon_table([(off, p.shape) for _, p, off, _ in store.entries], args["adjust_lr_fn"], device=dev)
        self.buf = torch.zeros_like(store.pflat)
        self.ws = torch.empty(self.layout.ws_bytes // 2, dtype=torch.bfloat16, device=dev) if self.layout.ws_bytes else None
        self.first = True

    @classmethod
    def _base_key(cls, store, args):
        return super()._base_key(store, args) + (tuple(tuple(p.shape) for _, p, _, _ in store.entries), args["adjust_lr_fn"])

    @staticmethod
    def validate(args):
        """torch.optim.Muon's constructor and Newton-Schulz checks, with its messages."""
        if not 0.0 <= args["momentum"]:
            raise ValueError(f"momentum should be >= 0 but is: {args['momentum']}")
        if args["adjust_lr_fn"] not in ops.MUON_ADJUST_LR:
            raise ValueError(f"Adjust learning rate function {args['adjust_lr_fn']} is not supported")
        if args["ns_steps"] >= 100:
            raise ValueError("Number of steps must be less than 100 for computational efficiency")
        if int(args["ns_steps"]) != args["ns_steps"] or args["ns_steps"] < 0:
            raise ValueError(f"Invalid ns_steps value: {args['ns_steps']}")
        if len(args["ns_coefficients"]) != 3:
            raise ValueError("Coefficients must be a tuple of exactly 3 values")
        if not float(args["eps"]) > 0.0:
            raise ValueError(f"Invalid eps value: {args['eps']}")
        args.update(ns_coefficients=tuple(float(c) for c in args["ns_coefficients"]), eps=float(args["eps"]), ns_steps=int(args["ns_steps"]),
                    nesterov=bool(args["nesterov"]), momentum=float(args["momentum"]))

    def buffers(self):
        self.first = False            # listed for a broadcast or a replica check: the state of a run that has stepped
        return [("buf", self.buf)]

    def step(self, store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale, args):
        self.validate(args)
        ops.muon_step(store.pflat, store.gflat, self.buf, self.ws, self.layout, lr, weight_decay, args["momentum"], args["nesterov"],
                      args["ns_coefficients"], args["eps"], args["ns_steps"], gnorm_sq=gnorm_sq, max_norm=max_norm, grad_scale=grad_scale)
        self.first = False

    @classmethod
    def save(cls, state, entries, step, args):
        """torch.optim.Muon's layout: per parameter {"momentum_buffer"} (no state before the first step); the group carries momentum,
        nesterov, ns_coefficients, eps, ns_steps, adjust_lr_fn next to lr and weight_decay."""
        group = {n: args[n] for n in cls.DEFAULTS}
        if state is None or state.first:
            return group, {}
        return group, {i: {"momentum_buffer": _out(state.buf, off, k, p.shape)} for i, (_, p, off, k) in enumerate(entries)}

    @classmethod
    def load(cls, store, sd, args):
        """torch keeps no step count: the train steps' own global_step carries it (0 for a file torch.optim.Muon wrote)."""
        cls.group_args(sd, args)
        if not sd["state"]:
            return None, 0
        state = cls(store, args)
        for i, p, off, k, e in cls.file_entries(store, sd):
            mb = e["momentum_buffer"]
            if tuple(mb.shape) != tuple(p.shape):
                raise ValueError(f"optimizer state of parameter {i}: momentum_buffer has shape {tuple(mb.shape)}, {tuple(p.shape)} expected")
            state.buf[off:off + k].copy_(mb.reshape(-1).float())
        state.first = False
        return state, 0


class ScheduleFreeAdamWState(FlatState):
    """schedulefree.AdamWScheduleFree: the base sequence z and exp_avg_sq (v) in fp32, indexed like pflat.  The parameter buffer
    itself holds y (train mode: where the gradient is taken) or the averaged x (eval mode: what is sampled from and saved); swap()
    moves it between the two.  The group's running scalars k, weight_sum, lr_max, train_mode and scheduled_lr are host values, as in
    the package (no step reads them back from the device); `sched` is their fp64 device image, written by buffers() for a broadcast
    or a replica check and read back by sync_host() on the ranks that received it.  k == 0 marks a state that has not stepped: its
    first step takes z = y and v = 0 in the kernel (the package creates both there), and a swap before it moves nothing."""
    NAMES = ("z", "v", "sched")
    FAMILY = "AdamWScheduleFree"
    DEFAULTS = dict(warmup_steps=0, r=0.0, weight_lr_power=2.0)
    SCHED = ("k", "weight_sum", "lr_max", "train_mode", "scheduled_lr")
    EVAL_STEP = ("optimizer step in eval mode: the parameters hold the averaged point x, not the point y the gradient belongs to; "
                 "call train() first")

    def __init__(self, store, args):
        super().__init__(store, args)
        self.z = torch.zeros_like(store.pflat)
        self.v = torch.zeros_like(store.pflat)
        self.sched = None
        self.k, self.weight_sum, self.lr_max, self.train_mode, self.scheduled_lr = 0, 0.0, -1.0, True, 0.0

    @staticmethod
    def validate(args):
        if int(args["warmup_steps"]) != args["warmup_steps"] or args["warmup_steps"] < 0:
            raise ValueError(f"Invalid warmup_steps value: {args['warmup_steps']}")
        args.update(warmup_steps=int(args["warmup_steps"]), r=float(args["r"]), weight_lr_power=float(args["weight_lr_power"]))

    def buffers(self):
        self.sched = torch.tensor([float(getattr(self, n)) for n in self.SCHED], dtype=torch.float64, device=self.z.device)
        return super().buffers()

    def sync_host(self):
        k, self.weight_sum, self.lr_max, tm, self.scheduled_lr = self.sched.cpu().tolist()
        self.k, self.train_mode = int(k), bool(tm)

    def swap(self, store, beta1, train):
        """y -> x (train=False) or x -> y (train=True) in place; nothing happens in the mode asked for."""
        if self.train_mode == bool(train):
            return
        if self.k > 0:
            ops.sf_swap(store.pflat, self.z, beta1, to_eval=not train)
        self.train_mode = bool(train)

    def step(self, store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale, args):
        if not self.train_mode:
            raise RuntimeError(self.EVAL_STEP)
        lr_t, bc2, ckp1, self.lr_max, self.weight_sum = ops.sfadamw_schedule(self.k, lr, betas[1], args["warmup_steps"], args["r"],
                                                                             args["weight_lr_power"], self.lr_max, self.weight_sum)
        self.scheduled_lr = lr_t
        ops.sfadamw_step(store.pflat, store.gflat, self.z, self.v, lr_t, betas[0], betas[1], eps, weight_decay, bc2, ckp1,
                         first=self.k == 0, gnorm_sq=gnorm_sq, max_norm=max_norm, grad_scale=grad_scale)
        self.k += 1

    @classmethod
    def save(cls, state, entries, step, args):
        """The package's layout: per parameter {"z", "exp_avg_sq"} (no state before the first step); the group carries warmup_steps, r,
        weight_lr_power, k, train_mode, weight_sum, lr_max, scheduled_lr and foreach next to lr, betas, eps and weight_decay."""
        group = dict(args, k=0, train_mode=True, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0, foreach=True)
        if state is None:
            return group, {}
        group.update({n: getattr(state, n) for n in cls.SCHED})
        if state.k == 0:
            return group, {}
        return group, {i: {"z": _out(state.z, off, k, p.shape), "exp_avg_sq": _out(state.v, off, k, p.shape)}
                       for i, (_, p, off, k) in enumerate(entries)}

    @classmethod
    def load(cls, store, sd, args):
        """The step count is the group's k (as Prodigy's).  A file without per-parameter state has not stepped: no state object, and
        its train_mode says nothing about the values (a swap before the first step moves none)."""
        g = cls.group_args(sd, args)
        if not sd["state"]:
            return None, 0
        state = cls(store, args)
        for i, p, off, k, e in cls.file_entries(store, sd):
            for n, buf in (("z", state.z), ("exp_avg_sq", state.v)):
                buf[off:off + k].copy_(cls.field(i, p, e, n, numel=k).reshape(-1).float())
        state.k, state.weight_sum, state.lr_max = int(g["k"]), float(g["weight_sum"]), float(g["lr_max"])
        state.train_mode, state.scheduled_lr = bool(g.get("train_mode", True)), float(g.get("scheduled_lr", 0.0))
        if state.k <= 0:
            raise ValueError(f"optimizer state with per-parameter z but a step count k = {g['k']}")
        return state, 0


class _AdamXState(AdamWState):
    """What torch.optim.RAdam, NAdam and Adamax share: exp_avg (m) and a second fp32 state (v: exp_avg_sq, Adamax's exp_inf) indexed
    like pflat, stepped by the ONE launch of qfx_adamx_step -- always the grouped entry, one row with one group.  A group's row is
    lr / betas / eps / weight_decay plus the class's own fields (DEFAULTS), read from the row where it carries them (the torch.optim
    classes' param_groups) and from the optimizer_args otherwise.  The per-step Python floats of torch's single-tensor functions
    are formed on the host (ops.adamx_rows); no step synchronises."""
    VARIANT = None
    SECOND = "exp_avg_sq"       # the file's name of v
    GROUPED = True
    REFUSED = ("maximize", "capturable", "differentiable")

    @staticmethod
    def validate(args):
        if "momentum_decay" in args:
            if not 0.0 <= args["momentum_decay"]:
                raise ValueError(f"Invalid momentum_decay value: {args['momentum_decay']}")
            args["momentum_decay"] = float(args["momentum_decay"])
        if "decoupled_weight_decay" in args:
            args["decoupled_weight_decay"] = bool(args["decoupled_weight_decay"])

    def _group_rows(self, lr, betas, eps, weight_decay, args, groups):
        rows = groups if groups is not None and len(groups) > 1 else [dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)]
        return [dict({n: args[n] for n in self.DEFAULTS}, **r) for r in rows]

    def step(self, store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale, args, groups=None):
        rows = self._group_rows(lr, betas, eps, weight_decay, args, groups)
        ops.adamx_step(self.VARIANT, store.pflat, store.gflat, self.m, self.v, rows, step, tile_group=self.group_map if len(rows) > 1 else None,
                       mu_products=getattr(self, "mu", None), gnorm_sq=gnorm_sq, max_norm=max_norm, grad_scale=grad_scale)

    @classmethod
    def _group_fields(cls, args):
        """The class's own fields of a torch param_group (its constructor's defaults for what the fused step does not implement)."""
        return dict({n: args[n] for n in cls.DEFAULTS}, maximize=False, foreach=None, capturable=False, differentiable=False)

    def _param_state(self, i, p, off, k, step):
        return {"step": torch.tensor(float(step)), "exp_avg": _out(self.m, off, k, p.shape), self.SECOND: _out(self.v, off, k, p.shape)}

    @classmethod
    def save(cls, state, entries, step, args):
        """torch's per-parameter {"step", "exp_avg", "exp_avg_sq" | "exp_inf"} (NAdam: and "mu_product"), step a 0-dim fp32 tensor
        as torch keeps it; no state before the first step, as in torch."""
        if state is None or step == 0:
            return cls._group_fields(args), {}
        return cls._group_fields(args), {i: state._param_state(i, p, off, k, step) for i, (_, p, off, k) in enumerate(entries)}

    @classmethod
    def load(cls, store, sd, args):
        for g in sd["param_groups"]:
            on = [n for n in cls.REFUSED if g.get(n, False)]
            if on:
                raise NotImplementedError(f"{cls.FAMILY} with {' / '.join(on)}=True is not implemented by the fused step")
        cls.group_args(sd, args)
        if not sd["state"]:
            return None, 0
        state, step = cls(store, args), 0
        for i, p, off, k, e in cls.file_entries(store, sd):
            for n, buf in (("exp_avg", state.m), (cls.SECOND, state.v)):
                buf[off:off + k].copy_(cls.field(i, p, e, n, numel=k).reshape(-1).float())
            step = max(step, int(float(cls.field(i, p, e, "step"))))
            state._load_entry(i, p, e)
        return state, step

    def _load_entry(self, i, p, e):
        pass


class RAdamState(_AdamXState):
    """torch.optim.RAdam: exp_avg and exp_avg_sq; rho_t, the rectification factor and which branch applies are host scalars."""
    VARIANT, FAMILY = "radam", "RAdam"
    DEFAULTS = dict(decoupled_weight_decay=False)


class NAdamState(_AdamXState):
    """torch.optim.NAdam: exp_avg, exp_avg_sq and the running product of the momentum schedule, mu_product -- per parameter in
    torch, one value per group here (it depends on the group's beta1, momentum_decay and the step count alone): `mu`, a 0-dim fp32 CPU
    tensor per group, advanced as torch advances its own (ops.nadam_scalars).  `sched` is its fp64 device image, written by
    buffers() for a broadcast or a replica check and read back by sync_host() on the ranks that received it.  A grouping that
    changes the number of groups mid-run hands every new group the product of group 0 (exact whenever the groups share beta1 and
    momentum_decay, as LoRA+'s do)."""
    VARIANT, FAMILY = "nadam", "NAdam"
    NAMES = ("m", "v", "sched")
    DEFAULTS = dict(momentum_decay=4e-3, decoupled_weight_decay=False)

    def __init__(self, store, args):
        super().__init__(store, args)
        self.mu = [torch.tensor(1.0)]
        self.sched = None
        self._file_mu = None        # entry index -> the file's mu_product, until regroup() knows the groups

    def regroup(self, store, members):
        super().regroup(store, members)
        firsts = [m[0] for m in self.members] if self.members is not None else [0]
        if self._file_mu is not None:
            self.mu = [torch.tensor(float(self._file_mu.get(i, 1.0))) for i in firsts]
            self._file_mu = None
        elif len(self.mu) != len(firsts):
            self.mu = [self.mu[0].clone() for _ in firsts]

    def buffers(self):
        self.sched = torch.tensor([float(m) for m in self.mu] + [1.0] * (ops.MAX_PARAM_GROUPS - len(self.mu)), dtype=torch.float64,
                                  device=self.m.device)
        return super().buffers()

    def sync_host(self):
        self.mu = [torch.tensor(float(x)) for x in self.sched.cpu().tolist()[:len(self.mu)]]

    def _param_state(self, i, p, off, k, step):
        at = 0 if self.members is None else next(j for j, m in enumerate(self.members) if i in m)
        return dict(super()._param_state(i, p, off, k, step), mu_product=self.mu[at].clone())

    def _load_entry(self, i, p, e):
        if self._file_mu is None:
            self._file_mu = {}
        self._file_mu[i] = float(self.field(i, p, e, "mu_product"))


class AdamaxState(_AdamXState):
    """torch.optim.Adamax: exp_avg and the exponentially weighted infinity norm exp_inf (v); weight decay in the L2 form only."""
    VARIANT, FAMILY, SECOND = "adamax", "Adamax", "exp_inf"


class _AdEMAMix:
    """What the two AdEMAMix states share: the family's own fields (alpha, t_alpha, t_beta3), their checks and the rows of a step.
    A group's row is lr / betas (the TRIPLE beta1, beta2, beta3) / eps / weight_decay plus those fields, read from the row where it
    carries them (the torch.optim classes' param_groups) and from the optimizer_args otherwise.  The schedules alpha_t and beta3_t
    and the bias corrections are functions of the step count alone and are formed on the host (ops.ademamix_rows): the count is the
    only thing a resumed run needs beside the buffers."""
    OWN = dict(alpha=5.0, t_alpha=None, t_beta3=None)
    BETAS = (0.9, 0.999, 0.9999)

    @classmethod
    def _check_own(cls, args):
        if not 0.0 <= args["alpha"]:
            raise ValueError(f"Invalid alpha value: {args['alpha']}")
        for n in ("t_alpha", "t_beta3"):
            if args[n] is not None and not args[n] > 0:
                raise ValueError(f"Invalid {n} value: {args[n]} (None or > 0)")
        args["alpha"] = float(args["alpha"])

    def _group_rows(self, lr, betas, eps, weight_decay, args, groups):
        rows = groups if groups is not None and len(groups) > 1 else [dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)]
        return [dict({n: args[n] for n in self.OWN}, **r) for r in rows]

    @classmethod
    def _group_fields(cls, args):
        return {n: args[n] for n in cls.OWN}


class AdEMAMixState(_AdEMAMix, FlatState):
    """bitsandbytes.optim.AdEMAMix / AdEMAMix32bit: the fast average m1, the slow average m2 and the second moment nu in fp32, indexed
    like pflat, stepped by the ONE launch of qfx_ademamix_step -- always the grouped entry, one row with one group.  In a file m1
    and m2 are ONE tensor "m1_m2" shaped [2, *p.shape] next to "nu" and "step"; the names follow the package's state_dict as far as
    it is known here -- compatibility with a file the package wrote is intended and could NOT be checked (no copy of bitsandbytes
    at hand)."""
    NAMES = ("m1", "m2", "nu")
    GROUPED, FAMILY = True, "AdEMAMix"
    DEFAULTS = dict(_AdEMAMix.OWN)

    def __init__(self, store, args):
        super().__init__(store, args)
        self.m1 = torch.zeros_like(store.pflat)
        self.m2 = torch.zeros_like(store.pflat)
        self.nu = torch.zeros_like(store.pflat)

    @classmethod
    def validate(cls, args):
        cls._check_own(args)

    def step(self, store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale, args, groups=None):
        rows = self._group_rows(lr, betas, eps, weight_decay, args, groups)
        ops.ademamix_step(store.pflat, store.gflat, self.m1, self.m2, self.nu, rows, step, tile_group=self.group_map if len(rows) > 1 else None,
                          gnorm_sq=gnorm_sq, max_norm=max_norm, grad_scale=grad_scale)

    @classmethod
    def save(cls, state, entries, step, args):
        """Per parameter {"step", "m1_m2" [2, *shape], "nu"}; the group carries alpha, t_alpha and t_beta3 next to lr, betas (the
        triple), eps and weight_decay.  No state before the first step."""
        if state is None or step == 0:
            return cls._group_fields(args), {}
        return cls._group_fields(args), {i: {"step": step, "m1_m2": torch.stack([_out(state.m1, off, k, p.shape), _out(state.m2, off, k, p.shape)]),
                                             "nu": _out(state.nu, off, k, p.shape)} for i, (_, p, off, k) in enumerate(entries)}

    @classmethod
    def load(cls, store, sd, args):
        cls.group_args(sd, args)
        if not sd["state"]:
            return None, 0
        state, step = cls(store, args), 0
        for i, p, off, k, e in cls.file_entries(store, sd):
            mm = cls.field(i, p, e, "m1_m2", shape=(2,) + tuple(p.shape)).reshape(2, -1).float()
            state.m1[off:off + k].copy_(mm[0]); state.m2[off:off + k].copy_(mm[1])
            state.nu[off:off + k].copy_(cls.field(i, p, e, "nu", numel=k).reshape(-1).float())
            step = max(step, int(float(cls.field(i, p, e, "step"))))
        return state, step


class AdEMAMixBlockwiseState(_AdEMAMix, _BlockwiseBase):
    """bitsandbytes.optim.AdEMAMix8bit / PagedAdEMAMix8bit: state1 holds BOTH averages as two planes of signed-map codes (q1 [2, n],
    absmax1 [2, blocks], m32 [2, ..] for the tensors below min_8bit_size), state2 is nu on the unsigned map (q2, absmax2, v32), over
    the block table of the other 8-bit families.  In a file: state1 [2, *p.shape], absmax1 [2, blocks], state2, absmax2, qmap1,
    qmap2, step -- key-compatible with the package's optimizer.bin by intent, NOT checked against one."""
    MOMENTS = 2
    FAMILY = "AdEMAMix8bit"
    DEFAULTS = dict(_BlockwiseBase.DEFAULTS, **_AdEMAMix.OWN)

    def __init__(self, store, args):
        super().__init__(store, args)
        dev = store.pflat.device
        plane = (store.pflat.numel() + 15) // 16 * 16      # the planes of q1 and m32 start on multiples of 4 (qfx.h)
        self.q1 = torch.zeros(2, plane, dtype=torch.uint8, device=dev)
        self.absmax1 = torch.zeros(2, max(1, self.layout.n_absmax), dtype=torch.float32, device=dev)
        self.m32 = torch.zeros(2, max(4, self.layout.n_fp32), dtype=torch.float32, device=dev)

    @classmethod
    def validate(cls, args, optimizer="blockwise 8-bit state"):
        _BlockwiseBase.validate(args, optimizer)
        cls._check_own(args)

    def step(self, store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale, args, groups=None):
        rows = self._group_rows(lr, betas, eps, weight_decay, args, groups)
        ops.ademamix8bit_step(store.pflat, store.gflat, self.q1, self.q2, self.absmax1, self.absmax2, self.m32, self.v32, self.layout,
                              self.qmap1, self.qmap2, rows, step, block_group=self.group_map if len(rows) > 1 else None, gnorm_sq=gnorm_sq,
                              max_norm=max_norm, grad_scale=grad_scale)

    def param_state(self, i, shape, step):
        off, k, eight, a0, nb, s0 = self.layout.tensors[i]
        two = lambda t, o, n, sh: t[:, o:o + n].reshape((2,) + tuple(sh)).detach().cpu().clone()
        if not eight:
            return {"step": step, "state1": two(self.m32, s0, k, shape), "state2": _out(self.v32, s0, k, shape)}
        return {"step": step, "state1": two(self.q1, off, k, shape), "state2": _out(self.q2, off, k, shape),
                "qmap1": self.qmap1.cpu().clone(), "qmap2": self.qmap2.cpu().clone(),
                "absmax1": two(self.absmax1, a0, nb, (nb,)), "absmax2": _out(self.absmax2, a0, nb)}

    def load_param_state(self, i, e):
        off, k, eight, a0, nb, s0 = self.layout.tensors[i]
        if (e["state1"].dtype == torch.uint8) != eight:
            raise ValueError(f"optimizer state of parameter {i} ({k} elements) is {'8-bit' if not eight else 'fp32'} in the file: it was "
                             f"saved with another min_8bit_size than {self.layout.min_8bit_size}")
        if e["state1"].numel() != 2 * k or e["state2"].numel() != k:
            raise ValueError(f"optimizer state of parameter {i}: state1 / state2 have {e['state1'].numel()} / {e['state2'].numel()} elements, "
                             f"{2 * k} / {k} expected")
        if not eight:
            self.m32[:, s0:s0 + k].copy_(e["state1"].reshape(2, -1))
            self.v32[s0:s0 + k].copy_(e["state2"].reshape(-1))
            return
        if e["absmax1"].numel() != 2 * nb or e["absmax2"].numel() != nb:
            raise ValueError(f"optimizer state of parameter {i}: {e['absmax1'].numel()} / {e['absmax2'].numel()} absmax blocks, {2 * nb} / {nb} expected")
        self.q1[:, off:off + k].copy_(e["state1"].reshape(2, -1))
        self.absmax1[:, a0:a0 + nb].copy_(e["absmax1"].reshape(2, -1))
        self.q2[off:off + k].copy_(e["state2"].reshape(-1))
        self.absmax2[a0:a0 + nb].copy_(e["absmax2"].reshape(-1))

    @classmethod
    def save(cls, state, entries, step, args):
        """bnb's layout with a two-plane state1 (param_state); the group carries alpha, t_alpha and t_beta3."""
        return cls._group_fields(args), super().save(state, entries, step, args)[1]

    @classmethod
    def load(cls, store, sd, args):
        """The block size is inferred from the file's absmax2 sizes (absmax1 holds two planes)."""
        cls.group_args(sd, args)
        one = {i: (dict(e, absmax1=e["absmax2"]) if "absmax2" in e else e) for i, e in sd["state"].items()}
        bs, q1, q2 = A8.file_layout(one, store.entries)
        if bs is not None:
            args["blocksize"] = bs
        state, step = cls(store, args), 0
        if q1 is not None:
            state.qmap1.copy_(q1); state.qmap2.copy_(q2)
        for i, p, off, k, e in cls.file_entries(store, sd):
            state.load_param_state(i, e)
            step = max(step, int(float(e["step"])))
        return state, step


class ScaledAdamWState(AdamWState):
    """Riemannian-preconditioned AdamW for LoRA pairs (Zhang & Pilanci 2024; include/qfx.h: qfx_scaled_adamw_step, whose listing is
    the specification -- the authors' package was not at hand): AdamW's exp_avg (m) and exp_avg_sq (v) in fp32, indexed like pflat,
    the table of adapter pairs of the layout and the device counter of pairs the last step left untouched (`skipped`).  The table
    is built from the store's entries: `X.lora_A.<adapter>.weight` [r, in] pairs with `X.lora_B.<adapter>.weight` [out, r].
    Parameter groups resolve on the host to the table's per-tensor fields -- a tensor's learning rate over the step's, and its
    weight decay -- so LoRA+ costs nothing; betas and eps are the launch's and cannot differ between groups.  The table is rebuilt
    when those fields change.  Files are torch.optim.AdamW's with reg and precondition in the group."""
    GROUPED, FAMILY = True, "scaled_adamw"
    DEFAULTS = dict(reg=1e-6, precondition=True)

    def __init__(self, store, args):
        super().__init__(store, args)
        self.pairs = self.adapter_pairs(store.entries)
        self.skipped = torch.zeros(1, dtype=torch.int32, device=store.pflat.device)
        self.layout = self._fields = None

    @staticmethod
    def adapter_pairs(entries):
        """(module, index of lora_A's entry, index of lora_B's entry, r, in_features, out_features) of every adapter pair, in the
        order of the lora_A entries.  NotImplementedError naming the module for a tensor without its partner, a shape that is no
        pair's and a rank above 64."""
        at = {n: i for i, (n, _, _, _) in enumerate(entries)}
        pairs, used = [], set()
        for i, (n, p, _, _) in enumerate(entries):
            if ".lora_A." not in n:
                continue
            module = n.split(".lora_A.")[0]
            j = at.get(n.replace(".lora_A.", ".lora_B."))
            if j is None:
                raise NotImplementedError(f"scaled_adamw: the adapter of {module!r} has a lora_A without its lora_B: the preconditioner "
                                          "of a tensor is taken from its partner")
            q = entries[j][1]
            if p.dim() != 2 or q.dim() != 2 or q.shape[1] != p.shape[0]:
                raise NotImplementedError(f"scaled_adamw: the adapter of {module!r} is no pair A [r, in], B [out, r]: lora_A is "
                                          f"{tuple(p.shape)}, lora_B is {tuple(q.shape)}")
            r, nin = (int(d) for d in p.shape)
            if r > ops.SCALED_ADAMW_MAX_RANK:
                raise NotImplementedError(f"scaled_adamw: the adapter of {module!r} has rank {r}; ranks above "
                                          f"{ops.SCALED_ADAMW_MAX_RANK} are not implemented")
            pairs.append((module, i, j, r, nin, int(q.shape[0])))
            used.update((i, j))
        for i, (n, _, _, _) in enumerate(entries):
            if i not in used:
                module = n.split(".lora_B.")[0]
                raise NotImplementedError(f"scaled_adamw: the adapter tensor {n!r} of {module!r} has no partner: the fused step is "
                                          "defined on lora_A / lora_B pairs only")
        return pairs

    @classmethod
    def _base_key(cls, store, args):
        return super()._base_key(store, args) + (tuple((n, tuple(p.shape)) for n, p, _, _ in store.entries),)

    @staticmethod
    def validate(args):
        reg, pre = args["reg"], args["precondition"]
        if isinstance(reg, bool) or not isinstance(reg, (int, float)) or not (reg > 0 and reg < float("inf")):
            raise ValueError(f"scaled_adamw: reg must be a finite float > 0, not {reg!r}")
        if not isinstance(pre, bool):
            raise ValueError(f"scaled_adamw: precondition must be a bool, not {pre!r}")
        args["reg"] = float(reg)

    @classmethod
    def check_rule_fields(cls, k, rule):
        on = [n for n in ("betas", "eps") if n in rule]
        if on:
            raise ParamGroupsNotImplemented(f"{cls.FAMILY}: param_groups[{k}] sets {' / '.join(on)}: a pair is stepped by one workgroup "
                                            "with the launch's betas and eps; a group may set lr and weight_decay")

    def build_group_map(self, store, assign, n_groups):
        """The group of every store entry, on the host: the groups become per-tensor fields of the pair table."""
        return tuple(assign)

    def table_fields(self, lr, betas, eps, weight_decay, groups):
        """(the launch's lr, [(lr_ratio_a, lr_ratio_b, wd_a, wd_b) of every pair as the fp32 values the table holds]).  One group: the
        step's lr, ratios 1 and the step's weight decay.  Several: the rows alone decide, as in the other grouped families -- the
        launch's lr is group 0's and every tensor carries its group's lr over that."""
        f32 = lambda x: float(torch.tensor(float(x), dtype=torch.float32))
        if groups is None or len(groups) <= 1 or self.group_map is None:
            return lr, [(1.0, 1.0, f32(weight_decay), f32(weight_decay))] * len(self.pairs)
        for k, row in enumerate(groups):
            if tuple(row.get("betas", betas)) != tuple(betas) or row.get("eps", eps) != eps:
                raise ParamGroupsNotImplemented(f"{self.FAMILY}: parameter group {k} has its own betas / eps: a pair is stepped by one "
                                                "workgroup with the launch's; a group may set lr and weight_decay")
        base = groups[0]["lr"]
        ratio = [f32(row["lr"] / base) if base != 0 else 1.0 for row in groups]
        wd = [f32(row["weight_decay"]) for row in groups]
        g = self.group_map
        return base, [(ratio[g[i]], ratio[g[j]], wd[g[i]], wd[g[j]]) for _, i, j, _, _, _ in self.pairs]

    def ensure_table(self, store, fields):
        if self.layout is None or self._fields != fields:
            off = [o for _, _, o, _ in store.entries]
            self.layout = ops.scaled_adamw_table([(off[i], off[j], r, nin, nout) + f for (_, i, j, r, nin, nout), f in zip(self.pairs, fields)],
                                                 device=store.pflat.device, n_elems=store.pflat.numel())
            self._fields = fields
        return self.layout

    def step(self, store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale, args, groups=None):
        self.validate(args)
        lr, fields = self.table_fields(lr, betas, eps, weight_decay, groups)
        layout = self.ensure_table(store, fields)
        ops.scaled_adamw_check(lr, betas, eps, args["reg"], args["precondition"])
        ops.scaled_adamw_step(store.pflat, store.gflat, self.m, self.v, layout, self.skipped, lr, betas[0], betas[1], eps, step,
                              reg=args["reg"], precondition=args["precondition"], gnorm_sq=gnorm_sq, max_norm=max_norm,
                              grad_scale=grad_scale)

    @classmethod
    def save(cls, state, entries, step, args):
        """torch.optim.AdamW's per-parameter {"step", "exp_avg", "exp_avg_sq"}; the group carries reg and precondition."""
        group, per = super().save(state, entries, step, args)
        return dict(group, **{n: args[n] for n in cls.DEFAULTS}), per

    @classmethod
    def load(cls, store, sd, args):
        cls.group_args(sd, args)
        if not sd["state"]:
            return None, 0
        return super().load(store, sd, args)


ADAMX = {"radam": RAdamState, "nadam": NAdamState, "adamax": AdamaxState}
ADEMAMIX = ("ademamix",) + A8.ADEMAMIX_BLOCKWISE
LION = ("lion",) + A8.LION_BLOCKWISE
# optimizer= name -> (state class, the weight decay that weight_decay=None stands for: the stood-in optimizer class's own default)
FAMILIES = {"adamw": (AdamWState, 0.01), "prodigy": (ProdigyState, 0.0), "sgd": (SgdState, 0.0), "adafactor": (AdafactorState, 0.0),
            "came": (CameState, 0.0),
            "lion": (LionState, 0.0), "muon": (MuonState, 0.1), "adamw_schedulefree": (ScheduleFreeAdamWState, 0.0),
            "adam8bit_blockwise": (BlockwiseState, 0.0), "adamw8bit_blockwise": (BlockwiseState, 0.01),
            "lion8bit_blockwise": (LionBlockwiseState, 0.0),
            "radam": (RAdamState, 0.0), "nadam": (NAdamState, 0.0), "adamax": (AdamaxState, 0.0),
            "ademamix": (AdEMAMixState, 0.01), "ademamix8bit_blockwise": (AdEMAMixBlockwiseState, 0.01),
            "scaled_adamw": (ScaledAdamWState, 0.01)}


def default_betas(optimizer):
    """The betas a train step uses when its caller gives none: the optimizer class's own default -- (0.9, 0.99) for Lion (both
    packages), came_pytorch.CAME's triple (0.9, 0.999, 0.9999) for CAME, AdEMAMix's triple (0.9, 0.999, 0.9999: beta1, beta2 and the
    slow average's beta3) for the two AdEMAMix families, (0.9, 0.999) for every other family (torch.optim.AdamW's and
    schedulefree.AdamWScheduleFree's, the train steps' default so far)."""
    if optimizer == "came":
        return CameState.BETAS
    if optimizer in ADEMAMIX:
        return _AdEMAMix.BETAS
    return (0.9, 0.99) if optimizer in LION else (0.9, 0.999)


def resolve_family(optimizer, weight_decay=None, optimizer_args=None):
    """The `optimizer=` keyword of the train steps (and of the torch.optim classes in qflux_amd.optim) -> (alias or None, family name,
    state class, weight decay, the family's optimizer_args with defaults filled in).
    optimizer: "adamw" (torch.optim.AdamW semantics, the train step's lr/betas/eps/weight_decay) or "prodigy" (prodigyopt.Prodigy, the
    reference's parameter-free choice: configs/face_seg_flux_kontext_fp16_prodigy.yaml:41-47); optimizer_args = the extra
    init_args of that class (use_bias_correction, safeguard_warmup, beta3, decouple, d0, d_coef, growth_rate).  With Prodigy
    `lr` is the schedule multiplier the reference sets to 1.0.
    "adam8bit_blockwise" / "adamw8bit_blockwise": bitsandbytes.optim.Adam8bit / AdamW8bit with their blockwise 8-bit moments and
    state layout (trainer/adam8bit.py; weight decay decoupled, defaults 0 / 1e-2); optimizer_args: min_8bit_size (4096), blocksize
    (256 or 2048).
    "sgd": torch.optim.SGD, the fourth optimizer the reference documents (docs/guide/training.md:768-826: momentum 0.9, weight_decay
    1e-4; weight decay in the L2 form, default 0); optimizer_args: momentum (0), dampening (0), nesterov (False); betas / eps unused.
    "adafactor": transformers.optimization.Adafactor (factored second moments per adapter matrix, update clipping; weight decay
    scaled by the step's learning rate, default 0); optimizer_args: eps ((1e-30, 1e-3)), clip_threshold (1.0), decay_rate (-0.8),
    beta1 (None), scale_parameter (True), relative_step (True), warmup_init (False).  lr must be None with relative_step (the
    default) and a float without it; betas / eps unused.
    "came": came_pytorch.CAME (Luo et al. 2023: Adafactor's factored second moments, a full first moment, and a second factored pair
    over the instability (update - moment)^2 that rescales the moment; no relative step, lr is required and > 0; weight decay scaled
    by lr, default 0); optimizer_args: eps ((1e-30, 1e-16)) and clip_threshold (1.0); betas is the package's TRIPLE (0.9, 0.999,
    0.9999), each in [0, 1]; the train step's scalar eps is unused.
    "lion": lion_pytorch.Lion / bitsandbytes.optim.Lion (one fp32 moment, the update is lr times the sign of the interpolated
    moment; weight decay decoupled, before the update, default 0); no optimizer_args; eps unused.  "lion8bit_blockwise":
    bitsandbytes.optim.Lion8bit / PagedLion8bit with the moment in blockwise 8-bit codes and bnb's one-state layout;
    optimizer_args: min_8bit_size (4096), blocksize (256 or 2048).
    "muon": torch.optim.Muon (per adapter matrix: Nesterov momentum, then five Newton-Schulz iterations in bf16 on the matrix
    units orthogonalise the update; weight decay decoupled, default the class's 0.1); optimizer_args: momentum (0.95), nesterov
    (True), ns_coefficients ((3.4445, -4.7750, 2.0315)), ns_steps (5), adjust_lr_fn (None = "original", or "match_rms_adamw") and
    eps (1e-7: Muon's own, the floor of the update's norm, not the train step constructor's Adam eps); betas / eps unused.
    "adamw_schedulefree": schedulefree.AdamWScheduleFree (Defazio et al. 2024: Adam's second moment, no first moment and no
    schedule -- the gradient is taken at y, an interpolation between the base sequence z and the running average x; made for a
    constant lr; weight decay in the L2 form on y, default 0; the package's lr is 0.0025); optimizer_args: warmup_steps (0: the
    optimizer's own linear warm-up), r (0.0) and weight_lr_power (2.0): the averaging weight of step k is (k + 1)^r lr_max^power.
    The adapter weights hold y while training: eval() / train() / eval_mode() swap them to x and back, save_checkpoint writes x,
    and the samplers take train_step= to sample from x.
    "radam" / "nadam" / "adamax": torch.optim.RAdam / NAdam / Adamax, stepped by one launch whose arithmetic is torch's
    single-tensor implementation operation for operation (include/qfx.h: qfx_adamx_step); weight decay default 0 (the classes'), in
    the L2 form unless decoupled_weight_decay; optimizer_args: decoupled_weight_decay (False; RAdam and NAdam) and momentum_decay
    (4e-3; NAdam); Adamax takes none.  The classes' own lr defaults (1e-3 / 2e-3 / 2e-3) are what optimizer_kwargs_from_config
    fills in for a config without lr.  maximize, capturable and differentiable are refused.
    "ademamix": bitsandbytes.optim.AdEMAMix (Pagliardini et al. 2024: Adam plus a slow gradient average m2 that enters the update
    with weight alpha; include/qfx.h: qfx_ademamix_step, whose listing is the specification); betas is the TRIPLE (0.9, 0.999,
    0.9999), each in [0, 1); weight decay decoupled, after the update, default the class's 1e-2; optimizer_args: alpha (5.0),
    t_alpha (None) and t_beta3 (None), the lengths in steps of the warm-ups of alpha and beta3.  "ademamix8bit_blockwise":
    bitsandbytes.optim.AdEMAMix8bit / PagedAdEMAMix8bit with the three states in blockwise 8-bit codes (both averages in one
    two-plane state1); optimizer_args: those three plus min_8bit_size (4096) and blocksize (256 or 2048).
    "scaled_adamw": Riemannian-preconditioned AdamW for LoRA pairs (Zhang & Pilanci, ICML 2024; include/qfx.h:
    qfx_scaled_adamw_step, whose listing is the specification -- the authors' package was not at hand): the gradient of each half of
    a pair is multiplied by the inverse of the other half's r x r Gram matrix plus reg I, then AdamW; weight decay decoupled,
    default 1e-2; optimizer_args: reg (1e-6; finite and > 0) and precondition (True; False is plain AdamW per tensor).  Parameter
    groups and LoRA+ set per-tensor lr and weight decay; per-group betas / eps are refused; ranks above 64 are refused.
    betas=None (the default) means the optimizer class's own default: (0.9, 0.99) for the two Lion families, CAME's and AdEMAMix's triples, (0.9, 0.999) --
    torch.optim.AdamW's, the train step constructor's default before Lion -- for every other one; betas given explicitly are never
    reinterpreted."""
    if optimizer not in ("adam", "adam8bit") and optimizer not in FAMILIES:
        raise ValueError(f"unknown optimizer {optimizer!r}")
    alias = None
    # weight_decay=None = "the optimizer class's own default": 0.01 for AdamW (torch.optim.AdamW), 0 for Adam / Adam8bit / SGD; Prodigy
    # keeps its explicit value (the reference's Prodigy configs pass 0.01).  An EXPLICIT value is never reinterpreted.
    if optimizer in ("adam", "adam8bit"):
        # bitsandbytes.optim.Adam8bit -- what most of the reference's YAMLs select (configs/face_seg_config.yaml:56-59:
        # lr + betas only) -- is Adam with blockwise 8-bit quantised moments, a device to fit 24-48 GB cards.  The LoRA state
        # here is 2 x 94 MB of fp32 next to 288 GB of HBM: the moments stay fp32 (strictly closer to exact Adam than the 8-bit
        # code book; optimizer.bin then holds fp32 exp_avg / exp_avg_sq in torch.optim.Adam's layout, not bnb's state1 / state2 /
        # absmax blocks; "adam8bit_blockwise" keeps those).  torch.optim.Adam's weight decay is the L2 form (added to the
        # gradient); bnb's 8-bit Adam decays decoupled, after the update (adam8bit_blockwise).  Only the configs' weight_decay = 0
        # is mapped here.
        if weight_decay is not None and float(weight_decay) != 0.0:
            raise NotImplementedError(f"{optimizer} with L2 weight decay {weight_decay} (bnb adds wd * p to the gradient; the fused "
                                      "kernel implements AdamW's decoupled form only; the reference's configs use none)")
        weight_decay = 0.0
        alias, optimizer = optimizer, "adamw"
    cls, default_wd = FAMILIES[optimizer]
    if weight_decay is None:
        weight_decay = default_wd
    # "adamw" has always returned Prodigy's defaults (nothing reads them) while taking no optimizer_args
    args = dict(ProdigyState.DEFAULTS if cls is AdamWState else cls.DEFAULTS)
    unknown = set(optimizer_args or {}) - set(args)
    if unknown or (optimizer_args and not cls.DEFAULTS):
        raise ValueError(f"unsupported optimizer_args for {optimizer}: {sorted(unknown) or sorted(optimizer_args)}")
    args.update(optimizer_args or {})
    cls.validate(args, optimizer) if issubclass(cls, _BlockwiseBase) else cls.validate(args)      # its message names the optimizer
    return alias, optimizer, cls, weight_decay, args


def state_dict(cls, state, store, step, args, lr, betas, eps, weight_decay, groups=None, members=None):
    """{"state": {i: per-parameter state}, "param_groups": [...], "global_step"} with one entry per LoRA parameter in
    named_parameters() order (what accelerate's optimizer.bin holds for the reference), in the family's own layout.
    Several groups (groups = their rows, members = their store entries): torch's format -- one dict per group with its own fields,
    the parameters numbered consecutively through the groups in order, "state" keyed by those numbers."""
    extra, per = cls.save(state, store.entries, step, args)
    members = norm_members(members)
    if members is None:
        group = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        group.update(extra, params=list(range(len(store.entries))))       # a family's own field wins (Adafactor's eps is its pair)
        return {"state": per, "param_groups": [group], "global_step": step}
    number, out = {}, []
    for row, m in zip(groups, members):
        group = dict(lr=row["lr"], betas=tuple(row["betas"]), eps=row["eps"], weight_decay=row["weight_decay"])
        group.update(extra)
        group.update({n: row[n] for n in list(extra) + ["initial_lr"] if n in row}, params=list(range(len(number), len(number) + len(m))))
        number.update({i: len(number) + j for j, i in enumerate(m)})
        out.append(group)
    return {"state": dict(sorted(((number[i], e) for i, e in per.items()), key=lambda t: t[0])), "param_groups": out, "global_step": step}


def _check_file_groups(sd, members, n_entries):
    """torch.optim.Optimizer.load_state_dict's two checks, with its messages (one group: the count alone, as before groups existed
    a file's parameter list was never compared)."""
    if len(sd["param_groups"]) != (len(members) if members is not None else 1):
        raise ValueError("loaded state dict has a different number of parameter groups")
    if members is not None and any(len(g["params"]) != len(m) for g, m in zip(sd["param_groups"], members)):
        raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")


def load_state_dict(cls, store, sd, args, hyper, groups=None, members=None):
    """Inverse of state_dict: updates args and hyper (lr, betas, eps, weight_decay; a family without betas / eps, such as
    torch.optim.SGD's or transformers' Adafactor's own file, keeps the current values) in place and returns (state or None, step count).
    Several groups: the file must have the optimizer's group count and group sizes (torch's ValueError otherwise); its numbers map
    back to store entries through the groups' lists by position, every row of `groups` takes its file group's fields, and hyper
    those of group 0."""
    members = norm_members(members)
    _check_file_groups(sd, members, len(store.entries))
    if members is not None:
        entry = {n: i for g, m in zip(sd["param_groups"], members) for n, i in zip(g["params"], m)}
        for row, g in zip(groups, sd["param_groups"]):
            row.update({n: (tuple(g[n]) if n == "betas" else g[n]) for n in row if n in g and n != "params"})
        sd = dict(sd, state={entry[n]: e for n, e in sd["state"].items()})
    g = sd["param_groups"][0]
    eps = g.get("eps", hyper["eps"])
    if isinstance(eps, (tuple, list)):      # Adafactor's / CAME's pair is one of its optimizer_args (cls.load reads it), not the scalar eps
        eps = hyper["eps"]
    hyper.update(lr=g["lr"], betas=tuple(g.get("betas", hyper["betas"])), eps=eps, weight_decay=g["weight_decay"])
    state, step = cls.load(store, sd, args)
    if state is not None:
        state.regroup(store, members)
    return state, max(int(sd.get("global_step", g.get("k", 0))), step)    # a package's own file: its group's count k, if any
