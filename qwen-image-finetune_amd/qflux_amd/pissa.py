"""PiSSA initialisation of the adapters (Meng et al., NeurIPS 2024; peft's init_lora_weights="pissa" / "pissa_niter_N"): every pair
starts at the principal rank-r part of its own base weight and the trunk keeps the residual,

    W ~ U S V^T (top r)      B0 = U sqrt(S / s)      A0 = sqrt(S / s) V^T      W_res = W - s B0 A0          (s = lora_alpha / r)

peft takes a full SVD ("pissa") or torch.svd_lowrank ("pissa_niter_N") per layer and subtracts an [out, in] fp32 product in torch;
here both spellings are the randomized factorisation of qflux_amd.extract -- qfx_lowrank_sketch of the base weight itself, then
qfx_lora_spectrum / qfx_lora_project with the transforms scaled to the balanced split -- and the residual is ONE qfx_lora_fold
launch per group of matrices (include/qfx.h).  Every launch is bit-reproducible, so the residual trunk is never stored: a fresh
model and the same (niter, oversample, seed) give the same W_res, A0, B0 on every run and on every data-parallel rank.

pissa_to_lora is peft's conversion (path_initial_model_for_weight_conversion): B' = [B | B0], A' = [A ; -A0] at rank 2r with
lora_alpha doubled applies to the ORIGINAL base weights.  peft is not a dependency and was not at hand: the formulas above are
the specification (tests/pissa_ref.py restates them).  Left out: OLoRA, LoftQ, conv layers and ranks above 64.
"""
from __future__ import annotations

import math
import re

import torch

from . import extract as _extract
from . import ops
from . import resize as _resize_mod
from .modules import QfxLoraLinear
from .spectrum import SpectrumState

__all__ = ["parse_init", "check_config", "pissa_init_", "pissa_to_lora", "MAX_RANK", "MAX_NITER", "DEFAULT_NITER"]

MAX_RANK = ops.LORA_FOLD_MAX_RANK
MAX_NITER = ops.LOWRANK_MAX_POWER_ITERS
DEFAULT_NITER = 2


def parse_init(init):
    """init_lora_weights -> the number of power iterations of a PiSSA initialisation, or None for every other value:
    "pissa" -> 2, "pissa_niter_N" -> N (0..4; above that a ValueError that names the limit)."""
    if not isinstance(init, str) or not init.lower().startswith("pissa"):
        return None
    if init.lower() == "pissa":
        return DEFAULT_NITER
    m = re.fullmatch(r"pissa_niter_(\d+)", init.lower())
    if m is None:
        raise ValueError(f"init_lora_weights={init!r}: expected 'pissa' or 'pissa_niter_N'")
    n = int(m.group(1))
    if n > MAX_NITER:
        raise ValueError(f"init_lora_weights={init!r}: at most {MAX_NITER} power iterations (pissa_niter_{MAX_NITER}) are implemented")
    return n


def check_config(r, lora_alpha, what="pissa_init_"):
    """What a PiSSA initialisation refuses of an adapter's rank and lora_alpha, before anything is touched."""
    s = float(lora_alpha) / float(r) if r else float("nan")
    if not (s > 0 and math.isfinite(s)):
        raise ValueError(f"{what}: scaling lora_alpha / r = {s}: it must be positive")
    if r > MAX_RANK:
        raise NotImplementedError(f"{what}: rank {r}; ranks above {MAX_RANK} are not implemented")


def _on_gpu(t):
    return t.is_cuda


def _align(n, a=64):
    return (n + a - 1) // a * a


@torch.no_grad()
def _factors(mats, ranks, scalings, k, niter, seed, index0):
    """The device part before the fold, over mats = [(name, W, None)] of one group: the sketch at width k, the spectrum, the
    transforms scaled in fp64 to the balanced split and the projection to each rank.  -> (qflat, [(off_a, off_b)] of A0 / B0 in
    it, sv [n, 64] fp64 / normsq [n] fp64 / info [n, 2] on the host, the names the sketch skipped).  A ValueError for a Jacobi
    solve of the sketch or of the spectrum that did not converge."""
    pflat, pairs, normsq, info, skipped = _extract._sketch(mats, k, niter, seed, index0=index0)
    if skipped:
        return None, None, None, normsq, info, [m[0] for m, ns, i in zip(mats, normsq.tolist(), info.tolist()) if ns == 0.0 and i[1] == 0]
    loose = [m[0] for m, i in zip(mats, info.tolist()) if not i[1]]
    state = SpectrumState.for_pairs(pflat, pairs, workspace=True)
    state.launch(pflat)
    sv, sinfo, sskipped = state.read()                              # the one readback of the group: spectra and verdicts
    loose += [m[0] for m, i in zip(mats, sinfo.tolist()) if not i[3] and m[0] not in loose]
    if loose or sskipped:                                           # raised before any fold (pissa_init_ factorises every group first)
        raise ValueError(f"pissa_init_: the eigen-solves of {len(loose)} factorisation(s) did not converge or met non-finite values, "
                         f"among {loose[:4]}; nothing was changed")
    dev, n = pflat.device, len(pairs)
    rr = torch.tensor(ranks, dtype=torch.int32, device=dev)
    s = torch.tensor(scalings, dtype=torch.float64, device=dev)
    keep = (torch.arange(64, device=dev)[None, :] < torch.minimum(state.info[:, 0], rr)[:, None]) & (state.sv[:, :64] > 0)
    sig = torch.where(keep, state.sv[:, :64], 1.0)                  # no division by a sigma outside the numeric rank
    g = torch.where(keep, torch.sqrt(sig / s[:, None]), 0.0)        # sqrt(sigma_i / s): the rows of T_A (-> V^T)
    f = torch.where(keep, g / sig, 0.0)                             # the columns of T_B (-> U S) come down to U sqrt(sigma_i / s)
    ws = state.ws.view(n, 2, 64, 64)
    ws[:, 0].mul_(f[:, None, :])
    ws[:, 1].mul_(g[:, :, None])
    dst, where, off = [], [], 0
    for r, (_, _, _, _, nin, nout, _) in zip(ranks, pairs):
        oa, ob = off, off + _align(r * nin)
        off = ob + _align(nout * r)
        dst.append((oa, ob, r, r))
        where.append((oa, ob))
    qflat = torch.zeros(off, dtype=torch.float32, device=dev)
    ops.lora_project(pflat, qflat, state.layout, ops.lora_project_table(state.layout, dst, device=dev, n_elems=off), state.ws)
    return qflat, where, sv, normsq, info, []


@torch.no_grad()
def _fold(weights, qflat, where, ranks, coeffs):
    """W <- W + c B0 A0 for the group's weights: one qfx_lora_fold launch."""
    rows = [(W, oa, ob, r, c) for W, (oa, ob), r, c in zip(weights, where, ranks, coeffs)]
    ops.lora_fold(ops.lora_fold_table(rows, device=qflat.device, n_elems=qflat.numel()), qflat)


def _groups(sizes, ranks, budget):
    """extract.byte_groups, and a change of rank also ends a group (one sketch width per launch sequence)."""
    out = []
    for g in _extract.byte_groups(sizes, budget):
        cur = [g[0]]
        for i in g[1:]:
            if ranks[i] != ranks[cur[-1]]:
                out.append(cur)
                cur = []
            cur.append(i)
        out.append(cur)
    return out


@torch.no_grad()
def pissa_init_(model, niter=DEFAULT_NITER, oversample=8, seed=0, group_bytes=2 << 30):
    """PiSSA for every QfxLoraLinear of `model` (blocks, embedders, output projection, conditioning head), in place: the active
    adapter becomes (A0, B0), the base weight the residual W - s B0 A0.  The sketch runs at k = min(64, r + oversample) columns
    with `niter` power iterations (0..4); the test matrix of a module is keyed by (seed, its position in the sorted module list),
    so the result does not depend on group_bytes, the cap on the matrices one sequence of launches covers.  Everything derived
    from the weights is dropped (prepared and quantised copies, plans, the modulation table).  model._pissa keeps A0, B0 (fp32, on
    the host) and (niter, oversample, seed).  Returns {module: dict(sigma, weight_norm, fro_retained, sketch_kept, sketch_converged)}.
    Raises ValueError for scaling <= 0, a merged model, a second call and a module with a non-finite weight (nothing is folded
    then), NotImplementedError for a rank above 64 and RuntimeError for weights that are not on a GPU."""
    if isinstance(niter, bool) or int(niter) != niter or not 0 <= int(niter) <= MAX_NITER:
        raise ValueError(f"pissa_init_: niter must lie in 0..{MAX_NITER}, not {niter!r}")
    if isinstance(oversample, bool) or int(oversample) != oversample or oversample < 0:
        raise ValueError(f"pissa_init_: oversample must be a non-negative integer, not {oversample!r}")
    niter, oversample, seed = int(niter), int(oversample), int(seed)
    mods = sorted(((n, m) for n, m in model.named_modules() if isinstance(m, QfxLoraLinear)), key=lambda nm: nm[0])
    if not mods:
        raise ValueError("pissa_init_: the model has no adapters")
    if getattr(model, "_pissa", None) is not None:
        raise ValueError("pissa_init_: the model has been initialised already (its base weights are residuals)")
    if getattr(model, "_merged", False) or any(m.merged for _, m in mods):
        raise ValueError("pissa_init_: the adapters are merged into the base weights: unmerge first")
    ranks = [int(m.r[m.active_adapter]) for _, m in mods]
    scalings = [float(m.scaling[m.active_adapter]) for _, m in mods]
    for (n, m), r, s in zip(mods, ranks, scalings):
        if not (s > 0 and math.isfinite(s)):
            raise ValueError(f"pissa_init_: the adapter of {n!r} has scaling {s}: lora_alpha / r must be positive")
        if r > MAX_RANK:
            raise NotImplementedError(f"pissa_init_: the adapter of {n!r} has rank {r}; ranks above {MAX_RANK} are not implemented")
        if not _on_gpu(m.base_layer.weight):
            raise RuntimeError(f"pissa_init_: the weight of {n!r} is on {m.base_layer.weight.device}, not on a GPU: move the model to "
                               "the device first (model.to('cuda'), then model.pissa_init_(...))")
    weights = [m.base_layer.weight.data for _, m in mods]
    sizes = [w.shape[0] * w.shape[1] * 4 for w in weights]
    done, skipped = [], []
    for group in _groups(sizes, ranks, int(group_bytes)):          # every factorisation first: a refusal leaves the trunk as it was
        mats = [(mods[i][0], weights[i], None) for i in group]
        rk, sc = [ranks[i] for i in group], [scalings[i] for i in group]
        qflat, where, sv, normsq, info, bad = _factors(mats, rk, sc, min(ops.LOWRANK_MAX_K, rk[0] + oversample), niter, seed, group[0])
        skipped += bad
        done.append((group, qflat, where, sv, normsq, info))
    if skipped:
        raise ValueError(f"pissa_init_: {len(skipped)} base weight(s) hold non-finite values, among {skipped[:4]}; nothing was changed")
    A0, B0, report = {}, {}, {}
    for group, qflat, where, sv, normsq, info in done:
        host = qflat.cpu()                                         # one device -> host copy per group; A0 / B0 are slices of it
        for j, i in enumerate(group):
            (name, m), r, (oa, ob) = mods[i], ranks[i], where[j]
            m.A.copy_(qflat[oa:oa + r * m.in_features].view(r, m.in_features))
            m.B.copy_(qflat[ob:ob + m.out_features * r].view(m.out_features, r))
            A0[name] = host[oa:oa + r * m.in_features].view(r, m.in_features).clone()
            B0[name] = host[ob:ob + m.out_features * r].view(m.out_features, r).clone()
            sigma = [float(x) for x in sv[j, :r]]
            wn = math.sqrt(float(normsq[j]))
            report[name] = dict(sigma=sigma, weight_norm=wn, fro_retained=(math.sqrt(math.fsum(x * x for x in sigma)) / wn if wn > 0 else 1.0),
                                sketch_kept=int(info[j][0]), sketch_converged=bool(info[j][1]))
        _fold([weights[i] for i in group], qflat, where, [ranks[i] for i in group], [-scalings[i] for i in group])
    model._pissa = dict(A0=A0, B0=B0, niter=niter, oversample=oversample, seed=seed)
    if hasattr(model, "_invalidate"):          # prepared / quantised copies of the weights, plans, the modulation table
        model._invalidate()
        model._adapter_gen += 1
        model._lora.tag()
    return report


@torch.no_grad()
def pissa_to_lora(model, rank=None, device=None):
    """peft's PiSSA -> LoRA conversion of the model's active adapters: {module: (A' [2r, in], B' [out, 2r])} on the host with
    B' = [B | B0], A' = [A ; -A0], and {module: lora_alpha'} with lora_alpha' = 2 lora_alpha (the same scaling), so that
    s B' A' = s (B A - B0 A0) is the change against the ORIGINAL base weights.  rank=k re-expresses every pair at rank k through
    resize.resize_pairs (uniform=True; on `device`, default the device of the adapters)."""
    st = getattr(model, "_pissa", None)
    if st is None:
        raise ValueError("pissa_to_lora: the model has no PiSSA initialisation (pissa_init_ / init_lora_weights='pissa')")
    tensors, alphas = {}, {}
    for name, m in model.named_modules():
        if not isinstance(m, QfxLoraLinear):
            continue
        if name not in st["A0"]:
            raise ValueError(f"pissa_to_lora: {name!r} was adapted after the PiSSA initialisation")
        A, B = m.A.detach().to("cpu", torch.float32), m.B.detach().to("cpu", torch.float32)
        r = A.shape[0]
        if 2 * r > MAX_RANK:
            raise NotImplementedError(f"pissa_to_lora: {name!r} has rank {r}: the converted pair has rank {2 * r}; ranks above "
                                      f"{MAX_RANK} are not implemented")
        if tuple(st["A0"][name].shape) != tuple(A.shape):
            raise ValueError(f"pissa_to_lora: the adapter of {name!r} no longer has the shape it was initialised with")
        tensors[name] = (torch.cat([A, -st["A0"][name]], dim=0).contiguous(), torch.cat([B, st["B0"][name]], dim=1).contiguous())
        alphas[name] = 2.0 * float(m.lora_alpha[m.active_adapter])
    if rank is None:
        return tensors, alphas
    dev = torch.device(device) if device is not None else next(m.A.device for m in model.modules() if isinstance(m, QfxLoraLinear))
    pairs, off = [], 0
    for name, (A2, B2) in tensors.items():
        oa, ob = off, off + _align(A2.numel())
        off = ob + _align(B2.numel())
        pairs.append((name, oa, ob, A2.shape[0], A2.shape[1], B2.shape[0], alphas[name] / A2.shape[0]))
    host = torch.zeros(off, dtype=torch.float32)
    for (name, oa, ob, *_), (A2, B2) in zip(pairs, tensors.values()):
        host[oa:oa + A2.numel()] = A2.reshape(-1)
        host[ob:ob + B2.numel()] = B2.reshape(-1)
    resized, new_alphas, _ = _resize_mod.resize_pairs(host.to(dev), pairs, int(rank))
    return {n: (a.cpu().contiguous(), b.cpu().contiguous()) for n, (a, b) in resized.items()}, new_alphas
