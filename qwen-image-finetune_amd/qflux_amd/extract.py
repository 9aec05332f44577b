"""Extract a LoRA from two checkpoints (kohya's extract_lora_from_models.py): the rank-r adapter that best reproduces the
difference W_tuned - W_base of every linear layer.

kohya takes a full SVD of each [out, in] difference; here a randomized range finder (qfx_lowrank_sketch, include/qfx.h: a handful
of skinny passes over each difference, k = rank + oversample columns wide, with power iterations) leaves every difference as a pair
Q [out, k], C [k, in] in one flat buffer -- exactly the (B, A) form resize.resize_pairs consumes -- and the spectrum, select_rank
and the projection to the final rank are the two launches of the rank resize.  No dense SVD and no [out, in] temporary.  kohya's
script is not a dependency and was not at hand: the semantics are restated (tests/lora_extract_ref.py); its --clamp_quantile is
left out on purpose, as are conv layers, OLoRA / LoftQ initialisation, merging several LoRAs by SVD and ranks above 64 (PiSSA
initialisation builds on the same sketch: qflux_amd.pissa).
"""
from __future__ import annotations

import math
import os
import re

import torch

from . import ops
from . import resize as _resize_mod

__all__ = ["extract_pairs", "extract_lora", "pair_weights", "byte_groups", "MAX_RANK"]

MAX_RANK = ops.LOWRANK_MAX_K
_DIFFUSERS_RENAMED = ("to_q", "to_k", "to_v", "to_out.0")


def _align(n, a=64):
    return (n + a - 1) // a * a


@torch.no_grad()
def _sketch(mats, k, power_iters, seed, index0=0):
    """The device part: qfx_lowrank_sketch over mats = [(name, W1, W0 or None)] -> (pflat, pairs as resize_pairs takes them with
    scaling 1, normsq [n] fp64 and info [n, 2] int32 on the host, skipped).  index0 + the position in mats keys the test matrix."""
    dev = mats[0][1].device
    rows, pairs, off = [], [], 0
    for i, (name, W1, W0) in enumerate(mats):
        nout, nin = W1.shape
        oa, ob = off, off + _align(k * nin)
        off = ob + _align(nout * k)
        rows.append((W1, W0, k, oa, ob, index0 + i))
        pairs.append((name, oa, ob, k, int(nin), int(nout), 1.0))
    table = ops.lowrank_table(rows, device=dev, n_elems=off)
    pflat = torch.zeros(off, dtype=torch.float32, device=dev)
    n = len(mats)
    packed = torch.zeros(n + 1, 3, dtype=torch.float64, device=dev)
    normsq = torch.zeros(n, dtype=torch.float64, device=dev)
    info = torch.zeros(n, 2, dtype=torch.int32, device=dev)
    skipped = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(table.ws_bytes, dtype=torch.uint8, device=dev)
    ops.lowrank_sketch(table, pflat, normsq, info, skipped, ws, power_iters=power_iters, seed=seed)
    packed[:n, 0].copy_(normsq)
    packed[:n, 1:].copy_(info)
    packed[n, 0:1].copy_(skipped)
    host = packed.cpu()                       # the one device -> host copy
    return pflat, pairs, host[:n, 0].clone(), host[:n, 1:].to(torch.int32), int(host[n, 0])


def _resize(pflat, pairs, rank, dynamic_method, dynamic_param, uniform):
    return _resize_mod.resize_pairs(pflat, pairs, rank, dynamic_method, dynamic_param, uniform)


@torch.no_grad()
def extract_pairs(mats, rank, oversample=8, power_iters=2, seed=0, dynamic_method=None, dynamic_param=None, uniform=True):
    """mats: [(name, W1, W0 or None)] device tensors [out, in], bfloat16 or float32.  The sketch at k = min(64, rank + oversample),
    then resize.resize_pairs (spectrum, select_rank, projection) at scaling 1.  Returns resize_pairs' (tensors, alphas, report);
    each report row also holds diff_norm = ||W1 - W0||_F and fro_retained_of_diff = sqrt(sum_{i<kept} sigma_i^2) / diff_norm
    (1 for a zero difference)."""
    if not mats:
        raise ValueError("extract_pairs: no matrices")
    if isinstance(rank, bool) or int(rank) != rank or rank < 1:
        raise ValueError(f"extract_pairs: rank must be a positive integer, not {rank!r}")
    if rank > MAX_RANK:
        raise NotImplementedError(f"extract_pairs: rank {rank}: ranks above {MAX_RANK} are not implemented")
    if isinstance(oversample, bool) or int(oversample) != oversample or oversample < 0:
        raise ValueError(f"extract_pairs: oversample must be a non-negative integer, not {oversample!r}")
    if not 0 <= int(power_iters) <= ops.LOWRANK_MAX_POWER_ITERS:
        raise ValueError(f"extract_pairs: power_iters must lie in 0..{ops.LOWRANK_MAX_POWER_ITERS}, not {power_iters!r}")
    _resize_mod.select_rank([1.0], rank, dynamic_method, dynamic_param)          # refuse a bad rule before anything is launched
    k = min(MAX_RANK, int(rank) + int(oversample))
    pflat, pairs, normsq, info, skipped = _sketch(mats, k, int(power_iters), int(seed))
    if skipped:
        bad = [m[0] for m, ns, i in zip(mats, normsq.tolist(), info.tolist()) if ns == 0.0 and i[1] == 0]
        raise ValueError(f"extract_pairs: {skipped} difference(s) hold non-finite values, among {bad[:4]}")
    tensors, alphas, report = _resize(pflat, pairs, int(rank), dynamic_method, dynamic_param, uniform)
    names = [m[0] for m in mats]
    kept_norm = torch.stack([tensors[n][1].double().pow(2).sum() for n in names]).sqrt().cpu().tolist()      # lora_down has orthonormal rows
    for n, ns, kn, i in zip(names, normsq.tolist(), kept_norm, info.tolist()):
        dn = math.sqrt(ns)
        report[n].update(diff_norm=dn, fro_retained_of_diff=(kn / dn if dn > 0 else 1.0), sketch_kept=int(i[0]),
                         sketch_converged=bool(i[1]))
    return tensors, alphas, report


def pair_weights(base_keys, tuned_keys, target_modules=None):
    """The modules to extract: every `<module>.weight` present in both key -> shape tables with the same 2-D shape, adapter
    tensors left out; target_modules: a regex searched in the module name, or a list of names / suffixes (as param_groups)."""
    out = []
    for key, shape in base_keys.items():
        if not key.endswith(".weight") or "lora_" in key or ".lora." in key or len(shape) != 2:
            continue
        if key not in tuned_keys or tuple(tuned_keys[key]) != tuple(shape):
            continue
        name = key[:-len(".weight")]
        if target_modules is not None:
            if isinstance(target_modules, str):
                if not re.search(target_modules, name):
                    continue
            elif not any(name == t or name.endswith("." + t) for t in target_modules):
                continue
        out.append(name)
    return out


def byte_groups(sizes, budget):
    """Consecutive groups of indices whose byte sizes sum to at most `budget`; a single item above the budget is a group of its own."""
    groups, cur, tot = [], [], 0
    for i, s in enumerate(sizes):
        if cur and tot + s > budget:
            groups.append(cur)
            cur, tot = [], 0
        cur.append(i)
        tot += s
    if cur:
        groups.append(cur)
    return groups


class _Source:
    """A key -> tensor table over a safetensors file or folder (read lazily), a state dict, or a model."""

    def __init__(self, src):
        self.file, self.sd = None, None
        if isinstance(src, (str, os.PathLike)):
            from safetensors import safe_open
            path = str(src)
            if os.path.isdir(path):
                cands = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
                if len(cands) != 1:
                    raise ValueError(f"extract_lora: {path} must hold exactly one .safetensors file, found {cands}")
                path = os.path.join(path, cands[0])
            self.file = safe_open(path, framework="pt")
            self.shapes = {k: tuple(self.file.get_slice(k).get_shape()) for k in self.file.keys()}
        else:
            self.sd = src if isinstance(src, dict) else {k: v for k, v in src.state_dict().items()}
            self.shapes = {k: tuple(v.shape) for k, v in self.sd.items() if torch.is_tensor(v)}

    def get(self, key):
        return self.file.get_tensor(key) if self.file is not None else self.sd[key].detach()


def _key_of(name):
    if name.endswith(_DIFFUSERS_RENAMED):
        return f"transformer.{name}.lora.down.weight", f"transformer.{name}.lora.up.weight"
    return f"transformer.{name}.lora_A.weight", f"transformer.{name}.lora_B.weight"


@torch.no_grad()
def extract_lora(base, tuned, save_to=None, rank=16, target_modules=None, min_diff=0.0, oversample=8, power_iters=2, seed=0,
                 dynamic_method=None, dynamic_param=None, uniform=True, device="cuda", group_bytes=2 << 30):
    """base: a loaded model of this package, a state dict or a safetensors path; tuned: a safetensors path or folder, a state dict
    or a model.  Every 2-D `<module>.weight` present in both (target_modules: a regex or a list, as param_groups) is streamed to
    `device` in groups of at most group_bytes (both sides counted), so that neither checkpoint has to be resident, and extracted
    at `rank`.  A module with ||W_tuned - W_base||_F <= min_diff is left out of the result and reported as unchanged.  With
    save_to: a safetensors file (or folder) in the key style and with the per-module lora_alpha metadata resize_lora_file
    writes (lora_up = U S, lora_down = V^T, alpha = the allocated rank, so the scaling is 1); lora_io.load_lora_adapter reads the
    uniform=True result.  Returns (tensors {module: (A, B)} on the host, alphas, report)."""
    bsrc, tsrc = _Source(base), _Source(tuned)
    names = pair_weights(bsrc.shapes, tsrc.shapes, target_modules)
    if not names:
        raise ValueError("extract_lora: no 2-D weight is present in both checkpoints" + (" under target_modules" if target_modules else ""))
    sizes = []
    for n in names:
        nout, nin = bsrc.shapes[n + ".weight"]
        sizes.append(2 * nout * nin * 4)
    tensors, alphas, report = {}, {}, {}
    for group in byte_groups(sizes, int(group_bytes)):
        mats = []
        for i in group:
            key = names[i] + ".weight"
            W0, W1 = bsrc.get(key), tsrc.get(key)
            dt = torch.bfloat16 if W0.dtype == torch.bfloat16 and W1.dtype == torch.bfloat16 else torch.float32
            mats.append((names[i], W1.to(device=device, dtype=dt).contiguous(), W0.to(device=device, dtype=dt).contiguous()))
        t, a, r = extract_pairs(mats, rank, oversample, power_iters, seed, dynamic_method, dynamic_param, uniform)
        for n in t:
            tensors[n] = (t[n][0].cpu().contiguous(), t[n][1].cpu().contiguous())
        alphas.update(a)
        report.update(r)
        del mats
    for n in names:
        report[n]["unchanged"] = bool(report[n]["diff_norm"] <= min_diff)
        if report[n]["unchanged"]:
            del tensors[n], alphas[n]
    if uniform and tensors and len({A.shape[0] for A, _ in tensors.values()}) > 1:      # groups chose different ranks: pad to the largest
        r_max = max(A.shape[0] for A, _ in tensors.values())
        for n, (A, B) in tensors.items():
            r = A.shape[0]
            if r < r_max:
                tensors[n] = (torch.cat([A, A.new_zeros(r_max - r, A.shape[1])]), torch.cat([B, B.new_zeros(B.shape[0], r_max - r)], dim=1))
                alphas[n] = alphas[n] / r * r_max
                report[n]["new_rank"] = r_max
    if save_to is not None:
        if not tensors:
            raise ValueError("extract_lora: every module is unchanged under min_diff: nothing to save")
        from safetensors.torch import save_file

        from .lora_io import WEIGHT_NAME
        out = {}
        for n, (A, B) in tensors.items():
            ka, kb = _key_of(n)
            out[ka], out[kb] = A.contiguous(), B.contiguous()
        save_to = str(save_to)
        if os.path.isdir(save_to) or not save_to.endswith(".safetensors"):
            os.makedirs(save_to, exist_ok=True)
            save_to = os.path.join(save_to, WEIGHT_NAME)
        save_file(out, save_to, metadata={"format": "pt", "lora_alpha": repr({n: str(a) for n, a in alphas.items()})})
    return tensors, alphas, report
