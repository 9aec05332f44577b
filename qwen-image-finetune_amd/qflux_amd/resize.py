"""Rank resize of trained adapters (kohya's resize_lora.py): every pair `scaling * B @ A` re-expressed at a lower rank by truncated
SVD -- a fixed rank, or the dynamic rules sv_ratio / sv_cumulative / sv_fro -- for a smaller file or to keep training at the new rank.

kohya takes a full SVD of each [out, in] product; here the decomposition of ALL pairs is one launch (qfx_lora_spectrum), one copy
of the spectra to the host where select_rank picks each pair's rank, and one more launch (qfx_lora_project) that writes
lora_up = U S and lora_down = V^T into a new flat buffer.  kohya's script is not a dependency and was not at hand: the semantics
are restated (include/qfx.h, tests/lora_svd_ref.py); in particular the clamps at the edges of its index functions -- what it
returns when a threshold is met exactly, or by no prefix -- could not be compared and are the ones written in select_rank.

uniform=True gives every pair the same allocated rank (the largest chosen, the others zero-padded: the same dW), which is what
lora_io.load_lora_adapter, a single-rank loader, can read; uniform=False files carry one rank per module and are for peft,
diffusers and ComfyUI.
"""
from __future__ import annotations

import ast
import math
import os

import torch

from . import ops
from .modules import _W, LoraConfig, QfxLoraLinear
from .regularize import _store_of, adapter_pairs
from .spectrum import SpectrumState

__all__ = ["select_rank", "resize_pairs", "resize_lora_file", "resize_adapter", "DYNAMIC_METHODS"]

DYNAMIC_METHODS = ("sv_ratio", "sv_cumulative", "sv_fro")


def select_rank(sv, new_rank, dynamic_method=None, dynamic_param=None, numeric_rank=None):
    """The number of components to keep of one descending spectrum -> (k, retained Frobenius share, retained sum share).
      no method:      k = new_rank
      sv_ratio:       (param >= 1)      k = #{s_i >= s_0 / param}
      sv_cumulative:  (0 < param <= 1)  the smallest k with sum_{i<k} s_i / sum s >= param
      sv_fro:         (0 < param <= 1)  the smallest k with sqrt(sum_{i<k} s_i^2 / sum s^2) >= param
    then k = max(1, min(k, new_rank, r, max(numeric_rank, 1))).  An all-zero spectrum gives 1 with both shares 1."""
    sv = [float(x) for x in sv]
    r = len(sv)
    if r < 1:
        raise ValueError("select_rank: an empty spectrum")
    if isinstance(new_rank, bool) or int(new_rank) != new_rank or new_rank < 1:
        raise ValueError(f"select_rank: new_rank must be a positive integer, not {new_rank!r}")
    new_rank = int(new_rank)
    s1, s2 = math.fsum(sv), math.fsum(x * x for x in sv)

    def fro_share(k):
        return math.sqrt(math.fsum(x * x for x in sv[:k]) / s2) if s2 > 0 else 1.0

    def sum_share(k):
        return math.fsum(sv[:k]) / s1 if s1 > 0 else 1.0

    if dynamic_method is None:
        k = new_rank
    elif dynamic_method == "sv_ratio":
        if dynamic_param is None or not dynamic_param >= 1:
            raise ValueError(f"select_rank: sv_ratio needs dynamic_param >= 1, not {dynamic_param!r}")
        k = sum(1 for x in sv if x >= sv[0] / dynamic_param)
    elif dynamic_method in ("sv_cumulative", "sv_fro"):
        if dynamic_param is None or not 0 < dynamic_param <= 1:
            raise ValueError(f"select_rank: {dynamic_method} needs 0 < dynamic_param <= 1, not {dynamic_param!r}")
        share = sum_share if dynamic_method == "sv_cumulative" else fro_share
        k = next((kk for kk in range(1, r + 1) if share(kk) >= dynamic_param), r)
    else:
        raise ValueError(f"select_rank: unknown dynamic_method {dynamic_method!r} (known: {', '.join(DYNAMIC_METHODS)})")
    nr = r if numeric_rank is None else int(numeric_rank)
    k = max(1, min(k, new_rank, r, max(nr, 1)))
    return k, fro_share(k), sum_share(k)


def _align(n, a=64):
    return (n + a - 1) // a * a


@torch.no_grad()
def resize_pairs(pflat, pairs, new_rank, dynamic_method=None, dynamic_param=None, uniform=True, rank_tol=ops.LORA_SVD_RANK_TOL,
                 max_sweeps=ops.LORA_SVD_MAX_SWEEPS):
    """The core, no model needed.  pflat: flat fp32 device buffer; pairs: (name, off_a, off_b, r, in_features, out_features,
    scaling) as regularize.adapter_pairs lists them.  Two launches and one device -> host copy between them.  Returns
      tensors  {name: (A' [r_dst, in], B' [out, r_dst])}  views of ONE new flat buffer on pflat's device
      alphas   {name: scaling * r_dst}                    the lora_alpha that keeps the pair's scaling
      report   {name: dict(old_rank, new_rank = r_dst, kept = k, fro_retained, sum_retained, sigma0 (of scaling B A), numeric_rank)}"""
    if not pairs:
        raise ValueError("resize_pairs: no pairs")
    select_rank([1.0], new_rank, dynamic_method, dynamic_param)        # refuse a bad rule before anything is launched
    if new_rank > ops.LORA_SVD_MAX_RANK:
        raise ValueError(f"resize_pairs: new_rank must be <= {ops.LORA_SVD_MAX_RANK}")
    state = SpectrumState.for_pairs(pflat, pairs, workspace=True)
    state.launch(pflat, rank_tol, max_sweeps)
    sv, info, skipped = state.read()
    if skipped:
        bad = [state.names[i] for i in range(len(pairs)) if not info[i, 3] and not bool(sv[i].any())]
        raise ValueError(f"resize_pairs: {skipped} pair(s) hold non-finite weights: {bad[:4]}")
    picks = [select_rank(sv[i, :r].tolist(), new_rank, dynamic_method, dynamic_param, int(info[i, 0]))
             for i, r in enumerate(state.ranks)]
    r_max = max(k for k, _, _ in picks)
    dst, off = [], 0
    for (k, _, _), (_, _, _, r, nin, nout, _) in zip(picks, pairs):
        r_dst = r_max if uniform else k
        dst.append((off, off + _align(r_dst * nin), k, r_dst))
        off += _align(r_dst * nin) + _align(nout * r_dst)
    qflat = torch.zeros(off, dtype=torch.float32, device=pflat.device)
    dst_table = ops.lora_project_table(state.layout, dst, device=pflat.device, n_elems=off)
    ops.lora_project(pflat, qflat, state.layout, dst_table, state.ws)
    tensors, alphas, report = {}, {}, {}
    for i, ((k, fro, cum), (name, _, _, r, nin, nout, scaling), (oa, ob, _, r_dst)) in enumerate(zip(picks, pairs, dst)):
        tensors[name] = (qflat[oa:oa + r_dst * nin].view(r_dst, nin), qflat[ob:ob + nout * r_dst].view(nout, r_dst))
        alphas[name] = float(scaling) * r_dst
        report[name] = dict(old_rank=int(r), new_rank=int(r_dst), kept=int(k), fro_retained=fro, sum_retained=cum,
                            sigma0=float(sv[i, 0]) * abs(float(scaling)), numeric_rank=int(info[i, 0]),
                            converged=bool(info[i, 3]))
    return tensors, alphas, report


def _file_alphas(meta, mods, lora_alpha):
    """Per-module lora_alpha of a source file: the metadata save_lora_weights writes, else the lora_alpha= argument."""
    if lora_alpha is not None:
        return {n: float(lora_alpha) for n in mods}
    if meta and "lora_alpha" in meta:
        table = ast.literal_eval(meta["lora_alpha"])
        missing = [n for n in mods if n not in table]
        if missing:
            raise ValueError(f"resize_lora_file: the file's lora_alpha metadata lacks {missing[:4]}")
        return {n: float(table[n]) for n in mods}
    raise ValueError("resize_lora_file: the file carries no lora_alpha metadata; pass lora_alpha=")


def resize_lora_file(src, dst, new_rank, dynamic_method=None, dynamic_param=None, uniform=True, lora_alpha=None, device="cuda"):
    """A safetensors file or folder -> a safetensors file or folder at the new rank, keys in the style each module had in the
    source, per-module lora_alpha metadata in the form save_lora_weights writes.  The source alphas come from that metadata, or
    from lora_alpha= when the file has none.  Returns the report of resize_pairs."""
    from safetensors import safe_open
    from safetensors.torch import save_file

    from .lora_io import WEIGHT_NAME, _normalise
    if os.path.isdir(src):
        src = os.path.join(src, WEIGHT_NAME)
    sd = {}
    with safe_open(src, framework="pt") as f:
        meta = f.metadata() or {}
        for k in f.keys():
            sd[k] = f.get_tensor(k)
    mods = _normalise(sd)
    if not mods or any("A" not in ab or "B" not in ab for ab in mods.values()):
        raise ValueError(f"resize_lora_file: no complete LoRA pairs recognised in {src}")
    keys = {}                                   # module -> (key of A, key of B) as the source spells them
    for k in sd:
        for n, ab in _normalise({k: sd[k]}).items():
            a, b = keys.get(n, (None, None))
            keys[n] = (k, b) if "A" in ab else (a, k)
    alphas_src = _file_alphas(meta, mods, lora_alpha)
    pairs, chunks, off = [], [], 0
    for n, ab in mods.items():
        A, B = ab["A"].to(torch.float32), ab["B"].to(torch.float32)
        r, nin = A.shape
        nout = B.shape[0]
        if B.shape[1] != r:
            raise ValueError(f"resize_lora_file: {n!r}: lora_A is {tuple(A.shape)}, lora_B is {tuple(B.shape)}")
        oa, ob = off, off + _align(A.numel())
        off = ob + _align(B.numel())
        pairs.append((n, oa, ob, int(r), int(nin), int(nout), alphas_src[n] / r))
        chunks.append((oa, A, ob, B))
    host = torch.zeros(off, dtype=torch.float32)
    for oa, A, ob, B in chunks:
        host[oa:oa + A.numel()] = A.reshape(-1)
        host[ob:ob + B.numel()] = B.reshape(-1)
    tensors, alphas, report = resize_pairs(host.to(device), pairs, new_rank, dynamic_method, dynamic_param, uniform)
    out = {}
    for n, (A2, B2) in tensors.items():
        ka, kb = keys[n]
        out[ka], out[kb] = A2.cpu().contiguous(), B2.cpu().contiguous()
    if os.path.isdir(dst) or not str(dst).endswith(".safetensors"):
        os.makedirs(dst, exist_ok=True)
        dst = os.path.join(dst, WEIGHT_NAME)
    save_file(out, dst, metadata={"format": "pt", "lora_alpha": repr({n: str(a) for n, a in alphas.items()})})
    return report


@torch.no_grad()
def resize_adapter(dit, new_rank, adapter_name="resized", dynamic_method=None, dynamic_param=None):
    """Re-express the model's active adapter at the new rank as a NEW named adapter and make it the active one: uniform=True (one
    rank for every module, r_dst = the largest rank chosen), LoraConfig(r=r_dst, lora_alpha=scaling * r_dst, target_modules=the
    same modules).  The old adapter keeps its weights (and its place in the flat store).  Returns the report of resize_pairs."""
    store = _store_of(dit)
    pairs = adapter_pairs(store)
    if not pairs:
        raise ValueError("resize_adapter: the model has no adapters")
    mods = {n: m for n, m in dit.named_modules() if isinstance(m, QfxLoraLinear)}
    if any(adapter_name in m.lora_A for m in mods.values()):
        raise ValueError(f"resize_adapter: an adapter named {adapter_name!r} exists already")
    tensors, alphas, report = resize_pairs(store.pflat, pairs, new_rank, dynamic_method, dynamic_param, uniform=True)
    r_dst = next(iter(report.values()))["new_rank"]
    for name, (A2, B2) in tensors.items():
        m = mods[name]
        m.r[adapter_name], m.lora_alpha[adapter_name] = r_dst, alphas[name]
        m.scaling[adapter_name] = alphas[name] / r_dst
        m.lora_A[adapter_name] = _W(A2.clone(), True)
        m.lora_B[adapter_name] = _W(B2.clone(), True)
    same = len(set(alphas.values())) == 1
    cfg = LoraConfig(r=r_dst, lora_alpha=next(iter(alphas.values())) if same else r_dst, target_modules=list(tensors))
    if not same:
        cfg.alpha_pattern = dict(alphas)        # peft's field for per-module alphas
    if not isinstance(getattr(dit, "peft_config", None), dict):
        dit.peft_config = {}
    dit.peft_config[adapter_name] = cfg
    dit._invalidate()
    dit._adapter_gen += 1
    dit._lora.tag()
    dit.set_adapter(adapter_name)
    return report
