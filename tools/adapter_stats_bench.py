#!/usr/bin/env python
"""The two adapter-statistics launches (qfx_adapter_stats, phase 0 and phase 1) against the AdamW launch on the same buffers, and
what adapter_stats_every=1 costs the headline training step.

Layout: "headline" -- Qwen-Image, 60 blocks, r = 16, to_q / to_k / to_v / to_out.0 (BASELINE.json configs[1]): 480 adapter tensors
of 16 x 3072 elements as LoraStore packs them.

Kernels, all in one process, interleaved round by round (device events on the launch stream around `iters` launches of one variant
per round, the order reversed every other round): phase 0 alone, phase 1 alone, the optimizer launches of the train step's
optimizer_step alone (qfx_sumsq_det + qfx_adamw_step: the parent commit's files unchanged, so this is the parent's optimizer step on
the same machine), and the optimizer launches bracketed by the two phases.  Per variant: median / min / max microseconds, beside the
bytes each phase moves (phase 0: g and p read, prev written; phase 1: p and prev read).

Step: the headline step (bench.py's model, batch and resolution) with adapter_stats_every 0 against 1, on one model in one process,
alternating runs, host clock around steps that end in a device synchronise.  With the option at 0 the step launches exactly what
the parent commit launches, so the "0" column is the parent's step time from the same run; its run-to-run spread is reported
beside the cost.  One read of last_adapter_stats is timed apart (the only host synchronisation of the feature).

Writes the record to --out (default adapter_stats.json; committed as profiles/adapter_stats.json).  --layers 0 skips the step part."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen-image-finetune_amd"))
from qflux_amd import ops  # noqa: E402

DEV = "cuda:0"
LAYOUTS = {"headline": (16, [(3072, 3072)] * 4, 60)}


def build(name):
    """(off, numel) of every adapter tensor of one layout as LoraStore packs it (A then B per pair, padded to 64 floats)."""
    r, shapes, blocks = LAYOUTS[name]
    entries, off = [], 0
    for _ in range(blocks):
        for nin, nout in shapes:
            for k in (r * nin, nout * r):
                entries.append((off, k))
                off += (k + 63) // 64 * 64
    return entries, off


def kernels(name, rounds, iters):
    entries, n = build(name)
    lay = ops.stats_table_entries(entries, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    p = torch.randn(n, device=DEV, generator=g) * 0.02
    g_ = torch.randn(n, device=DEV, generator=g) * 1e-3
    m1, v, prev = (torch.zeros(n, device=DEV) for _ in range(3))
    out = torch.zeros(32 * lay.n_entries, dtype=torch.uint8, device=DEV)
    gnorm, gparts = torch.zeros((), device=DEV), torch.zeros(1024, device=DEV)

    def opt():      # lr = 0: the weights stay where they are, the launches move the same bytes
        ops.sumsq_det(g_, gnorm, gparts)
        ops.adamw_step(p, g_, m1, v, 0.0, 0.9, 0.999, 1e-8, 0.0, 1, gnorm, 1.0, 1.0)

    def phase0():
        ops.adapter_stats(p, g_, prev, lay, out, 0, gnorm, 1.0, 1.0)

    def phase1():
        ops.adapter_stats(p, None, prev, lay, out, 1)

    variants = {"stats_phase0": phase0, "stats_phase1": phase1, "optimizer_launches": opt,
                "optimizer_launches_bracketed": lambda: (ops.sumsq_det(g_, gnorm, gparts), phase0(),
                                                         ops.adamw_step(p, g_, m1, v, 0.0, 0.9, 0.999, 1e-8, 0.0, 1, gnorm, 1.0, 1.0), phase1())}
    names = list(variants)
    for k in names:
        for _ in range(3):
            variants[k]()
    torch.cuda.synchronize()
    times = {k: [] for k in names}
    for r in range(rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                variants[k]()
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / iters * 1e3)
    med = {k: statistics.median(t) for k, t in times.items()}
    elems = sum(k for _, k in entries)
    return {"layout": name, "rank": LAYOUTS[name][0], "tensors": len(entries), "flat_elements": n, "rounds": rounds, "iters_per_round": iters,
            "order": "interleaved, reversed every other round",
            "bytes": {"stats_phase0": 12 * elems, "stats_phase1": 8 * elems, "qfx_adamw_step": 28 * elems},
            "variants_us": {k: {"median": med[k], "min": min(t), "max": max(t), "per_round": t} for k, t in times.items()},
            "phase0_GBps_median": 12 * elems / med["stats_phase0"] * 1e-3, "phase1_GBps_median": 8 * elems / med["stats_phase1"] * 1e-3,
            "stats_around_optimizer_us_median": med["optimizer_launches_bracketed"] - med["optimizer_launches"],
            "stats_over_optimizer_launches": (med["stats_phase0"] + med["stats_phase1"]) / med["optimizer_launches"]}


def step_cost(layers, rank, res, runs, steps, warmup):
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.modules import LoraConfig
    from qflux_amd.trainer import QwenLoraTrainStep
    dev = torch.device(DEV)
    torch.manual_seed(1234)
    with torch.device(dev):
        dit = QwenImageTransformer2DModel(num_layers=layers)
    with torch.no_grad():
        for n, p in dit.named_parameters():
            if p.ndim == 2:
                p.normal_(0.0, 0.02)
            elif "norm" in n:
                p.fill_(1.0)
            elif ".img_mod." in n or ".txt_mod." in n or "norm_out" in n:
                p.normal_(0.0, 0.02)
            else:
                p.zero_()
    dit.add_adapter(LoraConfig(r=rank, lora_alpha=rank, init_lora_weights="gaussian"), "default", generator=torch.Generator().manual_seed(1234))
    side, T, Jd = res // 16, 384, dit.config.joint_attention_dim
    emb = dict(image_latents=torch.randn(1, side * side, 64).half().to(dev), control_latents=torch.randn(1, side * side, 64).half().to(dev),
               prompt_embeds=(torch.randn(1, T, Jd) * 4).half().to(dev), prompt_embeds_mask=None, img_shapes=[[(1, side, side), (1, side, side)]])
    variants = {"adapter_stats_every_0": QwenLoraTrainStep(dit, lr=1e-4, max_grad_norm=1.0),
                "adapter_stats_every_1": QwenLoraTrainStep(dit, lr=1e-4, max_grad_norm=1.0, adapter_stats_every=1)}
    for s in variants.values():
        for _ in range(warmup):
            s.train_step(emb)
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for r in range(runs):
        for name in (list(variants) if r % 2 == 0 else list(variants)[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                variants[name].train_step(emb)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    on = variants["adapter_stats_every_1"]
    on.train_step(emb)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = on.last_adapter_stats
    read_ms = (time.perf_counter() - t0) * 1e3
    base, cost = ms["adapter_stats_every_0"], ms["adapter_stats_every_1"]
    return {"layers": layers, "rank": rank, "res": res, "batch": 1, "tensors": len(stats), "runs_each": runs, "steps_per_run": steps,
            "warmup_steps_each": warmup, "order": "alternating, reversed every other run",
            "parent": "adapter_stats_every_0 launches exactly the parent commit's step: its column is the parent's step time in this run",
            "ms_per_step": ms, "median_ms_per_step": {k: statistics.median(v) for k, v in ms.items()},
            "adapter_stats_cost_ms_median": statistics.median(cost) - statistics.median(base),
            "parent_run_to_run_spread_ms": max(base) - min(base), "read_last_adapter_stats_ms": read_ms,
            "summary_of_the_last_step": on.adapter_stats_summary()}


def main(a):
    res = {"what": "per-adapter telemetry: the two qfx_adapter_stats launches alone and around the optimizer launches on the headline "
                   "adapter set, and the headline step with adapter_stats_every 0 and 1", "measured": True,
           "device": torch.cuda.get_device_name(0)}
    res["kernels"] = {name: kernels(name, a.rounds, a.iters) for name in a.layouts.split(",")}
    if a.layers > 0:
        res["step"] = step_cost(a.layers, a.rank, a.res, a.step_runs, a.steps, a.warmup)
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({n: {k: round(v["median"], 1) for k, v in r["variants_us"].items()} for n, r in res["kernels"].items()}),
          json.dumps({k: res["step"][k] for k in ("median_ms_per_step", "adapter_stats_cost_ms_median", "parent_run_to_run_spread_ms",
                                                  "read_last_adapter_stats_ms")}) if "step" in res else "")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="adapter_stats.json", help="where the JSON record is written")
    ap.add_argument("--layouts", default="headline")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--layers", type=int, default=60, help="DiT blocks of the step part (0: kernels only)")
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--step-runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    main(ap.parse_args())
