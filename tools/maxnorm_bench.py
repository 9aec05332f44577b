#!/usr/bin/env python
"""The max-norm launch (qfx_maxnorm_apply, kohya's --scale_weight_norms) alone and behind the AdamW launch, and what it costs the
headline training step.

Layouts: "headline" -- Qwen-Image, 60 blocks, r = 16, to_q / to_k / to_v / to_out.0: 240 pairs of 3072 x 3072; "all_linear_r64" --
every linear of the 60 double blocks at r = 64: per block eight 3072 x 3072, two 3072 -> 12288, two 12288 -> 3072 and the two
3072 -> 18432 modulation linears, 840 pairs.  Weights are drawn so that the norms spread around the threshold: "scale_half" scales
about half of the pairs (and writes them), "measure" (threshold inf) writes nothing.

Variants per layout, all in one process, interleaved round by round (device events on the launch stream around `iters` launches of
one variant per round, the order reversed every other round): the max-norm launch alone (both thresholds), the optimizer launches of
the train step's optimizer_step alone (qfx_sumsq_det + qfx_adamw_step: the parent commit's files unchanged, so this is the parent's
optimizer step on the same machine), and the two together.  Per variant: median / min / max microseconds.  Beside them the counts the
algorithm needs: bytes read (and written when a pair is scaled) and fp64 multiply-adds of the Gram matrices' upper-triangle blocks.

Step: the headline step (bench.py's model, batch and resolution) with max_weight_norm against None, on one model in one process,
alternating runs, host clock around steps that end in a device synchronise.

Writes the record to --out (default max_norm.json; committed as profiles/max_norm.json).  --layers 0 skips the step part."""
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
LAYOUTS = {"headline": (16, [(3072, 3072)] * 4, 60),
           "all_linear_r64": (64, [(3072, 3072)] * 8 + [(3072, 12288)] * 2 + [(12288, 3072)] * 2 + [(3072, 18432)] * 2, 60)}


def build(name):
    """The flat buffer of one layout as LoraStore packs it (A then B per pair, every tensor padded to 64 floats) and the table."""
    r, shapes, blocks = LAYOUTS[name]
    rows, off = [], 0
    for _ in range(blocks):
        for nin, nout in shapes:
            off_a = off
            off += (r * nin + 63) // 64 * 64
            off_b = off
            off += (nout * r + 63) // 64 * 64
            rows.append((off_a, off_b, r, nin, nout, 1.0))
    g = torch.Generator(device=DEV).manual_seed(0)
    p = torch.randn(off, device=DEV, generator=g) * 0.02
    for i, (off_a, off_b, r, nin, nout, _) in enumerate(rows):      # spread the norms: B of pair i times 0.5 .. 2
        p[off_b:off_b + nout * r] *= 0.5 * 4 ** (i % 16 / 15)
    return p, ops.maxnorm_table(rows, device=DEV, n_elems=off), rows


def counts(rows, scaled):
    T = lambda r: 4 if r <= 64 else 8                                            # noqa: E731
    blocks = lambda r: ((r + T(r) - 1) // T(r)) * ((r + T(r) - 1) // T(r) + 1) // 2   # noqa: E731
    elems = [r * (nin + nout) for _, _, r, nin, nout, _ in rows]
    return {"pairs": len(rows), "bytes_read": 4 * sum(elems), "bytes_written": 4 * sum(e for e, s in zip(elems, scaled) if s),
            "fp64_multiply_adds": sum(blocks(r) * T(r) ** 2 * (nin + nout) for _, _, r, nin, nout, _ in rows),
            "product_multiply_adds_avoided": sum(r * nin * nout for _, _, r, nin, nout, _ in rows)}


def kernels(name, rounds, iters):
    p0, lay, rows = build(name)
    n = p0.numel()
    norms, ratios, summary = (torch.zeros(k, device=DEV) for k in (lay.n_pairs, lay.n_pairs, 4))
    ops.maxnorm_apply(p0.clone(), lay, float("inf"), norms, ratios, summary)
    raw = norms.clone()
    m = float(raw.median())
    p, g_, m1, v = p0.clone(), torch.randn(n, device=DEV) * 1e-3, torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    gnorm, gparts = torch.zeros((), device=DEV), torch.zeros(1024, device=DEV)

    def opt():      # lr = 0: the weights stay where they are, the launches move the same bytes
        ops.sumsq_det(g_, gnorm, gparts)
        ops.adamw_step(p, g_, m1, v, 0.0, 0.9, 0.999, 1e-8, 0.0, 1, gnorm, 1.0, 1.0)

    def clamp(thr):
        ops.maxnorm_apply(p, lay, thr, norms, ratios, summary)

    def scale_half():      # from the same weights every time: about half of the pairs are scaled and written
        p.copy_(p0)
        clamp(m)

    variants = {"copy_only": lambda: p.copy_(p0), "maxnorm_measure": lambda: clamp(float("inf")), "copy+maxnorm_scale_half": scale_half,
                "optimizer_launches": opt, "optimizer_launches+maxnorm_measure": lambda: (opt(), clamp(float("inf")))}
    names = list(variants)
    for k in names:
        for _ in range(3):
            variants[k]()
    torch.cuda.synchronize()
    scale_half()
    scaled = (ratios != 1).tolist()
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
    return {"layout": name, "rank": LAYOUTS[name][0], "flat_elements": n, "threshold": m, "pairs_scaled_at_threshold": sum(scaled),
            "rounds": rounds, "iters_per_round": iters, "order": "interleaved, reversed every other round",
            "counts_measure": counts(rows, [False] * len(rows)), "counts_scale_half": counts(rows, scaled),
            "variants_us": {k: {"median": med[k], "min": min(t), "max": max(t), "per_round": t} for k, t in times.items()},
            "maxnorm_scale_half_us_median_minus_copy": med["copy+maxnorm_scale_half"] - med["copy_only"],
            "maxnorm_behind_optimizer_us_median": med["optimizer_launches+maxnorm_measure"] - med["optimizer_launches"],
            "maxnorm_over_optimizer_launches": med["maxnorm_measure"] / med["optimizer_launches"]}


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
    variants = {"none": QwenLoraTrainStep(dit, lr=1e-4, max_grad_norm=1.0),
                "max_weight_norm_1.0": QwenLoraTrainStep(dit, lr=1e-4, max_grad_norm=1.0, max_weight_norm=1.0)}
    opt_ms = []
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
    for _ in range(runs):       # optimizer_step of the step without the option: the parent commit's, on this machine
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            variants["none"].optimizer_step()
        torch.cuda.synchronize()
        opt_ms.append((time.perf_counter() - t0) / steps * 1e3)
    base, on = ms["none"], ms["max_weight_norm_1.0"]
    return {"layers": layers, "rank": rank, "res": res, "batch": 1, "pairs": len(variants["max_weight_norm_1.0"].last_weight_norms.names),
            "runs_each": runs, "steps_per_run": steps, "warmup_steps_each": warmup, "order": "alternating, reversed every other run",
            "ms_per_step": ms, "median_ms_per_step": {k: statistics.median(v) for k, v in ms.items()},
            "max_weight_norm_cost_ms_median": statistics.median(on) - statistics.median(base),
            "none_run_to_run_spread_ms": max(base) - min(base),
            "optimizer_step_without_the_option_ms": opt_ms, "weight_norm_stats": variants["max_weight_norm_1.0"].weight_norm_stats()}


def main(a):
    res = {"what": "max-norm regularisation of the adapters: qfx_maxnorm_apply alone and behind the optimizer launches on two layouts, "
                   "and the headline step with and without max_weight_norm", "device": torch.cuda.get_device_name(0)}
    res["kernels"] = {name: kernels(name, a.rounds, a.iters if name == "headline" else max(1, a.iters // 10)) for name in a.layouts.split(",")}
    if a.layers > 0:
        res["step"] = step_cost(a.layers, a.rank, a.res, a.step_runs, a.steps, a.warmup)
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({n: {k: round(v["median"], 1) for k, v in r["variants_us"].items()} for n, r in res["kernels"].items()}),
          json.dumps({k: res["step"][k] for k in ("median_ms_per_step", "max_weight_norm_cost_ms_median", "none_run_to_run_spread_ms",
                                                  "optimizer_step_without_the_option_ms")}) if "step" in res else "")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="max_norm.json", help="where the JSON record is written")
    ap.add_argument("--layouts", default="headline,all_linear_r64")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--layers", type=int, default=60, help="DiT blocks of the step part (0: kernels only)")
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--step-runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    main(ap.parse_args())
