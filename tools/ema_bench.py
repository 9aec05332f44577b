#!/usr/bin/env python
"""The EMA launches on the headline LoRA parameter set (Qwen-Image, 60 blocks, r = 16, to_q / to_k / to_v / to_out.0: 23.59 M fp32
elements) and what EMA costs the headline training step.

Kernels: qfx_ema_update with 1 and with 4 shadows, qfx_ema_swap, and qfx_sf_swap as the yardstick -- csrc/qfx_schedulefree.hip is
the parent commit's file unchanged, and it moves 12 B per element like the one-shadow update.  All variants run in one process,
interleaved round by round (device events on the launch stream around `iters` launches of one variant per round, the order reversed
every other round).  Per variant: median / min / max microseconds per launch, achieved bytes per second from the bytes the
algorithm needs (4 + 8 n_shadows per element for the update, 16 for the swap, 12 for qfx_sf_swap), and the one-shadow update's
rate against qfx_sf_swap's with the yardstick's own round-to-round spread beside it.  One buffer of this set is 94 MB, so the
buffers of a launch fit the 256 MiB Infinity Cache together only for the two-buffer launches (one shadow, either swap), which the
timing loop repeats over the same buffers: their rates are what a launch right behind the optimizer's sees, not an HBM streaming
figure; the four-shadow update (472 MB) streams.

Step: the headline step (bench.py's model, batch and resolution) with ema_decay=0.999 against ema_decay=None, on one model in one
process, alternating `--step-runs` runs of `--steps` steps each, host clock around steps that end in a device synchronise.

Writes the record to --out (default ema.json; committed as profiles/ema.json).  --layers 0 skips the step part."""
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
HBM_TBPS = 8.0          # MI355X peak HBM3E bandwidth the fractions refer to


def kernels(rounds, iters):
    sizes = [16 * 3072] * (60 * 4 * 2)
    n = sum((k + 63) // 64 * 64 for k in sizes)
    torch.manual_seed(0)
    p = torch.randn(n, device=DEV) * 0.02
    mk = lambda: p + torch.randn(n, device=DEV) * 1e-3      # noqa: E731
    st = {"ema_update_1": (mk(),), "ema_update_4": tuple(mk() for _ in range(4)), "ema_swap": (p.clone(), mk()), "sf_swap": (p.clone(), mk())}
    bpe = {"ema_update_1": 12, "ema_update_4": 36, "ema_swap": 16, "sf_swap": 12}
    flip = {"v": False}

    def run(name):
        if name.startswith("ema_update"):
            ops.ema_update(p, list(st[name]), [1e-3] * len(st[name]))
        elif name == "ema_swap":
            ops.ema_swap(*st[name])
        else:
            ops.sf_swap(*st[name], 0.9, to_eval=flip["v"])      # there and back: the values stay bounded
            flip["v"] = not flip["v"]

    names = list(st)
    for name in names:                       # warm-up: code objects, first touch of every buffer
        for _ in range(6):
            run(name)
    torch.cuda.synchronize()
    times = {k: [] for k in names}
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                run(name)
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / iters * 1e3)
    out = {"flat_elements": n, "rounds": rounds, "iters_per_round": iters, "order": "interleaved, reversed every other round", "variants": {}}
    for name in names:
        t = times[name]
        med = statistics.median(t)
        rate = lambda us: bpe[name] * n / (us * 1e-6) / 1e9      # noqa: E731
        out["variants"][name] = {"median_us": med, "min_us": min(t), "max_us": max(t), "spread_us": max(t) - min(t), "per_round_us": t,
                                 "bytes_per_element": bpe[name], "bytes_per_launch": bpe[name] * n, "achieved_GBps": rate(med),
                                 "achieved_GBps_slowest_round": rate(max(t)), "achieved_GBps_fastest_round": rate(min(t)),
                                 "fraction_of_hbm_peak": rate(med) / 1e3 / HBM_TBPS}
    a, b = out["variants"]["ema_update_1"], out["variants"]["sf_swap"]
    out["update_1_against_sf_swap"] = {
        "ratio_GBps": a["achieved_GBps"] / b["achieved_GBps"], "delta_median_us": a["median_us"] - b["median_us"],
        "sf_swap_round_to_round_spread_us": b["spread_us"],
        "within_sf_swap_spread": b["achieved_GBps_slowest_round"] <= a["achieved_GBps"]}
    return out


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
    variants = {"ema_none": QwenLoraTrainStep(dit, lr=1e-4, max_grad_norm=1.0),
                "ema_0.999": QwenLoraTrainStep(dit, lr=1e-4, max_grad_norm=1.0, ema_decay=0.999)}
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
    base, ema = ms["ema_none"], ms["ema_0.999"]
    return {"layers": layers, "rank": rank, "res": res, "batch": 1, "flat_elements": dit.lora_store.pflat.numel(), "runs_each": runs,
            "steps_per_run": steps, "warmup_steps_each": warmup, "order": "alternating, reversed every other run",
            "ms_per_step": ms, "median_ms_per_step": {k: statistics.median(v) for k, v in ms.items()},
            "ema_cost_ms_median": statistics.median(ema) - statistics.median(base), "ema_none_run_to_run_spread_ms": max(base) - min(base),
            "ema_update_bytes_per_step": 12 * dit.lora_store.pflat.numel()}


def main(a):
    res = {"what": "EMA of the adapter weights: the update and swap launches on the headline LoRA set against qfx_sf_swap, and the headline "
                   "step with and without one shadow", "hbm_peak_TBps_assumed": HBM_TBPS, "device": torch.cuda.get_device_name(0)}
    res["kernels"] = kernels(a.rounds, a.iters)
    if a.layers > 0:
        res["step"] = step_cost(a.layers, a.rank, a.res, a.step_runs, a.steps, a.warmup)
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: [round(v["median_us"], 2), round(v["achieved_GBps"], 1)] for k, v in res["kernels"]["variants"].items()}),
          json.dumps(res["kernels"]["update_1_against_sf_swap"]),
          json.dumps({k: res["step"][k] for k in ("median_ms_per_step", "ema_cost_ms_median", "ema_none_run_to_run_spread_ms")}) if "step" in res else "")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="ema.json", help="where the JSON record is written")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--layers", type=int, default=60, help="DiT blocks of the step part (0: kernels only)")
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--step-runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    main(ap.parse_args())
