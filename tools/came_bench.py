#!/usr/bin/env python
"""What optimizer="came" costs: (1) the headline training step (bench.py's model, batch 1, 512 x 512, r = 16) with optimizer="came"
against optimizer="adamw" and optimizer="adafactor" -- one model in one process, one QwenLoraTrainStep per family over it, the runs
alternate between the families (order reversed every other run), host clock around steps that end in a device synchronise; (2) the
stand-alone time of the ONE qfx_came_step launch on the headline adapter set (480 tensors, A 16 x 3072 and B 3072 x 16 each: 23.6 M
parameters) against qfx_adafactor_step with beta1 = 0.9 and qfx_adamw_step, interleaved round by round, device events around
`iters` launches per round, on the same gradient buffer.

Writes the record to --out (default came.json; committed as profiles/came.json, whose "parity" key is written by the parity run of
tests/test_came_gpu.py and kept when this tool rewrites the file).  Reported, not gated."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen-image-finetune_amd"))

DEV = "cuda:0"


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def launch_bench(rounds, iters):
    from qflux_amd import ops
    shapes = [(16, 3072), (3072, 16)] * (60 * 4)
    ents, off = [], 0
    for s in shapes:
        ents.append((off, s))
        off += (s[0] * s[1] + 63) // 64 * 64
    n = off
    torch.manual_seed(0)
    g = torch.randn(n, device=DEV) * 1e-3
    gn, parts = torch.zeros((), device=DEV), torch.zeros(1024, device=DEV)
    ops.sumsq_det(g, gn, parts)
    z = lambda k: torch.zeros(max(1, k), device=DEV)
    P = lambda: torch.randn(n, device=DEV) * 0.02
    cl, al = ops.came_table(ents, device=DEV), ops.adafactor_table(ents, device=DEV)
    c = dict(p=P(), row=z(cl.n_row), col=z(cl.n_col), rrow=z(cl.n_row), rcol=z(cl.n_col), v=z(cl.n_v), rms=z(cl.n_tensors), m=z(n))
    a = dict(p=P(), row=z(al.n_row), col=z(al.n_col), v=z(al.n_v), rms=z(al.n_tensors), m=z(n))
    w = dict(p=P(), m=z(n), v=z(n))
    count = {"came": 0, "adafactor_beta1": 0, "adamw": 0}

    def run(name):
        count[name] += 1
        if name == "came":
            ops.came_step(c["p"], g, c["row"], c["col"], c["rrow"], c["rcol"], c["v"], c["m"], c["rms"], cl, 1e-4, gnorm_sq=gn, max_norm=1.0)
        elif name == "adafactor_beta1":
            ops.adafactor_step(a["p"], g, a["row"], a["col"], a["v"], a["m"], a["rms"], al, count[name], lr=1e-4, relative_step=False,
                               beta1=0.9, gnorm_sq=gn, max_norm=1.0)
        else:
            ops.adamw_step(w["p"], g, w["m"], w["v"], 1e-4, 0.9, 0.999, 1e-8, 0.01, count[name], gnorm_sq=gn, max_norm=1.0)

    names = list(count)
    for name in names:
        for _ in range(10):
            run(name)
    torch.cuda.synchronize()
    us = {k: [] for k in names}
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                run(name)
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) / iters * 1e3)
    assert all(bool(torch.isfinite(x["p"]).all()) for x in (c, a, w))
    med = {k: statistics.median(v) for k, v in us.items()}
    # bytes the algorithm needs from HBM per launch: p read + written, g read, m read + written (the vectors are noise next to them)
    return {"what": "one launch over the headline adapter set, device events around `iters` launches, interleaved rounds",
            "tensors": len(shapes), "parameters": sum(s[0] * s[1] for s in shapes), "rounds": rounds, "iters_per_round": iters,
            "us_per_launch": {k: spread(v) for k, v in us.items()}, "came_over_adafactor_beta1": med["came"] / med["adafactor_beta1"],
            "came_over_adamw": med["came"] / med["adamw"], "came_min_hbm_bytes": 5 * 4 * sum(s[0] * s[1] for s in shapes),
            "came_min_hbm_TBps_at_median": 5 * 4 * sum(s[0] * s[1] for s in shapes) / (med["came"] * 1e-6) / 1e12}


def step_bench(a):
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.modules import LoraConfig
    from qflux_amd.trainer import QwenLoraTrainStep
    dev = torch.device(DEV)
    torch.manual_seed(1234)
    with torch.device(dev):
        dit = QwenImageTransformer2DModel(num_layers=a.layers)
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
    dit.add_adapter(LoraConfig(r=a.rank, lora_alpha=a.rank, init_lora_weights="gaussian"), "default", generator=torch.Generator().manual_seed(1234))
    side, T, Jd = a.res // 16, 384, dit.config.joint_attention_dim
    emb = dict(image_latents=torch.randn(1, side * side, 64).half().to(dev), control_latents=torch.randn(1, side * side, 64).half().to(dev),
               prompt_embeds=(torch.randn(1, T, Jd) * 4).half().to(dev), prompt_embeds_mask=None, img_shapes=[[(1, side, side), (1, side, side)]])
    steps = {"adamw": QwenLoraTrainStep(dit, lr=1e-4, max_grad_norm=1.0),
             "adafactor": QwenLoraTrainStep(dit, lr=None, max_grad_norm=1.0, optimizer="adafactor"),
             "came": QwenLoraTrainStep(dit, lr=1e-4, max_grad_norm=1.0, optimizer="came")}
    names = list(steps)
    for name in names:
        for _ in range(a.warmup):
            steps[name].train_step(emb)
    torch.cuda.synchronize()
    ms = {k: [] for k in names}
    for r in range(a.runs):
        for name in (names if r % 2 == 0 else names[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = steps[name].train_step(emb)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dit.lora_store.pflat).all())
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"what": "the headline step (batch 1) under three optimizer families on one model, alternating runs, host clock around steps "
                    "that end in a device synchronise", "layers": a.layers, "rank": a.rank, "res": a.res, "batch": 1, "runs_each": a.runs,
            "steps_per_run": a.steps, "warmup_steps_each": a.warmup, "ms_per_step": {k: spread(v) for k, v in ms.items()},
            "came_minus_adamw_ms_median": med["came"] - med["adamw"], "came_minus_adafactor_ms_median": med["came"] - med["adafactor"],
            "adamw_run_to_run_spread_ms": max(ms["adamw"]) - min(ms["adamw"])}


def main(a):
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res["device"] = torch.cuda.get_device_name(0)
    res["launch"] = launch_bench(a.rounds, a.iters)
    print(json.dumps({k: v["median"] for k, v in res["launch"]["us_per_launch"].items()}))
    if not a.no_step:
        res["step"] = step_bench(a)
        print(json.dumps({k: v["median"] for k, v in res["step"]["ms_per_step"].items()}))
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="came.json", help="where the JSON record is written (an existing record's other keys are kept)")
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-step", action="store_true", help="only the stand-alone launch timing")
    main(ap.parse_args())
