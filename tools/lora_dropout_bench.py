#!/usr/bin/env python
"""What network_dropout / rank_dropout cost the headline training step: the extra launches (one qfx_lora_dropout_advance per forward,
one batched qfx_lora_dropout_apply behind every rank-r producer flush: 4 per block and pass position with the default targets) on
bench.py's model, batch and resolution.

One model in one process; the plan without the option and the plan with it live side by side in the plan cache (on / off is part
of its key), and the runs alternate between them (order reversed every other run), host clock around steps that end in a device
synchronise.  "off" runs exactly the parent commit's launch programs (tests/golden/plan_fingerprints.json), so its run-to-run
spread is the parent's own on this machine.  Also: the option on but inactive (eval(): the launches return at once), which
separates launch overhead from the kernels' work.

Writes the record to --out (default lora_dropout.json; committed as profiles/lora_dropout.json)."""
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


def main(a):
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
    step = QwenLoraTrainStep(dit, lr=1e-4, max_grad_norm=1.0)
    state = dit.set_lora_dropout(a.network_dropout, a.rank_dropout, seed=1234)

    def select(name):      # both plans stay cached: the key holds on / off, the "on" plan holds the state's address
        dit._dropout = None if name == "off" else state
        state.enabled = name != "on_inactive"

    names = ["off", "on", "on_inactive"]
    for name in names:
        select(name)
        for _ in range(a.warmup):
            step.train_step(emb)
    torch.cuda.synchronize()
    select("on")
    plan = dit.get_plan(1, 2 * side * side, T, emb["img_shapes"], None)
    launches = {k: sum(1 for prog in (plan.fwd, plan.bwd) for e in prog.calls if e[0] is not None and e[0].__name__ == k)
                for k in ("qfx_lora_dropout_apply", "qfx_lora_dropout_advance")}
    total = sum(len(prog.calls) for prog in (plan.fwd, plan.bwd))
    ms = {k: [] for k in names}
    for r in range(a.runs):
        for name in (names if r % 2 == 0 else names[::-1]):
            select(name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step.train_step(emb)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"what": "the headline step without network_dropout / rank_dropout (the parent's launch programs), with them, and with them "
                   "switched off by eval()", "device": torch.cuda.get_device_name(0), "layers": a.layers, "rank": a.rank, "res": a.res,
           "batch": 1, "network_dropout": a.network_dropout, "rank_dropout": a.rank_dropout, "runs_each": a.runs, "steps_per_run": a.steps,
           "warmup_steps_each": a.warmup, "order": "alternating, reversed every other run", "dropout_launches_per_step": launches,
           "program_entries_with_dropout": total, "ms_per_step": ms, "median_ms_per_step": med,
           "dropout_cost_ms_median": med["on"] - med["off"], "inactive_cost_ms_median": med["on_inactive"] - med["off"],
           "off_run_to_run_spread_ms": max(ms["off"]) - min(ms["off"]), "dropout_step_counter": state.step()}
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("median_ms_per_step", "dropout_cost_ms_median", "inactive_cost_ms_median",
                                          "off_run_to_run_spread_ms", "dropout_launches_per_step")}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="lora_dropout.json", help="where the JSON record is written")
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--network-dropout", type=float, default=0.1)
    ap.add_argument("--rank-dropout", type=float, default=0.1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    main(ap.parse_args())
