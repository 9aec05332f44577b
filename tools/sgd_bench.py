#!/usr/bin/env python
"""qfx_sgd_step (torch.optim.SGD with momentum: 20 bytes per parameter) against qfx_adamw_step (fp32 moments: 28 bytes) on the
headline LoRA parameter set: Qwen-Image, 60 blocks, r = 16, to_q / to_k / to_v / to_out.0 (23.6 M parameters).  The variants run
same-box, interleaved round by round (device events around `iters` launches of one variant per round), on the same gradient buffer
and with the fused clip active.  Writes the record to --out (default sgd_step.json; committed as profiles/sgd_step.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen-image-finetune_amd"))
from qflux_amd import ops  # noqa: E402

DEV = "cuda:0"


def main(out, rounds=15, iters=50):
    n = 16 * 3072 * (60 * 4 * 2)
    torch.manual_seed(0)
    p = torch.randn(n, device=DEV) * 0.02
    g = torch.randn(n, device=DEV) * 1e-3
    gn = torch.zeros((), device=DEV)
    parts = torch.zeros(1024, device=DEV)
    ops.sumsq_det(g, gn, parts)
    m, v, buf = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    names = ["adamw", "sgd_momentum", "sgd_plain"]
    pw = {k: p.clone() for k in names}
    step = {"t": 1}

    def run(name):
        if name == "adamw":
            ops.adamw_step(pw[name], g, m, v, 1e-4, 0.9, 0.999, 1e-8, 0.0, step["t"], gnorm_sq=gn, max_norm=1.0)
        elif name == "sgd_momentum":      # the documented setting: momentum 0.9, weight_decay 1e-4
            ops.sgd_step(pw[name], g, buf, 1e-4, 0.9, 0.0, 1e-4, False, first=False, gnorm_sq=gn, max_norm=1.0)
        else:
            ops.sgd_step(pw[name], g, None, 1e-4, gnorm_sq=gn, max_norm=1.0)

    for name in names:                       # warm-up: code objects, first-touch of every buffer
        for _ in range(5):
            run(name)
    torch.cuda.synchronize()
    times = {k: [] for k in names}
    for r in range(rounds):
        order = names if r % 2 == 0 else names[::-1]
        for name in order:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                run(name)
                step["t"] += 1
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / iters * 1e3)
    res = {"what": "optimizer launch alone, headline LoRA set (Qwen 60 blocks, r=16, 4 attention targets)", "params": n,
           "rounds": rounds, "iters_per_round": iters, "order": "interleaved, alternating per round", "variants": {}}
    bytes_moved = {"adamw": 28, "sgd_momentum": 20, "sgd_plain": 12}
    for name in names:
        t = times[name]
        med = statistics.median(t)
        res["variants"][name] = {"median_us": med, "min_us": min(t), "max_us": max(t), "per_round_us": t,
                                 "bytes_per_param": bytes_moved[name], "achieved_TBps": bytes_moved[name] * n / (med * 1e-6) / 1e12}
    res["ratio_median_vs_adamw"] = {k: res["variants"][k]["median_us"] / res["variants"]["adamw"]["median_us"] for k in names}
    res["expected_ratio_by_bytes"] = {k: bytes_moved[k] / 28 for k in names}
    res["device"] = torch.cuda.get_device_name(0)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v["median_us"] for k, v in res["variants"].items()}), json.dumps(res["ratio_median_vs_adamw"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="sgd_step.json", help="where the JSON record is written")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    main(a.out, a.rounds, a.iters)
