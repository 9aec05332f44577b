#!/usr/bin/env python
"""qfx_adafactor_step (factored second moments, one workgroup per tensor, three sweeps) against qfx_adamw_step (elementwise, fp32
moments) on the headline LoRA parameter set: Qwen-Image, 60 blocks, r = 16, to_q / to_k / to_v / to_out.0 (A 16 x 3072 and
B 3072 x 16 each: 23.6 M parameters in 480 tensors).  The variants (AdamW, Adafactor with the package's defaults, Adafactor with
beta1 = 0.9) run same-box, interleaved round by round (device events around `iters` launches of one variant per round), on the
same gradient buffer.  Also records the state bytes of each form.  Writes the record to --out (default adafactor_step.json;
committed as profiles/adafactor_step.json).  Reported, not gated."""
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
    shapes = [(16, 3072), (3072, 16)] * (60 * 4)
    ents, off = [], 0
    for s in shapes:
        ents.append((off, s))
        off += (s[0] * s[1] + 63) // 64 * 64
    n = off
    torch.manual_seed(0)
    p = torch.randn(n, device=DEV) * 0.02
    g = torch.randn(n, device=DEV) * 1e-3
    gn = torch.zeros((), device=DEV)
    parts = torch.zeros(1024, device=DEV)
    ops.sumsq_det(g, gn, parts)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    lay = ops.adafactor_table(ents, device=DEV)
    z = lambda k: torch.zeros(max(1, k), device=DEV)
    af = {name: dict(row=z(lay.n_row), col=z(lay.n_col), v=z(lay.n_v), rms=z(lay.n_tensors), m=torch.zeros(n, device=DEV) if b1 else None,
                     beta1=b1) for name, b1 in (("adafactor", None), ("adafactor_beta1", 0.9))}
    names = ["adamw", "adafactor", "adafactor_beta1"]
    pw = {k: p.clone() for k in names}
    step = {"t": 1}

    def run(name):
        if name == "adamw":
            ops.adamw_step(pw[name], g, m, v, 1e-4, 0.9, 0.999, 1e-8, 0.0, step["t"], gnorm_sq=gn, max_norm=1.0)
        else:
            s = af[name]
            ops.adafactor_step(pw[name], g, s["row"], s["col"], s["v"], s["m"], s["rms"], lay, step["t"], beta1=s["beta1"], gnorm_sq=gn,
                               max_norm=1.0)

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
    nparam = sum(a * b for a, b in shapes)
    res = {"what": "optimizer launch alone, headline LoRA set (Qwen 60 blocks, r=16, 4 attention targets)", "params": nparam,
           "tensors": len(shapes), "flat_elements": n, "rounds": rounds, "iters_per_round": iters,
           "order": "interleaved, alternating per round", "variants": {}}
    # bytes per parameter that must cross HBM once (p read + write, g read, moments read + write); Adafactor re-reads g and p from L2
    hbm = {"adamw": 28, "adafactor": 12, "adafactor_beta1": 20}
    for name in names:
        t = times[name]
        med = statistics.median(t)
        res["variants"][name] = {"median_us": med, "min_us": min(t), "max_us": max(t), "per_round_us": t,
                                 "hbm_bytes_per_param": hbm[name], "achieved_TBps_of_that": hbm[name] * nparam / (med * 1e-6) / 1e12}
    res["state_bytes"] = {"adamw_fp32_moments": 2 * 4 * nparam, "adafactor": 4 * (lay.n_row + lay.n_col + lay.n_tensors),
                          "adafactor_beta1": 4 * (lay.n_row + lay.n_col + lay.n_tensors + nparam)}
    res["ratio_median_vs_adamw"] = {k: res["variants"][k]["median_us"] / res["variants"]["adamw"]["median_us"] for k in names}
    res["finite"] = {k: bool(torch.isfinite(pw[k]).all()) for k in names}
    res["device"] = torch.cuda.get_device_name(0)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v["median_us"] for k, v in res["variants"].items()}), json.dumps(res["state_bytes"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="adafactor_step.json", help="where the JSON record is written")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    main(a.out, a.rounds, a.iters)
