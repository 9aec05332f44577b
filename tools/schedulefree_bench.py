#!/usr/bin/env python
"""qfx_sfadamw_step (Schedule-Free AdamW: y, z and exp_avg_sq read and written, g read) against qfx_adamw_step (p, m and v read and
written, g read) at the headline adapter size: 23 592 960 fp32 elements (Qwen-Image, 60 blocks, r = 16, to_q / to_k / to_v /
to_out.0).  Both move the same seven arrays, 28 B per element.  The two run in one process, interleaved round by round (device
events around `iters` launches of one variant per round), on the same gradient buffer; qfx_sf_swap (12 B per element) is timed the
same way.  The verdict compares the new launch's median with AdamW's: it should sit within AdamW's own round-to-round spread
(max - min), doubled.  Writes the record to --out (default schedulefree.json; committed as profiles/schedulefree.json).  Reported,
not gated."""
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
N = 23592960


def main(out, rounds=15, iters=50):
    torch.manual_seed(0)
    p = torch.randn(N, device=DEV) * 0.02
    g = torch.randn(N, device=DEV) * 1e-3
    gn = torch.zeros((), device=DEV)
    parts = torch.zeros(1024, device=DEV)
    ops.sumsq_det(g, gn, parts)
    names = ["adamw", "sfadamw", "sf_swap"]
    pw = {k: p.clone() for k in names}
    m, v = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    z, v2 = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    zs = p.clone() + 1e-3
    st = {"t": 1, "k": 0, "lr_max": -1.0, "wsum": 0.0, "eval": True}

    def run(name):
        if name == "adamw":
            ops.adamw_step(pw[name], g, m, v, 1e-4, 0.9, 0.999, 1e-8, 0.0, st["t"], gnorm_sq=gn, max_norm=1.0)
            st["t"] += 1
        elif name == "sfadamw":
            lr_t, bc2, ckp1, st["lr_max"], st["wsum"] = ops.sfadamw_schedule(st["k"], 1e-4, 0.999, 0, 0.0, 2.0, st["lr_max"], st["wsum"])
            ops.sfadamw_step(pw[name], g, z, v2, lr_t, 0.9, 0.999, 1e-8, 0.0, bc2, ckp1, first=st["k"] == 0, gnorm_sq=gn, max_norm=1.0)
            st["k"] += 1
        else:
            ops.sf_swap(pw[name], zs, 0.9, to_eval=st["eval"])
            st["eval"] = not st["eval"]

    for name in names:                       # warm-up: code objects, first-touch of every buffer, the `first` launch
        for _ in range(6):
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
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / iters * 1e3)
    res = {"what": "optimizer launch alone at the headline adapter size", "flat_elements": N, "rounds": rounds, "iters_per_round": iters,
           "order": "interleaved, alternating per round", "variants": {}}
    hbm = {"adamw": 28, "sfadamw": 28, "sf_swap": 12}
    for name in names:
        t = times[name]
        med = statistics.median(t)
        res["variants"][name] = {"median_us": med, "min_us": min(t), "max_us": max(t), "spread_us": max(t) - min(t), "per_round_us": t,
                                 "hbm_bytes_per_element": hbm[name], "achieved_TBps_of_that": hbm[name] * N / (med * 1e-6) / 1e12}
    a, s = res["variants"]["adamw"], res["variants"]["sfadamw"]
    res["sfadamw_minus_adamw_median_us"] = s["median_us"] - a["median_us"]
    res["allowance_us"] = 2 * a["spread_us"]
    res["within_twice_adamw_spread"] = abs(s["median_us"] - a["median_us"]) <= 2 * a["spread_us"]
    res["not_slower_than_adamw_plus_allowance"] = s["median_us"] <= a["median_us"] + 2 * a["spread_us"]
    res["ratio_median_vs_adamw"] = s["median_us"] / a["median_us"]
    res["finite"] = {k: bool(torch.isfinite(pw[k]).all()) for k in names}
    res["device"] = torch.cuda.get_device_name(0)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: [v["median_us"], v["spread_us"]] for k, v in res["variants"].items()}),
          json.dumps({k: res[k] for k in ("within_twice_adamw_spread", "not_slower_than_adamw_plus_allowance", "ratio_median_vs_adamw")}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="schedulefree.json", help="where the JSON record is written")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    main(a.out, a.rounds, a.iters)
