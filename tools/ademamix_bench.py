#!/usr/bin/env python
"""qfx_ademamix_step (three fp32 states) and qfx_ademamix8bit_step (blockwise 8-bit states, block sizes 256 and 2048) against their
yardsticks qfx_adamw_step and qfx_adam8bit_step on the headline LoRA parameter set: Qwen-Image, 60 blocks, r = 16, to_q / to_k /
to_v / to_out.0 (A 16 x 3072 and B 3072 x 16 each: 23.59 M parameters, every tensor above bnb's 8-bit threshold).  All six variants
run in one process, interleaved round by round (device events around `iters` launches of one variant per round, the order reversed
every other round), on the same gradient buffer; the step count advances, so both AdEMAMix schedules move as in a run.  Records the
median / min / max per launch, the fraction of HBM bandwidth the algorithmic bytes imply (44 B per element for fp32 AdEMAMix -- p,
m1, m2 and nu read and written, g read -- against 28 B for AdamW; 18 B against 16 B for the 8-bit forms) and the ratio of each
AdEMAMix launch to the yardstick of its class beside the run's round-to-round spread.  From the bytes alone the expectation is 11/7
of the AdamW launch in element traffic (11 accesses of an element against 7).  Writes the record to --out (default ademamix_bench.json; committed as
profiles/ademamix_bench.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen-image-finetune_amd"))
from qflux_amd import ops  # noqa: E402
from qflux_amd.trainer.adam8bit import dynamic_map  # noqa: E402

DEV = "cuda:0"
HBM_TBPS = 8.0          # MI355X peak HBM3E bandwidth the fractions refer to


def main(out, rounds=15, iters=50):
    sizes = [16 * 3072] * (60 * 4 * 2)
    offs, off = [], 0
    for k in sizes:
        offs.append(off)
        off += (k + 63) // 64 * 64
    n = off
    torch.manual_seed(0)
    p = torch.randn(n, device=DEV) * 0.02
    g = torch.randn(n, device=DEV) * 1e-3
    gn = torch.zeros((), device=DEV)
    parts = torch.zeros(1024, device=DEV)
    ops.sumsq_det(g, gn, parts)
    z = lambda *k, dt=torch.float32: torch.zeros(*(k or (n,)), dtype=dt, device=DEV)   # noqa: E731
    qm1, qm2 = dynamic_map(True).to(DEV), dynamic_map(False).to(DEV)
    lay = {bs: ops.adam8bit_block_table(list(zip(offs, sizes)), bs, 4096, device=DEV) for bs in (256, 2048)}
    names = ["adamw", "ademamix", "adam8bit_bs256", "ademamix8bit_bs256", "adam8bit_bs2048", "ademamix8bit_bs2048"]
    st = {"adamw": dict(m=z(), v=z()), "ademamix": dict(m1=z(), m2=z(), nu=z())}
    plane = (n + 15) // 16 * 16
    for bs in (256, 2048):
        na = lay[bs].n_absmax
        st[f"adam8bit_bs{bs}"] = dict(lay=lay[bs], q1=z(dt=torch.uint8), q2=z(dt=torch.uint8), a1=z(na), a2=z(na), m32=z(1), v32=z(1))
        st[f"ademamix8bit_bs{bs}"] = dict(lay=lay[bs], q1=z(2, plane, dt=torch.uint8), q2=z(dt=torch.uint8), a1=z(2, na), a2=z(na),
                                          m32=z(2, 4), v32=z(4))
    pw = {k: p.clone() for k in names}
    step = {"t": 1}
    row = [dict(lr=1e-4, betas=(0.9, 0.999, 0.9999), eps=1e-8, weight_decay=0.0, alpha=5.0, t_alpha=20000, t_beta3=20000)]

    def run(name):
        s = st[name]
        if name == "adamw":
            ops.adamw_step(pw[name], g, s["m"], s["v"], 1e-4, 0.9, 0.999, 1e-8, 0.0, step["t"], gnorm_sq=gn, max_norm=1.0)
        elif name == "ademamix":
            ops.ademamix_step(pw[name], g, s["m1"], s["m2"], s["nu"], row, step["t"], gnorm_sq=gn, max_norm=1.0)
        elif name.startswith("adam8bit"):
            ops.adam8bit_step(pw[name], g, s["q1"], s["q2"], s["a1"], s["a2"], s["m32"], s["v32"], s["lay"], qm1, qm2, 1e-4, (0.9, 0.999),
                              1e-8, 0.0, step["t"], gnorm_sq=gn, max_norm=1.0)
        else:
            ops.ademamix8bit_step(pw[name], g, s["q1"], s["q2"], s["a1"], s["a2"], s["m32"], s["v32"], s["lay"], qm1, qm2, row, step["t"],
                                  gnorm_sq=gn, max_norm=1.0)

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
    nparam = sum(sizes)
    res = {"what": "optimizer launch alone, headline LoRA set (Qwen 60 blocks, r=16, 4 attention targets)", "params": nparam,
           "flat_elements": n, "rounds": rounds, "iters_per_round": iters, "order": "interleaved, reversed every other round",
           "hbm_peak_TBps_assumed": HBM_TBPS, "variants": {}}
    # algorithmic bytes per element: p read + written, g read, every state read + written
    bytes_moved = {"adamw": 28, "ademamix": 44, "adam8bit_bs256": 16, "adam8bit_bs2048": 16, "ademamix8bit_bs256": 18, "ademamix8bit_bs2048": 18}
    for name in names:
        t = times[name]
        med = statistics.median(t)
        tbps = bytes_moved[name] * n / (med * 1e-6) / 1e12
        res["variants"][name] = {"median_us": med, "min_us": min(t), "max_us": max(t), "spread_us": max(t) - min(t), "per_round_us": t,
                                 "bytes_per_element": bytes_moved[name], "achieved_TBps": tbps, "fraction_of_hbm_peak": tbps / HBM_TBPS}
    res["state_bytes"] = {"adamw_fp32_moments": 2 * 4 * nparam, "ademamix_fp32_states": 3 * 4 * nparam,
                          **{f"adam8bit_bs{bs}_codes_absmax": 2 * nparam + 2 * 4 * lay[bs].n_absmax for bs in (256, 2048)},
                          **{f"ademamix8bit_bs{bs}_codes_absmax": 3 * nparam + 3 * 4 * lay[bs].n_absmax for bs in (256, 2048)}}
    res["against_yardstick"] = {}
    for new, old in (("ademamix", "adamw"), ("ademamix8bit_bs256", "adam8bit_bs256"), ("ademamix8bit_bs2048", "adam8bit_bs2048")):
        a, b = res["variants"][new], res["variants"][old]
        res["against_yardstick"][new] = {"yardstick": old, "ratio_median": a["median_us"] / b["median_us"],
                                         "ratio_of_bytes": a["bytes_per_element"] / b["bytes_per_element"],
                                         "delta_median_us": a["median_us"] - b["median_us"],
                                         "round_to_round_spread_us": max(a["spread_us"], b["spread_us"])}
    res["device"] = torch.cuda.get_device_name(0)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: round(v["median_us"], 2) for k, v in res["variants"].items()}), json.dumps(res["against_yardstick"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="ademamix_bench.json", help="where the JSON record is written")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    main(a.out, a.rounds, a.iters)
