#!/usr/bin/env python
"""qfx_adam8bit_step (blockwise 8-bit Adam, bitsandbytes' state layout; block sizes 256 and 2048) against qfx_adamw_step (fp32
moments) on the headline LoRA parameter set: Qwen-Image, 60 blocks, r = 16, to_q / to_k / to_v / to_out.0 (A 16 x 3072 and
B 3072 x 16 each: 23.6 M parameters, every tensor above bnb's 8-bit threshold).  The three variants run same-box, interleaved
round by round (device events around `iters` launches of one variant per round), on the same gradient buffer.  Also records the
state bytes of each form.  Writes the record to --out (default adam8bit_step.json; committed as profiles/adam8bit_step.json)."""
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
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    qm1, qm2 = dynamic_map(True).to(DEV), dynamic_map(False).to(DEV)
    st8 = {}
    for bs in (256, 2048):
        lay = ops.adam8bit_block_table(list(zip(offs, sizes)), bs, 4096, device=DEV)
        st8[bs] = dict(lay=lay, q1=torch.zeros(n, dtype=torch.uint8, device=DEV), q2=torch.zeros(n, dtype=torch.uint8, device=DEV),
                       a1=torch.zeros(lay.n_absmax, device=DEV), a2=torch.zeros(lay.n_absmax, device=DEV),
                       m32=torch.zeros(1, device=DEV), v32=torch.zeros(1, device=DEV))
    pw = {k: p.clone() for k in ("adamw", 256, 2048)}
    step = {"t": 1}

    def run(name):
        if name == "adamw":
            ops.adamw_step(pw[name], g, m, v, 1e-4, 0.9, 0.999, 1e-8, 0.0, step["t"], gnorm_sq=gn, max_norm=1.0)
        else:
            s = st8[name]
            ops.adam8bit_step(pw[name], g, s["q1"], s["q2"], s["a1"], s["a2"], s["m32"], s["v32"], s["lay"], qm1, qm2, 1e-4,
                              (0.9, 0.999), 1e-8, 0.0, step["t"], gnorm_sq=gn, max_norm=1.0)

    names = ["adamw", 256, 2048]
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
           "flat_elements": n, "rounds": rounds, "iters_per_round": iters, "order": "interleaved, alternating per round",
           "variants": {}}
    bytes_moved = {"adamw": 28, 256: 16, 2048: 16}
    for name in names:
        t = times[name]
        med = statistics.median(t)
        res["variants"][f"adam8bit_bs{name}" if name != "adamw" else "adamw"] = {
            "median_us": med, "min_us": min(t), "max_us": max(t), "per_round_us": t,
            "bytes_per_param": bytes_moved[name], "achieved_TBps": bytes_moved[name] * nparam / (med * 1e-6) / 1e12}
    res["state_bytes"] = {"adamw_fp32_moments": 2 * 4 * nparam,
                          "adam8bit_bs256_codes_absmax": 2 * nparam + 2 * 4 * st8[256]["lay"].n_absmax,
                          "adam8bit_bs2048_codes_absmax": 2 * nparam + 2 * 4 * st8[2048]["lay"].n_absmax}
    res["ratio_median_vs_adamw"] = {k: res["variants"][k]["median_us"] / res["variants"]["adamw"]["median_us"]
                                    for k in res["variants"]}
    res["device"] = torch.cuda.get_device_name(0)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v["median_us"] for k, v in res["variants"].items()}), json.dumps(res["state_bytes"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="adam8bit_step.json", help="where the JSON record is written")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    main(a.out, a.rounds, a.iters)
