#!/usr/bin/env python
"""What the fused RAdam / NAdam / Adamax launch costs and how accurate it is: (1) the stand-alone time of the ONE qfx_adamx_step
launch per variant on the headline adapter set (480 tensors, A 16 x 3072 and B 3072 x 16 each: 23.6 M parameters; one group, and
the two LoRA+ groups) next to qfx_adamw_step on the same box -- the launch every variant moves the same bytes as: p, exp_avg and the
second state read and written, g read -- interleaved round by round (order reversed every other round), device events around
`iters` launches per round, on the same gradient buffer; (2) the e_kernel / e_torch figures of tests/test_adamx_gpu.py, read
from the file its parity run dumps (--parity), so that one record holds both.

Writes the record to --out (default adam_variants.json; committed as profiles/adam_variants.json).  Reported, not gated."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen-image-finetune_amd"))

DEV = "cuda:0"
VARIANTS = ("radam", "nadam", "adamax")


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def launch_bench(rounds, iters):
    from qflux_amd import ops
    shapes = [(16, 3072), (3072, 16)] * (60 * 4)
    ents, off = [], 0
    for s in shapes:
        ents.append((off, s[0] * s[1]))
        off += (s[0] * s[1] + 63) // 64 * 64
    n = off
    torch.manual_seed(0)
    g = torch.randn(n, device=DEV) * 1e-3
    gn, parts = torch.zeros((), device=DEV), torch.zeros(1024, device=DEV)
    ops.sumsq_det(g, gn, parts)
    z = lambda: torch.zeros(n, device=DEV)      # noqa: E731
    P = lambda: torch.randn(n, device=DEV) * 0.02      # noqa: E731
    tmap = ops.tile_group_map(ents, [i % 2 for i in range(len(ents))], 2, numel=n, device=DEV)
    row = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    names = ["adamw"] + list(VARIANTS) + [v + "_loraplus" for v in VARIANTS]
    bufs = {k: dict(p=P(), m=z(), v=z(), mu=[torch.tensor(1.0), torch.tensor(1.0)]) for k in names}
    count = dict.fromkeys(names, 0)

    def run(name):
        count[name] += 1
        b = bufs[name]
        if name == "adamw":
            return ops.adamw_step(b["p"], g, b["m"], b["v"], 1e-4, 0.9, 0.999, 1e-8, 0.01, count[name], gnorm_sq=gn, max_norm=1.0)
        variant, _, plus = name.partition("_")
        rows = [row, dict(row, lr=4e-4, weight_decay=0.0)] if plus else [row]
        ops.adamx_step(variant, b["p"], g, b["m"], b["v"], rows, count[name], tile_group=tmap if plus else None, mu_products=b["mu"],
                       gnorm_sq=gn, max_norm=1.0)

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
    assert all(bool(torch.isfinite(b["p"]).all()) for b in bufs.values())
    med = {k: statistics.median(v) for k, v in us.items()}
    nbytes = 7 * 4 * n      # four fp32 streams read, three written
    return {"what": "one launch over the headline adapter set, device events around `iters` launches, interleaved rounds",
            "tensors": len(shapes), "elements_with_padding": n, "rounds": rounds, "iters_per_round": iters,
            "us_per_launch": {k: spread(v) for k, v in us.items()},
            "over_adamw_at_median": {k: med[k] / med["adamw"] for k in names if k != "adamw"},
            "adamw_run_to_run_spread_us": max(us["adamw"]) - min(us["adamw"]),
            "hbm_bytes_per_launch": nbytes, "TBps_at_median": {k: nbytes / (med[k] * 1e-6) / 1e12 for k in names}}


def parity_summary(path):
    with open(path) as f:
        recs = json.load(f)["records"]
    worst = {}
    for r in recs:
        fam = r["case"][0]
        for k in ("p", "exp_avg", "second"):
            if k in r and r[k]["e_torch"] > 0:
                w = worst.setdefault(fam, {})
                w[k] = max(w.get(k, 0.0), r[k]["e_kernel"] / r[k]["e_torch"])
    return {"what": "tests/test_adamx_gpu.py: largest absolute error against the fp64 restatement of the kernel and of torch's fp32 CPU "
                    "step per case; the bar is e_kernel <= 2 e_torch", "worst_e_kernel_over_e_torch": worst, "records": recs}


def main(a):
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res["device"] = torch.cuda.get_device_name(0)
    res["launch"] = launch_bench(a.rounds, a.iters)
    print(json.dumps({k: v["median"] for k, v in res["launch"]["us_per_launch"].items()}))
    if a.parity and os.path.exists(a.parity):
        res["parity"] = parity_summary(a.parity)
        print(json.dumps(res["parity"]["worst_e_kernel_over_e_torch"]))
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="adam_variants.json", help="where the JSON record is written (an existing record's other keys are kept)")
    ap.add_argument("--parity", default=None, help="the adamx_parity_gpu.json a run of tests/test_adamx_gpu.py wrote")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=50)
    main(ap.parse_args())
