#!/usr/bin/env python
"""The general criterion launch (qfx_criterion_fwd_bwd: two kernels) against qfx_mse_loss_fwd_bwd (csrc/qfx_elem.hip, unchanged from
the parent commit; one kernel plus the memset of its accumulated loss) at the headline shape: pred [1, 8192, 64], 4096 target rows.

Variants, all in one process, interleaved round by round (device events on the launch stream around `iters` calls of one variant per
round, the order reversed every other round): the older entry through ops.mse_loss_fwd_bwd; the new entry with L2 and unit weights;
with cosmap-style sample weights; with Huber and sample weights.  Each call is the ops wrapper, so it includes what a training step
pays: the output allocations from torch's caching allocator and, for the older entry, zeroing the loss.  Per variant: median / min /
max microseconds per call.  The criterion reads 8192 * 64 * 2 B of pred (half of them rows whose gradient is zero), 4096 * 64 * 2 B
of target and writes 8192 * 64 * 2 B of dpred: about 2.6 MB, far inside launch overhead; no share of peak is claimed.

Writes the record to --out (default criterion_options.json; committed as profiles/criterion_options.json)."""
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


def main(a):
    B, S_all, S_t, Cc = a.shape
    g = torch.Generator().manual_seed(0)
    pred = torch.randn(B, S_all, Cc, generator=g).to(torch.bfloat16).to(DEV)
    target = torch.randn(B, S_t, Cc, generator=g).to(torch.bfloat16).to(DEV)
    sw = (torch.rand(B, generator=g) + 0.5).to(DEV)
    hc = torch.full((B,), 0.1, device=DEV)
    ws = ops.criterion_workspace(B, S_t, Cc, DEV)
    variants = {
        "mse_loss_fwd_bwd (parent's entry)": lambda: ops.mse_loss_fwd_bwd(pred, target, S_t),
        "criterion l2, unit weights": lambda: ops.criterion_fwd_bwd(pred, target, S_t, workspace=ws),
        "criterion l2, sample weights": lambda: ops.criterion_fwd_bwd(pred, target, S_t, sample_w=sw, workspace=ws),
        "criterion huber, sample weights": lambda: ops.criterion_fwd_bwd(pred, target, S_t, sample_w=sw, huber_c=hc, kind="huber", workspace=ws),
    }
    names = list(variants)
    for name in names:
        for _ in range(10):
            variants[name]()
    torch.cuda.synchronize()
    times = {k: [] for k in names}
    for r in range(a.rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.iters):
                variants[name]()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / a.iters * 1e3)
    old = ops.mse_loss_fwd_bwd(pred, target, S_t)
    new = ops.criterion_fwd_bwd(pred, target, S_t)
    res = {"what": "general criterion entry against the parent's MSE entry, per call through the ops wrappers", "device": torch.cuda.get_device_name(0),
           "shape_B_Sall_St_C": list(a.shape), "bytes_moved": 2 * Cc * B * (2 * S_all + S_t), "rounds": a.rounds, "iters_per_round": a.iters,
           "order": "interleaved, reversed every other round",
           "same_dpred_bits_l2_unit": bool(torch.equal(old[1].view(torch.int16), new[2].view(torch.int16))),
           "loss_mse": float(old[0]), "loss_criterion": float(new[0]),
           "variants": {k: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t), "per_round_us": t} for k, t in times.items()}}
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: round(v["median_us"], 2) for k, v in res["variants"].items()}), res["same_dpred_bits_l2_unit"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="criterion_options.json", help="where the JSON record is written")
    ap.add_argument("--shape", type=int, nargs=4, default=[1, 8192, 4096, 64], metavar=("B", "S_all", "S_t", "C"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=200)
    main(ap.parse_args())
