"""Launch time of qfx_scaled_adamw_step against qfx_adamw_step on the same flat buffers at the headline adapter set (60 blocks, four
attention targets of width 3072, r = 16: 240 pairs), interleaved on one device; writes profiles/scaled_adamw_bench.json.
    python tools/scaled_adamw_bench.py [--reps 200] [--out profiles/scaled_adamw_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "qwen-image-finetune_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scaled_adamw_bench.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as G
    G.build()
    from qflux_amd import ops
    dev = "cuda:0"
    r, width, n_pairs = 16, 3072, 240
    pairs, at = [], 0
    for _ in range(n_pairs):
        pairs.append((at, at + r * width, r, width, width, 1.0, 1.0, 0.01, 0.01))
        at += 2 * r * width
    g = torch.Generator().manual_seed(0)
    p0 = (torch.randn(at, generator=g) * 0.02).to(dev)
    grad = (torch.randn(at, generator=g) * 1e-3).to(dev)
    lay = ops.scaled_adamw_table(pairs, device=dev, n_elems=at)
    skipped = torch.zeros(1, dtype=torch.int32, device=dev)
    bufs = {k: (p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)) for k in ("adamw", "scaled", "plain")}

    def launch(kind, t):
        p, m, v = bufs[kind]
        if kind == "adamw":
            ops.adamw_step(p, grad, m, v, 1e-4, 0.9, 0.999, 1e-8, 0.01, t)
        else:
            ops.scaled_adamw_step(p, grad, m, v, lay, skipped, 1e-4, 0.9, 0.999, 1e-8, t, precondition=kind == "scaled")

    times = {k: [] for k in bufs}
    for t in range(1, a.reps + 11):
        for kind in bufs:      # interleaved: every kind sees the same clocks and the same neighbours
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(kind, t)
            e1.record()
            e1.synchronize()
            if t > 10:
                times[kind].append(e0.elapsed_time(e1) * 1e3)
    res = {"what": "tools/scaled_adamw_bench.py: event-timed launches in microseconds, interleaved, 10 warm-up rounds dropped",
           "device": torch.cuda.get_device_name(0), "pairs": n_pairs, "r": r, "width": width, "elements": at, "reps": a.reps,
           "skipped": int(skipped.item())}
    for k, v in times.items():
        v.sort()
        res[k] = {"median_us": statistics.median(v), "p10_us": v[len(v) // 10], "p90_us": v[9 * len(v) // 10], "min_us": v[0]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
