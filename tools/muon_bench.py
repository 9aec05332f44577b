#!/usr/bin/env python
"""qfx_muon_step against qfx_adamw_step on the headline LoRA parameter set: Qwen-Image, 60 blocks, to_q / to_k / to_v / to_out.0,
A r x 3072 and B 3072 x r each -- 480 matrices, 23.59 M parameters at r = 16 (every X in LDS) and 94.37 M at r = 64 (every X in the
workspace).  The four variants run in one process, interleaved round by round (device events around `iters` launches of one variant
per round, the order reversed every other round), on the same gradient buffers.  Records the median / min / max per launch, the
round-to-round spread of the box, the ratio to AdamW at the same rank, the workspace and state bytes, and the number of device
kernels ONE step of torch.optim.Muon launches over the same 480 views at r = 16 (torch.profiler; null when it cannot be counted).
There is no pass / fail time: Muon is five iterations of three small matrix products per matrix, AdamW one elementwise sweep.
Writes the record to --out (default muon_bench.json; meant for profiles/muon_bench.json).

--parity LOG: instead of timing, collect the MUON_PARITY lines that `pytest -s tests/test_muon_gpu.py` prints (the measured errors of
torch.optim.Muon, the restatement and the kernel against the float64 iteration) into --out (meant for profiles/muon_parity.json).

--stage-measured FILE: merge the kernel's one-iteration shares that tests/test_muon_gpu.py wrote with QFX_MUON_STAGE_MEASURED_OUT=FILE
into --out (meant for profiles/muon_stage_parity.json, whose bars tests/test_muon_cpu.py writes) under kernel_measured."""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen-image-finetune_amd"))
DEV = "cuda:0"


def parity(log, out):
    rec = {"what": "relative Frobenius errors against the float64 Newton-Schulz iteration from the same bf16-normalised input "
                   "(tests/test_muon_gpu.py); requirement on Gaussian gradients: e_kernel <= 2 e_torch per matrix", "records": []}
    with open(log) as f:
        for line in f:
            m = re.search(r"MUON_PARITY (\w+) (.*)", line)
            if not m:
                continue
            d = {"test": m.group(1)}
            for k, v in re.findall(r"(\w+)=(\([^)]*\)|\S+)", m.group(2)):
                try:
                    d[k] = json.loads(v.replace("(", "[").replace(")", "]").replace("True", "true").replace("False", "false").replace("None", "null"))
                except ValueError:
                    d[k] = v
            rec["records"].append(d)
    ratios = [d["e_kernel"] / d["e_torch"] for d in rec["records"] if d["test"] != "rank1" and d.get("e_torch") and "e_kernel" in d]
    rec["worst_ratio_e_kernel_over_e_torch"] = max(ratios) if ratios else None
    rec["worst_buf_ulp"] = max((d["buf_ulp"] for d in rec["records"] if "buf_ulp" in d), default=None)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("worst_ratio_e_kernel_over_e_torch", "worst_buf_ulp")}), len(rec["records"]), "records")


def stage_measured(measured, out):
    with open(out) as f:
        doc = json.load(f)
    with open(measured) as f:
        doc["kernel_measured"] = json.load(f)
    assert set(doc["kernel_measured"]) == set(doc["bar"]), "the measured file and the bars name other shapes"
    doc["kernel_note"] = ("qfx_muon_step on one MI355X against the float64-accumulated iteration, "
                          "tests/test_muon_gpu.py (QFX_MUON_STAGE_MEASURED_OUT)")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: v["differing"] for k, v in doc["kernel_measured"].items()}))


def torch_muon_launches(shapes):
    """Device kernels of one torch.optim.Muon step over separate views of the same shapes (after a warm-up step)."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        ps = [torch.nn.Parameter(torch.randn(s, device=DEV) * 0.02) for s in shapes]
        opt = torch.optim.Muon(ps, lr=1e-4)
        for p in ps:
            p.grad = torch.randn_like(p) * 1e-3
        opt.step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            opt.step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception as e:      # noqa: BLE001 -- a count for the documents, not a measurement the record depends on
        print("torch.optim.Muon launch count unavailable:", e)
        return None


def main(out, rounds=15, iters=20):
    import torch
    from qflux_amd import ops
    torch.manual_seed(0)
    sets = {}
    for r in (16, 64):
        shapes = [(r, 3072), (3072, r)] * (60 * 4)
        offs, off = [], 0
        for s in shapes:
            offs.append(off)
            off += (s[0] * s[1] + 63) // 64 * 64
        lay = ops.muon_table(list(zip(offs, shapes)), None, device=DEV)
        g = torch.randn(off, device=DEV) * 1e-3
        gn, parts = torch.zeros((), device=DEV), torch.zeros(1024, device=DEV)
        ops.sumsq_det(g, gn, parts)
        z = lambda: torch.zeros(off, device=DEV)   # noqa: E731
        sets[r] = dict(n=off, shapes=shapes, lay=lay, g=g, gn=gn, p_a=torch.randn(off, device=DEV) * 0.02, p_m=torch.randn(off, device=DEV) * 0.02,
                       m=z(), v=z(), buf=z(), ws=torch.zeros(lay.ws_bytes // 2, dtype=torch.bfloat16, device=DEV) if lay.ws_bytes else None)
    names = ["adamw_r16", "muon_r16", "adamw_r64", "muon_r64"]
    step = {"t": 1}

    def run(name):
        s = sets[int(name[-2:])]
        if name.startswith("adamw"):
            ops.adamw_step(s["p_a"], s["g"], s["m"], s["v"], 1e-4, 0.9, 0.999, 1e-8, 0.0, step["t"], gnorm_sq=s["gn"], max_norm=1.0)
        else:
            ops.muon_step(s["p_m"], s["g"], s["buf"], s["ws"], s["lay"], 1e-4, 0.1, gnorm_sq=s["gn"], max_norm=1.0)

    for name in names:                       # warm-up: code objects, first-touch of every buffer
        for _ in range(3):
            run(name)
    torch.cuda.synchronize()
    times = {k: [] for k in names}
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                run(name)
                step["t"] += 1
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / iters * 1e3)
    res = {"what": "optimizer launch alone, headline LoRA set (Qwen 60 blocks, 4 attention targets, 480 matrices) at r = 16 and r = 64",
           "rounds": rounds, "iters_per_round": iters, "order": "interleaved, reversed every other round", "variants": {}}
    for name in names:
        t = times[name]
        s = sets[int(name[-2:])]
        res["variants"][name] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t), "spread_us": max(t) - min(t),
                                 "per_round_us": t, "flat_elements": s["n"], "params": sum(a * b for a, b in s["shapes"])}
    res["against_adamw"] = {}
    for r in (16, 64):
        a, b = res["variants"][f"muon_r{r}"], res["variants"][f"adamw_r{r}"]
        res["against_adamw"][f"r{r}"] = {"ratio_median": a["median_us"] / b["median_us"], "delta_median_us": a["median_us"] - b["median_us"],
                                         "round_to_round_spread_us": max(a["spread_us"], b["spread_us"])}
        res[f"r{r}_bytes"] = {"muon_momentum_fp32": 4 * sets[r]["n"], "muon_workspace_bf16": sets[r]["lay"].ws_bytes, "adamw_fp32_moments": 8 * sets[r]["n"]}
    res["finite_after_run"] = bool(all(torch.isfinite(sets[r]["p_m"]).all() for r in sets))
    res["torch_optim_muon_kernels_per_step_r16_480_views"] = torch_muon_launches(sets[16]["shapes"])
    res["device"] = torch.cuda.get_device_name(0)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: round(v["median_us"], 2) for k, v in res["variants"].items()}), json.dumps(res["against_adamw"]),
          "torch launches:", res["torch_optim_muon_kernels_per_step_r16_480_views"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="where the JSON record is written")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parity", default=None, metavar="LOG", help="collect MUON_PARITY lines of a pytest -s log instead of timing")
    ap.add_argument("--stage-measured", default=None, metavar="FILE", help="merge the one-iteration shares the GPU test wrote into --out")
    a = ap.parse_args()
    if a.parity:
        parity(a.parity, a.out or "muon_parity.json")
    elif a.stage_measured:
        stage_measured(a.stage_measured, a.out or "muon_stage_parity.json")
    else:
        main(a.out or "muon_bench.json", a.rounds, a.iters)
