#!/usr/bin/env python
"""What the per-timestep modulation table (qfx_mod_table_fetch / qfx_mod_gemv_unless) buys -> profiles/mod_table.json.

  python tools/mod_table_bench.py --parent DIR [--repeats 3] [--out profiles/mod_table.json] [--skip headline,trace,inproc]

DIR: a built checkout of the parent commit (bench.py + the package with its libqfx.so).  Sections:
  headline  `bench.py --gpus 1 --steps 40 --warmup 10` of the parent and of this tree, alternating, --repeats times each: every sample,
            the medians, the parent's spread (max - min of its own repeats) and whether the median gain exceeds three times that spread
  trace     one `rocprofv3 --kernel-trace --stats` run (no counters) of the same command per tree: time per step of mod_gemv_kernel
            and of mod_table_fetch_kernel
  inproc    this tree, one process, the headline model: table build time and bytes; 40 steps with an off-table timestep (the miss
            path: fetch + the four GEMVs computing), 40 with on-table timesteps, 40 with QFX_MOD_TABLE=0; bare launches of the fetch
            and of the four skipped GEMVs under HIP events
Every child runs under its own time limit and the first failure ends the tool (nothing more is started on the GPU)."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = ["bench.py", "--gpus", "1", "--steps", "40", "--warmup", "10"]


def run_bench(tree, limit=420):
    r = subprocess.run([sys.executable] + BENCH, cwd=tree, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"bench.py in {tree} -> {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    return {"ms_per_step": d["ms_per_step"], "images_per_s": d["value"], "loss": d["config"]["loss"]}


def headline(parent, repeats):
    runs = {"parent": [], "this": []}
    for i in range(repeats):
        for name, tree in (("parent", parent), ("this", ROOT)):
            runs[name].append(run_bench(tree))
            print(f"[headline {i}] {name}: {runs[name][-1]}", flush=True)
    ms = {k: [r["ms_per_step"] for r in v] for k, v in runs.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = max(ms["parent"]) - min(ms["parent"])
    gain = med["parent"] - med["this"]
    return {"command": "python " + " ".join(BENCH), "order": "parent, this, parent, this, ...", "samples": runs,
            "median_ms_per_step": med, "median_images_per_s": {k: statistics.median(r["images_per_s"] for r in v) for k, v in runs.items()},
            "parent_spread_ms": round(spread, 3), "this_spread_ms": round(max(ms["this"]) - min(ms["this"]), 3),
            "median_gain_ms": round(gain, 3), "median_gain_frac": round(gain / med["parent"], 5),
            "gain_exceeds_3x_parent_spread": bool(gain > 3 * spread),
            "same_loss": len({r["loss"] for v in runs.values() for r in v}) == 1}


def trace(tree, steps=50, limit=600):
    """Per-step time of the conditioning-head kernels from rocprofv3's kernel statistics (all launches of the run / its steps)."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="qfx_modtab_")
    try:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "p", "--", sys.executable] + BENCH,
                           cwd=tree, capture_output=True, text=True, timeout=limit)
        if r.returncode != 0:
            raise SystemExit(f"rocprofv3 in {tree} -> {r.returncode}\n{r.stderr[-4000:]}")
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv", "files": [os.path.relpath(f, tmp) for f in glob.glob(os.path.join(tmp, "**", "*"), recursive=True)][:20]}
        out, total = {}, 0.0
        with open(files[0]) as fh:
            for row in csv.DictReader(fh):
                total += float(row["TotalDurationNs"])
                for k in ("mod_gemv_kernel", "mod_table_fetch_kernel", "timestep_embed_kernel"):
                    if k in row["Name"] and "mod_gemv_t_kernel" not in row["Name"]:
                        o = out.setdefault(k, {"calls": 0, "total_us": 0.0, "max_us": 0.0, "min_us": 1e30})
                        o["calls"] += int(row["Calls"]); o["total_us"] += float(row["TotalDurationNs"]) / 1e3
                        o["max_us"] = max(o["max_us"], float(row["MaxNs"]) / 1e3); o["min_us"] = min(o["min_us"], float(row["MinNs"]) / 1e3)
        for o in out.values():
            o["us_per_step"] = round(o["total_us"] / steps, 2)      # (the table build's launches, once per run, are in the total)
            o["total_us"] = round(o["total_us"], 1)
        return {"kernels": out, "all_kernels_ms_per_step": round(total / 1e6 / steps, 3), "steps_in_run": steps}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def inproc():
    """Runs in a child (`--child`): one headline model, the three step variants and the bare launches."""
    sys.path.insert(0, os.path.join(ROOT, "qwen-image-finetune_amd"))
    import torch
    from qflux_amd import _lib as L
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.modules import LoraConfig
    from qflux_amd.trainer import QwenLoraTrainStep
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    with torch.device(dev):
        dit = QwenImageTransformer2DModel(num_layers=60)
    with torch.no_grad():
        for n, p in dit.named_parameters():
            if p.ndim == 2:
                p.normal_(0.0, 0.02)
            elif "norm" in n:
                p.fill_(1.0)
            elif ".img_mod." in n or ".txt_mod." in n:
                p.normal_(0.0, 0.02)
            else:
                p.zero_()
    dit.add_adapter(LoraConfig(r=16, lora_alpha=16, init_lora_weights="gaussian"), "default", generator=torch.Generator().manual_seed(1234))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step = QwenLoraTrainStep(dit, lr=1e-4, max_grad_norm=1.0)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    tb = dit.modulation_table
    res = {"table": {"build_s": round(build_s, 3), "keys": int(tb["keys"].numel()),
                     "bytes": int(tb["mods"].numel() * 2 + tb["out"].numel() * 2 + tb["keys"].numel() * 4)}}
    S_t, T, Jd = 1024, 384, dit.config.joint_attention_dim
    emb = dict(image_latents=torch.randn(1, S_t, 64).half().to(dev), control_latents=torch.randn(1, S_t, 64).half().to(dev),
               prompt_embeds=(torch.randn(1, T, Jd) * 4).half().to(dev), prompt_embeds_mask=None, img_shapes=[[(1, 32, 32), (1, 32, 32)]])

    def timed(tag, warm=10, steps=40):
        for _ in range(warm):
            step.train_step(emb)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(steps):
            step.train_step(emb)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t1) / steps * 1e3
        plan = list(dit._plans.values())[0]
        res[tag] = {"ms_per_step": round(ms, 3), "hit_cell_after": int(plan.A["mod_hit"].item()) if "mod_hit" in plan.A else None}
        print(tag, res[tag], flush=True)

    timed("steps_on_table")
    off = torch.tensor([123.45])
    draw = step.sample_timesteps
    step.sample_timesteps = lambda batch_size, u=None: (off, off / 1000)
    timed("steps_off_table_miss_path")
    step.sample_timesteps = draw
    # bare launches of the head on the hit path: the fetch, then the four guarded GEMVs leaving at once
    plan = list(dit._plans.values())[0]
    calls = plan.fwd.calls[:6]
    assert calls[1][0] is L.lib.qfx_mod_table_fetch and all(c[0] is L.lib.qfx_mod_gemv_unless for c in calls[2:6])
    plan.A["t"].copy_(tb["keys"][287:288])
    st = torch.cuda.current_stream().cuda_stream
    names = ["timestep_embed", "fetch_hit", "unless_t1_skipped", "unless_t2_skipped", "unless_mods_skipped_138240_blocks", "unless_norm_out_skipped"]
    bare = {}
    for rep in range(3):          # the first pass warms up
        for nm, (fn, args) in zip(names, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                assert fn(*args, st) == 0
            e1.record()
            torch.cuda.synchronize()
            bare[nm] = round(e0.elapsed_time(e1) / 20 * 1e3, 2)
    res["bare_launch_us_back_to_back"] = bare
    os.environ["QFX_MOD_TABLE"] = "0"
    dit.drop_modulation_table()
    timed("steps_lever_off")
    print("__INPROC__" + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mod_table.json"))
    ap.add_argument("--skip", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return inproc()
    skip = set(filter(None, a.skip.split(",")))
    if not a.parent and not {"headline", "trace"} <= skip:
        ap.error("--parent DIR (a built checkout of the parent commit) is needed for the headline and trace sections")
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out["what"] = ("per-timestep table of the AdaLN modulation vectors (qfx_mod_table_fetch + qfx_mod_gemv_unless) against the parent commit, "
                   "one MI355X, tools/mod_table_bench.py")

    def save():
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    if "headline" not in skip:
        out["headline"] = headline(os.path.abspath(a.parent), a.repeats)
        save()
    if "inproc" not in skip:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"in-process section -> {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        out["this_tree_in_process"] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("__INPROC__")][-1][len("__INPROC__"):])
        save()
    if "trace" not in skip:
        out["kernel_trace_note"] = ("kernel_trace.this: mod_gemv_kernel and timestep_embed_kernel totals include the table build of the run (4 and 1 "
                                    "launches per batch of 8 keys, computing); per step the four guarded launches leave at once -- their cost is "
                                    "this_tree_in_process.bare_launch_us_back_to_back")
        out["kernel_trace"] = {"command": "rocprofv3 --kernel-trace --stats -- python " + " ".join(BENCH),
                               "parent": trace(os.path.abspath(a.parent)), "this": trace(ROOT)}
        save()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
