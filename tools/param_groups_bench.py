#!/usr/bin/env python
"""The grouped optimizer launches against their ungrouped parents on the headline LoRA parameter set: Qwen-Image, 60 blocks, r = 16,
to_q / to_k / to_v / to_out.0 (A 16 x 3072 and B 3072 x 16 each: 23.59 M fp32 elements), two groups (the LoRA+ split: every other
tensor).  Timed: qfx_adamw_step_grouped against qfx_adamw_step, qfx_adam8bit_step_grouped against qfx_adam8bit_step (block sizes
256 and 2048).  The parent is the ungrouped kernel of the PARENT COMMIT, not this tree's own single-group path: build the parent
commit's qfx_optim.hip and qfx_adam8bit.hip into a library of their own (tools/_ab/, kept out of git) --

    git archive HEAD~1 qwen-image-finetune_amd/csrc include | tar -x -C tools/_ab/parent
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Itools/_ab/parent/include -Itools/_ab/parent/qwen-image-finetune_amd/csrc \\
        tools/_ab/parent/qwen-image-finetune_amd/csrc/qfx_optim.hip -o tools/_ab/libparent_optim.so
    (the same for qfx_adam8bit.hip with -ffp-contract=off -> tools/_ab/libparent_adam8bit.so)

-- and pass the directory as --parent-dir.  Without it the tree's own ungrouped entries stand in and the record says so.  All
variants run in one process, interleaved round by round (device events around `iters` launches of one variant per round, the order
reversed every other round), on the same gradient buffer.  With a parent library the tree's own ungrouped entries are timed too
(`*_tree`: they were refactored around the shared element functions).  Records median / min / max per launch, the ratio of each grouped launch
to its parent and whether it is slower by more than the parent's own round-to-round spread.  Writes the record to --out (default
param_groups.json; committed as profiles/param_groups.json)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen-image-finetune_amd"))
from qflux_amd import _lib as L  # noqa: E402
from qflux_amd import ops  # noqa: E402
from qflux_amd.trainer.adam8bit import dynamic_map  # noqa: E402

DEV = "cuda:0"
HBM_TBPS = 8.0          # MI355X peak HBM3E bandwidth the fractions refer to
ROWS = [(1e-4, 0.9, 0.999, 1e-8, 0.01), (1.6e-3, 0.9, 0.999, 1e-8, 0.0)]      # LoRA+ at ratio 16, no decay on lora_B


def _parent(parent_dir):
    """The parent commit's two entry points, from libraries of their own (None: this tree's)."""
    if not parent_dir:
        return None
    out = {}
    for key, sym in (("optim", "qfx_adamw_step"), ("adam8bit", "qfx_adam8bit_step")):
        lib = C.CDLL(os.path.join(parent_dir, f"libparent_{key}.so"))
        fn = getattr(lib, sym)
        fn.restype, fn.argtypes = L.SYMBOLS[sym]
        out[sym] = fn
    return out


def main(out, rounds=15, iters=50, parent_dir=None):
    sizes = [16 * 3072] * (60 * 4 * 2)
    offs, off = [], 0
    for k in sizes:
        offs.append(off)
        off += (k + 63) // 64 * 64
    n = off
    entries, assign = list(zip(offs, sizes)), [i % 2 for i in range(len(sizes))]
    torch.manual_seed(0)
    p = torch.randn(n, device=DEV) * 0.02
    g = torch.randn(n, device=DEV) * 1e-3
    gn = torch.zeros((), device=DEV)
    ops.sumsq_det(g, gn, torch.zeros(1024, device=DEV))
    z = lambda k=n, dt=torch.float32: torch.zeros(k, dtype=dt, device=DEV)   # noqa: E731
    qm1, qm2 = dynamic_map(True).to(DEV), dynamic_map(False).to(DEV)
    lay = {bs: ops.adam8bit_block_table(entries, bs, 4096, device=DEV) for bs in (256, 2048)}
    tg = ops.tile_group_map(entries, assign, 2, numel=n, device=DEV)
    bg = {bs: ops.block_group_map(lay[bs], assign, 2, device=DEV) for bs in (256, 2048)}
    parent = _parent(parent_dir)
    pairs = [("adamw", "adamw_grouped"), ("adam8bit_bs256", "adam8bit_bs256_grouped"), ("adam8bit_bs2048", "adam8bit_bs2048_grouped")]
    names = [x for pr in pairs for x in pr]
    tree = [old + "_tree" for old, _ in pairs] if parent else []      # this tree's ungrouped entries (refactored around the shared
    names += tree                                                      # element functions) against the parent commit's, same protocol
    st = {}
    for name in names:
        if name.startswith("adamw"):
            st[name] = dict(p=p.clone(), m=z(), v=z())
        else:
            bs = 256 if "256" in name else 2048
            st[name] = dict(p=p.clone(), bs=bs, q1=z(dt=torch.uint8), q2=z(dt=torch.uint8), a1=z(lay[bs].n_absmax), a2=z(lay[bs].n_absmax),
                            m32=z(1), v32=z(1))
    step = {"t": 1}
    lr, b1, b2, eps, wd = ROWS[0]
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def run(name):
        s, t = st[name], step["t"]
        if name == "adamw" or name == "adamw_tree":
            if parent and name == "adamw":
                L.check(parent["qfx_adamw_step"](ptr(s["p"]), ptr(g), ptr(s["m"]), ptr(s["v"]), n, lr, b1, b2, eps, wd, 1.0 - b1 ** t,
                                                 1.0 - b2 ** t, ptr(gn), 1.0, 1.0, ops.stream_ptr()), "parent qfx_adamw_step")
            else:
                ops.adamw_step(s["p"], g, s["m"], s["v"], lr, b1, b2, eps, wd, t, gnorm_sq=gn, max_norm=1.0)
        elif name == "adamw_grouped":
            ops.adamw_step_grouped(s["p"], g, s["m"], s["v"], tg, ROWS, t, gnorm_sq=gn, max_norm=1.0)
        elif name.endswith("grouped"):
            ops.adam8bit_step_grouped(s["p"], g, s["q1"], s["q2"], s["a1"], s["a2"], s["m32"], s["v32"], lay[s["bs"]], qm1, qm2, bg[s["bs"]],
                                      ROWS, t, gnorm_sq=gn, max_norm=1.0)
        elif parent and not name.endswith("_tree"):
            la = lay[s["bs"]]
            a = L.Adam8bitArgs(ptr(s["p"]), ptr(g), ptr(s["q1"]), ptr(s["q2"]), ptr(s["a1"]), ptr(s["a2"]), ptr(s["m32"]), ptr(s["v32"]),
                               ptr(la.table), la.n_blocks, la.blocksize, ptr(qm1), ptr(qm2), lr, b1, b2, eps, wd, t, ptr(gn), 1.0, 1.0)
            L.check(parent["qfx_adam8bit_step"](a, ops.stream_ptr()), "parent qfx_adam8bit_step")
        else:
            ops.adam8bit_step(s["p"], g, s["q1"], s["q2"], s["a1"], s["a2"], s["m32"], s["v32"], lay[s["bs"]], qm1, qm2, lr, (b1, b2), eps, wd,
                              t, gnorm_sq=gn, max_norm=1.0)

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
    res = {"what": "grouped optimizer launch against its ungrouped parent, headline LoRA set (Qwen 60 blocks, r=16, 4 attention targets), "
                   "two groups (every other tensor)", "params": sum(sizes), "flat_elements": n, "groups": 2, "rounds": rounds,
           "iters_per_round": iters, "order": "interleaved, reversed every other round", "hbm_peak_TBps_assumed": HBM_TBPS,
           "parent": "the parent commit's kernels, built into libraries of their own" if parent else
                     "THIS tree's ungrouped entries (no --parent-dir): not the comparison the record is meant to hold",
           "variants": {}, "against_parent": {}}
    for name in names:
        t = times[name]
        med = statistics.median(t)
        bpe = (28 if name.startswith("adamw") else 16) + (1 / 64 if name.endswith("grouped") and name.startswith("adamw") else 0)
        tbps = bpe * n / (med * 1e-6) / 1e12
        res["variants"][name] = {"median_us": med, "min_us": min(t), "max_us": max(t), "spread_us": max(t) - min(t), "per_round_us": t,
                                 "bytes_per_element": bpe, "achieved_TBps": tbps, "fraction_of_hbm_peak": tbps / HBM_TBPS}
    for old, new in pairs + [(t[:-5], t) for t in tree]:
        a, b = res["variants"][new], res["variants"][old]
        res["against_parent"][new] = {"parent": old, "ratio_median": a["median_us"] / b["median_us"],
                                      "delta_median_us": a["median_us"] - b["median_us"], "parent_round_to_round_spread_us": b["spread_us"],
                                      "slower_beyond_parent_spread": a["median_us"] - b["median_us"] > b["spread_us"]}
    res["device"] = torch.cuda.get_device_name(0)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: round(v["median_us"], 2) for k, v in res["variants"].items()}), json.dumps(res["against_parent"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="param_groups.json", help="where the JSON record is written")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--parent-dir", default=None, help="directory with libparent_optim.so / libparent_adam8bit.so built from the parent commit")
    a = ap.parse_args()
    main(a.out, a.rounds, a.iters, a.parent_dir)
