"""Extract a LoRA from the difference of two checkpoints: kohya's extract_lora_from_models.py flags over
qflux_amd.extract.extract_lora (a randomized range finder per linear layer on the GPU instead of a full SVD; see include/qfx.h,
qfx_lowrank_sketch).

    python tools/extract_lora.py --model_org base.safetensors --model_tuned tuned.safetensors --save_to lora.safetensors \
        --dim 16 --min_diff 0.01 --verbose

kohya's --clamp_quantile is not offered.  Without --per_module_rank every module is allocated the largest rank chosen, which
qflux_amd.lora_io.load_lora_adapter can load; the dynamic-rank flags are those of tools/resize_lora.py.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen-image-finetune_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model_org", required=True, help="the base checkpoint: safetensors file or folder")
    ap.add_argument("--model_tuned", required=True, help="the tuned checkpoint: safetensors file or folder")
    ap.add_argument("--save_to", required=True, help="destination safetensors file or folder")
    ap.add_argument("--dim", type=int, default=4, help="the rank (at most 64), or the cap of a dynamic method")
    ap.add_argument("--min_diff", type=float, default=0.0, help="modules whose difference has a Frobenius norm <= this are left out")
    ap.add_argument("--target_modules", default=None, help="a regex searched in the module names")
    ap.add_argument("--oversample", type=int, default=8, help="extra sketch columns: k = min(64, dim + oversample)")
    ap.add_argument("--power_iters", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dynamic_method", choices=("sv_ratio", "sv_cumulative", "sv_fro"), default=None)
    ap.add_argument("--dynamic_param", type=float, default=None)
    ap.add_argument("--per_module_rank", action="store_true", help="one rank per module instead of one zero-padded rank")
    ap.add_argument("--group_gib", type=float, default=2.0, help="weights streamed to the device per group, both sides counted")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--verbose", action="store_true")
    a = ap.parse_args(argv)
    if a.dynamic_method and a.dynamic_param is None:
        ap.error("--dynamic_method needs --dynamic_param")
    from qflux_amd.extract import extract_lora
    _, _, report = extract_lora(a.model_org, a.model_tuned, save_to=a.save_to, rank=a.dim, target_modules=a.target_modules,
                                min_diff=a.min_diff, oversample=a.oversample, power_iters=a.power_iters, seed=a.seed,
                                dynamic_method=a.dynamic_method, dynamic_param=a.dynamic_param, uniform=not a.per_module_rank,
                                device=a.device, group_bytes=int(a.group_gib * (1 << 30)))
    kept = {n: v for n, v in report.items() if not v["unchanged"]}
    if a.verbose:
        for name, v in report.items():
            print(f"{name:<60} " + ("unchanged" if v["unchanged"] else f"rank {v['new_rank']} (kept {v['kept']})") +
                  f"  |dW| {v['diff_norm']:.4g}  retained {100 * v['fro_retained_of_diff']:.2f}% of it")
    ranks = sorted({v["new_rank"] for v in kept.values()})
    print(f"extracted {len(kept)} modules ({len(report) - len(kept)} unchanged) at rank {ranks[0] if len(ranks) == 1 else ranks} -> {a.save_to}")


if __name__ == "__main__":
    main()
