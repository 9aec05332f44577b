"""Resize a LoRA file to a lower rank by truncated SVD: kohya's resize_lora.py flags over qflux_amd.resize.resize_lora_file (two
launches for the whole file on the GPU; see include/qfx.h, qfx_lora_spectrum / qfx_lora_project).

    python tools/resize_lora.py --model in.safetensors --save_to out.safetensors --new_rank 8 \
        --dynamic_method sv_fro --dynamic_param 0.9 --verbose

Without --per_module_rank every module is allocated the largest rank chosen (zero-padded: the same weights), which
qflux_amd.lora_io.load_lora_adapter can load; with it each module keeps its own rank (for peft, diffusers and ComfyUI).
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen-image-finetune_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", required=True, help="source safetensors file or folder")
    ap.add_argument("--save_to", required=True, help="destination safetensors file or folder")
    ap.add_argument("--new_rank", type=int, required=True, help="the rank, or the cap of a dynamic method")
    ap.add_argument("--dynamic_method", choices=("sv_ratio", "sv_cumulative", "sv_fro"), default=None)
    ap.add_argument("--dynamic_param", type=float, default=None)
    ap.add_argument("--lora_alpha", type=float, default=None, help="the source's lora_alpha when the file carries no metadata")
    ap.add_argument("--per_module_rank", action="store_true", help="one rank per module instead of one zero-padded rank")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--verbose", action="store_true")
    a = ap.parse_args(argv)
    if a.dynamic_method and a.dynamic_param is None:
        ap.error("--dynamic_method needs --dynamic_param")
    from qflux_amd.resize import resize_lora_file
    report = resize_lora_file(a.model, a.save_to, a.new_rank, a.dynamic_method, a.dynamic_param, uniform=not a.per_module_rank,
                              lora_alpha=a.lora_alpha, device=a.device)
    if a.verbose:
        for name, v in report.items():
            print(f"{name:<60} rank {v['old_rank']} -> {v['new_rank']} (kept {v['kept']}, numeric {v['numeric_rank']})  "
                  f"fro retained {100 * v['fro_retained']:.2f}%  sum retained {100 * v['sum_retained']:.2f}%  sigma0 {v['sigma0']:.4g}")
    ranks = sorted({v["new_rank"] for v in report.values()})
    print(f"resized {len(report)} modules to rank {ranks[0] if len(ranks) == 1 else ranks} -> {a.save_to}")


if __name__ == "__main__":
    main()
