"""Time the spectrum launch (qfx_lora_spectrum, with its workspace) and the project launch (qfx_lora_project) at the headline adapter
set -- 240 pairs, 3072 x 3072, r = 16 and r = 64 -- against the same work in torch on the same GPU:
  torch_qr   QR of B and A^T plus an r x r SVD, for all pairs (a host loop of torch.linalg calls)
  torch_full kohya's formulation: torch.linalg.svd of the [out, in] product -- FOUR pairs only, stated as four pairs
Warm-up, then the variants interleaved over --repeats rounds; median and min..max of each are reported.

    python tools/lora_svd_bench.py [--pairs 240] [--repeats 7] [--out profiles/lora_svd_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen-image-finetune_amd"))


def _timed(fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def bench_rank(r, n_pairs, dim, repeats, new_rank):
    import torch
    from qflux_amd import ops
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(r)
    na, nb = r * dim, dim * r
    p = torch.randn(n_pairs * (na + nb), device=dev, generator=g) * 0.05
    rows = [(i * (na + nb), i * (na + nb) + na, r, dim, dim) for i in range(n_pairs)]
    lay = ops.lora_svd_table(rows, device=dev, n_elems=p.numel())
    sv = torch.zeros(n_pairs, 64, dtype=torch.float64, device=dev)
    info = torch.zeros(n_pairs, 4, dtype=torch.int32, device=dev)
    skipped = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.zeros(n_pairs * ops.LORA_SVD_WS_DOUBLES, dtype=torch.float64, device=dev)
    k = new_rank
    dst = [(i * 2 * k * dim, i * 2 * k * dim + k * dim, k, k) for i in range(n_pairs)]
    q = torch.zeros(n_pairs * 2 * k * dim, device=dev)
    tab = ops.lora_project_table(lay, dst, device=dev, n_elems=q.numel())
    views = [(p[oa:oa + na].view(r, dim), p[ob:ob + nb].view(dim, r)) for oa, ob, *_ in rows]

    def torch_qr():
        for A, B in views:
            qb, rb = torch.linalg.qr(B)
            qa, ra = torch.linalg.qr(A.T)
            u, s, vh = torch.linalg.svd(rb @ ra.T)
            (qb @ u[:, :k]) * s[:k]
            vh[:k] @ qa.T

    def torch_full():
        for A, B in views[:4]:
            u, s, vh = torch.linalg.svd(B @ A, full_matrices=False)
            u[:, :k] * s[:k]
            vh[:k]

    variants = {"spectrum": lambda: ops.lora_spectrum(p, lay, sv, info, skipped, ws=ws),
                "spectrum_only": lambda: ops.lora_spectrum(p, lay, sv, info, skipped),
                "project": lambda: ops.lora_project(p, q, lay, tab, ws),
                "torch_qr": torch_qr, "torch_full_4_pairs": torch_full}
    for fn in variants.values():          # warm-up: code objects, rocSOLVER / hipBLAS handles, caches
        fn()
        fn()
    times = {name: [] for name in variants}
    for _ in range(repeats):              # interleaved: drift hits every variant alike
        for name, fn in variants.items():
            times[name].append(_timed(fn))
    assert int(skipped.item()) == 0 and bool((info[:, 3] == 1).all())
    return {name: dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=240)
    ap.add_argument("--dim", type=int, default=3072)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "dim": a.dim, "repeats": a.repeats,
           "note": "torch_full_4_pairs times FOUR pairs, every other row all pairs; project keeps r / 2 components",
           "r16": bench_rank(16, a.pairs, a.dim, a.repeats, 8), "r64": bench_rank(64, a.pairs, a.dim, a.repeats, 32)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
