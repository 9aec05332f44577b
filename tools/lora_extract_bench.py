"""Time the LoRA extraction (qfx_lowrank_sketch, then qfx_lora_spectrum + qfx_lora_project) against torch on one GPU.

Workload: sixteen 3072 x 3072 and four 12288 x 3072 bf16 difference matrices with a decaying spectrum, at rank 16 (k = 24) and
rank 56 (k = 64), q = 2.  Timed: the sketch alone, and the sketch plus spectrum plus projection (extract_pairs).  Comparators on
the same GPU: torch.svd_lowrank(D, q=k, niter=2) over all twenty matrices (the fair one), and a full torch.linalg.svd of four
3072 x 3072 matrices (what kohya's script does per layer).  Warm-up, then the variants interleaved over --repeats rounds; median and
min..max of each are reported, with the bytes/s of one sketch pass and each method's error ratio to the Eckart-Young optimum.

    python tools/lora_extract_bench.py --out profiles/lora_extract_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen-image-finetune_amd"))

import torch  # noqa: E402

DEV = "cuda:0"
HBM_ROOF = 8.0e12          # bytes/s, MI355X data sheet


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _matrix(nout, nin, g, decay=0.9, n_sv=256):
    """bf16(U diag(decay^i) V^T): a decaying spectrum over the bf16 rounding floor."""
    U, _ = torch.linalg.qr(torch.randn(nout, n_sv, generator=g, device=DEV))
    V, _ = torch.linalg.qr(torch.randn(nin, n_sv, generator=g, device=DEV))
    s = decay ** torch.arange(n_sv, device=DEV, dtype=torch.float32)
    return ((U * s) @ V.T).to(torch.bfloat16)


def _stats(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from qflux_amd import ops
    from qflux_amd.extract import _align, extract_pairs
    g = torch.Generator(device=DEV).manual_seed(1)
    shapes = [(3072, 3072)] * 16 + [(12288, 3072)] * 4
    mats = [(f"m{i}", _matrix(no, ni, g), None) for i, (no, ni) in enumerate(shapes)]
    bytes_pass = sum(no * ni * 2 for no, ni in shapes)
    res = dict(device=torch.cuda.get_device_name(0), workload="16 x [3072, 3072] + 4 x [12288, 3072] bf16, q = 2", repeats=a.repeats,
               bytes_per_pass=bytes_pass, hbm_roof_bytes_per_s=HBM_ROOF)
    # the optimum of the first 3072 x 3072 and the first 12288 x 3072 matrix, for the error ratios
    probe = {0: None, 16: None}
    for i in probe:
        probe[i] = torch.linalg.svdvals(mats[i][1].float())
    for rank, k in ((16, 24), (56, 64)):
        rows, off = [], 0
        for _, W1, _ in mats:
            no, ni = W1.shape
            rows.append((W1, None, k, off, off + _align(k * ni)))
            off += _align(k * ni) + _align(no * k)
        lay = ops.lowrank_table(rows, device=DEV, n_elems=off)
        p = torch.zeros(off, device=DEV)
        normsq = torch.zeros(len(mats), dtype=torch.float64, device=DEV)
        info = torch.zeros(len(mats), 2, dtype=torch.int32, device=DEV)
        skipped = torch.zeros(1, dtype=torch.int32, device=DEV)
        ws = torch.empty(lay.ws_bytes, dtype=torch.uint8, device=DEV)
        out = {}

        def sketch():
            ops.lowrank_sketch(lay, p, normsq, info, skipped, ws, power_iters=2)

        def full():
            out["full"] = extract_pairs(mats, rank, oversample=k - rank)

        def lowrank():
            out["torch"] = [torch.svd_lowrank(W1.float(), q=k, niter=2) for _, W1, _ in mats]

        variants = dict(sketch=sketch, sketch_spectrum_project=full, torch_svd_lowrank=lowrank)
        times = {n: [] for n in variants}
        for fn in variants.values():
            fn()                                  # warm-up
        for _ in range(a.repeats):                # interleaved: drift hits every variant alike
            for n, fn in variants.items():
                times[n].append(_timed(fn))
        row = {n: _stats(t) for n, t in times.items()}
        passes = 2 + 2 * 2                        # D Omega, q x (D^T Q, D Z), Q^T D
        row["sketch"]["bytes_per_s_of_a_pass_if_only_passes_took_time"] = bytes_pass * passes / (row["sketch"]["median_ms"] * 1e-3)
        row["sketch"]["fraction_of_hbm_roof"] = row["sketch"]["bytes_per_s_of_a_pass_if_only_passes_took_time"] / HBM_ROOF
        ratios = {}
        for i, sv in probe.items():
            D = mats[i][1].double()
            best = float(sv[rank:].double().pow(2).sum().sqrt())
            A2, B2 = out["full"][0][f"m{i}"]
            U, S, V = out["torch"][i]
            ratios[f"m{i}"] = dict(qfx=float(torch.linalg.norm(B2.double() @ A2.double() - D)) / best,
                                   torch_svd_lowrank=float(torch.linalg.norm((U[:, :rank] * S[:rank]).double() @ V[:, :rank].T.double() - D)) / best)
        row["error_ratio_to_optimum"] = ratios
        res[f"rank{rank}_k{k}"] = row
        print(f"rank {rank} k {k}", json.dumps(row), flush=True)
    four = [m[1].float() for m in mats[:4]]

    def dense():
        for D in four:
            torch.linalg.svd(D, full_matrices=False)

    dense()
    res["torch_linalg_svd_four_3072x3072"] = _stats([_timed(dense) for _ in range(a.repeats)])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
