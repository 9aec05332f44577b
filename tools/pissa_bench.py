"""Times the PiSSA initialisation on the headline adapter set -- 240 pairs of [3072, 3072] bf16 at r = 16, and at r = 64 -- split
into sketch, spectrum + projection and fold, the fold's achieved bytes/s against the HBM roof, and the torch route on the same
GPU (torch.svd_lowrank(q = r, niter = 2) plus the fp32 W - s B A per layer).  One process, the routes interleaved, 5 repeats after
one warm-up; a missing GPU is an error.  Writes profiles/pissa_bench.json (or --out).

    python tools/pissa_bench.py [--pairs 240] [--dim 3072] [--repeats 5] [--out profiles/pissa_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "qwen-image-finetune_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_ROOF = 8.0e12            # bytes/s, the spec figure; a float4 copy reaches about 6.3e12 on this part
HBM_COPY = 6.3e12


def _ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def _stats(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=240)
    ap.add_argument("--dim", type=int, default=3072)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pissa_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pissa_bench: needs a GPU")
    import __graft_entry__ as g
    g.build()
    from qflux_amd import extract, ops, pissa
    dev, n, d = "cuda:0", args.pairs, args.dim
    gen = torch.Generator(device=dev).manual_seed(0)
    master = [(torch.randn(d, d, device=dev, generator=gen) * 0.02).to(torch.bfloat16) for _ in range(n)]
    work = [w.clone() for w in master]
    notes = dict(fold="host clock around ops.lora_fold with the descriptor table built before the window: the enqueue (host check of "
                      "the table) plus the prefix and fold launches, not a profiler's kernel time; bytes_per_s, fraction_of_* and "
                      "fp64_fma_per_s are that call's rates",
                 torch_total="one window over all layers without a synchronisation inside; torch_svd_lowrank / torch_residual are a "
                             "second pass with a synchronisation behind every part of every layer",
                 qfx_total="sketch + spectrum + projection + fold; leaves out building the fold table, the copies of A0 / B0 into the "
                           "adapter parameters and the one readback of A0 / B0 per group that pissa_init_ also does")
    doc = dict(notes=notes, device=torch.cuda.get_device_name(0), workload=f"{n} x [{d}, {d}] bf16, niter = 2, oversample = 8", repeats=args.repeats,
               hbm_roof_bytes_per_s=HBM_ROOF, hbm_copy_bytes_per_s=HBM_COPY)
    for r in (16, 64):
        s, k = 1.0, min(64, r + 8)
        names = [f"m{i:03d}" for i in range(n)]
        fold_bytes = n * (2 * d * d * 2) + n * 2 * r * d * 4           # W read + written, A and B read once (re-reads hit the caches)
        rows = dict(sketch=[], spectrum_project=[], fold=[], qfx_total=[], torch_svd_lowrank=[], torch_residual=[], torch_total=[])
        sketch_ms = []
        inner = extract._sketch

        def timed_sketch(*a, **kw):
            ms, out = _ms(lambda: inner(*a, **kw))
            sketch_ms.append(ms)
            return out

        def ours():
            mats = [(nm, w, None) for nm, w in zip(names, work)]
            extract._sketch = timed_sketch
            try:
                t_fac, (qflat, where, _, _, _, bad) = _ms(lambda: pissa._factors(mats, [r] * n, [s] * n, k, 2, 0, 0))
            finally:
                extract._sketch = inner
            assert not bad
            table = ops.lora_fold_table([(w, oa, ob, r, -s) for w, (oa, ob) in zip(work, where)], device=dev, n_elems=qflat.numel())
            t_fold, _ = _ms(lambda: ops.lora_fold(table, qflat))       # the enqueue (host check of the table included) and the two launches
            return sketch_ms.pop(), t_fac, t_fold

        def torch_whole():                                            # one window, no synchronisation inside
            def run():
                for w in work:
                    U, S, V = torch.svd_lowrank(w.float(), q=r, niter=2)
                    g_ = torch.sqrt(S / s)
                    w.copy_((w.float() - s * ((U * g_) @ (g_[:, None] * V.t()))).to(torch.bfloat16))
            return _ms(run)[0]

        def torch_route():                                            # the split: a synchronisation behind every part of every layer
            t_svd = t_res = 0.0
            for w in work:
                ms, (U, S, V) = _ms(lambda: torch.svd_lowrank(w.float(), q=r, niter=2))
                t_svd += ms
                g_ = torch.sqrt(S / s)

                def residual():
                    B, A = U * g_, g_[:, None] * V.t()
                    w.copy_((w.float() - s * (B @ A)).to(torch.bfloat16))
                ms, _ = _ms(residual)
                t_res += ms
            return t_svd, t_res

        def reset():
            for w, m in zip(work, master):
                w.copy_(m)

        for rep in range(args.repeats + 1):                            # repeat 0 warms both routes up
            reset()
            t_sk, t_fac, t_fold = ours()
            reset()
            t_svd, t_res = torch_route()
            reset()
            t_torch = torch_whole()
            if rep == 0:
                continue
            rows["sketch"].append(t_sk)
            rows["spectrum_project"].append(t_fac - t_sk)
            rows["fold"].append(t_fold)
            rows["qfx_total"].append(t_fac + t_fold)
            rows["torch_svd_lowrank"].append(t_svd)
            rows["torch_residual"].append(t_res)
            rows["torch_total"].append(t_torch)
        out = {key: _stats(v) for key, v in rows.items()}
        fold_s = out["fold"]["median_ms"] * 1e-3
        out["fold"].update(bytes=fold_bytes, bytes_per_s=fold_bytes / fold_s, fraction_of_hbm_roof=fold_bytes / fold_s / HBM_ROOF,
                           fraction_of_copy_rate=fold_bytes / fold_s / HBM_COPY, fp64_fma_per_s=n * d * d * r / fold_s)
        out["speedup_total"] = out["torch_total"]["median_ms"] / out["qfx_total"]["median_ms"]
        out["speedup_residual_pass"] = out["torch_residual"]["median_ms"] / out["fold"]["median_ms"]
        doc[f"rank{r}_k{k}"] = out
        print(f"r = {r}: sketch {out['sketch']['median_ms']:.2f} ms, spectrum + projection {out['spectrum_project']['median_ms']:.2f} ms, "
              f"fold {out['fold']['median_ms']:.3f} ms ({out['fold']['bytes_per_s'] / 1e12:.2f} TB/s); torch: svd_lowrank "
              f"{out['torch_svd_lowrank']['median_ms']:.1f} ms, residual {out['torch_residual']['median_ms']:.1f} ms, one window {out['torch_total']['median_ms']:.1f} ms; "
              f"qfx total {out['qfx_total']['median_ms']:.2f} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
