"""numpy fp64 restatement of the listing of qfx_lowrank_sketch in include/qfx.h: the difference D = W1 - W0, the Philox +-1 test
matrix, the range finder with q power iterations, the rank-revealing orth (Gram matrix, the cyclic Jacobi solve of
tests/lora_svd_ref.py, T = V L^-1/2, applied twice) and C = Q^T D.  Nothing here calls the library.

fp32=True rounds D, Y, Z, Q and C to float32 where the kernel stores fp32 (the sums themselves stay fp64): an independent
emulation of the kernel's storage precision, used only to size the tolerances of the GPU tests.

Also here: the case list the CPU and the GPU tests share, the metrics both compute, and the stand-ins that replace the device
part of qflux_amd.extract in the CPU plumbing tests."""
import math

import numpy as np

import lora_svd_ref as S
from lora_dropout_ref import philox4x32_10

OMEGA_TAG = 0x4C524B58
ORTH_TOL = 1e-12
MAX_K = 64
ROW_CHUNK = 64          # rows of D a workgroup of the D X launch owns
COL_CHUNK = 64          # columns of D a workgroup of the D^T X launch owns


def omega(nin, k, index=0, seed=0):
    """[in, k] of +-1: +1 where bit j & 31 of word j >> 5 of Philox(key = seed, counter = (i, index, tag, 0)) is clear."""
    w = np.stack(philox4x32_10(np.arange(nin), index, OMEGA_TAG, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), axis=1)      # [in, 4]
    j = np.arange(k)
    bit = (w[:, j >> 5] >> (j & 31).astype(np.uint32)) & np.uint32(1)
    return np.where(bit == 0, 1.0, -1.0)


def _r32(x, fp32):
    return x.astype(np.float32).astype(np.float64) if fp32 else x


def orth_once(Y, orth_tol=ORTH_TOL, fp32=False, max_sweeps=S.MAX_SWEEPS):
    """o(Y) of the listing -> (Y T, kept, converged)."""
    k = Y.shape[1]
    lam, V, _, conv = S.jacobi(Y.T @ Y, max_sweeps)
    perm = sorted(range(k), key=lambda i: (-lam[i], i))
    ls = lam[perm]
    kept = int((ls > orth_tol * ls[0]).sum()) if ls[0] > 0.0 else 0
    T = np.zeros((k, k))
    if kept:
        T[:, :kept] = V[:, perm[:kept]] / np.sqrt(ls[:kept])[None, :]
    return _r32(Y @ T, fp32), kept, conv


def orth(Y, orth_tol=ORTH_TOL, fp32=False):
    Y1, _, c1 = orth_once(Y, orth_tol, fp32)
    Y2, kept, c2 = orth_once(Y1, orth_tol, fp32)
    return Y2, kept, bool(c1 and c2)


def difference(W1, W0=None, fp32=False):
    """D as float64 values: the exact difference of the inputs, or (fp32=True) the one fp32 subtraction of the kernel."""
    if fp32:
        a = np.asarray(W1).astype(np.float32)
        return (a if W0 is None else a - np.asarray(W0).astype(np.float32)).astype(np.float64)
    a = np.asarray(W1, dtype=np.float64)
    return a if W0 is None else a - np.asarray(W0, dtype=np.float64)


def sketch(W1, W0, k, q=2, seed=0, index=0, orth_tol=ORTH_TOL, fp32=False):
    """-> dict(Q [out, k], C [k, in], normsq, kept, converged, skipped)."""
    with np.errstate(all="ignore"):
        D = difference(W1, W0, fp32)
    nout, nin = D.shape
    if not np.isfinite(D).all():
        return dict(Q=np.zeros((nout, k)), C=np.zeros((k, nin)), normsq=0.0, kept=0, converged=False, skipped=True)
    Q, kept, conv = orth(_r32(D @ omega(nin, k, index, seed), fp32), orth_tol, fp32)
    for _ in range(q):
        Z, _, c1 = orth(_r32(D.T @ Q, fp32), orth_tol, fp32)
        Q, kept, c2 = orth(_r32(D @ Z, fp32), orth_tol, fp32)
        conv = conv and c1 and c2
    return dict(Q=Q, C=_r32(Q.T @ D, fp32), normsq=float((D * D).sum()), kept=kept, converged=bool(conv), skipped=False)


def truncate(Q, C, rank):
    """The best rank-`rank` part of Q C (Q's kept columns orthonormal): (U S [out, rank], V^T [rank, in], sv of C)."""
    u, s, vt = np.linalg.svd(C, full_matrices=False)
    return Q @ (u[:, :rank] * s[:rank]), vt[:rank], s


def metrics(D, Q, C, rank, kept):
    """The quantities the GPU tests compare, none of which hangs on the choice of basis."""
    D = np.asarray(D, dtype=np.float64)
    Q, C = np.asarray(Q, dtype=np.float64), np.asarray(C, dtype=np.float64)
    nd = float(np.linalg.norm(D))
    s = np.linalg.svd(C, compute_uv=False)
    P = Q @ C
    return dict(residual=float(np.linalg.norm(D - P)) / nd if nd > 0 else 0.0,
                sv=(s[:rank] / s[0]) if s[0] > 0 else s[:rank],
                orth=float(np.abs(Q[:, :kept].T @ Q[:, :kept] - np.eye(kept)).max()) if kept else 0.0,
                product=P / nd if nd > 0 else P)


def well_determined(D, k):
    """Q C is well determined: rank(D) <= k, or a spectral gap at k (s_{k+1} / s_k <= 0.1)."""
    s = np.linalg.svd(np.asarray(D, dtype=np.float64), compute_uv=False)
    if k >= len(s) or s[0] == 0.0 or s[k] <= 1e-10 * s[0]:
        return True
    return bool(s[k] <= 0.1 * s[k - 1])


# ---------------------------------------------------------------------- the case list the CPU and the GPU tests share

def _orthonormal(rng, n, m):
    q, _ = np.linalg.qr(rng.standard_normal((n, m)))
    return q


def with_spectrum(rng, nout, nin, s):
    """U diag(s) V^T [out, in] fp64, len(s) <= min(out, in)."""
    s = np.asarray(s, dtype=np.float64)
    return (_orthonormal(rng, nout, len(s)) * s[None, :]) @ _orthonormal(rng, nin, len(s)).T


def _gap(n, k):
    """0.9^i with a drop by 100 behind the first k."""
    i = np.arange(n)
    return 0.9 ** i * np.where(i < k, 1.0, 0.01)


# label, out, in, k, spectrum, dtype, base (W0: None = absent, else the scale of a Gaussian W0), odd (unaligned addresses and odd ld)
CASES = [
    ("160x224_k16_gap", 160, 224, 16, lambda n: _gap(n, 16), "fp32", 1.0, False),
    ("97x131_k5_odd", 97, 131, 5, lambda n: _gap(n, 5), "fp32", 1.0, True),
    ("48x1000_k24", 48, 1000, 24, lambda n: _gap(n, 24), "fp32", None, False),
    ("1000x48_k24", 1000, 48, 24, lambda n: 0.8 ** np.arange(n), "fp32", None, False),
    ("192x256_k64", 192, 256, 64, lambda n: _gap(n, 64), "fp32", None, False),
    ("8x300_k16", 8, 300, 16, lambda n: 1.0 / (1.0 + np.arange(n)), "fp32", None, False),          # k > out
    ("65x96_k8_rowchunk+1", ROW_CHUNK + 1, 96, 8, lambda n: _gap(n, 8)[:8], "fp32", None, False),      # exact rank 8
    ("96x65_k8_colchunk+1", 96, COL_CHUNK + 1, 8, lambda n: _gap(n, 8), "fp32", 1.0, True),
    ("160x224_k16_bf16", 160, 224, 16, lambda n: _gap(n, 16), "bf16", 1.0, False),
    ("97x131_k5_bf16_odd", 97, 131, 5, lambda n: 0.8 ** np.arange(n), "bf16", None, True),
]


def _bf16_round(x):
    """float array -> the nearest bf16 values (ties to even), as float32."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    return r.astype(np.uint32).view(np.float32)


def make_cases(seed=11):
    """[dict(label, W1, W0 (or None), k, dtype, odd, rank)]: W1 / W0 float32 arrays holding fp32 or bf16 values."""
    rng = np.random.default_rng(seed)
    out = []
    for label, nout, nin, k, spec, dtype, base, odd in CASES:
        D = with_spectrum(rng, nout, nin, spec(min(nout, nin)))
        if base is None:
            W1, W0 = D.astype(np.float32), None
        else:
            W0 = (rng.standard_normal((nout, nin)) * base * 0.05).astype(np.float32)
            W1 = (W0.astype(np.float64) + D).astype(np.float32)
        if dtype == "bf16":
            W1, W0 = _bf16_round(W1), (None if W0 is None else _bf16_round(W0))
        out.append(dict(label=label, W1=W1, W0=W0, k=k, dtype=dtype, odd=odd, rank=max(1, k // 2)))
    return out


def deviations(ref, got_metrics, got_normsq):
    """The five deviations (a) .. (e) of one result from the fp64 restatement's metrics `ref` (with ref['normsq'])."""
    return dict(residual=abs(got_metrics["residual"] - ref["residual"]),
                sv=float(np.abs(got_metrics["sv"] - ref["sv"]).max()),
                orth=abs(got_metrics["orth"] - ref["orth"]),
                normsq=abs(got_normsq - ref["normsq"]) / ref["normsq"] if ref["normsq"] > 0 else abs(got_normsq),
                product=float(np.abs(got_metrics["product"] - ref["product"]).max()))


# ---------------------------------------------------------------------- stand-ins for the device part of qflux_amd.extract

def sketch_standin(mats, k, power_iters, seed):
    """What qflux_amd.extract._sketch returns, from the restatement: (pflat, pairs, normsq, info, skipped) with torch tensors."""
    import torch
    chunks, pairs, normsq, info, off, skipped = [], [], [], [], 0, 0
    for i, (name, W1, W0) in enumerate(mats):
        r = sketch(W1.float().numpy(), None if W0 is None else W0.float().numpy(), k, power_iters, seed, i, fp32=True)
        nout, nin = W1.shape
        oa, ob = off, off + (k * nin + 63) // 64 * 64
        off = ob + (nout * k + 63) // 64 * 64
        chunks.append((oa, r["C"], ob, r["Q"]))
        pairs.append((name, oa, ob, k, nin, nout, 1.0))
        normsq.append(r["normsq"])
        info.append((r["kept"], int(r["converged"])))
        skipped += int(r["skipped"])
    p = torch.zeros(off, dtype=torch.float32)
    for oa, C, ob, Q in chunks:
        p[oa:oa + C.size] = torch.from_numpy(C.astype(np.float32)).reshape(-1)
        p[ob:ob + Q.size] = torch.from_numpy(Q.astype(np.float32)).reshape(-1)
    return p, pairs, torch.tensor(normsq, dtype=torch.float64), torch.tensor(info, dtype=torch.int32), skipped


def resize_standin(pflat, pairs, new_rank, dynamic_method=None, dynamic_param=None, uniform=True):
    """resize.resize_pairs from tests/lora_svd_ref.py: the same (tensors, alphas, report)."""
    import torch
    picks = []
    for name, oa, ob, r, nin, nout, scaling in pairs:
        A = pflat[oa:oa + r * nin].view(r, nin).numpy()
        B = pflat[ob:ob + nout * r].view(nout, r).numpy()
        sp = S.spectrum(A, B)
        k, fro, cum = S.select_rank(sp["sv"].tolist(), new_rank, dynamic_method, dynamic_param, sp["rho"])
        picks.append((name, A, B, sp, k, fro, cum, r, scaling))
    r_max = max(p[4] for p in picks)
    tensors, alphas, report = {}, {}, {}
    for name, A, B, sp, k, fro, cum, r, scaling in picks:
        r_dst = r_max if uniform else k
        A2, B2 = S.project(A, B, sp["T_B"], sp["T_A"], k, r_dst)
        tensors[name] = (torch.from_numpy(A2), torch.from_numpy(B2))
        alphas[name] = float(scaling) * r_dst
        report[name] = dict(old_rank=int(r), new_rank=int(r_dst), kept=int(k), fro_retained=fro, sum_retained=cum,
                            sigma0=float(sp["sv"][0]) * abs(float(scaling)), numeric_rank=int(sp["rho"]), converged=bool(sp["converged"]),
                            sv=[float(x) for x in sp["sv"]])
    return tensors, alphas, report


def fro(x):
    return math.sqrt(float((np.asarray(x, dtype=np.float64) ** 2).sum()))
