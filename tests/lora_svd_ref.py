"""numpy fp64 restatement of the listing of qfx_lora_spectrum / qfx_lora_project in include/qfx.h: the two Gram matrices, the two
cyclic Jacobi solves (round-robin ordering, the rotations of a round formed from one state of the matrix), the transforms T_B / T_A,
the projection and resize.select_rank.  Every fp64 operation rounds once, as the kernel's do (the file is built without FMA
contraction); only the order of the Gram sums differs (numpy's matmul here, the kernel's fixed sweep there)."""
import math

import numpy as np

MAX_RANK = 64
RANK_TOL = 1e-6
MAX_SWEEPS = 30


def round_pairs(n, rd):
    """The disjoint index pairs (p < q) of round rd of a sweep over n indices; pairs with the padding index of an odd n left out."""
    m = (n + 1) & ~1
    mod = m - 1
    out = []
    for k in range(m // 2):
        a, b = (mod, rd) if k == 0 else ((rd + k) % mod, (rd - k) % mod)
        p, q = min(a, b), max(a, b)
        if q < n:
            out.append((p, q))
    return out


def jacobi(M, max_sweeps=MAX_SWEEPS):
    """Symmetric M [n, n] -> (diagonal, V, sweeps, converged) with M = V diag V^T."""
    M = np.array(M, dtype=np.float64)
    n = M.shape[0]
    V = np.eye(n)
    thr = 2.0 ** -52 * math.sqrt(float((M * M).sum())) / n
    iu = np.triu_indices(n, 1)
    sweeps, conv = 0, False
    m = (n + 1) & ~1
    with np.errstate(all="ignore"):
        for s in range(max_sweeps + 1):
            off = np.abs(M[iu]).max() if n > 1 else 0.0
            if off <= thr:
                conv = True
                break
            if s == max_sweeps:
                break
            for rd in range(m - 1):
                pq = round_pairs(n, rd)
                if not pq:
                    continue
                P = np.array([p for p, _ in pq])
                Q = np.array([q for _, q in pq])
                apq = M[P, Q]
                tau = (M[Q, Q] - M[P, P]) / (2.0 * apq)
                t = np.copysign(1.0, tau) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                sn = t * c
                rot = np.abs(apq) > 0.0
                c = np.where(rot, c, 1.0)
                sn = np.where(rot, sn, 0.0)
                for X in (M, V):
                    x, y = X[:, P].copy(), X[:, Q].copy()
                    X[:, P] = c * x - sn * y
                    X[:, Q] = sn * x + c * y
                x, y = M[P, :].copy(), M[Q, :].copy()
                M[P, :] = c[:, None] * x - sn[:, None] * y
                M[Q, :] = sn[:, None] * x + c[:, None] * y
                M[P, Q] = 0.0
                M[Q, P] = 0.0
            sweeps += 1
    return np.diag(M).copy(), V, sweeps, conv


def _dot_in_order(X, Y):
    """X [a, r] @ Y [r, b], the r terms added in index order from 0."""
    acc = np.zeros((X.shape[0], Y.shape[1]))
    for k in range(X.shape[1]):
        acc = acc + X[:, k:k + 1] * Y[k:k + 1, :]
    return acc


def spectrum(A, B, rank_tol=RANK_TOL, max_sweeps=MAX_SWEEPS, transforms=True):
    """A [r, in], B [out, r] fp32 -> dict(sv [r], rho, sweeps (2), converged, T_B [r, r], T_A [r, r])."""
    A64, B64 = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    r = A64.shape[0]
    GA, GB = A64 @ A64.T, B64.T @ B64
    if not (np.isfinite(GA).all() and np.isfinite(GB).all()):
        z = np.zeros((r, r))
        return dict(sv=np.zeros(r), rho=0, sweeps=(0, 0), converged=False, T_B=z, T_A=z.copy(), skipped=True)
    lam, V, sw_a, conv_a = jacobi(GA, max_sweeps)
    lamh = np.where(lam > 0.0, np.sqrt(np.where(lam > 0.0, lam, 0.0)), 0.0)
    K = lamh[:, None] * _dot_in_order(V.T.copy(), GB)
    H = _dot_in_order(K, V) * lamh[None, :]
    Hs = 0.5 * (H + H.T)
    H = np.where(np.eye(r, dtype=bool), H, Hs)
    th, W, sw_h, conv_h = jacobi(H, max_sweeps)
    th = np.where(th > 0.0, th, 0.0)
    perm = sorted(range(r), key=lambda i: (-th[i], i))
    ths = th[perm]
    sv = np.sqrt(ths)
    rho = int((sv > rank_tol * sv[0]).sum()) if sv[0] > 0.0 else 0
    out = dict(sv=sv, rho=rho, sweeps=(sw_a, sw_h), converged=bool(conv_a and conv_h), skipped=False)
    if transforms:
        Wp = W[:, perm]
        TB = _dot_in_order(V * lamh[None, :], Wp)
        TB[:, rho:] = 0.0
        TA = np.zeros((r, r))
        if rho:
            TA[:rho] = _dot_in_order(Wp.T.copy(), K)[:rho] / ths[:rho, None]
        out.update(T_B=TB, T_A=TA)
    return out


def project(A, B, T_B, T_A, k, r_dst):
    """-> (A' [r_dst, in], B' [out, r_dst]) fp32: fp64 products and sums in index order, one rounding to fp32; +0.0 beyond k."""
    A64, B64 = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    A2 = np.zeros((r_dst, A64.shape[1]), dtype=np.float32)
    B2 = np.zeros((B64.shape[0], r_dst), dtype=np.float32)
    B2[:, :k] = _dot_in_order(B64, T_B[:, :k]).astype(np.float32)
    A2[:k] = _dot_in_order(T_A[:k], A64).astype(np.float32)
    return A2, B2


def select_rank(sv, new_rank, dynamic_method=None, dynamic_param=None, numeric_rank=None):
    """The listing of resize.select_rank: (k, retained Frobenius share, retained sum share) over one descending spectrum."""
    sv = [float(x) for x in sv]
    r = len(sv)
    if r < 1 or int(new_rank) < 1:
        raise ValueError("select_rank: an empty spectrum or new_rank < 1")
    s1, s2 = math.fsum(sv), math.fsum(x * x for x in sv)
    if dynamic_method is None:
        k = int(new_rank)
    elif dynamic_method == "sv_ratio":
        if dynamic_param is None or not dynamic_param >= 1:
            raise ValueError("sv_ratio: dynamic_param must be >= 1")
        k = sum(1 for x in sv if x >= sv[0] / dynamic_param)
    elif dynamic_method in ("sv_cumulative", "sv_fro"):
        if dynamic_param is None or not 0 < dynamic_param <= 1:
            raise ValueError(f"{dynamic_method}: dynamic_param must be in (0, 1]")
        k = r
        for kk in range(1, r + 1):
            if dynamic_method == "sv_cumulative":
                share = math.fsum(sv[:kk]) / s1 if s1 > 0 else 1.0
            else:
                share = math.sqrt(math.fsum(x * x for x in sv[:kk]) / s2) if s2 > 0 else 1.0
            if share >= dynamic_param:
                k = kk
                break
    else:
        raise ValueError(f"unknown dynamic_method {dynamic_method!r}")
    nr = r if numeric_rank is None else int(numeric_rank)
    k = max(1, min(k, int(new_rank), r, max(nr, 1)))
    fro = math.sqrt(math.fsum(x * x for x in sv[:k]) / s2) if s2 > 0 else 1.0
    cum = math.fsum(sv[:k]) / s1 if s1 > 0 else 1.0
    return k, fro, cum


# ---------------------------------------------------------------------- the case list the CPU and the GPU tests share

SHAPES = [(1, 5, 3), (4, 70, 37), (16, 256, 192), (64, 320, 128), (16, 64, 8)]      # the last: r > out, numeric rank <= 8
FULL = (16, 3072, 3072)


def _orth(rng, n, k):
    q, _ = np.linalg.qr(rng.standard_normal((n, k)))
    return q


def make_cases(full=True, seed=7):
    """[(label, A [r, in] fp32, B [out, r] fp32)]: the shapes above with Gaussian weights, one full-width pair, a pair with B = 0,
    a pair with two equal rows in A, a pair built with a graded spectrum (s_i / s_0 from 1 down to 1e-4)."""
    rng = np.random.default_rng(seed)
    cases = []
    for r, nin, nout in SHAPES + ([FULL] if full else []):
        cases.append((f"{r}x{nin}x{nout}", (rng.standard_normal((r, nin)) * 0.1).astype(np.float32),
                      (rng.standard_normal((nout, r)) * 0.1).astype(np.float32)))
    cases.append(("b_zero", (rng.standard_normal((8, 48)) * 0.1).astype(np.float32), np.zeros((40, 8), dtype=np.float32)))
    A = (rng.standard_normal((8, 96)) * 0.1).astype(np.float32)
    A[5] = A[2]
    cases.append(("equal_rows", A, (rng.standard_normal((64, 8)) * 0.1).astype(np.float32)))
    s = 10.0 ** np.linspace(0.0, -4.0, 16)
    mix = rng.standard_normal((16, 16)) + 4.0 * np.eye(16)                              # B = U S X, A = X^-1 V^T: B A = U S V^T
    cases.append(("graded", (np.linalg.inv(mix) @ _orth(rng, 128, 16).T).astype(np.float32),
                  (_orth(rng, 96, 16) * s[None, :] @ mix).astype(np.float32)))
    return cases


def lapack_sv(A, B):
    """The singular values of the fp64 product B A by LAPACK, length r, descending."""
    import torch
    P = torch.from_numpy(np.asarray(B, dtype=np.float64)) @ torch.from_numpy(np.asarray(A, dtype=np.float64))
    s = torch.linalg.svdvals(P).numpy()
    r = A.shape[0]
    return np.concatenate([s, np.zeros(max(0, r - len(s)))])[:r]


def sq_error(sv, ref):
    """max_i |sv_i^2 - ref_i^2| / ref_0^2; an all-zero reference asks for an all-zero spectrum (error 0, else inf)."""
    d = float(np.abs(np.asarray(sv) ** 2 - np.asarray(ref) ** 2).max())
    if ref[0] == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / float(ref[0]) ** 2


def unambiguous(ref, lo=1e-8, hi=1e-5):
    """No singular value with s_i / s_0 in [lo, hi]: the numeric rank at rank_tol = 1e-6 does not hang on rounding."""
    if ref[0] == 0.0:
        return True
    q = np.asarray(ref) / ref[0]
    return not bool(((q >= lo) & (q <= hi)).any())
