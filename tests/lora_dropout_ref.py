"""Independent numpy restatement of the adapter-dropout mask (include/qfx.h): Philox4x32-10, the counter layout, the factor
f[token, rank], and the kernel's arithmetic on the split rank-r activation.  Nothing here calls the library."""
from __future__ import annotations

import zlib

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
RANK_C0 = 0xFFFFFFE0
U32 = np.uint32
U64 = np.uint64


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Arrays (broadcast together) of counters and keys -> the four uint32 output words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=U64) for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    mask = U64(0xFFFFFFFF)
    for _ in range(10):
        p0 = U64(M0) * c0
        p1 = U64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> U64(32)) ^ c1 ^ k0) & mask, p1 & mask, ((p0 >> U64(32)) ^ c3 ^ k1) & mask, p0 & mask
        k0 = (k0 + U64(W0)) & mask
        k1 = (k1 + U64(W1)) & mask
    return tuple(v.astype(U32) for v in (c0, c1, c2, c3))


def site_key(name: str) -> int:
    """The 32-bit key of an adapter: crc32 of the adapted module's qualified name."""
    return zlib.crc32(name.encode()) & 0xFFFFFFFF


def threshold(p: float) -> int:
    return int(np.floor(float(p) * 4294967296.0))


def make_state(seed=0, step=0, active=1, network_dropout=0.0, rank_dropout=0.0, sample0=0):
    """The 8 state words as the host forms them."""
    scale = np.float32(1.0 / ((1.0 - float(network_dropout)) * (1.0 - float(rank_dropout))))
    return np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, step, active, threshold(network_dropout), threshold(rank_dropout),
                     int(scale.view(U32)), sample0], dtype=U32)


def factors(state, site, b, t, r):
    """f [len(b), len(t), r] (float32) of adapter `site`: local samples b, tokens t, ranks 0..r-1."""
    seed_lo, seed_hi, step, _, thr_e, thr_r, scale_bits, sample0 = (int(v) for v in np.asarray(state, dtype=U32))
    scale = np.array([scale_bits], dtype=U32).view(np.float32)[0]
    b = np.asarray(b, dtype=U64).reshape(-1, 1, 1)
    t = np.asarray(t, dtype=U64).reshape(1, -1, 1)
    nq = (r + 3) // 4
    q = np.arange(nq, dtype=U64).reshape(1, 1, -1)
    sample = (b + U64(sample0)) & U64(0xFFFFFFFF)
    keep = np.ones((b.shape[0], t.shape[1], nq * 4), dtype=bool)
    if thr_e:
        w = philox4x32_10((t * U64(32) + q) & U64(0xFFFFFFFF), sample, step, site, seed_lo, seed_hi)
        keep &= np.stack(w, axis=-1).reshape(keep.shape) >= U32(thr_e)
    if thr_r:
        w = philox4x32_10(U64(RANK_C0) + q, sample, step, site, seed_lo, seed_hi)
        kr = np.stack(w, axis=-1).reshape(b.shape[0], 1, nq * 4) >= U32(thr_r)
        keep &= kr
    return np.where(keep[:, :, :r], scale, np.float32(0.0)).astype(np.float32)


def problem_factors(state, sites, M, rows_per_batch, group_R):
    """f [M, len(sites) * group_R] of one kernel problem: row m = sample m // rows_per_batch, token m % rows_per_batch."""
    nb = (M + rows_per_batch - 1) // rows_per_batch
    cols = []
    for s in sites:
        f = factors(state, s, np.arange(nb), np.arange(rows_per_batch), group_R)      # [nb, rpb, gR]
        cols.append(f.reshape(nb * rows_per_batch, group_R)[:M])
    return np.concatenate(cols, axis=1)


def bf16_rne(x):
    """float32 array -> bf16 bits (uint16), round to nearest even (finite inputs)."""
    u = np.asarray(x, dtype=np.float32).view(U32).astype(U64)
    r = (u + U64(0x7FFF) + ((u >> U64(16)) & U64(1))) >> U64(16)
    return r.astype(np.uint16)


def bf16_float(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(U32) << U32(16)).view(np.float32)


def apply_ref(ut_hi, ut_lo, f):
    """The kernel's arithmetic: ut_hi / ut_lo uint16 [R, M] (bf16 bits), f float32 [M, R] -> (hi', lo') uint16 [R, M]."""
    u = bf16_float(ut_hi) + bf16_float(ut_lo)
    v = np.where(f.T == 0, np.float32(0.0), (u * f.T).astype(np.float32)).astype(np.float32)      # dropped: +0, not -0
    hi = bf16_rne(v)
    lo = bf16_rne((v - bf16_float(hi)).astype(np.float32))
    return hi, lo


def ext_ref(hi, lo, M, group_R, group_stride, ld_ext, base=None):
    """ext uint16 [M, ld_ext] from the transposed split [R, >= M]: per group [hi | lo | hi] at column g * group_stride."""
    R = hi.shape[0]
    ext = np.zeros((M, ld_ext), dtype=np.uint16) if base is None else base.copy()
    for g in range(R // group_R):
        h = hi[g * group_R:(g + 1) * group_R, :M].T
        l_ = lo[g * group_R:(g + 1) * group_R, :M].T
        c = g * group_stride
        ext[:, c:c + group_R] = h
        ext[:, c + group_R:c + 2 * group_R] = l_
        ext[:, c + 2 * group_R:c + 3 * group_R] = h
    return ext
