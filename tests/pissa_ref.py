"""Numpy restatement of the PiSSA pieces (include/qfx.h, qfx_lora_fold; qflux_amd/pissa.py): the fold listing operation for
operation, the balanced split from numpy.linalg.svd, and peft's PiSSA -> LoRA conversion.  Nothing here calls the library; peft
was not at hand: the formulas of the header and of pissa.py's docstring are the specification."""
import numpy as np

from lora_dropout_ref import bf16_float, bf16_rne      # fp32 -> bf16 bits, nearest even; bits -> fp32

BF16, FP32 = 0, 1


def fold(W, A, B, c, dtype=FP32):
    """The qfx_lora_fold listing for one matrix.  W: float32 [out, in] for dtype FP32, uint16 bf16 bits for BF16; A [r, in] and
    B [out, r] float32; c a float32 coefficient.  Returns the new W in W's own representation."""
    A64, B64 = np.asarray(A, dtype=np.float32).astype(np.float64), np.asarray(B, dtype=np.float32).astype(np.float64)
    w = (bf16_float(W) if dtype == BF16 else np.asarray(W, dtype=np.float32)).astype(np.float64)
    s = np.zeros(w.shape, dtype=np.float64)                      # +0
    for j in range(A64.shape[0]):                                # ascending j; the product of two widened fp32 values is exact
        s = s + B64[:, j:j + 1] * A64[j:j + 1, :]                # one rounding: the addition
    t = np.float64(np.float32(c)) * s                            # one rounding
    wn = w + t                                                   # one rounding
    w32 = wn.astype(np.float32)                                  # nearest even
    return bf16_rne(w32) if dtype == BF16 else w32


def split(W, r, s):
    """The balanced split of the truncated SVD of W (fp64): B0 = U sqrt(S / s) [out, r], A0 = sqrt(S / s) V^T [r, in], and the
    singular values.  Components with sigma_i == 0 are zero columns / rows."""
    U, sig, Vt = np.linalg.svd(np.asarray(W, dtype=np.float64), full_matrices=False)
    k = min(r, sig.shape[0])
    g = np.zeros(r)
    g[:k] = np.sqrt(sig[:k] / s)
    B0, A0 = np.zeros((W.shape[0], r)), np.zeros((r, W.shape[1]))
    B0[:, :k], A0[:k] = U[:, :k] * g[:k], g[:k, None] * Vt[:k]
    return B0, A0, sig


def retained(sig, r):
    """sqrt(sum_{i<r} sigma_i^2) / ||W||_F from the full spectrum."""
    tot = float(np.sqrt((sig ** 2).sum()))
    return float(np.sqrt((sig[:r] ** 2).sum())) / tot if tot > 0 else 1.0


def to_lora(A, B, A0, B0, lora_alpha):
    """peft's conversion: (A' [2r, in], B' [out, 2r], lora_alpha') with s B' A' = s (B A - B0 A0) at the unchanged scaling."""
    return np.concatenate([A, -A0], axis=0), np.concatenate([B, B0], axis=1), 2.0 * lora_alpha


def planted(rng, nout, nin, sigmas=(8.0, 4.0, 2.0, 1.0), tail=1e-3):
    """A matrix with the leading singular values `sigmas` and a full-rank tail at `tail` and below: its rank-len(sigmas)
    factorisation is well determined."""
    n = min(nout, nin)
    U, _ = np.linalg.qr(rng.standard_normal((nout, n)))
    V, _ = np.linalg.qr(rng.standard_normal((nin, n)))
    sv = np.concatenate([np.asarray(sigmas, dtype=np.float64), tail * (0.9 ** np.arange(n - len(sigmas)))])
    return (U * sv) @ V.T
