"""CPU restatement (torch only) of the attention entry points of csrc/qfx_attn.hip, csrc/qfx_attn64.hip and csrc/qfx_attn_bwd1.hip as
include/qfx.h states them -- qfx_attn_fwd, qfx_attn_bwd_prep, qfx_attn_bwd_dq, qfx_attn_bwd_dkv, qfx_attn_bwd_fused -- the yardstick
of tests/test_attn_gpu.py.  With c2 = scale log2 e, s2 = c2 Q K^T + key_mask log2 e (the log2-domain scores) and q = round to bf16:

    forward    P = exp2(s2 - rowmax),  l = rowsum(P),  O = q(P V / l),  lse2 = rowmax + log2 l  (fp32),
               part[0][h] = O_h (W_hi + W_lo)_h^T  (fp32, from the bf16 O)
    backward   dsum = rowsum(dO O)  of the O that was PASSED IN,  P = exp2(s2 - lse2)  of the lse2 that was passed in,
               dP = dO V^T,  dS = P (dP - dsum),  dV = q(P^T dO),  dQ = q(scale dS K),  dK = q(scale dS^T Q)
    fused      (qk_saved != NULL) dQ, dK = rowkernel_ref.qk_bwd of the bf16-ROUNDED dQ, dK above (the header's wording: "the arithmetic
               of qfx_qk_norm_rope_bwd on the bf16-rounded attention gradient"); part[1..3][h] = X_h (W_hi + W_lo)_h^T with X the
               bf16 d(pre-norm q), d(pre-norm k), dV; rows s < T use the text weights (w_pk[1]), a stream without weights writes nothing.

Rounding policy.  The fp64 reference does NOT round P or dS: every kernel rounds them to bf16 at its own exponent reference (the
forward kernels' lazy maximum) and in its own order, which is no part of the contract.  The fp32 evaluation (dt = fp32, the floor
measurement) DOES round them; in the forward at a reference `shift` in [0, 8) log2 units below the row maximum (P in [1, 256): the lazy
maximum); the backward kernels have no reference of their own (P comes from lse2), so there P and dS are rounded as they are.

Every function returns per output (value, scale).  scale follows gemm_ref: the larger of the output itself (the largest bf16-rounded
intermediate on its path) and the largest addend of its contractions (max_j |p_j v_jd| with the normalised p, ...: an fp32 sum that
cancels is no more accurate than its terms); the fused outputs add the scale of the attention gradient carried through |w| rstd.
bf16 outputs are judged in bf16 ulps of scale (err_ulps), the fp32 ones (lse2, dsum, part) in fp32 ulps of scale (err_ulps32).  lse2:
scale = max(|lse2|, max |s2|, 1) -- log2 l of an l >= 1 is accurate to ulps of 1, the maximum to ulps of the scores.  part is judged
against part_ref of the bf16 X THE KERNEL STORED (an ulp of X is 2^16 fp32 ulps: the projection is checked as a projection).

Arguments: dt (fp64 = the reference, fp32 = the floor), flip (False, True = reversed, "perm" = a fixed permutation; applied to every
contraction axis: keys, queries, dh), rnd (False: every rounding point off).  The fp32 contractions have an explicit order (_mm: steps
of KSTEP elements, each formed in fp64 and rounded to fp32 once, added one after the other; dsum and part: one fp32 addition per
element), so the floors are the same numbers on every host.

Data kinds.
  rand    randn bf16, as the existing tests.
  spike   rand plus planted keys.  Coordinate 0 is reserved: planted key j holds b_j there, every other key 0; the query rows that are
          HIT (i % 64 in SPIKE_ROWS: some rows of every 32-row and 64-row wave) hold SPIKE_A there and a quarter-scale random rest, so
          a hit row's score at a planted key is c2 SPIKE_A b_j = the planted height (log2 units) against a background of about one
          unit.  regimes() reports, in fp64, what a lazy reference over `tile` keys voted by `wave` rows does on the case.
  select  the exact kind.  Keys are the product code k_j = A [onehot(j mod dh/2) | onehot(j div dh/2)], A = SELECT_A = 2; q_i = k_sel(i)
          with sel a permutation of the keys (redirected to unmasked keys where the case masks some at -inf); v, dO are integers in
          {-2, -1, 1, 2} (never zero: a sum of signed zeros has no agreed sign); scale = SELECT_SCALE = 32.  Magnitude argument: the
          selected raw score is 2 A^2 = 8, every other at most A^2 = 4, all exact in fp32; c2 = 32 log2 e = 46.17 (a power of two
          times the fp32 log2 e: the product is exact), so the selected s2 = 369.3 exceeds every other by >= 184.7 > 160 units: an
          unselected P is below 2^-184 < 2^-149 and is ZERO in fp32, the selected one is exp2(0) = 1, l = 1, 1 / l = 1.  In the
          backward P_sel = exp2(8 c2 - lse2) = exp2(0) with lse2 = fp32(8 c2) exactly, dP_sel and dsum are the same integer dO_i . v_sel
          (|.| <= 4 dh = 512, exact in any order), so dS = 0 everywhere.  Every fp32-accumulating kernel must therefore give, in any key
          order, O == V[sel] and dV == scatter-add of dO over sel BIT FOR BIT (integers, |.| <= 2 x the multiplicity of a key),
          dsum exactly, and dQ == dK == +-0; a selected key that arrives after tile 0 forces the rescale with alpha = 0.  The adapter
          weights of select data are integers in [-2, 2] (hi) and in [-2, 2] / 16 (lo): the rank-r sums are exact as well."""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, replace   # noqa: F401  (replace: re-exported)

import torch

from rowkernel_ref import BF, CANARY_BF16, CANARY_F32, bits, canary_bf16, canary_f32   # noqa: F401  (re-exported to the tests)
from rowkernel_ref import _pair_scale, _qk_view, _qk_w, err_ulps, q_bf16, qk_bwd
from skinny_ref import down_ref

F64, F32 = torch.float64, torch.float32
LOG2E = 1.4426950408889634
NEG_INF = float("-inf")
KSTEP = 32                     # elements per fp32 accumulation step of the noise model (one MFMA k-step)
FLOOR_DRAWS = 4                # as gemm_ref
FLOOR_EXTRA_DRAWS = 8
FLOOR_EXTRA_ELEMS = 1 << 16
NORM_EPS = 1e-6                # as the model passes it
SELECT_A, SELECT_SCALE, SELECT_GAP = 2.0, 32.0, 160.0
SPIKE_A, SPIKE_ROWS = 8.0, (3, 17, 40)

# ---------------------------------------------------------------------------------------------- bars
# BARS[output] = 2 x the floor measured by tests/test_attn_ref_cpu.py::test_bars_are_twice_the_reference_noise (the restatement in fp32,
# keys / queries / dh reversed and permuted, P and dS rounded to bf16, the forward's at a reference shifted by [0, 8) units, against fp64
# with neither rounded; every case list below, FLOOR_DRAWS draws, FLOOR_EXTRA_DRAWS more of the small cases), rounded up to a whole ulp,
# at least one.  bf16 ulps of scale for O, dQ, dK, dV; fp32 ulps of scale for lse2, dsum, part.  Never taken from what the kernels give.
BARS = {
    "O": 16,           # floor 8.00   (577 keys' P rounded 7 units below the row maximum, against addends the size of the output)
    "lse2": 7,         # floor 3.17   (fp32 ulps)
    "dsum": 24,        # floor 12.0   (fp32 ulps: 128 fp32 additions one after the other)
    "dQ": 19,          # floor 9.25
    "dK": 19,          # floor 9.38
    "dV": 12,          # floor 6.00
    "dQ.fused": 27,    # floor 13.3   (a flipped bf16 dQ carried through the rotation, the weight and the row statistics)
    "dK.fused": 10,    # floor 5.00
    "part": 228,       # floor 113.9  (fp32 ulps: 256 fp32 additions one after the other; an ulp of X would be 65536 of them)
}


def ulp_f32(s):
    _, e = torch.frexp(s.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(s, dtype=F64), e - 24)


def err_ulps32(got, ref, scale):
    """Worst |got - ref| in fp32 ulps of scale; a non-finite `got` is infinitely wrong."""
    g = got.double()
    if not torch.isfinite(g).all():
        return float("inf")
    return ((g - ref.double()).abs() / ulp_f32(scale)).max().item() if g.numel() else 0.0


def err_of(key, got, ref, scale):
    return (err_ulps32 if key in ("lse2", "dsum", "part") else err_ulps)(got, ref, scale)


# ---------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    """One attention problem.  mask: none | finite | head (-inf on the keys [T_valid, T_m) inside tile 0, the real padding mask) | tile
    (-inf on the whole interior tile [64, 128)) | tail (-inf on the last S // 5 keys) | per_sample (sample 0: head, the others: finite).
    fused: qk_saved and the rank-r slots are set (R = 0: no slots).  rope_b: one RoPE table per sample (rope_bstride = S dh).  c0: first
    column of the sums inside a part row of ld_part = R + 4 (c0 = 4, or narrow) or R + 8.  no_txt / no_img: w_pk[1] / w_pk[0] == NULL.
    slots: the rank-r slots whose part is set.  slice_: Q, K, V are column slices of ONE buffer (else three buffers, three strides).
    narrow: ldo = lddq = lddk = lddv = D + 4 (the 8-byte store path), else D + 8, + 16, + 24.  plant: spike data, (key, height in log2
    units) pairs (a negative key counts from S); expect: the regimes the case was built for, at (tile, wave) = (64, 32)."""
    S: int
    H: int = 1
    B: int = 1
    dh: int = 128
    kind: str = "rand"
    mask: str = "none"
    fused: bool = False
    flags: int = 0
    rope_b: bool = False
    T: int = 0
    R: int = 0
    c0: int = 0
    no_txt: bool = False
    no_img: bool = False
    slots: tuple = (0, 1, 2, 3)
    slice_: bool = False
    narrow: bool = False
    plant: tuple = ()
    expect: tuple = ()

    @property
    def scale(self):
        return SELECT_SCALE if self.kind == "select" else 1.0 / math.sqrt(self.dh)

    @property
    def D(self):
        return self.H * self.dh

    @property
    def S_pad(self):
        return (self.S + 63) // 64 * 64

    @property
    def ld_part(self):
        return self.R + (4 if self.c0 or self.narrow else 8)

    def onepass(self):
        return self.dh == 128 and self.S >= 64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(case, draw):
    key = repr((case.S, case.H, case.B, case.dh, case.kind, case.mask, case.fused, case.T, case.R, case.plant))
    return (zlib.crc32(key.encode()) & 0xFFFFFF) * 16 + draw      # (not hash(): string hashes change from process to process)


def key_mask_of(case, g):
    """[B, S] fp32 additive key mask, or None.  At least one key per sample stays finite (include/qfx.h)."""
    B, S = case.B, case.S
    if case.mask == "none":
        return None
    fin = (torch.randn(S, generator=g) * 2.0).float()
    Tm = case.T if case.T else (48 if S > 64 else 16)
    head = torch.zeros(S)
    head[Tm - max(1, Tm // 3):Tm] = NEG_INF
    one = {"finite": fin, "head": head}
    if case.mask in one:
        assert case.mask != "head" or S > Tm
        m = one[case.mask]
    elif case.mask == "tile":
        assert S > 128
        m = torch.zeros(S)
        m[64:128] = NEG_INF
    elif case.mask == "tail":
        assert S >= 5
        m = torch.zeros(S)
        m[S - S // 5:] = NEG_INF
    else:
        assert case.mask == "per_sample" and S > Tm
        return torch.stack([head if b == 0 else fin + 0.25 * b for b in range(B)]).contiguous()
    return m[None].expand(B, S).contiguous()


def _ints_nz(g, *shape):
    v = torch.randint(1, 3, shape, generator=g).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
    return v.to(BF)


def make_inputs(case, draw=0):
    """Logical (tight) operands: q, k, v, dO [B, S, H, dh] bf16; mask [B, S] fp32 or None; fused: saved [B, S, 2 H dh] bf16, rope [1 or B,
    S, dh / 2, 2] fp32, ws 4 x [dh] bf16; W[slot] = ((hi, lo) image stream, (hi, lo) text stream), each [R, H dh] bf16; select: sel [B, S]."""
    g = _gen(_seed(case, draw))
    B, S, H, dh = case.B, case.S, case.H, case.dh
    inp = {"mask": key_mask_of(case, g)}
    if case.kind == "select":
        half = dh // 2
        assert S <= half * half
        j = torch.arange(S)
        k = torch.zeros(S, dh)
        k[j, j % half] = SELECT_A
        k[j, half + j // half] = SELECT_A
        sel = torch.stack([torch.randperm(S, generator=g) for _ in range(B)])
        if inp["mask"] is not None:
            for b in range(B):
                dead = torch.isinf(inp["mask"][b])
                live = torch.nonzero(~dead).flatten()
                bad = dead[sel[b]]
                sel[b, bad] = live[torch.arange(int(bad.sum())) % live.numel()]
        inp["sel"] = sel
        inp["k"] = k[None, :, None, :].expand(B, S, H, dh).contiguous().to(BF)
        inp["q"] = torch.stack([k[sel[b]] for b in range(B)])[:, :, None, :].expand(B, S, H, dh).contiguous().to(BF)
        inp["v"], inp["dO"] = _ints_nz(g, B, S, H, dh), _ints_nz(g, B, S, H, dh)
    else:
        for n in ("q", "k", "v", "dO"):
            inp[n] = torch.randn(B, S, H, dh, generator=g).to(BF)
        if case.kind == "spike":
            hit = torch.tensor([i % 64 in SPIKE_ROWS for i in range(S)])
            qf, kf = inp["q"].float(), inp["k"].float()
            qf[:, hit] *= 0.25
            qf[:, :, :, 0] = 0.0
            qf[:, hit, :, 0] = SPIKE_A
            kf[:, :, :, 0] = 0.0
            for key, height in case.plant:
                kf[:, key % S, :, 0] = height / (case.scale * LOG2E * SPIKE_A)
            inp["q"], inp["k"] = qf.to(BF), kf.to(BF)
    if case.fused:
        inp["saved"] = torch.randn(B, S, 2 * H * dh, generator=g).to(BF)
        ang = torch.rand(B if case.rope_b else 1, S, dh // 2, generator=g) * 6.28
        inp["rope"] = torch.stack([torch.cos(ang), torch.sin(ang)], -1).float().contiguous()
        inp["ws"] = [(1.0 + 0.1 * torch.randn(dh, generator=g)).to(BF) for _ in range(4)]
    if case.R:
        def w():
            if case.kind == "select":
                return (torch.randint(-2, 3, (case.R, H * dh), generator=g).float().to(BF),
                        (torch.randint(-2, 3, (case.R, H * dh), generator=g).float() / 16).to(BF))
            hi = (torch.randn(case.R, H * dh, generator=g) * 0.1)
            return hi.to(BF), (hi - hi.to(BF).float()).to(BF)
        inp["W"] = {slot: (w(), w()) for slot in range(4)}
    return inp


# ---------------------------------------------------------------------------------------------- arithmetic
_PERM = {}


def _korder(K, flip):
    if flip is False:
        return None
    if flip is True:
        return torch.arange(K - 1, -1, -1)
    if K not in _PERM:
        _PERM[K] = torch.randperm(K, generator=_gen(K))
    return _PERM[K]


def _mm(A, Bm, dt, flip):
    """A [..., M, K] . Bm [..., K, N].  fp64: the host's product.  fp32: the K axis in the order `flip` selects, cut into steps of KSTEP;
    each step's partial product is formed in fp64 and rounded to fp32 once, the steps are added one after the other in fp32."""
    idx = _korder(A.shape[-1], flip)
    if idx is not None:
        A, Bm = A[..., idx], Bm[..., idx, :]
    if dt == F64:
        return A.double() @ Bm.double()
    K = A.shape[-1]
    acc = torch.zeros(*A.shape[:-1], Bm.shape[-1], dtype=F32)
    for k0 in range(0, K, KSTEP):
        acc = acc + (A[..., k0:k0 + KSTEP].double() @ Bm[..., k0:k0 + KSTEP, :].double()).float()
    return acc


def _seq_sum(t, dt, flip):
    """Sum over the last axis; fp32: one addition per element, in the order `flip` selects."""
    idx = _korder(t.shape[-1], flip)
    if idx is not None:
        t = t[..., idx]
    if dt == F64:
        return t.sum(-1)
    acc = torch.zeros(t.shape[:-1], dtype=F32)
    for i in range(t.shape[-1]):
        acc = acc + t[..., i]
    return acc


def _max_term(A, Bm):
    """max_k |A[..., m, k] Bm[..., k, n]| as fp64 [..., M, N], chunked over m (fp32 products of bf16-sized factors: exact enough for a
    scale, which only enters through its binade)."""
    a, b = A.float().abs(), Bm.float().abs()
    M = a.shape[-2]
    out = torch.zeros(*a.shape[:-1], b.shape[-1], dtype=F32)
    step = max(1, (1 << 22) // max(1, b.shape[-2] * b.shape[-1]))
    for m0 in range(0, M, step):
        out[..., m0:m0 + step, :] = (a[..., m0:m0 + step, :, None] * b[..., None, :, :]).amax(-2)
    return out.double()


def _heads(t, dt):
    return t.to(dt).permute(0, 2, 1, 3)        # [B, S, H, dh] -> [B, H, S, dh]


def _tok(t):
    return t.permute(0, 2, 1, 3).contiguous()  # back to [B, S, H, dh]


def scores2(inp, case, dt=F64, flip=False):
    """s2 [B, H, S, S]: the log2-domain scores c2 Q K^T + mask log2 e.  fp32: c2 and mask log2 e are the kernels' fp32 products."""
    Q, K = _heads(inp["q"], dt), _heads(inp["k"], dt)
    raw = _mm(Q, K.transpose(-1, -2), dt, flip)
    s32 = torch.tensor(case.scale, dtype=F32)
    if dt == F32:
        s2 = raw * (s32 * torch.tensor(LOG2E, dtype=F32))
        if inp["mask"] is not None:
            s2 = s2 + (inp["mask"] * torch.tensor(LOG2E, dtype=F32))[:, None, None, :]
        return s2
    s2 = raw * (s32.double() * LOG2E)
    if inp["mask"] is not None:
        s2 = s2 + (inp["mask"].double() * LOG2E)[:, None, None, :]
    return s2


def fwd_shift(case, draw=0):
    """[B, H, S, 1] offsets in [0, 8): how far below the row maximum the fp32 evaluation puts its exponent reference."""
    return torch.rand(case.B, case.H, case.S, 1, generator=_gen(7 + _seed(case, draw))) * 7.999


def attn_fwd_ref(inp, case, dt=F64, flip=False, rnd=True, shift=None):
    """{"O": [B, S, H, dh], "lse2": [B, H, S]} as (value, scale).  shift (fp32 evaluation only): see fwd_shift."""
    q = q_bf16 if rnd else (lambda t: t)
    s2 = scores2(inp, case, dt, flip)
    V = _heads(inp["v"], dt)
    m = s2.amax(-1, keepdim=True)
    mref = m if shift is None else m - shift.to(dt)
    P = torch.exp2(s2 - mref)
    ones = torch.ones(*P.shape[:-2], P.shape[-1], 1, dtype=dt)
    l = _mm(P, ones, dt, flip)
    Pq = q(P) if dt == F32 else P
    O = q(_mm(Pq, V, dt, flip) / l)
    lse2 = (mref + torch.log2(l)).squeeze(-1)
    if dt != F64:
        z = torch.zeros(1, dtype=F64)
        return {"O": (_tok(O), z), "lse2": (lse2, z)}
    sc = torch.maximum(O.abs(), _max_term(P / l, V))
    fin = torch.where(torch.isfinite(s2), s2.abs(), torch.zeros_like(s2)).amax(-1)
    return {"O": (_tok(O), _tok(sc)), "lse2": (lse2, torch.maximum(torch.maximum(lse2.abs(), fin), torch.ones_like(fin)))}


def attn_bwd_ref(inp, case, O, lse2, dt=F64, flip=False, rnd=True):
    """{"dsum": [B, H, S], "dQ", "dK", "dV": [B, S, H, dh]} as (value, scale) for the O [B, S, H, dh] and lse2 [B, H, S] passed in.
    case.fused: dQ, dK are d(pre-norm q), d(pre-norm k)."""
    q = q_bf16 if rnd else (lambda t: t)
    B, S, H, dh = case.B, case.S, case.H, case.dh
    s2 = scores2(inp, case, dt, flip)
    Q, K, V, dO, Oh = (_heads(t, dt) for t in (inp["q"], inp["k"], inp["v"], inp["dO"], O))
    dsum = _seq_sum(dO * Oh, dt, flip)
    P = torch.exp2(s2 - lse2.to(dt)[..., None])
    dP = _mm(dO, V.transpose(-1, -2), dt, flip)
    dS = P * (dP - dsum[..., None])
    Pq, dSq = (q(P), q(dS)) if dt == F32 else (P, dS)
    s32 = torch.tensor(case.scale, dtype=F32).to(dt)
    dV = q(_mm(Pq.transpose(-1, -2), dO, dt, flip))
    dQ = q(_mm(dSq, K, dt, flip) * s32)
    dK = q(_mm(dSq.transpose(-1, -2), Q, dt, flip) * s32)
    z = torch.zeros(1, dtype=F64)
    sc = {}
    if dt == F64:
        sc["dsum"] = torch.maximum(dsum.abs(), (dO * Oh).abs().amax(-1))
        sc["dV"] = _tok(torch.maximum(dV.abs(), _max_term(P.transpose(-1, -2), dO)))
        # dS = P (dP - dsum) cancels: what is left of two fp32 sums is no more accurate than 2^-24 of THEIR terms, and 2^-24 of a term is
        # one bf16 ulp of 2^-16 of it -- the addends of the dQ / dK contractions are taken from a dS no smaller than that
        dSm = P * torch.maximum(dS.abs() / P.clamp_min(2.0 ** -1000), 2.0 ** -16 * torch.maximum(dP.abs(), sc["dsum"][..., None]))
        sc["dQ"] = _tok(torch.maximum(dQ.abs(), _max_term(dSm, K) * s32.abs()))
        sc["dK"] = _tok(torch.maximum(dK.abs(), _max_term(dSm.transpose(-1, -2), Q) * s32.abs()))
    dQ, dK, dV = _tok(dQ), _tok(dK), _tok(dV)
    if case.fused:
        dqkv = torch.cat([dQ.reshape(B, S, H * dh), dK.reshape(B, S, H * dh), torch.zeros(B, S, H * dh, dtype=dt)], -1)
        r = qk_bwd(dqkv, inp["saved"], inp["rope"], inp["ws"], case.T, H, dh, case.flags, NORM_EPS, dt=dt, flip=flip is not False, rnd=rnd)
        val, rsc = r["out"]                                    # [B, S, 2, H, dh]
        dQ, dK = val[:, :, 0].contiguous(), val[:, :, 1].contiguous()
        if dt == F64:
            x = _qk_view(inp["saved"], H, dh).double()
            rstd = torch.rsqrt((x * x).mean(-1, keepdim=True) + NORM_EPS)
            # what the attention gradient's own scale becomes on the way: dn = rot(dy) w carries it, the output is (dn - xh dot) rstd with
            # dot = mean(dn xh) -- one large coordinate reaches EVERY coordinate of its row through the largest addend of dot
            dn_sc = _pair_scale(torch.stack([sc["dQ"], sc["dK"]], 2)) * _qk_w(inp["ws"], S, case.T, F64).abs()
            xh = (x * rstd).abs()
            rsc = torch.maximum(rsc, torch.maximum(dn_sc, xh * (dn_sc * xh).amax(-1, keepdim=True) / dh) * rstd)
            sc["dQ"], sc["dK"] = rsc[:, :, 0].contiguous(), rsc[:, :, 1].contiguous()
    return {k: (v, sc.get(k, z)) for k, v in (("dsum", dsum), ("dQ", dQ), ("dK", dK), ("dV", dV))}


def part_rows(case, slot):
    """[B * S] bool: the joint rows the kernels write in part[slot] (rows of a stream without adapter weights are left alone)."""
    s = torch.arange(case.S)
    txt = s < case.T
    live = torch.where(txt, torch.tensor(not case.no_txt), torch.tensor(not case.no_img))
    return live.repeat(case.B)


def part_ref(X, inp, case, slot, dt=F64, flip=False):
    """(value, scale) [H, B * S, R] of the rank-r sums of slot `slot` over X [B, S, H, dh] (bf16 values): part[h] = X_h (W_hi + W_lo)_h^T,
    text weights for the rows s < T.  Rows part_rows() excludes hold zeros here and are never compared."""
    B, S, H, dh, R = case.B, case.S, case.H, case.dh, case.R
    (ihi, ilo), (thi, tlo) = inp["W"][slot]
    txt = (torch.arange(S) < case.T).repeat(B)
    Xr = X.to(BF).reshape(B * S, H, dh)
    vals, scs = [], []
    for h in range(H):
        xh = Xr[:, h].double()
        cols = slice(h * dh, (h + 1) * dh)
        if dt == F64:
            vi = down_ref(Xr[:, h], ihi[:, cols], ilo[:, cols], torch.arange(B * S))
            vt = down_ref(Xr[:, h], thi[:, cols], tlo[:, cols], torch.arange(B * S))
            wabs = torch.where(txt[:, None, None], torch.maximum(thi[:, cols].abs(), tlo[:, cols].abs()).double()[None],
                               torch.maximum(ihi[:, cols].abs(), ilo[:, cols].abs()).double()[None])           # [rows, R, dh]
            scs.append((xh.abs()[:, None, :] * wabs).amax(-1))
        else:       # hi then lo per element, one fp32 addition each, in the order `flip` selects
            def seq(hi, lo):
                terms = torch.stack([xh[:, None, :] * hi[:, cols].double()[None], xh[:, None, :] * lo[:, cols].double()[None]], -1)
                return _seq_sum(terms.flatten(-2).float(), F32, flip)
            vi, vt = seq(ihi, ilo), seq(thi, tlo)
            scs.append(torch.zeros(B * S, R, dtype=F64))
        vals.append(torch.where(txt[:, None], vt, vi))
    return torch.stack(vals), torch.stack(scs)


def slot_x(slot, fwd, bwd):
    return {0: fwd["O"][0] if fwd else None, 1: bwd["dQ"][0] if bwd else None, 2: bwd["dK"][0] if bwd else None, 3: bwd["dV"][0] if bwd else None}[slot]


def reference(inp, case):
    """Everything the GPU tests compare against, once per case: the forward, then the backward of the reference's own q(O) and fp32 lse2."""
    fwd = attn_fwd_ref(inp, case)
    O_in, lse_in = fwd["O"][0].to(BF), fwd["lse2"][0].float()
    bwd = attn_bwd_ref(inp, case, O_in, lse_in)
    return fwd, bwd, O_in, lse_in


def select_expected(inp, case):
    """The closed form of select data: O = V[sel], dV = scatter-add of dO over sel, dsum = dO . V[sel]."""
    B = case.B
    O = torch.stack([inp["v"][b, inp["sel"][b]] for b in range(B)]).double()
    dV = torch.zeros_like(O)
    for b in range(B):
        dV[b].index_add_(0, inp["sel"][b], inp["dO"][b].double())
    return O, dV, (inp["dO"].double() * O).sum(-1).permute(0, 2, 1)


# ---------------------------------------------------------------------------------------------- regimes of the lazy reference
REGIMES = ("rescale", "deferred", "staircase", "ragged", "mixed", "masked")


def regimes(inp, case, tile=64, wave=32):
    """What the forward kernels' lazy exponent reference does on this case (fp64): per voting unit of `wave` query rows (32 in all three
    forward kernels: a wave of attn_fwd_kernel, a 32-query block of a 64-query wave; rows past S ride on row
    S - 1, as in the kernels) and key tile of `tile` keys, d = tile maximum - reference per row; the wave moves its references to the
    running maxima when some row has d > 8 (or no reference yet).  Reported for tiles of index >= 1:
      rescale    some row moved a FINITE reference (d > 8);        mixed    ... while another row of the same wave had d <= 8;
      deferred   a wave did NOT move although a row had 4 < d <= 8 (P up to 256);
      staircase  some wave moved a finite reference on EVERY tile >= 1 (at least 3 tiles);
      ragged     a rescale inside a last tile that is ragged;      masked   a rescale whose tile maximum sits on a key with a finite
                                                                            non-zero mask."""
    s2 = scores2(inp, case)
    B, H, S = case.B, case.H, case.S
    nt = (S + tile - 1) // tile
    nw = (S + wave - 1) // wave
    rows = torch.arange(nw * wave).clamp(max=S - 1)
    out = set()
    for b in range(B):
        mk = inp["mask"][b] if inp["mask"] is not None else torch.zeros(S)
        for h in range(H):
            s = s2[b, h][rows].view(nw, wave, S)
            ref = torch.full((nw, wave), NEG_INF, dtype=F64)
            every = torch.ones(nw, dtype=torch.bool)
            for t in range(nt):
                seg = s[:, :, t * tile:(t + 1) * tile]
                tm, arg = seg.max(-1)
                d = tm - ref
                need = ~(d <= 8.0)
                real = need & torch.isfinite(ref) & torch.isfinite(tm)
                upd = need.any(1)
                if t >= 1:
                    wreal = real.any(1)
                    every &= wreal
                    if wreal.any():
                        out.add("rescale")
                        if (wreal[:, None] & ~need).any():
                            out.add("mixed")
                        if t == nt - 1 and S % tile:
                            out.add("ragged")
                        mval = mk[(arg + t * tile)[real]]
                        if ((mval != 0) & torch.isfinite(mval)).any():
                            out.add("masked")
                    if (~upd[:, None] & (d > 4.0) & (d <= 8.0)).any():
                        out.add("deferred")
                ref = torch.where(upd[:, None], torch.maximum(ref, tm), ref)
            if nt >= 3 and every.any():
                out.add("staircase")
    return out


# ---------------------------------------------------------------------------------------------- case lists (CPU and GPU tests walk these)
SHAPES = (1, 31, 64, 65, 127, 129, 257, 321, 577)
MASKS = ("none", "finite", "head", "tile", "tail", "per_sample")


def _bh(S, i):
    """(B, H) per shape: everything from {1, 2} x {1, 2, 3}, the large S with few heads."""
    if S >= 321:
        return ((1, 2), (2, 1), (1, 1))[i % 3]
    return ((2, 3), (1, 2), (2, 1), (1, 3), (2, 2), (1, 1))[i % 6]


def _mask_for(S, i):
    m = MASKS[i % 6]
    if m == "tile" and S <= 128:
        m = "finite"
    if m in ("head", "per_sample") and S <= 16:
        m = "none"
    if m == "tail" and S < 5:
        m = "none"
    return m


def _t_for(S, i):
    return (0, 16, 48, S // 16 * 16)[i % 4] if S > 48 else (0, 16, S // 16 * 16, 0)[i % 4] if S > 16 else 0


def _variety(kind, S, i):
    """Spread the argument space over the shapes: dh, masks, strides, the fused block (norm_flags, rope stride, T), the rank-r block
    (R, c0 / ld_part, a missing stream, unset slots)."""
    B, H = _bh(S, i)
    fused = i % 2 == 1
    T = _t_for(S, i // 2) if fused or i % 4 == 0 else 0
    R = (16, 32, 0)[(i // 2) % 3] if fused else (16 if i % 4 == 0 else 0)
    mask = _mask_for(S, i)
    if mask == "per_sample":
        B = 2
    if mask in ("head", "per_sample") and T and S <= T:
        T = 0
    no_img = R > 0 and T > 0 and i % 7 == 3
    # a missing text adapter only shows where there ARE text rows: the cases without one carry 0 < T < S
    no_txt = R > 0 and S > 16 and not no_img and (i % 8 == 4 or (fused and i >= 7))
    if no_txt and not 0 < T < S:
        T = 16 if S <= 64 or i % 8 == 1 else 48
    return Case(S, H=H, B=B, dh=64 if i % 5 == 2 else 128, kind=kind, mask=mask, fused=fused, flags=(i // 2) % 2, rope_b=fused and i % 3 == 0, T=T,
                R=R, c0=4 if i % 3 == 1 else 0, no_txt=no_txt, no_img=no_img,
                slots=(0, 1, 2, 3) if i % 4 != 3 else (0, 1, 3), slice_=i % 3 == 2, narrow=i % 4 in (1, 2))


def _grid(kind, off):
    return [_variety(kind, S, n + off) for n, S in enumerate(SHAPES)] + [_variety(kind, S, n + off + 4) for n, S in enumerate(SHAPES)]


RAND_CASES = _grid("rand", 0)
SELECT_CASES = _grid("select", 1)


def _spike(S, plant, expect, i, **kw):
    c = _variety("spike", S, i)
    return replace(c, plant=plant, expect=expect, mask=kw.pop("mask", "none"), B=kw.pop("B", 1), **kw)


# key 70 sits in tile 1 (sub-tile 2 of 32); heights in log2 units over a background of about one
SPIKE_CASES = [
    _spike(129, ((70, 16.0),), ("rescale", "mixed"), 0),
    _spike(129, ((70, 6.0),), ("deferred",), 1),
    _spike(257, ((70, 16.0), (140, 22.0), (-1, 40.0)), ("rescale", "deferred", "mixed"), 2, H=2),
    _spike(321, tuple((32 * t + 5, 12.0 * t) for t in range(1, 10)) + ((-1, 130.0),), ("staircase", "rescale", "mixed"), 3, H=1),
    _spike(65, ((-1, 16.0),), ("rescale", "ragged", "mixed"), 4),
    _spike(577, ((70, 14.0), (-1, 30.0)), ("rescale", "ragged"), 5, H=1),
    _spike(127, ((70, 26.0),), ("rescale", "masked"), 6, mask="finite", B=2),
    _spike(129, ((-1, 16.0),), ("rescale", "ragged"), 7, dh=64),
    _spike(257, ((200, 18.0),), ("rescale", "mixed"), 9, mask="head", T=48),
]

ALL_FAMILIES = {"rand": RAND_CASES, "spike": SPIKE_CASES, "select": SELECT_CASES}


def measure_floors(families=None, draws=FLOOR_DRAWS, extra=FLOOR_EXTRA_DRAWS):
    """{BARS key: worst error of the fp32 restatement (keys / queries / dh reversed on even draws, permuted on odd ones; P and dS rounded,
    the forward's at the shifted reference) against the fp64 one, in ulps of scale} over every case list -- the reference's own noise;
    nothing here runs the code under test.  Draw 0 is the data of the GPU tests.  The backward is evaluated on the fp64 forward's q(O) and
    fp32 lse2, as the GPU tests pass them; part on the fp64 reference's bf16 X.  dQ, dK of select data are outside the bars (asserted +-0)."""
    floors = {}

    def put(key, got, ref, sc):
        floors[key] = max(floors.get(key, 0.0), err_of(key, got, ref, sc))

    seen = set()
    for fam, cases in ALL_FAMILIES.items():
        if families is not None and fam not in families:
            continue
        for case in cases:
            if case in seen:
                continue
            seen.add(case)
            n = draws + (extra if case.B * case.S * case.D <= FLOOR_EXTRA_ELEMS else 0)
            for draw in range(n):
                flip = True if draw % 2 == 0 else "perm"
                inp = make_inputs(case, draw)
                fwd, bwd, O_in, lse_in = reference(inp, case)
                # (select data: a lazy reference cannot lag behind a score that exceeds it by SELECT_GAP > 8 -- no shift there)
                f32 = attn_fwd_ref(inp, case, F32, flip, shift=None if case.kind == "select" else fwd_shift(case, draw))
                b32 = attn_bwd_ref(inp, case, O_in, lse_in, F32, flip)
                for k in ("O", "lse2"):
                    put(k, f32[k][0], *fwd[k])
                for k in ("dsum", "dQ", "dK", "dV"):
                    if case.kind == "select" and k in ("dQ", "dK"):
                        continue        # asserted to be +-0, not judged by a bar (the fp64 value is a 2^-184 that fp32 flushes)
                    put(k + ".fused" if case.fused and k in ("dQ", "dK") else k, b32[k][0], *bwd[k])
                if case.R:
                    for slot in case.slots:
                        if case.kind == "select" and slot in (1, 2):
                            continue
                        X = slot_x(slot, fwd, bwd if case.fused else None)
                        if X is None:
                            continue
                        live = part_rows(case, slot)
                        v, sc = part_ref(X, inp, case, slot)
                        put("part", part_ref(X, inp, case, slot, F32, flip)[0][:, live], v[:, live], sc[:, live])
    return floors
