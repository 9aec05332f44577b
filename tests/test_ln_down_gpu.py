"""GPU parity tests of the fused LayerNorm+modulate forward + rank-r down projection (ln_down_kernel<NF> of csrc/qfx_skinny.hip) and of
qfx_gate_mul, through the C ABI, against tests/ln_down_ref.py: every instantiation (NF = R / 16 in {1, 2, 3}), all twelve legal widths
(1 .. 12 k-steps per wave: the weight ring partly filled, exactly full, refilled), row tails, sample boundaries inside a block, every
weight layout, both problem slots, the MX-FP8 image beside adapted rows, and the refusals of the host code.

The two halves of the kernel are judged apart: y against the fp64 restatement of the LayerNorm (bf16 ulps of the largest rounded
intermediate, ln_down_ref.BAR_Y), the contraction against U64 = y (W_hi + W_lo)^T computed from the KERNEL'S OWN y bits.  On `exact` data
every fp32 partial sum is exactly representable (tests/test_ln_down_ref_cpu.py proves the premise, verify() asserts it of the kernel's y), so
ext, Ut_hi and Ut_lo must equal the images of fp32(U64) bit for bit; on `rand` data hi + lo lies within ln_down_ref.BAR_U of U64 and the
three column sets of ext and Ut agree bit for bit with each other.

Every output buffer is larger than what may be written and starts as a canary (0x7FC1 for bf16, 0xFF bytes for yq / ys); whole buffers are
compared, so a store past `rows`, into the ld padding or into the Ut columns >= rows (which the header leaves to the caller) fails the
test.  Row-major weights stand in NaN-padded buffers, and a launch that reads the fragment image gets all-NaN row-major weights: a load
from the wrong place poisons the result.

What the host code does NOT check, and a caller has to guarantee: ld_ext >= (R / group_R - 1) * group_stride + 3 * group_R and
group_stride >= 3 * group_R (qfx_lora_head_reduce refuses these, qfx_ln_down_fwd and qfx_lora_down do not), and 16-byte alignment of x,
the modulation vectors, y and the row-major weights.

Which case runs which arm: ln_down_ref.arms(case) for the n = 1 launches of CASES; the plain-row early return and the second problem slot
in test_ln_down_two_problems (TWO_PROBLEM_CASES), the yq arm in test_ln_down_mxfp8_image_with_adapted_rows (MX_CASES).
Worst observed figures: ln_down_parity.json, beside skinny_parity.json."""
import ctypes as C
import functools

import pytest
import torch

import ln_down_ref as LD
import rowkernel_ref as R
import skinny_ref as S
from parity_util import _observe

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda:0"
_STATS = {}


def _L():
    from qflux_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def record_worst(key, unit, case, err, bar):
    """ln_down_parity.json: per output the worst ulps / relative error, its bar and the case."""
    old = _STATS.get(key)
    if old is None or err >= old[unit]:
        _STATS[key] = {unit: err, "bar": bar, "case": str(case)}
        _observe(None, None, dump=("ln_down_parity.json", _STATS))


def same_bits(a, b):
    if a.dtype == torch.uint8:
        return a.shape == b.shape and b.dtype == torch.uint8 and torch.equal(a, b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(S.bits(a), S.bits(b))


def is_canary(t):
    t = t.cpu()
    return bool((t == 0xFF).all()) if t.dtype == torch.uint8 else bool((S.bits(t) == S.CANARY_BF16).all())


def nan_bf16(*shape):
    return torch.full(shape, float("nan"), dtype=BF)


@functools.lru_cache(maxsize=4)
def _inputs(case, kind, salt):
    """CPU inputs of one case, generated once and never modified."""
    return LD.make(case, kind, salt)


class Prob:
    """One problem of a qfx_ln_down_fwd launch: inputs on the device, canaried output buffers, the reference."""

    def __init__(self, case, kind, *, adapted=True, salt=0, mx=False, weights=None):
        self.case, self.kind, self.adapted, self.salt, self.mx = case, kind, adapted, salt, mx
        self.weights = weights or case.weights
        self.inp = inp = _inputs(case, kind, salt)
        rows, D, Rr = case.rows, case.D, case.R
        self.rpb = LD.rpb_of(case)
        self.x = inp["x"].to(DEV)
        self.mod = inp["mod"].to(DEV)
        (self.shift, self.bstride), (self.scale, _) = R.mod_views(self.mod, D, case.stride, 0), R.mod_views(self.mod, D, case.stride, 1)
        self.y = S.canary_bf16(rows + 3, D, device=DEV)
        self.gR, self.gs, self.ld_ext = LD.group_of(case)
        self.ld_ut = rows + 9
        self.E = self.Th = self.Tl = self.Wh = self.Wl = self.Wfr = None
        if adapted:
            if self.weights == "frag":       # the fragment image is what the launch reads: the row-major weights are poison
                self.Wfr = _L().down_fragment_image(inp["W_hi"].to(DEV), inp["W_lo"].to(DEV))
                self.Wh, self.Wl, self.ldw = nan_bf16(Rr, D).to(DEV), nan_bf16(Rr, D).to(DEV), D
            else:
                self.ldw = D + (8 if self.weights == "wide" else 0)
                wh, wl = nan_bf16(Rr, self.ldw), nan_bf16(Rr, self.ldw)
                wh[:, :D], wl[:, :D] = inp["W_hi"], inp["W_lo"]
                self.Wh, self.Wl = wh.to(DEV), wl.to(DEV)
            if "E" in case.outs:
                self.E = S.canary_bf16(rows + 2, self.ld_ext, device=DEV)
            if "T" in case.outs:
                self.Th, self.Tl = S.canary_bf16(Rr + 1, self.ld_ut, device=DEV), S.canary_bf16(Rr + 1, self.ld_ut, device=DEV)
        self.yq = self.ys = None
        if mx:
            self.ldyq, self.ys_rows = D + LD.MX_LDYQ_EXTRA, rows + LD.MX_YS_ROWS_EXTRA
            self.yq = torch.full((rows + 2, self.ldyq), 0xFF, dtype=torch.uint8, device=DEV)
            self.ys = torch.full(((D // 128) * self.ys_rows * 4 + 16,), 0xFF, dtype=torch.uint8, device=DEV)

    def twin(self, **kw):
        """The same problem with buffers of its own (other addresses)."""
        return Prob(self.case, self.kind, **dict(dict(adapted=self.adapted, salt=self.salt, mx=self.mx, weights=self.weights), **kw))

    def args(self):
        a = _L().LnDownArgs()
        c = self.case
        a.ln.x, a.ln.shift, a.ln.scale, a.ln.mod_bstride, a.ln.y = self.x.data_ptr(), self.shift.data_ptr(), self.scale.data_ptr(), self.bstride, self.y.data_ptr()
        a.ln.rows, a.ln.D, a.ln.rows_per_batch, a.ln.eps = c.rows, c.D, self.rpb, LD.EPS
        if self.mx:
            a.ln.yq, a.ln.ys, a.ln.ldyq, a.ln.ys_rows = self.yq.data_ptr(), self.ys.data_ptr(), self.ldyq, self.ys_rows
        if self.adapted:
            a.W_hi, a.W_lo, a.ldw, a.R = self.Wh.data_ptr(), self.Wl.data_ptr(), self.ldw, c.R
            a.W_fr = self.Wfr.data_ptr() if self.Wfr is not None else None
            if self.E is not None:
                a.ext, a.ld_ext = self.E.data_ptr(), self.ld_ext
            if self.Th is not None:
                a.Ut_hi, a.Ut_lo, a.ld_ut = self.Th.data_ptr(), self.Tl.data_ptr(), self.ld_ut
            a.group_R, a.group_stride = self.gR, self.gs
        return a

    def outputs(self):
        return [(n, t.cpu()) for n, t in (("y", self.y), ("ext", self.E), ("Ut_hi", self.Th), ("Ut_lo", self.Tl), ("yq", self.yq), ("ys", self.ys))
                if t is not None]

    def same_outputs(self, other, names=None):
        mine, theirs = dict(self.outputs()), dict(other.outputs())
        names = names or mine.keys()
        return [n for n in names if not same_bits(mine[n], theirs[n])]

    def all_canary(self):
        return all(is_canary(t) for _, t in self.outputs())

    def verify(self, name):
        """y against the LayerNorm restatement; ext / Ut against the contraction of the kernel's own y; every buffer whole."""
        c, what = self.case, f"{self.kind} {self.case} adapted={self.adapted}"
        rows, Rr = c.rows, c.R
        yb = self.y.cpu()
        assert is_canary(yb[rows:]), f"{what}: y written past row {rows}"
        y = yb[:rows].contiguous()
        shift, scale = LD.mod_of(self.inp, c)
        ref = LD.ln_down(self.inp["x"], shift, scale, self.rpb)["y"]
        e = R.err_ulps(y, *ref)
        record_worst(f"{name}.y", "ulps", what, e, LD.BAR_Y)
        assert e <= LD.BAR_Y, f"{what}: y {e:.3f} ulps of scale > {LD.BAR_Y}"
        if not self.adapted:
            return y
        if self.kind == "exact":      # the premise of bit-equality, on what the kernel itself feeds its MFMAs
            ya = y.double().abs()
            assert (ya >= LD.EXACT_Y_MIN).all() and (ya < LD.EXACT_Y_MAX).all() and ((ya / LD.EXACT_Y_GRAN) == (ya / LD.EXACT_Y_GRAN).round()).all() \
                and c.D <= LD.EXACT_MAX_D, f"{what}: y left the range the exactness premise is proven for"
        r = LD.ln_down(self.inp["x"], shift, scale, self.rpb, self.inp["W_hi"], self.inp["W_lo"], y=y, group_R=self.gR, group_stride=self.gs,
                       ld_ext=self.ld_ext, ld_ut=self.ld_ut)
        want = {"ext": torch.cat([r["ext"], S.canary_bf16(2, self.ld_ext)]), "Ut_hi": torch.cat([r["Ut_hi"], S.canary_bf16(1, self.ld_ut)]),
                "Ut_lo": torch.cat([r["Ut_lo"], S.canary_bf16(1, self.ld_ut)])}
        got = {n: t for n, t in self.outputs() if n in want}
        assert set(got) == ({"ext"} if c.outs == "E" else {"Ut_hi", "Ut_lo"} if c.outs == "T" else set(want))
        for n, t in got.items():      # written exactly where the image is written: rows >= rows, the ld padding, Ut columns >= rows keep the canary
            assert torch.equal(S.bits(t) == S.CANARY_BF16, S.bits(want[n]) == S.CANARY_BF16), f"{what}: {n} written outside the problem, or not written inside"
        if self.kind == "exact":
            for n, t in got.items():
                assert same_bits(t, want[n]), f"{what}: {n} differs from the image of the exact sum"
            record_worst(f"{name}.u_exact", "rel", "bit-equal", 0.0, 0.0)
            return y
        splits = []
        if "ext" in got:
            ch, cl, ch2 = LD.ext_columns(Rr, self.gR, self.gs)
            ext = got["ext"][:rows]
            assert same_bits(ext[:, ch], ext[:, ch2]), f"{what}: the two hi column sets of ext differ"
            splits.append((ext[:, ch], ext[:, cl]))
        if "Ut_hi" in got:
            splits.append((got["Ut_hi"][:Rr, :rows].t(), got["Ut_lo"][:Rr, :rows].t()))
        if len(splits) == 2:
            assert same_bits(splits[0][0].contiguous(), splits[1][0].contiguous()) and same_bits(splits[0][1].contiguous(), splits[1][1].contiguous()), \
                f"{what}: ext and Ut hold different splits"
        hi, lo = splits[0]
        e = LD.rel_u(hi.double() + lo.double(), r["U"])
        record_worst(f"{name}.u", "rel", what, e, LD.BAR_U)
        assert e <= LD.BAR_U, f"{what}: hi + lo misses U64 by {e:.3e} of its maximum > {LD.BAR_U:.3e}"
        return y


def launch(probs, want_rc=0):
    L = _L()
    arr = (L.LnDownArgs * len(probs))(*[p.args() for p in probs])
    rc = L.lib.qfx_ln_down_fwd(arr, len(probs), _stream())
    torch.cuda.synchronize()
    assert rc == want_rc, rc


def case_id(c):
    return f"D{c.D}-R{c.R}-rows{c.rows}-rpb{c.rpb}-{c.stride}-{c.weights}-{'grouped' if c.grouped else 'onegroup'}-{c.outs}"


# ================================================================================================ n = 1: every instantiation
@pytest.mark.parametrize("case", LD.CASES, ids=case_id)
def test_ln_down_every_instantiation(case):
    for kind in LD.KINDS:
        p = Prob(case, kind)
        launch([p])
        p.verify(f"NF{case.R // 16}")
        if case.weights == "frag":       # the fragment image changes the loads, not a bit of the result
            q = p.twin(weights="tight")
            launch([q])
            assert not p.same_outputs(q), f"{kind} {case}: W_fr and row-major launches differ in {p.same_outputs(q)}"


# ================================================================================================ n = 2: both problem slots
@pytest.mark.parametrize("Dp,Rr,pair", LD.TWO_PROBLEM_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_ln_down_two_problems(Dp, Rr, pair):
    """Every output of a two-problem launch is bit-identical to the problem's own n = 1 launch: the blocks of the second problem start at
    start[1] = ceil(rows0 / 16) and read the second problem's pointers (x, modulation and W differ between the problems, so do D, the
    modulation stride and the weight layout); a plain problem (W_hi = NULL) leaves through the early return in either slot."""
    for kind in LD.KINDS:
        probs = [Prob(LD.Case(Dp[i], Rr, rows, 3, ("six", "tight")[i], ("frag", "wide")[i], Rr > 16, "ET"), kind, adapted=adapted, salt=1 + i)
                 for i, (rows, adapted) in enumerate(pair)]
        launch(probs)
        for i, p in enumerate(probs):
            one = p.twin()
            launch([one])
            one.verify(f"two_problems_NF{Rr // 16}")
            diff = p.same_outputs(one)
            assert not diff, f"{kind} problem {i} of {pair} (D={Dp[i]} R={Rr}): {diff} differ from the n = 1 launch"      # whole buffers, canaries included


# ================================================================================================ the MX-FP8 image of y
@pytest.mark.parametrize("D,rows", LD.MX_CASES)
def test_ln_down_mxfp8_image_with_adapted_rows(D, rows):
    """ln.yq beside the rank-r outputs: the bytes and the tile-major E8M0 scales equal the CPU quantisation of the kernel's own y, with
    ldyq > D and ys_rows > rows; the padding and the rows past `rows` keep their canary; y, ext and Ut do not change by a bit."""
    from oracle import mxfp8 as QX
    from test_mxfp8_gpu import mx_quant_ref
    Rr = {256: 16, 1280: 32, 3072: 48}[D]
    for adapted in (True, False):
        case = LD.Case(D, Rr, rows, LD.MX_RPB, "six", "frag" if rows == 33 else "wide", Rr > 16, "ET")
        p = Prob(case, "rand", adapted=adapted, mx=True)
        launch([p])
        y = p.verify(f"mxfp8_NF{Rr // 16}")
        q, s = mx_quant_ref(y)                                   # bytes [rows, D], scale bytes [rows, D / 32]
        deq = q.view(torch.float8_e4m3fn).float().view(rows, D // 32, 32) * torch.pow(2.0, s.float() - 127)[:, :, None]
        assert torch.equal(deq.view(rows, D), QX.mx_qdq(y)), "the byte form of the CPU quantisation disagrees with oracle/mxfp8.py"
        want_q = torch.full((rows + 2, p.ldyq), 0xFF, dtype=torch.uint8)
        want_q[:rows, :D] = q
        want_s = torch.full((D // 128, p.ys_rows, 4), 0xFF, dtype=torch.uint8)
        want_s[:, :rows, :] = s.view(rows, D // 128, 4).permute(1, 0, 2)     # scale of k-block kb of row m at ((kb / 4) * ys_rows + m) * 4 + kb % 4
        want_s = torch.cat([want_s.reshape(-1), torch.full((16,), 0xFF, dtype=torch.uint8)])
        what = f"D={D} rows={rows} adapted={adapted}"
        assert same_bits(p.yq.cpu(), want_q), f"{what}: yq (or its ldyq padding, or the rows past `rows`) differs"
        assert same_bits(p.ys.cpu(), want_s), f"{what}: ys (or its rows past `rows`) differs"
        plain = p.twin(mx=False)
        launch([plain])
        diff = p.same_outputs(plain, [n for n, _ in plain.outputs()])
        assert not diff, f"{what}: {diff} change when yq is set"


# ================================================================================================ determinism
def test_ln_down_is_bit_reproducible():
    a = Prob(LD.REPRO_CASE, "rand")
    b = a.twin()
    assert LD.REPRO_CASE[:3] == (3072, 48, 33) and a.y.data_ptr() != b.y.data_ptr() and a.x.data_ptr() != b.x.data_ptr()
    launch([a])
    launch([b])
    a.verify("repro")
    assert not a.same_outputs(b), a.same_outputs(b)


# ================================================================================================ refusals
def test_ln_down_refusals_leave_every_output_alone():
    """(mutation of a valid launch, the code the host function returns for it); nothing is launched, every buffer keeps its canary."""
    L = _L()
    INV, UNS = L.QFX_EINVAL, L.QFX_EUNSUPPORTED
    base = Prob(LD.Case(512, 48, 17, 3, "six", "frag", False, "ET"), "rand", mx=True)
    second = Prob(LD.Case(512, 48, 5, 3, "six", "tight", False, "ET"), "rand", salt=1)
    D, rows = 512, 17

    def ln(**kw):
        return lambda a: [setattr(a.ln, k, v) for k, v in kw.items()]

    def top(**kw):
        return lambda a: [setattr(a, k, v) for k, v in kw.items()]

    def both(r0, r1):
        def f(a, b):
            a.R, a.group_R, b.R, b.group_R = r0, r0, r1, r1
        return f
    table = [("n = 0", 0, None, INV), ("n = 3", 3, None, INV)]
    table += [(f"{k} = NULL", 1, ln(**{k: None}), INV) for k in ("x", "shift", "scale", "y")]
    table += [("rows = 0", 1, ln(rows=0), INV), ("rows_per_batch = 0", 1, ln(rows_per_batch=0), INV)]
    table += [(f"D = {d}", 1, ln(D=d), UNS) for d in (128, 264, 3328)]
    table += [("mod_bstride = 4", 1, ln(mod_bstride=4), UNS), ("W_lo = NULL", 1, top(W_lo=None), UNS), ("ldw = D + 4", 1, top(ldw=D + 4), UNS)]
    table += [(f"R = {r}", 1, top(R=r, group_R=r), UNS) for r in (8, 24, 64)]
    table += [("R = 16 and R = 32 in one call", 2, both(16, 32), INV)]
    table += [("group_R = 0", 1, top(group_R=0), INV), ("group_R = 32 with R = 48", 1, top(group_R=32), INV)]
    table += [("Ut_lo = NULL", 1, top(Ut_lo=None), INV), ("ld_ut = rows - 1", 1, top(ld_ut=rows - 1), INV)]
    table += [("W_fr misaligned by 8 bytes", 1, top(W_fr=base.Wfr.data_ptr() + 8), INV)]
    table += [("yq without ys", 1, ln(ys=None), INV), ("ldyq = D - 8", 1, ln(ldyq=D - 8), INV), ("ldyq = D + 4", 1, ln(ldyq=D + 4), INV),
              ("ys_rows = rows - 1", 1, ln(ys_rows=rows - 1), INV)]
    assert base.args().R == 48 and base.args().ext and base.args().ln.yq
    for what, n, mutate, code in table:
        a, b = base.args(), second.args()
        if mutate is not None:
            mutate(a, b) if n == 2 else mutate(a)
        arr = (L.LnDownArgs * 3)(a, b, b)
        rc = L.lib.qfx_ln_down_fwd(arr, n, _stream())
        torch.cuda.synchronize()
        assert rc == code, f"{what}: returned {rc}, the host code says {code}"
        assert base.all_canary() and second.all_canary(), f"{what}: a refused call wrote to an output"
    assert L.lib.qfx_ln_down_fwd(None, 1, _stream()) == INV
    launch([base, second])                   # and the unmutated arguments are a valid launch
    base.verify("refusal_base")
    second.verify("refusal_base")


# ================================================================================================ gate_mul
@pytest.mark.parametrize("rows,D,rpb,stride", LD.GATE_CASES)
def test_gate_mul(rows, D, rpb, stride):
    """dyg = bf16(gate[row // rpb] * dx): bit-equal to the fp64 product rounded once (the product of two bf16 values is exact in fp32);
    the last case is one trip and a tail past the capped grid (4096 blocks x 256 threads x 8 elements)."""
    L = _L()
    B = (rows + rpb - 1) // rpb
    d = R.rand_case(300 + rows + D, dx=(rows, D), mod=(B, 6 * D))
    want = R.flat_image(LD.gate_mul(d["dx"], R.mod_views(d["mod"], D, stride, 2)[0], rpb), rows * D + 64)
    dx, mod = d["dx"].to(DEV), d["mod"].to(DEV)
    gate, bstride = R.mod_views(mod, D, stride, 2)
    assert bstride == {"shared": 0, "tight": D, "six": 6 * D}[stride]
    out = S.canary_bf16(rows * D + 64, device=DEV)
    rc = L.lib.qfx_gate_mul(dx.data_ptr(), gate.data_ptr(), bstride, out.data_ptr(), rows, D, rpb, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    got = out.cpu()
    assert is_canary(got[rows * D:]), "written past the end"
    assert same_bits(got, want), f"{int((S.bits(got) != S.bits(want)).sum())} of {rows * D} elements differ"
    record_worst("gate_mul", "rel", "bit-equal", 0.0, 0.0)
    # refusals: nothing is launched
    out2 = S.canary_bf16(rows * D + 64, device=DEV)
    good = dict(dx=dx.data_ptr(), gate=gate.data_ptr(), bstride=bstride, dyg=out2.data_ptr(), rows=rows, D=D, rpb=rpb)
    for bad in (dict(dx=None), dict(gate=None), dict(dyg=None), dict(D=12), dict(bstride=4), dict(rows=0), dict(rpb=0)):
        a = dict(good, **bad)
        rc = L.lib.qfx_gate_mul(a["dx"], a["gate"], a["bstride"], a["dyg"], a["rows"], a["D"], a["rpb"], _stream())
        torch.cuda.synchronize()
        assert rc == L.QFX_EINVAL, (bad, rc)
        assert is_canary(out2), bad
