"""GPU parity tests of the rank-r LoRA kernels (csrc/qfx_skinny.hip) at every dispatch path, through the C ABI: each template
instantiation of the down projection (NF = R / 16 in {1, 2, 3, 4, 6}, one and two 16-row groups per block), of the weight gradient and
of its chunk reduction, the batched entries with n > 1, qfx_lora_head_reduce and qfx_lora_pack -- against tests/skinny_ref.py.

Two kinds of data.  exact_case: every partial sum is exactly representable in fp32, so the kernel's fp32 result must equal the fp64
reference BIT FOR BIT whatever its summation order (tests/test_skinny_ref_cpu.py proves the premise).  rand_case: the bars of
tests/test_kernels_gpu.py (2e-5 of the maximum for the down projection, 1e-4 for the gradient, 1e-6 between the atomic and the
deterministic gradient), and the bf16 images bit-equal to the images built from the fp32 U of the same launch.

Every output buffer is larger than what the kernel may write and starts as a canary (NaN for fp32, 0x7FC1 for bf16); whole buffers are
compared, so a store outside the problem's rows, columns or scratch fails the test.  The gradient buffers, which the kernel adds to,
carry a finite canary (a NaN would swallow the addition) and are padded up to the next multiple of the 128-column strip, so even a
kernel that lost its column mask stays inside them.
Worst observed errors: skinny_parity.json, beside kernel_parity.json."""
import ctypes as C
import functools

import pytest
import torch

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


def record(name, **kw):
    """skinny_parity.json, where tests/test_kernels_gpu.py leaves kernel_parity.json."""
    _STATS[name] = kw
    _observe(None, None, dump=("skinny_parity.json", _STATS))


def record_worst(name, case, err, tol):
    old = _STATS.get(name)
    if old is None or err >= old["rel"]:
        record(name, rel=err, tol=tol, case=case)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(S.bits(a), S.bits(b))


def untouched(buf, *written, canary=None):
    """True when `buf` still holds its canary everywhere outside the index tuples `written`."""
    b = S.bits(buf.cpu()).clone()
    can = canary if canary is not None else (S.CANARY_BF16 if buf.dtype == BF else S.CANARY_F32)
    for idx in written:
        b[idx] = can
    return bool((b == can).all())


def rel_max(got, ref):
    return ((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-300)).item()


def roundup(a, b):
    return (a + b - 1) // b * b


@functools.lru_cache(maxsize=3)
def _case_data(kind, seed, x_shape, w_shape, w_scale):
    """CPU inputs of one case, generated once and never modified."""
    if kind == "exact":
        return S.exact_case(seed, x_shape, w_shape)
    return S.rand_case(seed, x_shape, w_shape, w_scale)


# ================================================================================================ down projection
class Down:
    """One qfx_lora_down problem: inputs on the device, canaried output buffers, the fp64 reference."""

    def __init__(self, kind, seed, M, K, R, *, remap=None, ldx_extra=0, col0=0, group_R=None, group_stride=0, outs="UET", share=None):
        assert K <= S.EXACT_MAX_K
        self.kind, self.M, self.K, self.R, self.outs = kind, M, K, R, outs
        self.rpb, self.batch_rows, self.off = remap if remap else (M, 0, 0)
        self.group_R = R if group_R is None else group_R
        self.group_stride = group_stride
        self.rows = S.remap_rows(M, self.rpb, self.batch_rows, self.off)
        if share is None:
            xrows, ldx = int(self.rows.max()) + 3, col0 + K + ldx_extra
            X, hi, lo = _case_data(kind, seed, (xrows, ldx), (R, K), 0.1)
            self.ref = S.down_ref(X[:, col0:], hi, lo, self.rows)
            self.Xd, self.hid, self.lod, self.col0 = X.to(DEV), hi.to(DEV), lo.to(DEV), col0
        else:
            self.ref, self.Xd, self.hid, self.lod, self.col0 = share.ref, share.Xd, share.hid, share.lod, share.col0
        ngrp = R // self.group_R
        self.ld_ext = (ngrp - 1) * group_stride + 3 * self.group_R + 11
        self.Ub = S.canary_f32(M + 3, R + 5, device=DEV) if "U" in outs else None
        self.Eb = S.canary_bf16(M + 2, self.ld_ext, device=DEV) if "E" in outs else None
        self.Th = S.canary_bf16(R + 1, M + 9, device=DEV) if "T" in outs else None
        self.Tl = S.canary_bf16(R + 1, M + 9, device=DEV) if "T" in outs else None

    def fresh(self, outs="UET"):
        """The same problem with new output buffers (its own n = 1 launch)."""
        return Down(self.kind, 0, self.M, self.K, self.R, remap=(self.rpb, self.batch_rows, self.off), group_R=self.group_R,
                    group_stride=self.group_stride, outs=outs, share=self)

    def args(self):
        a = _L().LoraDownArgs()
        a.X, a.ldx, a.M, a.K = self.Xd.data_ptr() + 2 * self.col0, self.Xd.stride(0), self.M, self.K
        a.W_hi, a.W_lo, a.ldw, a.R = self.hid.data_ptr(), self.lod.data_ptr(), self.hid.stride(0), self.R
        if self.Ub is not None:
            a.U, a.ldu = self.Ub.data_ptr(), self.Ub.stride(0)
        if self.Eb is not None:
            a.ext, a.ld_ext = self.Eb.data_ptr(), self.ld_ext
        if self.Th is not None:
            a.Ut_hi, a.Ut_lo, a.ld_ut = self.Th.data_ptr(), self.Tl.data_ptr(), self.Th.stride(0)
        a.group_R, a.group_stride = self.group_R, self.group_stride
        a.rows_per_batch, a.x_batch_rows, a.x_row_off = self.rpb, self.batch_rows, self.off
        return a

    def verify(self, name, case):
        """All outputs of a launch with outs = "UET" against the reference; the images against the U of the same launch."""
        M, R = self.M, self.R
        Ub = self.Ub.cpu()
        assert untouched(Ub, (slice(0, M), slice(0, R))), f"{case}: U written outside [M, R]"
        U = Ub[:M, :R].contiguous()
        assert torch.isfinite(U).all(), f"{case}: U has unwritten or non-finite elements"
        if self.kind == "exact":
            assert same_bits(U, self.ref.float()), f"{case}: U differs from the exact sum, max |d| = {(U.double() - self.ref).abs().max().item()}"
        else:
            e = rel_max(U, self.ref)
            record_worst(name, case, e, 2e-5)
            assert e <= 2e-5, f"{case}: rel err {e:.3e} > 2e-5"
        ext = torch.cat([S.ext_image(U, self.group_R, self.group_stride, self.ld_ext), S.canary_bf16(2, self.ld_ext)])
        assert same_bits(self.Eb.cpu(), ext), f"{case}: ext image (or its surroundings) differs"
        th, tl = S.ut_image(U, M + 9)
        can = S.canary_bf16(1, M + 9)
        assert same_bits(self.Th.cpu(), torch.cat([th, can])) and same_bits(self.Tl.cpu(), torch.cat([tl, can])), f"{case}: Ut image differs"

    def same_outputs(self, other):
        for a, b in ((self.Ub, other.Ub), (self.Eb, other.Eb), (self.Th, other.Th), (self.Tl, other.Tl)):
            if a is not None and not same_bits(a.cpu(), b.cpu()):
                return False
        return True


def launch_down(probs, want_rb):
    """One launch of all `probs`; the row-group form the host code picks (qfx_lora_down_batch) must be the one the case is about."""
    L = _L()
    groups = sum((p.M + 15) // 16 for p in probs)
    assert (2 if groups >= 300 and probs[0].R <= 48 else 1) == want_rb, (groups, probs[0].R, want_rb)
    if len(probs) == 1:
        rc = L.lib.qfx_lora_down(C.byref(probs[0].args()), _stream())
    else:
        arr = (L.LoraDownArgs * len(probs))(*[p.args() for p in probs])
        rc = L.lib.qfx_lora_down_batch(arr, len(probs), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()


NF_R = (16, 32, 48, 64, 96)
K_EDGES = (32, 96, 224, 1568, 3072, 3104)     # < 256: idle waves; 1568 / 3104: one k-step past the chunk of the RB = 2 / RB = 1 form
RB1_M = (1, 16, 17, 77)
RB2_M = (4801, 4816, 4817, 4831)              # >= 300 row groups; M % 32 = 1, 16 (second group dead), 17, 31 (partly dead)
DOWN_CASES = [(R, K, RB1_M[(i + j) % 4], 1) for i, R in enumerate(NF_R) for j, K in enumerate(K_EDGES)]
DOWN_CASES += [(R, K_EDGES[(4 * i + j) % 6], M, 2) for i, R in enumerate(NF_R[:3]) for j, M in enumerate(RB2_M)]
DOWN_CASES += [(16, 12288, 77, 1), (96, 12288, 77, 1)]     # the MLP down projection's K: four trips of the outer loop


@pytest.mark.parametrize("R,K,M,rb", DOWN_CASES)
def test_lora_down_every_instantiation(R, K, M, rb):
    for kind in ("exact", "rand"):
        p = Down(kind, 100 + R + K + M, M, K, R)
        launch_down([p], rb)
        p.verify(f"down_NF{R // 16}_RB{rb}", f"{kind} R={R} K={K} M={M}")


# (R, group_R, group_stride, remap (rows_per_batch, x_batch_rows, x_row_off), M, K, ldx_extra, col0, rb)
DOWN_REMAP_CASES = [
    (96, 32, 104, (25, 40, 7), 70, 224, 72, 8, 1),          # three samples, the last one short
    (48, 16, 56, (30, 47, 5), 60, 1568, 40, 16, 1),
    (48, 16, 56, (2409, 2420, 3), 4818, 96, 40, 8, 2),      # M % 32 = 18
    (32, 16, 72, (1607, 1610, 1), 4821, 224, 8, 0, 2),      # three samples
]


@pytest.mark.parametrize("R,gR,gs,remap,M,K,ldx_extra,col0,rb", DOWN_REMAP_CASES)
def test_lora_down_row_remap_and_strides(R, gR, gs, remap, M, K, ldx_extra, col0, rb):
    for kind in ("exact", "rand"):
        p = Down(kind, 7 + R + M, M, K, R, remap=remap, ldx_extra=ldx_extra, col0=col0, group_R=gR, group_stride=gs)
        launch_down([p], rb)
        p.verify(f"down_remap_NF{R // 16}_RB{rb}", f"{kind} R={R} group_R={gR} remap={remap} M={M} K={K}")


@pytest.mark.parametrize("R,rb", [(16, 1), (16, 2), (48, 1), (48, 2), (96, 1)])
def test_lora_down_batch_matches_single_launches(R, rb):
    """Eight problems of one rank in one grid: every output equals the problem's own n = 1 launch bit for bit -- also when the batch
    runs the two-row-group form and the single launch does not (each wave walks its k-steps in the same order under both chunk depths)."""
    gR = R // 3 if R % 48 == 0 else R
    gs = 3 * gR + 8 if gR != R else 0
    last_M = 4700 if rb == 2 else 40           # one large problem lifts the launch over 300 row groups
    specs = [   # M, K, outs, remap, ldx_extra, grouped
        (1, 32, "UET", None, 0, False),
        (17, 96, "U", (9, 14, 2), 0, False),
        (77, 224, "E", None, 0, True),
        (33, 1568, "UET", None, 8, True),
        (16, 3104, "ET", None, 0, False),
        (100, 3072, "UT", (34, 50, 11), 24, True),
        (50, 64, "E", (25, 25, 0), 0, False),
        (last_M, 256, "UET", None, 0, True),
    ]
    for kind in ("exact", "rand"):
        probs = [Down(kind, 300 + R + i, M, K, R, remap=remap, ldx_extra=ex, col0=8 if ex else 0, group_R=gR if grouped else R,
                      group_stride=gs if grouped else 0, outs=outs) for i, (M, K, outs, remap, ex, grouped) in enumerate(specs)]
        launch_down(probs, rb)
        for i, p in enumerate(probs):
            case = f"{kind} R={R} RB={rb} problem {i} (M={p.M} K={p.K} outs={p.outs})"
            one = p.fresh()
            launch_down([one], 1)
            one.verify(f"down_batch_NF{R // 16}_RB{rb}", case)
            assert p.same_outputs(one), f"{case}: the batched launch differs from the n = 1 launch"      # whole buffers, canaries included


# ================================================================================================ weight gradient
# G is accumulated onto (plain "+=" or atomic add): a NaN around the valid region would absorb a stray update unseen, so the canary of
# the gradient buffers is a finite value whose bits any addend of the tests' magnitudes changes
G_CANARY = 12345.678
G_CANARY_BITS = int(torch.tensor(G_CANARY, dtype=torch.float32).view(torch.int32))
class Grad:
    """One qfx_lora_grad problem: inputs on the device and the fp64 reference; every run() gets fresh canaried outputs."""

    def __init__(self, kind, seed, M, K, R, group_R, r_valid, layout, out_scale, remap=None):
        assert M <= S.EXACT_MAX_M
        self.kind, self.M, self.K, self.R, self.group_R, self.r_valid, self.layout, self.out_scale = kind, M, K, R, group_R, r_valid, layout, out_scale
        self.rpb, self.batch_rows, self.off = remap if remap else (M, 0, 0)
        self.ngrp = R // group_R
        rows = S.remap_rows(M, self.rpb, self.batch_rows, self.off)
        X, hi, lo = _case_data(kind, seed, (int(rows.max()) + 3, K + 8), (R, M), 1.0)
        g = torch.Generator().manual_seed(seed + 1)
        shape = (r_valid, K)
        self.G0 = [S.exact_ints(g, shape) if kind == "exact" else torch.randn(*shape, generator=g) for _ in range(self.ngrp)]
        ref = S.grad_ref(hi, lo, X[:, :K], rows, group_R, r_valid)
        self.ref = [g0.double() + out_scale * r for g0, r in zip(self.G0, ref)]        # [r_valid, K] per group, fp64
        self.ldvt = roundup(M, 32) + 8
        Vt = torch.zeros(2, R, self.ldvt, dtype=BF)      # columns >= M are zero, as the header requires
        Vt[0, :, :M], Vt[1, :, :M] = hi, lo
        self.Xd, self.Vtd = X.to(DEV), Vt.to(DEV)
        self.Kp = roundup(K, 128)
        self.need = int(_L().lib.qfx_lora_grad_ws_floats(M, K, R))
        assert (self.need > 0) == (M > 512)

    def region(self):
        return (slice(0, self.r_valid), slice(0, self.K)) if self.layout == "A" else (slice(0, self.K), slice(0, self.r_valid))

    def run(self, scratch, ws=None):
        """Fresh G buffers (canary around the initial values); returns the launch arguments and what to read back."""
        gR, Kp = self.group_R, self.Kp
        Gb = []
        for g0 in self.G0:
            b = torch.full((gR + 2, Kp + 8) if self.layout == "A" else (Kp + 2, gR + 3), G_CANARY)
            b[self.region()] = g0 if self.layout == "A" else g0.t()
            Gb.append(b.to(DEV))
        a = _L().LoraGradArgs()
        a.Vt_hi, a.Vt_lo, a.ldvt, a.R, a.r_valid, a.group_R = self.Vtd[0].data_ptr(), self.Vtd[1].data_ptr(), self.ldvt, self.R, self.r_valid, gR
        a.X, a.ldx, a.M, a.K = self.Xd.data_ptr(), self.Xd.stride(0), self.M, self.K
        a.G = Gb[0].data_ptr()
        a.G1 = Gb[1].data_ptr() if self.ngrp > 1 else None
        a.G2 = Gb[2].data_ptr() if self.ngrp > 2 else None
        a.g_sr, a.g_sc = (Gb[0].stride(0), 1) if self.layout == "A" else (1, Gb[0].stride(0))
        a.rows_per_batch, a.x_batch_rows, a.x_row_off, a.out_scale = self.rpb, self.batch_rows, self.off, self.out_scale
        run = dict(args=a, Gb=Gb, ws=None, cnt=None)
        if scratch:
            if ws is None:       # a scratch of its own: 16 canary floats on either side of exactly the floats the problem needs
                run["ws"] = S.canary_f32(self.need + 32, device=DEV)
                ptr = run["ws"].data_ptr() + 64
            else:
                ptr = ws.data_ptr()
            run["cnt"] = torch.zeros((self.K + 127) // 128, dtype=torch.int32, device=DEV)
            # (a single chunk needs no floats: the pointer only selects the plain-store path)
            a.ws, a.ws_count, a.ws_floats = ptr, run["cnt"].data_ptr(), self.need
        return run

    def collect(self, run, case):
        """The written regions [r_valid, K] per group, after the canary checks."""
        out = []
        for b in run["Gb"]:
            assert untouched(b, self.region(), canary=G_CANARY_BITS), f"{case}: G written outside its [r_valid, K] region"
            r = b.cpu()[self.region()]
            out.append((r if self.layout == "A" else r.t()).contiguous())
        if run["cnt"] is not None:
            assert int(run["cnt"].abs().max()) == 0
        if run["ws"] is not None:
            assert untouched(run["ws"], slice(16, 16 + self.need)), f"{case}: scratch written outside the problem's floats"
        return out


def launch_grad(runs):
    L = _L()
    if len(runs) == 1:
        rc = L.lib.qfx_lora_grad(C.byref(runs[0]["args"]), _stream())
    else:
        arr = (L.LoraGradArgs * len(runs))(*[r["args"] for r in runs])
        rc = L.lib.qfx_lora_grad_batch(arr, len(runs), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()


def check_grad(p, got, name, case):
    """Exact data: bit equality with the fp64 sum.  Gaussian data: 1e-4 of the maximum (the bar of test_lora_grad)."""
    for grp, (g, ref) in enumerate(zip(got, p.ref)):
        assert torch.isfinite(g).all(), f"{case}: group {grp} has unwritten or non-finite elements"
        if p.kind == "exact":
            assert same_bits(g, ref.float()), f"{case}: group {grp} differs from the exact sum, max |d| = {(g.double() - ref).abs().max().item()}"
        else:
            e = rel_max(g, ref)
            record_worst(name, case, e, 1e-4)
            assert e <= 1e-4, f"{case}: group {grp} rel err {e:.3e} > 1e-4"


def close_1e6(a, b):
    return all(((x - y).abs().max() / x.abs().max()).item() < 1e-6 for x, y in zip(a, b))


def two_samples(M):
    rpb = (M + 1) // 2
    return (rpb, rpb + 9, 4)


# R, group_R, r_valid, M, K, layout ("A": (g_sr, g_sc) = (ld, 1), "B": (1, ld)), out_scale, row remap over two samples
GRAD_CASES = [
    (16, 16, 16, 1, 8, "A", 1.0, False), (16, 16, 12, 31, 64, "B", 2.0, False), (16, 16, 1, 513, 136, "A", 2.0, True),
    (32, 32, 32, 32, 200, "B", 1.0, False), (32, 16, 12, 33, 384, "A", 1.0, True), (32, 32, 28, 1025, 136, "B", 2.0, False),
    (48, 16, 16, 512, 200, "A", 2.0, True), (48, 48, 44, 513, 64, "B", 1.0, False), (48, 16, 1, 1025, 384, "A", 1.0, False),
    (64, 32, 32, 33, 136, "A", 2.0, False), (64, 32, 28, 1025, 200, "B", 1.0, True), (64, 32, 1, 512, 8, "A", 1.0, False),
    (96, 32, 32, 513, 200, "A", 1.0, True), (96, 32, 28, 31, 136, "B", 2.0, False), (96, 32, 1, 1025, 384, "A", 2.0, False),
    (96, 32, 32, 32, 64, "B", 1.0, False), (16, 16, 16, 1025, 384, "B", 1.0, True), (32, 32, 32, 512, 8, "B", 2.0, False),
]


@pytest.mark.parametrize("R,gR,rv,M,K,layout,scale,remap", GRAD_CASES)
def test_lora_grad_every_instantiation(R, gR, rv, M, K, layout, scale, remap):
    """The atomic form (no scratch) and the deterministic form (scratch: plain stores for one token chunk, the reduce launch for more)
    accumulate out_scale * Vt X onto a non-zero G."""
    for kind in ("exact", "rand"):
        p = Grad(kind, 500 + R + M + K, M, K, R, gR, rv, layout, scale, two_samples(M) if remap else None)
        case = f"{kind} R={R} group_R={gR} r_valid={rv} M={M} K={K} layout={layout} scale={scale} remap={remap}"
        got = {}
        for mode, scratch in (("atomic", False), ("scratch", True), ("scratch2", True)):
            run = p.run(scratch)
            launch_grad([run])
            got[mode] = p.collect(run, f"{case} {mode}")
            check_grad(p, got[mode], f"grad_NF{R // 16}_{'multi' if M > 512 else 'single'}_{mode.rstrip('2')}", f"{case} {mode}")
        assert all(same_bits(a, b) for a, b in zip(got["scratch"], got["scratch2"])), f"{case}: two deterministic launches differ"
        assert close_1e6(got["atomic"], got["scratch"]), f"{case}: atomic and deterministic forms differ by more than 1e-6"


@pytest.mark.parametrize("R,gR,rv", [(16, 16, 16), (48, 16, 12), (96, 32, 32), (64, 32, 28)])
def test_lora_grad_batch_matches_single_launches(R, gR, rv):
    """Five problems in one launch: the grid is as wide as the widest K (narrower problems return early), problems 1 and 2 take the
    reduce launch, which must be a no-op for the other three; the scratches lie apart in one canaried buffer."""
    specs = [   # M, K, scratch, layout, out_scale, remap
        (33, 8, False, "A", 1.0, False),         # one chunk, atomics
        (513, 136, True, "B", 2.0, True),        # two chunks, scratch
        (1025, 384, True, "A", 1.0, False),      # three chunks, scratch: the widest K
        (100, 64, True, "A", 2.0, True),         # one chunk, scratch: plain stores
        (600, 200, False, "B", 1.0, False),      # two chunks, atomics
    ]
    for kind in ("exact", "rand"):
        probs = [Grad(kind, 700 + R + i, M, K, R, gR, rv, lay, sc, two_samples(M) if rm else None) for i, (M, K, _, lay, sc, rm) in enumerate(specs)]
        gap = 64
        total = gap + sum(p.need + gap for p, s in zip(probs, specs) if s[2])
        wsbuf = S.canary_f32(total, device=DEV)
        runs, spans, o = [], [], gap
        for p, s in zip(probs, specs):
            if s[2]:
                runs.append(p.run(True, ws=wsbuf[o:o + p.need] if p.need else wsbuf[o:o + 4]))
                spans.append(slice(o, o + p.need))
                o += p.need + gap
            else:
                runs.append(p.run(False))
        launch_grad(runs)
        assert untouched(wsbuf, *spans), f"{kind} R={R}: scratch written between the problems' floats"
        for i, (p, s, run) in enumerate(zip(probs, specs, runs)):
            case = f"{kind} R={R} problem {i} (M={p.M} K={p.K} scratch={s[2]})"
            got = p.collect(run, case)
            check_grad(p, got, f"grad_batch_NF{R // 16}", case)
            one = p.run(s[2])
            launch_grad([one])
            alone = p.collect(one, case + " alone")
            if s[2] or kind == "exact":
                assert all(same_bits(a, b) for a, b in zip(got, alone)), f"{case}: the batched launch differs from the n = 1 launch"
            else:
                assert close_1e6(got, alone), f"{case}: batched and single atomic launches differ by more than 1e-6"


# ================================================================================================ head reduce
# R, group_R, group_stride, H, problems [(outs, M, remap)]
HEAD_CASES = [
    (48, 16, 56, 1, [("E", 7, None)]),                                   # 5 rows per block, 16 idle threads
    (96, 32, 104, 24, [("T", 7, None)]),                                 # 2 rows per block
    (144, 48, 150, 25, [("ET", 7, (4, 9, 2))]),                          # 1 row per block; a second trip of the 24-slab loop
    (48, 48, 0, 49, [("ET", 13, None), ("ET", 7, (4, 6, 1))]),           # three trips; two problems
    (96, 32, 96, 25, [("E", 9, (5, 8, 3)), ("T", 3, None)]),
    (144, 48, 144, 49, [("T", 5, None), ("E", 11, (6, 7, 1))]),
    (48, 16, 48, 24, [("ET", 11, (6, 7, 1)), ("ET", 4, None)]),
]


@pytest.mark.parametrize("R,gR,gs,H,problems", HEAD_CASES)
def test_lora_head_reduce_edges(R, gR, gs, H, problems):
    L = _L()
    ld_part, ngrp = R + 4, R // gR
    ld_ext = (ngrp - 1) * gs + 3 * gR + 5
    g = torch.Generator().manual_seed(900 + R + H)
    built = []
    for outs, M, remap in problems:
        rpb, batch_rows, off = remap if remap else (M, 0, 0)
        rows = S.remap_rows(M, rpb, batch_rows, off)
        prow = int(rows.max()) + 2
        vals = S.exact_ints(g, (H, M, R)) + S.exact_ints(g, (H, M, R), 2.0 ** -4)
        part = torch.full((H, prow, ld_part), float("nan"))       # a read outside the problem's rows or columns poisons the output
        part[:, rows, :R] = vals
        U = torch.zeros(M, R)
        for h in range(H):                                         # head order, fp32 (exact on these values in any order)
            U += vals[h]
        assert torch.equal(U.double(), vals.double().sum(0))
        Eb = S.canary_bf16(M + 2, ld_ext, device=DEV) if "E" in outs else None
        Th = S.canary_bf16(R + 1, M + 9, device=DEV) if "T" in outs else None
        Tl = S.canary_bf16(R + 1, M + 9, device=DEV) if "T" in outs else None
        a = L.LoraHeadReduceArgs()
        partd = part.to(DEV)
        a.part, a.part_hstride, a.ld_part, a.H, a.M, a.R = partd.data_ptr(), prow * ld_part, ld_part, H, M, R
        if Eb is not None:
            a.ext, a.ld_ext = Eb.data_ptr(), ld_ext
        if Th is not None:
            a.Ut_hi, a.Ut_lo, a.ld_ut = Th.data_ptr(), Tl.data_ptr(), M + 9
        a.group_R, a.group_stride, a.rows_per_batch, a.x_batch_rows, a.x_row_off = gR, gs, rpb, batch_rows, off
        built.append((a, partd, U, Eb, Th, Tl, M))
    arr = (L.LoraHeadReduceArgs * len(built))(*[b[0] for b in built])
    rc = L.lib.qfx_lora_head_reduce(arr, len(built), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for i, (_, _, U, Eb, Th, Tl, M) in enumerate(built):
        case = f"R={R} H={H} problem {i} of {len(built)} (M={M})"
        if Eb is not None:
            want = torch.cat([S.ext_image(U, gR, gs, ld_ext), S.canary_bf16(2, ld_ext)])
            assert same_bits(Eb.cpu(), want), f"{case}: ext image (or its surroundings) differs"
        if Th is not None:
            th, tl = S.ut_image(U, M + 9)
            can = S.canary_bf16(1, M + 9)
            assert same_bits(Th.cpu(), torch.cat([th, can])) and same_bits(Tl.cpu(), torch.cat([tl, can])), f"{case}: Ut image differs"
    record(f"head_reduce_R{R}_H{H}_n{len(built)}", rel=0.0, tol=0.0, case="bit-equal")


# ================================================================================================ operand packing
@pytest.mark.parametrize("seed,scale", [(0, 2.0), (1, 0.75)])
def test_lora_pack_edges(seed, scale):
    """Four descriptors of different size in one launch: a dimension above the 64 x 256 threads of the grid (N = 18432, the strided
    loop), one adapter smaller than a block, every padded rank (zero tails of 16, 32, 48 and 0 columns), ranks that are no multiple of 8,
    the optional fragment images on one descriptor only."""
    from qflux_amd import ops
    L = _L()
    big = (256, 18432)
    descs = [   # r, Rp, K, N, optional images
        (12, 16, *(big if seed == 0 else (192, 136)), False),
        (24, 32, 128, 192, True),
        (33, 48, 64, 96, False),
        (64, 64, *(big if seed == 1 else (320, 72)), False),
    ]
    g = torch.Generator().manual_seed(40 + seed)
    keep, built = [], []
    for r, Rp, K, N, opt in descs:
        Kext = roundup(3 * Rp, 64)
        A, B = torch.randn(r, K, generator=g), torch.randn(N, r, generator=g)
        ref = S.pack_ref(A, B, r, Rp, Kext, scale)
        Ad, Bd = A.to(DEV), B.to(DEV)
        bufs = dict(A_hi=S.canary_bf16(Rp + 1, K + 8, device=DEV), A_lo=S.canary_bf16(Rp + 1, K + 8, device=DEV),
                    Bt_hi=S.canary_bf16(Rp + 1, N + 8, device=DEV), Bt_lo=S.canary_bf16(Rp + 1, N + 8, device=DEV),
                    We=S.canary_bf16(N + 1, Kext + 8, device=DEV), WeT=S.canary_bf16(K + 1, Kext + 8, device=DEV))
        d = L.LoraPackArgs()
        d.A, d.B, d.r, d.K, d.N, d.scale = Ad.data_ptr(), Bd.data_ptr(), r, K, N, scale
        d.A_hi, d.A_lo, d.ld_a = bufs["A_hi"].data_ptr(), bufs["A_lo"].data_ptr(), K + 8
        d.Bt_hi, d.Bt_lo, d.ld_bt = bufs["Bt_hi"].data_ptr(), bufs["Bt_lo"].data_ptr(), N + 8
        d.We, d.ld_we, d.WeT, d.ld_wet, d.Rp, d.Kext = bufs["We"].data_ptr(), Kext + 8, bufs["WeT"].data_ptr(), Kext + 8, Rp, Kext
        if opt:      # head dim 64: K = 2 heads, N = 3 heads; this adapter = rows Rp .. 2 Rp of a three-adapter fragment group
            bufs["A_hl"], bufs["Bt_hl"] = S.canary_bf16(2 * Rp * K, device=DEV), S.canary_bf16(2 * Rp * N, device=DEV)
            bufs["A_fr"] = S.canary_bf16(2 * 3 * Rp * K, device=DEV)
            d.A_hl, d.Bt_hl, d.hl_dh = bufs["A_hl"].data_ptr(), bufs["Bt_hl"].data_ptr(), 64
            d.A_fr, d.fr_row0, d.fr_nf = bufs["A_fr"].data_ptr(), Rp, 3 * Rp // 16
        keep.append((Ad, Bd))
        built.append((d, bufs, ref))
    t = ops.pack_descs_tensor([b[0] for b in built], DEV)
    ops.lora_pack(t, len(built), max(max(K, N) for _, _, K, N, _ in descs))
    torch.cuda.synchronize()
    for (r, Rp, K, N, opt), (_, bufs, ref) in zip(descs, built):
        case = f"r={r} Rp={Rp} K={K} N={N}"
        for name, cols in (("A_hi", K), ("A_lo", K), ("Bt_hi", N), ("Bt_lo", N)):
            got = bufs[name].cpu()
            assert untouched(got, (slice(0, Rp), slice(0, cols))), f"{case}: {name} written outside [Rp, {cols}]"
            assert same_bits(got[:Rp, :cols].contiguous(), ref[name]), f"{case}: {name} differs"
            assert (S.bits(got)[r:Rp, :cols] == 0).all(), f"{case}: {name} rows r.. are not zero"
        Kext = roundup(3 * Rp, 64)
        for name, nrows in (("We", N), ("WeT", K)):
            got = bufs[name].cpu()
            assert untouched(got, (slice(0, nrows), slice(0, Kext))), f"{case}: {name} written outside [{nrows}, Kext]"
            assert (S.bits(got)[:nrows, 3 * Rp:Kext] == 0).all(), f"{case}: the zero tail of {name} is not zero"
            assert same_bits(got[:nrows, :Kext].contiguous(), ref[name]), f"{case}: {name} differs"
        if opt:
            assert same_bits(bufs["A_hl"].cpu(), L.head_fragment_image(ref["A_hi"], ref["A_lo"], 64)), f"{case}: A_hl differs"
            assert same_bits(bufs["Bt_hl"].cpu(), L.head_fragment_image(ref["Bt_hi"], ref["Bt_lo"], 64)), f"{case}: Bt_hl differs"
            g_hi, g_lo = S.canary_bf16(3 * Rp, K), S.canary_bf16(3 * Rp, K)       # the other adapters' rows stay as they were
            g_hi[Rp:2 * Rp], g_lo[Rp:2 * Rp] = ref["A_hi"], ref["A_lo"]
            assert same_bits(bufs["A_fr"].cpu(), L.down_fragment_image(g_hi, g_lo)), f"{case}: A_fr differs"
    record(f"pack_seed{seed}", rel=0.0, tol=0.0, case="bit-equal")
