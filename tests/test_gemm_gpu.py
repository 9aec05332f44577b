"""GPU parity tests of the bf16 and MX-FP8 GEMMs (csrc/qfx_gemm.hip, csrc/qfx_gemm_fp8.hip) at every dispatch path, through the C
ABI, against the fp64 restatement of tests/gemm_ref.py.

Acceptance.  exact_case data: the outputs in gemm_ref.EXACT_OUTPUTS must equal the fp64 value BIT FOR BIT.  Everything else: the
worst error per element, in bf16 ulps of the reference's `scale`, stays within gemm_ref.BARS -- twice the reference's own fp32
noise (tests/test_gemm_ref_cpu.py), never what the kernels give; no tensor-max normalisation.  Every output buffer has 3 extra rows
and (except pad = 0 cases) a row stride wider than N, starts as a canary (bf16 0x7FC1, bytes 0xA5) and is compared WHOLE; inputs sit
in NaN-filled wider buffers (row strides wider than K, column slices, the text rows of a joint buffer).  Masked rows must be +0.
Worst errors per dispatch family and the wall time of this file: gemm_parity.json.

Which case list reaches which instantiation, launcher branch or refusal arm:
  (gemm_kernel<EPI> and gemm_fp8_kernel<EPI> are the two instantiations of ONE tile body, gemm_tile_body<EPI, FP8> of
  csrc/qfx_gemm_tile.h: the tile map, staging, segment switch, mid-rounding and epilogue each case list below reaches are the same text)
  gemm_kernel<0..3>            qfx_gemm_bf16 below 160 tiles of 256x128: SMALL_CASES (M 1 .. 257, N 4 .. 260 incl. N % 8 != 0, K1 64 .. 320
                               = 1 .. 5 K tiles on the 2-stage buffer, K2 0 / 64 / 128), ARM_CASES, SWEEP_CASES
  gemm256_kernel<0..3, 256x128 | 256x256 | 160x192>
                               qfx_gemm_grouped, n = 1, geometry forced by qfx_gemm_tune: PERSIST_CASES (M 1, 16, BMT - 1, BMT, BMT + 1,
                               2 BMT + 17: dead, partial and full waves; N 8, TN - 8, TN, 2 TN + 8, whole tiles only on 256x256; K1 64 .. 320:
                               one K tile against the 2- / 3-stage ring, the ring, a wrapped ring), ARM_CASES, SWEEP_CASES, MANY_TILE_CASES
                               (260 tiles on 256 CUs: a block runs two tiles, the loaders cross the boundary), GROUPED_CASES
  use_dma (d(GELU) aux rows by LDS-DMA, 256x256 and 160x192)      LANDING_CASES: both sides of row mask / M % 16 / ragged columns /
                               pending bias / sample boundary inside a wave / aux_unmapped, and the early return of a short tile
  launcher: persistent threshold   qfx_gemm_bf16 and qfx_gemm_mxfp8 on both sides (test_persistent_threshold_of_the_single_entries)
  launcher: geometry choice    forced per test; 256x256 with N % 256 != 0 falls back (FALLBACK_CASES)
  launcher: gm                 n = 6 -> gm = 4, five M-tiles per problem (GROUPED_CASES[3], [4]); n = 2, 3 -> gm = 8
  launcher: tile_start         300 tiles on 152 blocks, the boundary between two problems inside a block's tile list (GROUPED_CASES[5])
  aux_unmapped, seg2_plain, GATE_RES C2 + row mask, gate_bstride with 3 samples, a_* with c_* maps      ARM_CASES, on every kernel
  gemm_fp8_kernel<0..3>        qfx_gemm_mxfp8 below the threshold: FP8_SMALL_CASES (K1 128 / 256 / 384, K2 0 / 64, c_* maps)
  gemm256_kernel<0..3, 256x128, FP8>   qfx_gemm_mxfp8_grouped: FP8_PERSIST_CASES, FP8_GROUPED_CASES (n = 3), FP8_QUANT_EPI_CASES (cq / cs bit-equal
                               to quant_mxfp8_ref of the bf16 output, cq_only 0 / 1, each epilogue with and without a row mask)
  quant_mxfp8_kernel           QUANT_CASES: ldx > K, ldq > K, row remap, the edge blocks of gemm_ref.quant_input (mx_quant8 of
                               csrc/qfx_common.h, the quantiser of the epilogue above as well)
  refusals                     validate: NULL A1 / B1 / C; M, N, K1 <= 0; K1, K2 % 64; K2 < 0; N % 4; lda1, ldb1 % 8; ldc % 4; K2 > 0 with NULL
                               A2 / B2 or lda2, ldb2 % 8; rows_per_batch <= 0; GELU without C2, ldc2 % 4; GATE_RES without gate / aux,
                               ldaux % 4; DGELU without aux, ldaux % 4; epi 4 / -1 -> QFX_EUNSUPPORTED (test_refusals_validate)
                               qfx_gemm_grouped: n = 0, 7; mixed epilogues; ok256: N % 8, ldc % 8, ldc2 % 8 (GELU; GATE_RES with C2), ldaux % 8
                               (GATE_RES, DGELU), gate_bstride % 8 (test_refusals_grouped)
                               MX-FP8, both entries through validate_fp8: NULL sa / sb; K1 % 128; lda1, ldb1 % 16; a_batch_rows != 0; the arms of
                               validate on the halved problem (N % 4, ldc % 4, rows_per_batch, A2, lda2, epi 5 / -1); two faults at once (QFX_EINVAL
                               wins over the epilogue out of range); seg2_plain (grouped, also with epi 5); cq without cs, with
                               GATE_RES, N % 128, ldcq < N, cq_rows too small (whole and ragged last sample); cq_only without cq; cq / cq_only on the small path ->
                               QFX_EUNSUPPORTED (test_refusals_mxfp8)
The same-XCD split-K lever stays off (its default); tests/test_kernels_gpu.py::test_gemm_same_xcd_split_k_lever covers it."""
import ctypes as C
import functools
import time

import pytest
import torch

import gemm_ref as G
from gemm_ref import DGELU, GATE_RES, GELU, NONE, replace
from parity_util import _observe

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda:0"
EINVAL, EUNSUPPORTED = -1, -2
KINDS = ("exact", "rand")
_STATS = {"what": "tests/test_gemm_gpu.py: worst error in bf16 ulps of the reference's scale (tests/gemm_ref.py), per output kind and per "
                  "dispatch family (bit-equal outputs of exact_case data are asserted, not listed); wall_s: seconds this file took",
          "bars": dict(G.BARS), "worst_ulps_per_output_kind": {}, "worst": {}, "wall_s": 0.0}
_T0 = [None]


def _L():
    from qflux_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(autouse=True)
def _restore_gemm_policy():
    """qfx_gemm_tune is process-wide: back to every geometry after each test; the wall time of the file so far goes to the table."""
    if _T0[0] is None:
        _T0[0] = time.time()
    yield
    assert _L().lib.qfx_gemm_tune(b"all", None) == 0
    _STATS["wall_s"] = round(time.time() - _T0[0], 2)
    _observe(None, None, dump=("gemm_parity.json", _STATS))


def tune(geo):
    assert _L().lib.qfx_gemm_tune(geo.encode(), None) == 0


def record_worst(fam, key, case, err):
    kinds = _STATS["worst_ulps_per_output_kind"]
    kinds[key] = max(kinds.get(key, 0.0), err)
    slot = _STATS["worst"].setdefault(fam, {})
    if key not in slot or err >= slot[key]["ulps"]:
        slot[key] = dict(ulps=err, bar=G.BARS[key], case=repr(case))


@functools.lru_cache(maxsize=8)
def _case(case, kind):
    """(inputs, fp64 reference) of one case: computed once, shared by the launches that need it, never modified."""
    inp = G.make_inputs(case, kind)
    return inp, G.gemm_ref(inp, case)


# ---------------------------------------------------------------------------------------------- buffers
def _put(t, pad, rows=None, buf_rows=None):
    """Device copy of t [r, K] (bf16 or fp8 bytes) inside a NaN-filled buffer [buf_rows, K + pad'] at the rows `rows`, at column 8
    (16 for bytes) when pad >= 16, with 16384 more NaN elements behind it (a kernel that lost a row map reads NaN, not another allocation).  Returns (keep-alive, pointer of element [0, 0], row stride)."""
    r, K = t.shape
    by = t.dtype == torch.uint8
    unit = 16 if by else 8
    p = pad // 8 * unit
    off = unit if pad >= 16 else 0
    buf_rows = buf_rows or r
    ld = K + p
    flat = torch.full((buf_rows * ld + 16384,), 0x7F if by else G.CANARY_BF16, dtype=torch.uint8 if by else torch.int16, device=DEV)
    flat = flat if by else flat.view(BF)
    view = flat[:buf_rows * ld].view(buf_rows, ld)
    idx = torch.arange(r) if rows is None else rows
    view[idx.to(DEV), off:off + K] = t.to(DEV)
    return flat, flat.data_ptr() + off * t.element_size(), ld


def _vec(t):
    flat = torch.zeros(t.numel() + 4104, dtype=t.dtype, device=DEV)
    flat[:t.numel()] = t.flatten().to(DEV)
    return flat


class Out:
    def __init__(self, rows, buf_rows, N, ld):
        self.rows, self.buf_rows, self.N, self.ld = rows, buf_rows + 3, N, ld
        self.buf = G.canary_bf16(self.buf_rows * ld, device=DEV)

    def host(self):
        return self.buf.cpu().view(self.buf_rows, self.ld)


class Built:
    pass


def build(case, kind, cq=False, cq_only=False):
    """GemmArgs / GemmFp8Args of a case with every buffer behind it."""
    L = _L()
    inp, _ = _case(case, kind)
    M, N, K1, K2 = case.M, case.N, case.K1, case.K2
    pad = case.pad
    add = (0, 0, 0) if pad == 0 else (0, 8, 16)          # three different output strides: a mixed-up one shows
    b = Built()
    b.case, b.keep, b.outs = case, [], {}
    a = L.GemmArgs()
    arows, abuf, a.a_batch_rows, a.a_row_off = case.row_map(case.a_map)
    crows, cbuf, a.c_batch_rows, a.c_row_off = case.row_map(case.c_map)

    def operand(t, **kw):
        keep, ptr, ld = _put(t, pad, **kw)
        b.keep.append(keep)
        return ptr, ld

    if case.fp8:
        a.A1, a.lda1 = operand(inp["A1q"])
        a.B1, a.ldb1 = operand(inp["B1q"])
    else:
        a.A1, a.lda1 = operand(inp["A1"], rows=arows, buf_rows=abuf)
        a.B1, a.ldb1 = operand(inp["B1"])
    a.K1, a.K2, a.M, a.N = K1, K2, M, N
    if K2:
        a.A2, a.lda2 = operand(inp["A2"])
        a.B2, a.ldb2 = operand(inp["B2"])
    if inp["bias"] is not None:
        b.keep.append(_vec(inp["bias"]))
        a.bias = b.keep[-1].data_ptr()
    b.outs["C"] = Out(crows, cbuf, N, N + pad + add[0])
    a.C, a.ldc = b.outs["C"].buf.data_ptr(), b.outs["C"].ld
    if case.epi == GELU:
        b.outs["C2"] = Out(crows, cbuf, N, N + pad + add[1])
    elif case.epi == GATE_RES and case.c2:
        b.outs["C2"] = Out(torch.arange(M), M, N, N + pad + add[1])
    if "C2" in b.outs:
        a.C2, a.ldc2 = b.outs["C2"].buf.data_ptr(), b.outs["C2"].ld
    if case.epi in (GATE_RES, DGELU):
        if case.aux_unmapped or not case.c_map:
            keep, a.aux, a.ldaux = _put(inp["aux"], pad + add[2])
        else:
            keep, a.aux, a.ldaux = _put(inp["aux"], pad + add[2], rows=crows, buf_rows=cbuf)
        b.keep.append(keep)
    if case.epi == GATE_RES:
        keep, a.gate, ldg = _put(inp["gate"], pad)
        b.keep.append(keep)
        a.gate_bstride = 0 if case.gate_shared else ldg
    a.rows_per_batch = case.rows_per_batch
    a.epi = case.epi
    if inp["mask"] is not None:
        b.keep.append(_vec(inp["mask"]))
        a.row_mask = b.keep[-1].data_ptr()
    a.aux_unmapped, a.seg2_plain = int(case.aux_unmapped), int(case.seg2_plain)
    b.g = a
    if case.fp8:
        f = L.GemmFp8Args()
        f.g = a
        b.keep += [_vec(inp["sa"]), _vec(inp["sb"])]
        f.sa, f.sb = b.keep[-2].data_ptr(), b.keep[-1].data_ptr()
        if cq:
            b.ldcq = N + (16 if pad else 0)
            b.cq = torch.full((b.outs["C"].buf_rows * b.ldcq,), G.CANARY_U8, dtype=torch.uint8, device=DEV)
            b.cs = torch.full((N // 128 * b.outs["C"].buf_rows * 4,), G.CANARY_U8, dtype=torch.uint8, device=DEV)
            f.cq, f.cs, f.ldcq, f.cq_rows, f.cq_only = b.cq.data_ptr(), b.cs.data_ptr(), b.ldcq, b.outs["C"].buf_rows, int(cq_only)
        b.f = f
    return b


def launch(b, entry):
    lib = _L().lib
    if entry == "bf16":
        return lib.qfx_gemm_bf16(C.byref(b.g), _stream())
    if entry == "grouped":
        return lib.qfx_gemm_grouped(C.byref(b.g), 1, _stream())
    if entry == "fp8":
        return lib.qfx_gemm_mxfp8(C.byref(b.f), _stream())
    return lib.qfx_gemm_mxfp8_grouped(C.byref(b.f), 1, _stream())


def launch_group(bs, fp8=False):
    L = _L()
    arr = ((L.GemmFp8Args if fp8 else L.GemmArgs) * len(bs))(*[(b.f if fp8 else b.g) for b in bs])
    fn = L.lib.qfx_gemm_mxfp8_grouped if fp8 else L.lib.qfx_gemm_grouped
    return fn(arr, len(bs), _stream())


def untouched(b):
    return all(bool((G.bits(o.buf) == G.CANARY_BF16).all()) for o in b.outs.values())


def verify(b, kind, fam, skip=()):
    """Whole-buffer comparison of every output of a launched case."""
    case = b.case
    _, ref = _case(case, kind)
    for name, o in b.outs.items():
        got = o.host()
        if name in skip:
            assert bool((G.bits(got) == G.CANARY_BF16).all()), f"{fam} {case}: {name} was written"
            continue
        val, scale = ref[name]
        key = G.key_of(case, name)
        want = G.image(val, o.rows, o.buf_rows, o.ld)
        outside = G.bits(want) == G.CANARY_BF16
        outside[o.rows, :o.N] = False
        assert bool((G.bits(got)[outside] == G.CANARY_BF16).all()), f"{fam} {case} {kind}: {name} written outside its rows / columns"
        inner = got[o.rows, :o.N]
        if kind == "exact" and key in G.EXACT_OUTPUTS or case.sweep and name == "C" and case.epi == GELU:
            bad = G.bits(inner) != G.bits(val.to(BF))
            assert not bad.any(), f"{fam} {case} {kind}: {name} not bit-equal at {int(bad.sum())} elements, max |d| = {(inner.double() - val).abs().max().item()}"
            continue
        if case.mask:
            rows = [r for r in case.mask if r < case.M]
            assert not G.bits(inner[rows]).any(), f"{fam} {case} {kind}: masked rows of {name} are not +0"
        if case.sweep:
            fl = G.flushed(val)
            assert bool((inner[fl].double().abs() < G.FLUSH).all())
            inner, val, scale = inner[~fl], val[~fl], scale[~fl]
        e = G.err_ulps(inner, val, scale)
        record_worst(fam, key, case, e)
        assert e <= G.BARS[key], f"{fam} {key} {kind} {case}: {e:.3f} ulps of scale > {G.BARS[key]}"


def run(case, kind, entry, fam, rc=0):
    b = build(case, kind)
    assert launch(b, entry) == rc, (fam, case)
    torch.cuda.synchronize()
    verify(b, kind, fam)


# ---------------------------------------------------------------------------------------------- bf16
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("epi", G.EPIS)
def test_small_kernel(epi, kind):
    for case in G.SMALL_CASES[epi]:
        run(case, kind, "bf16", "small")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("epi", G.EPIS)
@pytest.mark.parametrize("geo", list(G.GEOS))
def test_persistent_kernel(geo, epi, kind):
    tune(geo)
    for case in G.PERSIST_CASES[(geo, epi)]:
        run(case, kind, "grouped", f"persist_{geo}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geo", list(G.GEOS))
def test_more_tiles_than_cus(geo, kind):
    tune(geo)
    for case in G.MANY_TILE_CASES[geo]:
        run(case, kind, "grouped", f"many_tiles_{geo}")


@pytest.mark.parametrize("kind", KINDS)
def test_wide_tile_falls_back_on_ragged_n(kind):
    tune("256x256")
    for case in G.FALLBACK_CASES:
        run(case, kind, "grouped", "fallback")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("entry", ["small"] + list(G.GEOS))
def test_arms_no_other_test_reaches(entry, kind):
    if entry != "small":
        tune(entry)
    for case in G.ARM_CASES:
        run(case, kind, "bf16" if entry == "small" else "grouped", f"arms_{entry}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geo", list(G.LANDING_CASES))
def test_dgelu_landing_buffer_conditions(geo, kind):
    tune(geo)
    for case in G.LANDING_CASES[geo]:
        run(case, kind, "grouped", f"landing_{geo}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("idx", range(len(G.GROUPED_CASES)))
def test_grouped_launches(idx, kind):
    geo, probs = G.GROUPED_CASES[idx]
    tune(geo)
    bs = [build(c, kind) for c in probs]
    assert launch_group(bs) == 0
    torch.cuda.synchronize()
    for b in bs:
        verify(b, kind, f"grouped_n{len(probs)}")


@pytest.mark.parametrize("entry", ["small"] + list(G.GEOS))
def test_gelu_sweep(entry):
    """Every bf16 h with 2^-64 <= |h| <= 16: C (GELU) bit-equal, C2 and the d(GELU) output within their bars."""
    if entry != "small":
        tune(entry)
    for case in G.SWEEP_CASES:
        run(case, "rand", "bf16" if entry == "small" else "grouped", f"sweep_{entry}")


def test_persistent_threshold_of_the_single_entries():
    """qfx_gemm_bf16 / qfx_gemm_mxfp8 take the small kernel below 160 tiles of 256x128 and the persistent one from there on: both sides
    against the reference; the quantising epilogue is refused below it (nothing written) and served from it on."""
    for fp8 in (False, True):
        below = G.Case(NONE, 17, 159 * 128, 128, 0, fp8=fp8)
        above = G.Case(NONE, 17, 160 * 128, 128, 0, fp8=fp8)
        for case in (below, above):
            run(case, "exact", "fp8" if fp8 else "bf16", "threshold")
        # the quantising epilogue exists on the persistent side only
        for case, rc in ((below, EUNSUPPORTED), (above, 0)):
            if fp8:
                b = build(case, "exact", cq=True)
                assert launch(b, "fp8") == rc
                torch.cuda.synchronize()
                assert (rc == 0) != untouched(b)
                assert (rc == 0) != bool((b.cq == G.CANARY_U8).all()) and (rc == 0) != bool((b.cs == G.CANARY_U8).all())


# ---------------------------------------------------------------------------------------------- MX-FP8
@pytest.mark.parametrize("case", G.QUANT_CASES)
def test_quant_mxfp8_is_the_reference(case):
    L = _L()
    M, K, rpb, T = case
    x = G.quant_input(case)
    c = G.Case(NONE, M, 8, K, rpb=rpb)
    rows, buf_rows, br, off = c.row_map(T)
    keep, xptr, ldx = _put(x, 24, rows=rows, buf_rows=buf_rows)
    ldq = K + 32
    Q = torch.full(((M + 3) * ldq,), G.CANARY_U8, dtype=torch.uint8, device=DEV)
    S = torch.full((K // 128 * M * 4 + 64,), G.CANARY_U8, dtype=torch.uint8, device=DEV)
    a = L.QuantArgs(xptr, ldx, M, K, Q.data_ptr(), ldq, S.data_ptr(), 0, c.rows_per_batch, br, off)
    assert L.lib.qfx_quant_mxfp8(C.byref(a), _stream()) == 0
    torch.cuda.synchronize()
    qb, sb, _ = G.quant_mxfp8_ref(x)
    want = torch.full((M + 3, ldq), G.CANARY_U8, dtype=torch.uint8)
    want[:M, :K] = qb
    assert torch.equal(Q.cpu().view(M + 3, ldq), want)
    assert torch.equal(S.cpu()[:sb.numel()], sb) and bool((S.cpu()[sb.numel():] == G.CANARY_U8).all())
    for bad in (dict(K=K + 64), dict(ldx=ldx + 4), dict(ldq=ldq + 8), dict(M=0), dict(rows_per_batch=0), dict(X=None), dict(Q=None), dict(S=None)):
        a2 = L.QuantArgs.from_buffer_copy(a)
        for k, v in bad.items():
            setattr(a2, k, v)
        assert L.lib.qfx_quant_mxfp8(C.byref(a2), _stream()) == EINVAL, bad


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("epi", G.EPIS)
def test_mxfp8_small_kernel(epi, kind):
    for case in G.FP8_SMALL_CASES[epi]:
        run(case, kind, "fp8", "fp8_small")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("epi", G.EPIS)
def test_mxfp8_persistent_kernel(epi, kind):
    for case in G.FP8_PERSIST_CASES[epi]:
        run(case, kind, "fp8_grouped", "fp8_persist")


@pytest.mark.parametrize("kind", KINDS)
def test_mxfp8_grouped_launch(kind):
    for probs in G.FP8_GROUPED_CASES:
        bs = [build(c, kind) for c in probs]
        assert launch_group(bs, fp8=True) == 0
        torch.cuda.synchronize()
        for b in bs:
            verify(b, kind, "fp8_grouped")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", G.FP8_QUANT_EPI_CASES, ids=lambda c: G.EPI_NAME[c.epi] + ("-masked" if c.mask else ""))
def test_mxfp8_quantising_epilogue(case, kind):
    """cq / cs = quant_mxfp8_ref of the bf16 output the next GEMM contracts over (C2 of GELU, C otherwise), bit for bit, at the rows of
    C; with cq_only the same bytes and that bf16 output keeps its canary everywhere, masked rows included (C of GELU, the
    pre-activation, is still written)."""
    name = "C2" if case.epi == GELU else "C"
    b = build(case, kind, cq=True)
    assert launch(b, "fp8_grouped") == 0
    torch.cuda.synchronize()
    verify(b, kind, "fp8_quant_epi")
    o = b.outs[name]
    bf = o.host()[o.rows, :o.N]
    qb, sb, _ = G.quant_mxfp8_ref(bf)
    want = torch.full((o.buf_rows, b.ldcq), G.CANARY_U8, dtype=torch.uint8)
    want[o.rows, :o.N] = qb
    cq0, cs0 = b.cq.cpu(), b.cs.cpu()
    assert torch.equal(cq0.view(o.buf_rows, b.ldcq), want)
    assert torch.equal(cs0, G.scale_image(sb, case.M, o.rows, o.buf_rows))
    b1 = build(case, kind, cq=True, cq_only=True)
    assert launch(b1, "fp8_grouped") == 0
    torch.cuda.synchronize()
    verify(b1, kind, "fp8_quant_epi", skip=(name,))
    assert torch.equal(b1.cq.cpu(), cq0) and torch.equal(b1.cs.cpu(), cs0)


# ---------------------------------------------------------------------------------------------- refusals
def _refused(b, call, rc, what):
    assert call() == rc, what
    torch.cuda.synchronize()
    assert untouched(b), f"{what}: refused, yet an output was written"


def _mutations(b, muts, call_of, fp8=False):
    L = _L()
    for fields, rc in muts:
        g = L.GemmArgs.from_buffer_copy(b.g)
        f = L.GemmFp8Args.from_buffer_copy(b.f) if fp8 else None
        for k, v in fields.items():
            if f is not None and k in ("sa", "sb", "cq", "cs", "ldcq", "cq_rows", "cq_only"):
                setattr(f, k, v)
            else:
                setattr(g, k, v)
        if f is not None:
            f.g = g
        _refused(b, call_of(f if fp8 else g), rc, fields)


def test_refusals_validate():
    lib = _L().lib
    call_of = lambda g: (lambda: lib.qfx_gemm_bf16(C.byref(g), _stream()))       # noqa: E731
    base = G.Case(NONE, 17, 72, 128, 64)
    b = build(base, "exact")
    N, ld = 72, b.g.ldc
    common = [(dict(A1=None), EINVAL), (dict(B1=None), EINVAL), (dict(C=None), EINVAL), (dict(M=0), EINVAL), (dict(M=-1), EINVAL), (dict(N=0), EINVAL),
              (dict(K1=0), EINVAL), (dict(K1=-64), EINVAL), (dict(K1=96), EINVAL), (dict(K2=32), EINVAL), (dict(K2=-64), EINVAL), (dict(N=70), EINVAL),
              (dict(lda1=b.g.lda1 + 4), EINVAL), (dict(ldb1=b.g.ldb1 + 4), EINVAL), (dict(ldc=ld + 2), EINVAL), (dict(A2=None), EINVAL),
              (dict(B2=None), EINVAL), (dict(lda2=b.g.lda2 + 4), EINVAL), (dict(ldb2=b.g.ldb2 + 4), EINVAL), (dict(rows_per_batch=0), EINVAL),
              (dict(rows_per_batch=-3), EINVAL), (dict(epi=4), EUNSUPPORTED), (dict(epi=-1), EUNSUPPORTED)]
    _mutations(b, common, call_of)
    assert lib.qfx_gemm_bf16(None, _stream()) == EINVAL
    for epi, muts in ((GELU, [dict(C2=None), dict(ldc2=N + 2)]), (GATE_RES, [dict(gate=None), dict(aux=None), dict(ldaux=N + 2)]),
                      (DGELU, [dict(aux=None), dict(ldaux=N + 2)])):
        be = build(replace(base, epi=epi, c2=True), "exact")
        _mutations(be, [(m, EINVAL) for m in muts], call_of)
    # ... and the accepted launch right after them is still right
    assert launch(b, "bf16") == 0
    torch.cuda.synchronize()
    verify(b, "exact", "small")


def test_refusals_grouped():
    L = _L()
    lib = L.lib
    one = lambda g: (lambda: lib.qfx_gemm_grouped(C.byref(g), 1, _stream()))       # noqa: E731
    base = G.Case(NONE, 17, 72, 128, 64)
    b = build(base, "exact")
    arr = (L.GemmArgs * 6)(*[b.g] * 6)
    _refused(b, lambda: lib.qfx_gemm_grouped(arr, 0, _stream()), EINVAL, "n = 0")
    _refused(b, lambda: lib.qfx_gemm_grouped(arr, 7, _stream()), EINVAL, "n = 7")
    _refused(b, lambda: lib.qfx_gemm_grouped(None, 1, _stream()), EINVAL, "NULL list")
    bg = build(replace(base, epi=GELU), "exact")
    mixed = (L.GemmArgs * 2)(b.g, bg.g)
    _refused(b, lambda: lib.qfx_gemm_grouped(mixed, 2, _stream()), EINVAL, "mixed epilogues")
    assert untouched(bg)
    # a refused SECOND problem stops the whole launch
    bad = L.GemmArgs.from_buffer_copy(b.g)
    bad.K1 = 96
    second = (L.GemmArgs * 2)(b.g, bad)
    _refused(b, lambda: lib.qfx_gemm_grouped(second, 2, _stream()), EINVAL, "second problem invalid")
    _mutations(b, [(dict(N=68), EINVAL), (dict(ldc=b.g.ldc + 4), EINVAL), (dict(epi=4), EUNSUPPORTED)], one)      # ok256: N % 8, ldc % 8
    _mutations(bg, [(dict(ldc2=bg.g.ldc2 + 4), EINVAL)], one)
    br = build(replace(base, epi=GATE_RES, c2=True, rpb=9), "exact")
    _mutations(br, [(dict(ldc2=br.g.ldc2 + 4), EINVAL), (dict(ldaux=br.g.ldaux + 4), EINVAL), (dict(gate_bstride=br.g.gate_bstride + 4), EINVAL)], one)
    bd = build(replace(base, epi=DGELU), "exact")
    _mutations(bd, [(dict(ldaux=bd.g.ldaux + 4), EINVAL)], one)
    # ... and the untouched arguments still launch, on the geometry the launcher picks by itself
    for bb in (b, bg, br, bd):
        assert launch(bb, "grouped") == 0
        torch.cuda.synchronize()
        verify(bb, "exact", "persist_auto")


def test_refusals_mxfp8():
    lib = _L().lib
    single = lambda f: (lambda: lib.qfx_gemm_mxfp8(C.byref(f), _stream()))                  # noqa: E731
    grouped = lambda f: (lambda: lib.qfx_gemm_mxfp8_grouped(C.byref(f), 1, _stream()))      # noqa: E731
    base = G.Case(NONE, 17, 128, 128, 64, fp8=True)
    b = build(base, "exact", cq=True)
    plain = build(base, "exact")
    both = [(dict(sa=None), EINVAL), (dict(sb=None), EINVAL), (dict(K1=192), EINVAL), (dict(K1=64), EINVAL), (dict(K2=32), EINVAL),
            (dict(lda1=plain.g.lda1 + 8), EINVAL), (dict(ldb1=plain.g.ldb1 + 8), EINVAL), (dict(a_batch_rows=24, a_row_off=1), EINVAL),
            (dict(A1=None), EINVAL), (dict(C=None), EINVAL), (dict(M=0), EINVAL), (dict(epi=5), EUNSUPPORTED), (dict(epi=-1), EUNSUPPORTED),
            (dict(N=130), EINVAL), (dict(ldc=plain.g.ldc + 2), EINVAL), (dict(rows_per_batch=0), EINVAL), (dict(A2=None), EINVAL),
            (dict(lda2=plain.g.lda2 + 4), EINVAL)]
    # two faults at once: every QFX_EINVAL arm wins over the epilogue out of range, whichever check states it
    both += [(dict(epi=5, sa=None), EINVAL), (dict(epi=5, K1=192), EINVAL), (dict(epi=5, lda1=plain.g.lda1 + 8), EINVAL),
             (dict(epi=5, a_batch_rows=24, a_row_off=1), EINVAL), (dict(epi=5, N=130), EINVAL), (dict(epi=5, rows_per_batch=0), EINVAL),
             (dict(epi=5, K2=32), EINVAL), (dict(epi=5, cq_only=1), EUNSUPPORTED)]
    _mutations(plain, both, single, fp8=True)
    _mutations(plain, both + [(dict(seg2_plain=1), EINVAL), (dict(cq_only=1), EINVAL), (dict(epi=5, seg2_plain=1), EINVAL)], grouped, fp8=True)
    rows = b.outs["C"].buf_rows
    _mutations(b, [(dict(cs=None), EINVAL), (dict(N=136), EINVAL), (dict(ldcq=120), EINVAL), (dict(ldcq=b.ldcq + 4), EINVAL), (dict(cq_rows=16), EINVAL)],
               grouped, fp8=True)
    assert b.f.cq_rows == rows and bool((b.cq == G.CANARY_U8).all()) and bool((b.cs == G.CANARY_U8).all())
    bm = build(replace(base, M=18, rpb=9, c_map=5), "exact", cq=True)
    _mutations(bm, [(dict(cq_rows=18), EINVAL), (dict(cq_rows=27), EINVAL)], grouped, fp8=True)      # 18 compact rows, but C's rows reach to 28
    # a ragged last sample counts as a sample: 17 rows of 9 per sample are two samples of 14 joint rows
    bm = build(replace(base, M=17, rpb=9, c_map=5), "exact", cq=True)
    _mutations(bm, [(dict(cq_rows=14), EINVAL), (dict(cq_rows=27), EINVAL)], grouped, fp8=True)
    bm.f.cq_rows = 28
    bm.cs = torch.full((28 * 4,), G.CANARY_U8, dtype=torch.uint8, device=DEV)
    bm.f.cs = bm.cs.data_ptr()
    assert launch(bm, "fp8_grouped") == 0
    torch.cuda.synchronize()
    verify(bm, "exact", "fp8_quant_epi")
    o = bm.outs["C"]
    _, sb, _ = G.quant_mxfp8_ref(o.host()[o.rows, :o.N])
    assert torch.equal(bm.cs.cpu(), G.scale_image(sb, 17, o.rows, 28))
    bg = build(replace(base, epi=GATE_RES), "exact", cq=True)
    _mutations(bg, [(dict(), EINVAL)], grouped, fp8=True)                                    # cq with GATE_RES
    # the quantising epilogue on the small-kernel path
    _mutations(b, [(dict(), EUNSUPPORTED), (dict(cq=None, cs=None, cq_only=1), EUNSUPPORTED)], single, fp8=True)
    assert bool((b.cq == G.CANARY_U8).all()) and bool((b.cs == G.CANARY_U8).all())
    assert launch(plain, "fp8") == 0
    torch.cuda.synchronize()
    verify(plain, "exact", "fp8_small")
