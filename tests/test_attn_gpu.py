"""GPU parity tests of the attention kernels (csrc/qfx_attn.hip, csrc/qfx_attn64.hip, csrc/qfx_attn_bwd1.hip) at every dispatch line,
through the C ABI, against the fp64 restatement of tests/attn_ref.py.

Acceptance.  select data: O, dV and dsum must equal the fp64 value BIT FOR BIT (a zero that is a sum may have either sign), dQ and dK
must be +-0, the rank-r sums of an exact X must be exact.  Everything else: the worst error per element, in ulps of the reference's
`scale` (bf16 ulps for O, dQ, dK, dV; fp32 ulps for lse2, dsum, part), stays within attn_ref.BARS -- twice the reference's own fp32
noise (tests/test_attn_ref_cpu.py), never what the kernels give; no tensor-max normalisation.
Every output -- O, lse2, dsum, dQ, dK, dV, every part -- starts as a canary (bf16 0x7FC1,
fp32 0x7FC00000), has 3 extra rows (lse2 / dsum: one extra head slab) and a row stride wider than its extent, and is compared WHOLE:
the pad columns [S, S_pad) of lse2 / dsum, the other heads' slabs, the columns [0, c0) and [c0 + R, ld_part) of a part row and the part
rows of a stream without adapter weights must keep the canary (include/qfx.h says so since this file).  Inputs sit in NaN-filled wider
buffers: the backward's lse2 / dsum inputs carry NaN in their pad columns as well.  part is judged against attn_ref.part_ref of the bf16
X the kernel itself stored.  The backward entries get the reference's q(O) and fp32 lse2, so each kernel is judged alone; one chained
case per backward family feeds the forward kernel's own outputs and is judged against the reference of THOSE inputs.
Worst errors per dispatch line and the wall time of this file: attn_parity.json.

Which line reaches which kernel (each forced through qfx_attn_tune; every line runs rand, spike and select data, plain and fused mode):
  fwd32w4 / fwd32w8   attn_fwd_kernel<64 | 128, 4 | 8>          fwd64=0, fwd_waves=4 / 8        every case
  fwd64 / fwd64p      the skewed 64-query forward / its pipelined form   fwd64=1 / 1p            dh = 128
  prep                attn_prep_kernel<64 | 128>                                                 every case
  dq32                attn_bwd_dq_kernel<64 | 128, 4>           dq64=0                           every case
  dq64                the 64-query dQ kernel                    dq64=1                           dh = 128
  dkv                 attn_bwd_dkv_kernel<64 | 128>                                              every case
  onepass             qfx_attn_bwd_fused (prep + the one-pass kernel): dh = 128, S >= 64; turn counters zero afterwards, the accumulator
                      workspace pre-filled with NaN
  "fused mode" of the forward = the rank-r slot hl[0]; of the backward = qk_saved (norm_flags 0 / 1, rope_bstride 0 / S dh, T 0 / 16 / 48 /
  S rounded down to 16) with the slots hl[1..3] (R 16 / 32, c0 = 4 with ld_part = R + 4, w_pk[0] or w_pk[1] NULL, a slot left unset).
  Strides: Q, K, V in three buffers with three strides or as column slices of one; ldo = lddq = lddk = lddv = D + 4 (store_frag's
  8-byte path) or multiples of 8.  Key masks: none, finite, -inf inside tile 0, -inf on a whole interior tile, -inf on the tail, one
  mask per sample.  Shapes: attn_ref.SHAPES x H 1..3 x B 1..2.
  refusals            one table per entry point (test_refusals_*): every arm returns its code and leaves every canary intact."""
import ctypes as C
import functools
import time

import pytest
import torch

import attn_ref as A
from parity_util import _observe

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda:0"
EINVAL, EUNSUPPORTED = -1, -2
KINDS = ("rand", "spike", "select")
ANY, DH128 = (lambda c: True), (lambda c: c.dh == 128)
FWD_LINES = {"fwd32w4": ("fwd64=0,fwd_waves=4", ANY), "fwd32w8": ("fwd64=0,fwd_waves=8", ANY), "fwd64": ("fwd64=1", DH128), "fwd64p": ("fwd64=1p", DH128)}
DQ_LINES = {"dq32": ("dq64=0", ANY), "dq64": ("dq64=1", DH128)}
_STATS = {"what": "tests/test_attn_gpu.py: worst error in ulps of the reference's scale (tests/attn_ref.py; bf16 ulps for O, dQ, dK, dV, fp32 ulps "
                  "for lse2, dsum, part), per output kind and per dispatch line (bit-equal outputs of select data are asserted, not listed); "
                  "wall_s: seconds spent inside this file's tests, the shared references included (tests_run of them; launches: accepted launches, each verified whole)",
          "bars": dict(A.BARS), "worst_ulps_per_output_kind": {}, "worst": {}, "wall_s": 0.0}


def _L():
    from qflux_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def tune(spec):
    assert _L().lib.qfx_attn_tune(spec.encode()) == 0


@pytest.fixture(autouse=True)
def _restore_attn_policy():
    """qfx_attn_tune is process-wide: back to the shape-driven choice after each test; the time spent in the file's tests so far goes to the table."""
    t0 = time.time()
    yield
    tune("fwd64=auto,dq64=auto,fwd_waves=0")
    _STATS["wall_s"] = round(_STATS["wall_s"] + time.time() - t0, 2)
    _STATS["tests_run"] = _STATS.get("tests_run", 0) + 1
    _observe(None, None, dump=("attn_parity.json", _STATS))


def record_worst(line, key, case, err):
    kinds = _STATS["worst_ulps_per_output_kind"]
    kinds[key] = max(kinds.get(key, 0.0), err)
    slot = _STATS["worst"].setdefault(line, {})
    if key not in slot or err >= slot[key]["ulps"]:
        slot[key] = dict(ulps=err, bar=A.BARS[key], case=repr(case))


@functools.lru_cache(maxsize=None)
def _case(case):
    """(inputs, forward reference, backward reference of the reference's q(O) and fp32 lse2, those two): once per case, never modified."""
    inp = A.make_inputs(case)
    return (inp,) + A.reference(inp, case)


# ---------------------------------------------------------------------------------------------- buffers
def _put(t, ld, off=0, dtype=BF):
    """Device copy of t [rows, n] inside a NaN-filled buffer of row stride ld at column `off`, 16384 more NaN elements behind it.
    Returns (keep-alive, pointer of element [0, 0])."""
    rows, n = t.shape
    assert ld >= off + n
    flat = (A.canary_bf16 if dtype == BF else A.canary_f32)(rows * ld + 16384, device=DEV)
    flat[:rows * ld].view(rows, ld)[:, off:off + n] = t.to(dtype).to(DEV)
    return flat, flat.data_ptr() + off * flat.element_size()


class Out:
    """A canary-filled output [rows + 3, ld] (bf16) whose kernel-owned part is [:rows, :n]."""
    def __init__(self, rows, n, ld, dtype=BF, extra=3):
        self.rows, self.n, self.ld, self.buf_rows, self.dtype = rows, n, ld, rows + extra, dtype
        self.buf = (A.canary_bf16 if dtype == BF else A.canary_f32)(self.buf_rows * ld, device=DEV)

    def host(self):
        return self.buf.cpu().view(self.buf_rows, self.ld)

    def untouched(self):
        return bool((A.bits(self.buf) == (A.CANARY_BF16 if self.dtype == BF else A.CANARY_F32)).all())


class Built:
    pass


def _stat_in(val, case):
    """A [B, H, S] fp32 statistic as the backward reads it: [B H + 1, S_pad] with NaN in the pad columns and the extra slab."""
    o = Out(case.B * case.H, case.S, case.S_pad, F32, extra=1)
    o.buf.view(o.buf_rows, o.ld)[:o.rows, :o.n] = val.reshape(o.rows, case.S).float().to(DEV)
    return o


def build(case, entry, O_in=None, lse_in=None, dsum_in=None):
    """qfx_attn_args of a case for one entry point ("fwd", "prep", "dq", "dkv", "onepass") with every buffer behind it."""
    L = _L()
    inp, _, _, O_ref, lse_ref = _case(case)
    O_in = O_ref if O_in is None else O_in
    lse_in = lse_ref if lse_in is None else lse_in
    B, S, H, dh, D = case.B, case.S, case.H, case.dh, case.D
    rows = B * S
    b = Built()
    b.case, b.entry, b.keep, b.outs, b.parts = case, entry, [], {}, {}
    a = L.AttnArgs()
    a.B, a.S, a.S_pad, a.H, a.dh, a.scale = B, S, case.S_pad, H, dh, case.scale
    flat = lambda n: inp[n].reshape(rows, D)       # noqa: E731
    if case.slice_:
        ld = 3 * D + 24
        keep, ptr = _put(torch.cat([flat("q"), flat("k"), flat("v")], 1), ld, 8)
        b.keep.append(keep)
        a.Q, a.K, a.V, a.ldq, a.ldk, a.ldv = ptr, ptr + 2 * D, ptr + 4 * D, ld, ld, ld
    else:
        for n, fld, ldf, ld, off in (("q", "Q", "ldq", D + 8, 0), ("k", "K", "ldk", D + 16, 8), ("v", "V", "ldv", D + 24, 16)):
            keep, ptr = _put(flat(n), ld, off)
            b.keep.append(keep)
            setattr(a, fld, ptr)
            setattr(a, ldf, ld)
    if inp["mask"] is not None:
        b.keep.append(inp["mask"].to(DEV).contiguous())
        a.key_mask = b.keep[-1].data_ptr()
    a.T = case.T
    wide = (D + 4,) * 4 if case.narrow else (D + 8, D + 8, D + 16, D + 24)

    def out(name, fld, ldf, ld):
        b.outs[name] = Out(rows, D, ld)
        setattr(a, fld, b.outs[name].buf.data_ptr())
        setattr(a, ldf, ld)

    def stat_out(name, fld):
        b.outs[name] = Out(B * H, S, case.S_pad, F32, extra=1)
        setattr(a, fld, b.outs[name].buf.data_ptr())

    def slot(i):
        if not case.R or i not in case.slots:
            return
        ldp = case.ld_part
        o = Out(H * (rows + 3), ldp, ldp, F32, extra=0)
        b.parts[i] = o
        hl = a.hl[i]
        hl.part, hl.part_hstride, hl.ld_part, hl.c0, hl.R = o.buf.data_ptr(), (rows + 3) * ldp, ldp, case.c0, case.R
        for s, (hi, lo) in enumerate(inp["W"][i]):
            if (s == 0 and case.no_img) or (s == 1 and case.no_txt):
                continue
            b.keep.append(L.head_fragment_image(hi.to(DEV), lo.to(DEV), dh))
            hl.w_pk[s] = b.keep[-1].data_ptr()

    if entry == "fwd":
        out("O", "O", "ldo", wide[0])
        stat_out("lse2", "lse2")
        slot(0)
    else:
        keep, a.O = _put(O_in.reshape(rows, D), D + 16)
        b.keep.append(keep)
        a.ldo = D + 16
        keep, a.dO = _put(flat("dO"), D + 8, 8)
        b.keep.append(keep)
        a.lddo = D + 8
        if entry != "prep":
            b.lse_in = _stat_in(lse_in, case)
            a.lse2 = b.lse_in.buf.data_ptr()
        if entry == "dkv":
            b.dsum_in = _stat_in(dsum_in, case)
            a.dsum = b.dsum_in.buf.data_ptr()
        else:
            stat_out("dsum", "dsum")
        if entry in ("dq", "onepass"):
            out("dQ", "dQ", "lddq", wide[1])
        if entry in ("dkv", "onepass"):
            out("dK", "dK", "lddk", wide[2])
            out("dV", "dV", "lddv", wide[3])
        if case.fused and entry != "prep":
            lds = 2 * D + (4 if case.narrow else 8)
            keep, a.qk_saved = _put(inp["saved"].reshape(rows, 2 * D), lds)
            b.keep.append(keep)
            a.ld_saved = lds
            b.keep.append(torch.cat([inp["rope"].flatten(), torch.full((64,), float("nan"))]).to(DEV))
            a.rope, a.rope_bstride = b.keep[-1].data_ptr(), (S * dh if case.rope_b else 0)
            for fld, w in zip(("wq_txt", "wk_txt", "wq_img", "wk_img"), inp["ws"]):
                b.keep.append(w.to(DEV).contiguous())
                setattr(a, fld, b.keep[-1].data_ptr())
            a.norm_flags, a.norm_eps = case.flags, A.NORM_EPS
            for i in {"dq": (1,), "dkv": (2, 3), "onepass": (1, 2, 3)}[entry]:
                slot(i)
        if entry == "onepass":
            nb1, nb2 = C.c_int64(-1), C.c_int64(-1)
            assert L.lib.qfx_attn_bwd_fused_workspace(C.byref(a), C.byref(nb1), C.byref(nb2)) == 0 and nb1.value > 0 and nb2.value > 0
            assert nb1.value == B * H * ((S + 63) // 64) * 64 * 128 * 4 and nb2.value == B * H * ((S + 63) // 64) * 4
            b.acc = A.canary_f32(nb1.value // 4, device=DEV)              # garbage: the first key block of every tile overwrites
            b.turn = torch.zeros(nb2.value // 4, dtype=torch.int32, device=DEV)
            a.dq_acc, a.dq_turn = b.acc.data_ptr(), b.turn.data_ptr()
    b.a = a
    return b


ENTRY_FN = {"fwd": "qfx_attn_fwd", "prep": "qfx_attn_bwd_prep", "dq": "qfx_attn_bwd_dq", "dkv": "qfx_attn_bwd_dkv", "onepass": "qfx_attn_bwd_fused"}


def launch(b, a=None):
    return getattr(_L().lib, ENTRY_FN[b.entry])(C.byref(b.a if a is None else a), _stream())


def untouched(b):
    return all(o.untouched() for o in list(b.outs.values()) + list(b.parts.values()))


# ---------------------------------------------------------------------------------------------- verification
def _check_bf16(b, name, key, ref, line, mode):
    """mode: "bar" | "bits" | "zero".  Returns the [B, S, H, dh] bf16 tensor the kernel stored."""
    case, o = b.case, b.outs[name]
    val, scale = ref
    got = o.host()
    outside = torch.ones(o.buf_rows, o.ld, dtype=torch.bool)
    outside[:o.rows, :o.n] = False
    assert bool((A.bits(got)[outside] == A.CANARY_BF16).all()), f"{line} {case}: {name} written outside its rows / columns"
    inner = got[:o.rows, :o.n].reshape(case.B, case.S, case.H, case.dh)
    if mode == "bits":
        # bf16 values on both sides, so equal values are equal bits -- up to the sign of a zero that is a SUM (a key no query selects,
        # selectors that cancel), which has no agreed sign
        bad = inner.double() != val
        assert not bad.any(), f"{line} {case}: {name} not bit-equal at {int(bad.sum())} elements, max |d| = {(inner.double() - val).abs().max().item()}"
    elif mode == "zero":
        assert bool((inner.float() == 0).all()), f"{line} {case}: {name} is not +-0 on select data, max |.| = {inner.float().abs().max().item()}"
    else:
        e = A.err_ulps(inner, val, scale)
        record_worst(line, key, case, e)
        assert e <= A.BARS[key], f"{line} {key} {case}: {e:.3f} ulps of scale > {A.BARS[key]}"
    return inner


def _check_stat(b, name, ref, line, exact=False):
    case, o = b.case, b.outs[name]
    val, scale = ref
    got = o.host()
    outside = torch.ones(o.buf_rows, o.ld, dtype=torch.bool)
    outside[:o.rows, :o.n] = False
    assert bool((A.bits(got)[outside] == A.CANARY_F32).all()), f"{line} {case}: {name} written in its pad columns or past its slabs"
    inner = got[:o.rows, :o.n].reshape(case.B, case.H, case.S)
    if exact:
        assert bool((inner.double() == val).all()), f"{line} {case}: {name} not exact"
        return
    e = A.err_ulps32(inner, val, scale)
    record_worst(line, name, case, e)
    assert e <= A.BARS[name], f"{line} {name} {case}: {e:.3f} fp32 ulps of scale > {A.BARS[name]}"


def _check_part(b, slot, X, line):
    """part[slot] against the projection of the bf16 X the kernel stored; canary everywhere else."""
    if slot not in b.parts:
        return
    case, o = b.case, b.parts[slot]
    inp = _case(case)[0]
    rows = case.B * case.S
    got = o.host().view(case.H, rows + 3, case.ld_part)
    live = A.part_rows(case, slot)
    own = torch.zeros(case.H, rows + 3, case.ld_part, dtype=torch.bool)
    own[:, :rows][:, live, case.c0:case.c0 + case.R] = True
    assert bool((A.bits(got)[~own] == A.CANARY_F32).all()), f"{line} {case}: part[{slot}] written outside its rows / columns"
    val, scale = A.part_ref(X, inp, case, slot)
    inner = got[:, :rows][:, live, case.c0:case.c0 + case.R]
    e = A.err_ulps32(inner, val[:, live], scale[:, live])
    if case.kind == "select":
        assert e == 0.0, f"{line} {case}: part[{slot}] of exact data is not exact ({e} ulps)"
        return
    record_worst(line, "part", case, e)
    assert e <= A.BARS["part"], f"{line} part[{slot}] {case}: {e:.3f} fp32 ulps of scale > {A.BARS['part']}"


def verify(b, line, bwd=None):
    case = b.case
    _, fwd, bwd_ref, _, _ = _case(case)
    bwd = bwd_ref if bwd is None else bwd
    sel = case.kind == "select"
    if b.entry == "fwd":
        X = _check_bf16(b, "O", "O", fwd["O"], line, "bits" if sel else "bar")
        _check_stat(b, "lse2", fwd["lse2"], line)
        _check_part(b, 0, X, line)
        return
    if "dsum" in b.outs:
        _check_stat(b, "dsum", bwd["dsum"], line, exact=sel)
    fz = ".fused" if case.fused else ""
    if "dQ" in b.outs:
        _check_part(b, 1, _check_bf16(b, "dQ", "dQ" + fz, bwd["dQ"], line, "zero" if sel else "bar"), line)
    if "dK" in b.outs:
        _check_part(b, 2, _check_bf16(b, "dK", "dK" + fz, bwd["dK"], line, "zero" if sel else "bar"), line)
        _check_part(b, 3, _check_bf16(b, "dV", "dV", bwd["dV"], line, "bits" if sel else "bar"), line)
    if b.entry == "onepass":
        assert int(b.turn.abs().max()) == 0, f"{line} {case}: turn counters not back at zero"


def run(case, entry, line, **kw):
    b = build(case, entry, **kw)
    assert launch(b) == 0, (line, case)
    torch.cuda.synchronize()
    _STATS["launches"] = _STATS.get("launches", 0) + 1
    return b


# ---------------------------------------------------------------------------------------------- the dispatch lines
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("line", list(FWD_LINES))
def test_forward(line, kind):
    spec, ok = FWD_LINES[line]
    tune(spec)
    n = 0
    for case in A.ALL_FAMILIES[kind]:
        if ok(case):
            verify(run(case, "fwd", line), line)
            n += 1
    assert n >= 5


@pytest.mark.parametrize("kind", KINDS)
def test_prep(kind):
    for case in A.ALL_FAMILIES[kind]:
        verify(run(case, "prep", "prep"), "prep")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("line", list(DQ_LINES))
def test_backward_dq(line, kind):
    spec, ok = DQ_LINES[line]
    tune(spec)
    n = 0
    for case in A.ALL_FAMILIES[kind]:
        if ok(case):
            verify(run(case, "dq", line), line)
            n += 1
    assert n >= 5


@pytest.mark.parametrize("kind", KINDS)
def test_backward_dkv(kind):
    for case in A.ALL_FAMILIES[kind]:
        dsum = _case(case)[2]["dsum"][0].float()
        verify(run(case, "dkv", "dkv", dsum_in=dsum), "dkv")


@pytest.mark.parametrize("kind", KINDS)
def test_backward_onepass(kind):
    n = 0
    for case in A.ALL_FAMILIES[kind]:
        if case.onepass():
            verify(run(case, "onepass", "onepass"), "onepass")
            n += 1
    assert n >= 4


CHAIN_CASE = next(c for c in A.RAND_CASES if c.onepass() and c.fused and c.R and c.S >= 129)


@pytest.mark.parametrize("family", ["dq32+dkv", "dq64+dkv", "onepass"])
def test_backward_chained_to_the_forward_kernel(family):
    """The forward kernel's OWN O and lse2 go into the backward; the yardstick is the reference of those inputs."""
    case = CHAIN_CASE
    inp = _case(case)[0]
    f = run(case, "fwd", "chain")
    O_k = f.outs["O"].host()[:f.outs["O"].rows, :case.D].reshape(case.B, case.S, case.H, case.dh).clone()
    lse_k = f.outs["lse2"].host()[:case.B * case.H, :case.S].reshape(case.B, case.H, case.S).clone()
    ref = A.attn_bwd_ref(inp, case, O_k, lse_k)
    line = "chain_" + family
    if family == "onepass":
        verify(run(case, "onepass", line, O_in=O_k, lse_in=lse_k), line, bwd=ref)
        return
    tune("dq64=0" if family.startswith("dq32") else "dq64=1")
    verify(run(case, "dq", line, O_in=O_k, lse_in=lse_k), line, bwd=ref)
    verify(run(case, "dkv", line, O_in=O_k, lse_in=lse_k, dsum_in=ref["dsum"][0].float()), line, bwd=ref)


# ---------------------------------------------------------------------------------------------- refusals
def _mutated(b, fields):
    L = _L()
    a = L.AttnArgs.from_buffer_copy(b.a)
    for k, v in fields.items():
        if k.startswith("hl"):
            i, f = int(k[2]), k[4:]
            if f.startswith("w_pk"):
                a.hl[i].w_pk[int(f[4])] = v
            else:
                setattr(a.hl[i], f, v)
        else:
            setattr(a, k, v)
    return a


def _table(b, muts):
    for fields, rc in muts:
        a = _mutated(b, fields)
        assert launch(b, a) == rc, (b.entry, fields)
        torch.cuda.synchronize()
        assert untouched(b), f"{b.entry} {fields}: refused, yet an output was written"
    assert getattr(_L().lib, ENTRY_FN[b.entry])(None, _stream()) == EINVAL


REF_CASE = A.Case(65, H=2, B=2, dh=128, fused=True, T=16, R=16, c0=4)


def _common(a):
    """The arms of check_common: argument values only, nothing is allocated for them."""
    return [(dict(B=0), EINVAL), (dict(B=-1), EINVAL), (dict(S=0), EINVAL), (dict(S=-5), EINVAL), (dict(H=0), EINVAL), (dict(H=-1), EINVAL),
            (dict(S_pad=a.S_pad + 32), EINVAL), (dict(S_pad=a.S_pad - 64), EINVAL), (dict(dh=96), EUNSUPPORTED), (dict(dh=0), EUNSUPPORTED),
            (dict(ldq=1 << 24), EUNSUPPORTED), (dict(ldk=1 << 24), EUNSUPPORTED), (dict(ldv=1 << 24), EUNSUPPORTED), (dict(lddo=1 << 24), EUNSUPPORTED),
            (dict(ldk=-8), EUNSUPPORTED), (dict(S=600, S_pad=640, ldv=1 << 23), EUNSUPPORTED), (dict(S=1 << 24, S_pad=1 << 24), EUNSUPPORTED)]


def _head_lora(b, i):
    hl = b.a.hl[i]
    p = f"hl{i}."
    return [({p + "R": 8}, EUNSUPPORTED), ({p + "R": 48}, EUNSUPPORTED), (dict(T=8), EINVAL), (dict(T=-16), EINVAL), ({p + "ld_part": hl.ld_part + 2}, EINVAL),
            ({p + "c0": 2}, EINVAL), ({p + "c0": -4}, EINVAL), ({p + "c0": 8}, EINVAL), ({p + "part": hl.part + 4}, EINVAL),
            ({p + "part_hstride": b.case.B * b.case.S * hl.ld_part - 1}, EINVAL), ({p + "w_pk0": hl.w_pk[0] + 8}, EINVAL), ({p + "w_pk1": hl.w_pk[1] + 2}, EINVAL)]


def test_refusals_forward():
    b = build(REF_CASE, "fwd")
    a = b.a
    own = [(dict(Q=None), EINVAL), (dict(K=None), EINVAL), (dict(V=None), EINVAL), (dict(O=None), EINVAL), (dict(lse2=None), EINVAL),
           (dict(ldq=a.ldq + 4), EINVAL), (dict(ldk=a.ldk + 4), EINVAL), (dict(ldv=a.ldv + 4), EINVAL), (dict(ldo=a.ldo + 2), EINVAL)]
    for spec in ("fwd64=0", "fwd64=1", "fwd64=1p"):
        tune(spec)
        _table(b, _common(a) + own + _head_lora(b, 0))
    # ... and the accepted launch right after them is still right
    assert launch(b) == 0
    torch.cuda.synchronize()
    verify(b, "fwd64p")


def test_refusals_prep():
    b = build(REF_CASE, "prep")
    a = b.a
    _table(b, _common(a) + [(dict(O=None), EINVAL), (dict(dO=None), EINVAL), (dict(dsum=None), EINVAL), (dict(ldo=a.ldo + 4), EINVAL),
                            (dict(lddo=a.lddo + 4), EINVAL)])
    assert launch(b) == 0
    torch.cuda.synchronize()
    verify(b, "prep")


def _saved_arms(a, which):
    arms = [(dict(rope=None), EINVAL), (dict(ld_saved=a.ld_saved + 2), EINVAL), (dict(T=-16), EINVAL)]
    return arms + [({f"w{x}_{s}": None}, EINVAL) for x in which for s in ("txt", "img")]


def test_refusals_backward_dq():
    b = build(REF_CASE, "dq")
    a = b.a
    own = [({k: None}, EINVAL) for k in ("Q", "K", "V", "O", "dO", "lse2", "dsum", "dQ")]
    own += [({k: getattr(a, k) + 4}, EINVAL) for k in ("ldq", "ldk", "ldv", "ldo", "lddo")] + [(dict(lddq=a.lddq + 2), EINVAL)]
    no_saved = [(dict(qk_saved=None), EINVAL)]                      # a backward slot projects d(PRE-norm q): it needs qk_saved
    for spec in ("dq64=0", "dq64=1"):
        tune(spec)
        _table(b, _common(a) + own + _saved_arms(a, "q") + _head_lora(b, 1) + no_saved)
    assert launch(b) == 0
    torch.cuda.synchronize()
    verify(b, "dq64")


def test_refusals_backward_dkv():
    b = build(REF_CASE, "dkv", dsum_in=_case(REF_CASE)[2]["dsum"][0].float())
    a = b.a
    own = [({k: None}, EINVAL) for k in ("Q", "K", "V", "dO", "lse2", "dsum", "dK", "dV")]
    own += [({k: getattr(a, k) + 4}, EINVAL) for k in ("ldq", "ldk", "ldv", "lddo")] + [(dict(lddk=a.lddk + 2), EINVAL), (dict(lddv=a.lddv + 2), EINVAL)]
    _table(b, _common(a) + own + _saved_arms(a, "k") + _head_lora(b, 2) + _head_lora(b, 3) + [(dict(qk_saved=None), EINVAL)])
    assert launch(b) == 0
    torch.cuda.synchronize()
    verify(b, "dkv")


def test_refusals_backward_onepass_and_its_workspace():
    L = _L()
    b = build(REF_CASE, "onepass")
    a = b.a
    own = [({k: None}, EINVAL) for k in ("Q", "K", "V", "O", "dO", "lse2", "dsum", "dQ", "dK", "dV", "dq_acc", "dq_turn")]
    own += [({k: getattr(a, k) + 4}, EINVAL) for k in ("ldq", "ldk", "ldv", "ldo", "lddo")]
    own += [({k: getattr(a, k) + 2}, EINVAL) for k in ("lddq", "lddk", "lddv")]
    own += [(dict(dh=64), EUNSUPPORTED), (dict(dq_acc=a.dq_acc + 4), EINVAL), (dict(dq_turn=a.dq_turn + 2), EINVAL), (dict(qk_saved=None), EINVAL)]
    _table(b, _common(a) + own + _saved_arms(a, "qk") + _head_lora(b, 1) + _head_lora(b, 2) + _head_lora(b, 3))
    assert int(b.turn.abs().max()) == 0
    # qfx_attn_bwd_fused_workspace: the arms of check_common, dh = 64 and S < 64 report sizes 0
    for fields, rc in _common(a) + [(dict(dh=64), EUNSUPPORTED), (dict(S=63, S_pad=64), EUNSUPPORTED)]:
        nb1, nb2 = C.c_int64(-1), C.c_int64(-1)
        assert L.lib.qfx_attn_bwd_fused_workspace(C.byref(_mutated(b, fields)), C.byref(nb1), C.byref(nb2)) == rc, fields
        assert nb1.value == 0 and nb2.value == 0, fields
    assert launch(b) == 0
    torch.cuda.synchronize()
    verify(b, "onepass")
