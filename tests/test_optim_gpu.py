"""GPU: csrc/qfx_optim.hip through the C ABI against tests/optim_ref.py -- qfx_sumsq, qfx_sumsq_det, qfx_adamw_step(_grouped),
qfx_sgd_step(_grouped), qfx_prodigy_step, the clip prologue and every refusal of include/qfx.h.

One re-synchronised step per comparison.  Every buffer is over-allocated with a canary before and after it, at a 16-byte boundary
(shift 0) or one element past it (shift 1: the grouped kernels' scalar form); after each launch the canaries hold, g / p0 / gnorm_sq
keep their bits and zero slots stay +0.  AdamW and SGD must give the BITS of the fp32 restatement wherever the clip coefficient is
pinned (optim_ref's docstring), and stay within optim_ref.BARS of the fp64 restatement with grad_scale = 1/3; Prodigy's element states
within BARS, its double scalars to 1e-12 on `select` data, d_denom and the two norms within their derived bounds, exactly on `select`
data.  Worst errors, launch count and time are dumped as optim_parity_gpu.json by parity_util._observe (kept in profiles/optim_parity.json)."""
import ctypes as C
import itertools
import math
import time

import numpy as np
import pytest
import torch

import optim_ref as R
from parity_util import _observe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
EINVAL, EUNSUPPORTED = -1, -2
CANARY, GUARD = 0x5A5AA5A5, 64
N, SEED = 1027, 3
_STATS = {"what": "tests/test_optim_gpu.py: worst error per line and output in fp32 ulps of the reference's scale against its bar "
                  "(bit-equal comparisons are asserted, counted in exact_launches); sums: worst error over its derived bound; wall_s: the "
                  "host's seconds inside this file's tests, building the CPU references included",
          "bars_ulps": R.BARS, "worst_ulps": {}, "worst_sum_err_over_bound": {}, "launches": 0, "exact_launches": 0, "wall_s": 0.0}


def _L():
    from qflux_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(autouse=True)
def _record():
    t0 = time.time()
    yield
    _STATS["wall_s"] = round(_STATS["wall_s"] + time.time() - t0, 2)
    _observe(None, None, dump=("optim_parity_gpu.json", _STATS))


class Buf:
    """A device buffer between two canaries; `shift` elements past a 16-byte boundary."""

    def __init__(self, host, shift=0, dtype=F32):
        host = np.ascontiguousarray(np.asarray(host, dtype))
        self.w = host.itemsize // 4
        self.n, self.lo = host.size * self.w, GUARD + shift * self.w
        raw = np.full(self.lo + self.n + GUARD, CANARY, np.uint32)
        raw[self.lo:self.lo + self.n] = host.view(np.uint32)
        self.before, self.dtype = raw, dtype
        self.t = torch.from_numpy(raw.view(np.int32).copy()).to(DEV)
        self.ptr = self.t.data_ptr() + 4 * self.lo
        assert (self.ptr % 16 == 0) == (shift == 0) or self.w == 2

    def raw(self):
        r = self.t.cpu().numpy().view(np.uint32)
        assert (r[:self.lo] == CANARY).all() and (r[self.lo + self.n:] == CANARY).all(), "canary overwritten"
        return r

    def get(self):
        return self.raw()[self.lo:self.lo + self.n].view(self.dtype).copy()

    def unchanged(self):
        assert np.array_equal(self.raw(), self.before)
        return True


def _ptr(b):
    return None if b is None else b.ptr


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def record(line, key, err):
    w = _STATS["worst_ulps"].setdefault(line, {})
    w[key] = max(w.get(key, 0.0), err)


def judge(line, got, ref64, want32, exact, where):
    """got / want32: {output: fp32 array}; ref64: {output: (value, scale)}."""
    for k, x in got.items():
        if exact:
            assert same_bits(x, want32[k]), (where, k, R.err_ulps(x, *ref64[k]), int((x.view(np.uint32) != want32[k].view(np.uint32)).sum()))
        else:
            e = R.err_ulps(x, *ref64[k])
            record(line, k, e)
            assert e <= R.BARS[line][k], (where, k, e, R.BARS[line][k])
    _STATS["exact_launches"] += int(bool(exact))


def pads_stay_zero(n, got, where):
    for a, b in R.pad_slots(n):
        for k, x in got.items():
            assert not x[a:b].view(np.uint32).any(), (where, k)       # +0, not -0


def tile_map(n, pattern):
    return np.array([pattern(t) for t in range((n + 63) // 64)], np.uint8)


# ---------------------------------------------------------------- AdamW
def launch_adamw(d, rows, clipargs, shift=0, tg=None, n_groups=None):
    """rows: [adamw_args]; tg None: qfx_adamw_step with rows[0], else qfx_adamw_step_grouped with that tile map."""
    L = _L()
    n = d["p"].size
    B = {k: Buf(d[k], shift) for k in "pgmv"}
    gsq, mx, gs = clipargs
    gn = None if gsq is None else Buf([gsq])
    if tg is None:
        a = rows[0]
        rc = L.lib.qfx_adamw_step(B["p"].ptr, B["g"].ptr, B["m"].ptr, B["v"].ptr, n, a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], a["bc1"],
                                  a["bc2"], _ptr(gn), mx, gs, _stream())
    else:
        tgb = Buf(np.frombuffer(np.pad(tg, (0, -len(tg) % 4)).tobytes(), np.uint32), 0, np.uint32)
        arr = (L.AdamwGroup * len(rows))(*[L.AdamwGroup(a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], a["bc1"], a["bc2"]) for a in rows])
        rc = L.lib.qfx_adamw_step_grouped(B["p"].ptr, B["g"].ptr, B["m"].ptr, B["v"].ptr, n, tgb.ptr, arr, n_groups or len(rows), _ptr(gn), mx, gs,
                                          _stream())
    torch.cuda.synchronize()
    assert rc == 0
    _STATS["launches"] += 1
    assert B["g"].unchanged() and (gn is None or gn.unchanged()) and (tg is None or tgb.unchanged())
    return {k: B[k].get() for k in "pmv"}


def adamw_refs(d, rows, clipname, groups=None):
    """fp64 and fp32 restatement; groups: per-element row index (None: row 0)."""
    c64, forms, exact, cargs = R.clips_of(clipname, d["g"])
    r64 = [R.adamw_f64(d["p"], d["g"], d["m"], d["v"], c64, **a) for a in rows]
    r32 = [dict(zip("pmv", R.adamw_f32(d["p"], d["g"], d["m"], d["v"], forms[0], **a))) for a in rows]
    if groups is None:
        return r64[0], r32[0], exact, cargs
    sel = lambda xs: sum(np.where(groups == i, x, 0) for i, x in enumerate(xs))      # noqa: E731
    ref64 = {k: (sel([r[k][0] for r in r64]), sel([r[k][1] for r in r64])) for k in "pmv"}
    want = {k: np.select([groups == i for i in range(len(rows))], [r[k] for r in r32]).astype(F32) for k in "pmv"}
    return ref64, want, exact, cargs


def adamw_case(n, hn, cn, t, seed=SEED, shifts=(0, 1)):
    d = R.case_data(n, seed, hn)
    rows = [R.adamw_args(R.ADAMW_HP[hn], t)]
    ref64, want, exact, cargs = adamw_refs(d, rows, cn)
    outs = []
    for shift, grouped in itertools.product(shifts, (False, True)):
        got = launch_adamw(d, rows, cargs, shift, tile_map(n, lambda t_: 0) if grouped else None)
        judge("adamw", got, ref64, want, exact, (n, hn, cn, t, shift, grouped))
        if hn != "eps0":
            pads_stay_zero(n, got, (n, hn, cn, t))
        outs.append(got)
    for o in outs[1:]:           # grouped == ungrouped, scalar form == 16-byte form: the same bits, pinned clip or not
        assert all(same_bits(o[k], outs[0][k]) for k in "pmv"), (n, hn, cn, t)


def test_adamw_every_hyperparameter_set_clip_and_step():
    for hn, cn, t in itertools.product(R.ADAMW_HP, R.CLIPS, R.STEPS):
        adamw_case(N, hn, cn, t)


@pytest.mark.parametrize("n", [1, 3, 255, 257])
def test_adamw_short_lengths(n):
    hs, cs = list(R.ADAMW_HP), list(R.CLIPS)
    for i in range(6):
        adamw_case(n, hs[(i + n) % len(hs)], cs[i], R.STEPS[i % 3], seed=n + i)


def test_adamw_second_grid_stride_trip():
    adamw_case(R.N_STEP_TRIP2, "default", "clip_gs_half", 2, shifts=(0,))


def _loraplus_groups(n):
    tg = tile_map(n, lambda t: (t // 3) % 2)
    return tg, np.repeat(tg, 64)[:n].astype(np.int64)


@pytest.mark.parametrize("n", [N, R.N_GROUPED_VEC_TRIP2])
def test_adamw_loraplus_groups(n):
    d = R.case_data(n, 5)
    rows = [R.adamw_args(hp, 2) for hp in R.ADAMW_LORAPLUS]
    tg, groups = _loraplus_groups(n)
    for cn in (("clip_gs_half", "clip_gs_third", "null_norm") if n == N else ("clip_gs_half",)):
        ref64, want, exact, cargs = adamw_refs(d, rows, cn, groups)
        outs = [launch_adamw(d, rows, cargs, shift, tg) for shift in (0, 1)]
        judge("adamw", outs[0], ref64, want, exact, (n, cn))
        assert all(same_bits(outs[1][k], outs[0][k]) for k in "pmv")
        pads_stay_zero(n, outs[0], (n, cn))


def test_adamw_map_entries_past_n_groups_take_the_last_row():
    """include/qfx.h: an entry >= n_groups steps its tile with groups[n_groups - 1] -- 2 and 255 with n_groups = 2, in the 16-byte and
    the scalar form, in the body and in the n % 4 tail's tile."""
    d = R.case_data(N, 6)
    rows = [R.adamw_args(hp, 2) for hp in R.ADAMW_LORAPLUS]
    tg, groups = _loraplus_groups(N)
    bad = tg.copy()
    ones = np.flatnonzero(tg == 1)
    bad[ones[0]], bad[ones[1]], bad[-1], tg[-1] = 2, 255, 255, 1
    groups = np.repeat(tg, 64)[:N].astype(np.int64)
    ref64, want, exact, cargs = adamw_refs(d, rows, "clip_gs_half", groups)
    for shift in (0, 1):
        got = launch_adamw(d, rows, cargs, shift, bad)
        judge("adamw", got, ref64, want, exact, ("out of range", shift))


# ---------------------------------------------------------------- SGD
def launch_sgd(d, rows, first, clipargs, shift=0, tg=None, buf="data"):
    """buf: "data", "nan" (a first step must not read it) or None (NULL)."""
    L = _L()
    n = d["p"].size
    B = {k: Buf(d[k], shift) for k in "pg"}
    bhost = None if buf is None else (d["buf"] if buf == "data" else np.full(n, np.nan, F32))
    bb = None if bhost is None else Buf(bhost, shift)
    gsq, mx, gs = clipargs
    gn = None if gsq is None else Buf([gsq])
    if tg is None:
        a = rows[0]
        rc = L.lib.qfx_sgd_step(B["p"].ptr, B["g"].ptr, _ptr(bb), n, a["lr"], a["mom"], a["damp"], a["wd"], a["nesterov"], first, _ptr(gn), mx, gs,
                                _stream())
    else:
        tgb = Buf(np.frombuffer(np.pad(tg, (0, -len(tg) % 4)).tobytes(), np.uint32), 0, np.uint32)
        arr = (L.SgdGroup * len(rows))(*[L.SgdGroup(a["lr"], a["mom"], a["damp"], a["wd"], a["nesterov"]) for a in rows])
        rc = L.lib.qfx_sgd_step_grouped(B["p"].ptr, B["g"].ptr, _ptr(bb), n, tgb.ptr, arr, len(rows), first, _ptr(gn), mx, gs, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    _STATS["launches"] += 1
    assert B["g"].unchanged() and (gn is None or gn.unchanged()) and (tg is None or tgb.unchanged())
    out = {"p": B["p"].get()}
    if bb is not None:
        out["buf"] = bb.get()
    return out, (None if bhost is None else np.asarray(bhost, F32))


def sgd_case(n, hn, cn, first, seed=SEED, shifts=(0, 1)):
    d = R.case_data(n, seed)
    a = R.sgd_args(R.SGD_HP[hn])
    c64, forms, exact, cargs = R.clips_of(cn, d["g"])
    ref64 = R.sgd_f64(d["p"], d["g"], d["buf"], c64, first=first, **a)
    pn, bn = R.sgd_f32(d["p"], d["g"], d["buf"], forms[0], first=first, **a)
    want = {"p": pn} if bn is None else {"p": pn, "buf": bn}
    bufs = ["nan" if first else "data"] + ([None] if a["mom"] == 0 else [])
    outs = []
    for shift, grouped, buf in itertools.product(shifts, (False, True), bufs):
        got, b0 = launch_sgd(d, [a], first, cargs, shift, tile_map(n, lambda t_: 0) if grouped else None, buf)
        if a["mom"] == 0:
            assert b0 is None or same_bits(got.pop("buf"), b0), "momentum 0: buf neither read nor written"
        judge("sgd", got, ref64, want, exact, (n, hn, cn, first, shift, grouped, buf))
        pads_stay_zero(n, got, (n, hn, cn, first))
        outs.append(got)
    for o in outs[1:]:
        assert all(same_bits(o[k], outs[0][k]) for k in o), (n, hn, cn, first)


def test_sgd_every_hyperparameter_set_clip_and_first():
    for hn, cn, first in itertools.product(R.SGD_HP, R.CLIPS, (0, 1)):
        sgd_case(N, hn, cn, first)


@pytest.mark.parametrize("n", [1, 3, 255, 257])
def test_sgd_short_lengths(n):
    hs, cs = list(R.SGD_HP), list(R.CLIPS)
    for i in range(6):
        sgd_case(n, hs[(i + n) % len(hs)], cs[i], i % 2, seed=n + i)


def test_sgd_second_grid_stride_trip():
    sgd_case(R.N_STEP_TRIP2, "nesterov", "clip_gs_half", 0, shifts=(0,))


@pytest.mark.parametrize("n", [N, R.N_GROUPED_VEC_TRIP2])
def test_sgd_groups_with_a_zero_momentum_group_and_out_of_range_entries(n):
    d = R.case_data(n, 7)
    rows = [R.sgd_args(hp) for hp in R.SGD_LORAPLUS]
    tg, groups = _loraplus_groups(n)
    c64, forms, exact, cargs = R.clips_of("clip_gs_half", d["g"])
    for first in ((0, 1) if n == N else (0,)):
        r32 = [R.sgd_f32(d["p"], d["g"], d["buf"], forms[0], first=first, **a) for a in rows]
        want_p = np.where(groups == 0, r32[0][0], r32[1][0])
        outs = []
        for shift, tmap in itertools.product((0, 1), ("good", "bad")):
            m = tg.copy()
            if tmap == "bad":
                ones = np.flatnonzero(tg == 1)
                m[ones[0]], m[ones[-1]] = 2, 255
            got, b0 = launch_sgd(d, rows, first, cargs, shift, m, "nan" if first else "data")
            assert same_bits(got["p"], want_p), (n, first, shift, tmap)
            assert same_bits(got["buf"][groups == 0], r32[0][1][groups == 0])
            assert same_bits(got["buf"][groups == 1], b0[groups == 1]), "a zero-momentum group's slice of buf is untouched"
            pads_stay_zero(n, {"p": got["p"]}, (n, first))
            _STATS["exact_launches"] += 1


# ---------------------------------------------------------------- the two sums
def _sum_check(name, got, ref, bound):
    err = abs(float(got) - ref)
    _STATS["worst_sum_err_over_bound"][name] = max(_STATS["worst_sum_err_over_bound"].get(name, 0.0), err / (bound * ref) if ref else 0.0)
    assert err <= bound * ref, (name, float(got), ref, err / ref, bound)


@pytest.mark.parametrize("n", R.LENGTHS_SMALL + [R.N_SUM_TRIP2])
def test_sumsq_adds_into_out(n):
    L = _L()
    for kind, shift, start in itertools.product(("rand", "select"), (0, 1), (0.0, 0.75)):
        g = (R.select_data(n) if kind == "select" else R.rand_data(n, 8, pad=False))["g"]
        gb, out = Buf(g, shift), Buf([start])
        assert L.lib.qfx_sumsq(gb.ptr, n, out.ptr, _stream()) == 0
        torch.cuda.synchronize()
        _STATS["launches"] += 1
        assert gb.unchanged()
        ref = R.sumsq_f64(g) + start
        if kind == "select":
            assert float(out.get()[0]) == ref, (n, shift, start)
        else:
            _sum_check("sumsq", out.get()[0], ref, R.sum_bound(R.sumsq_depth(n, False)))


@pytest.mark.parametrize("n", R.LENGTHS_SMALL + [R.N_SUM_TRIP2])
def test_sumsq_det_is_bounded_exact_on_select_data_and_deterministic(n):
    L = _L()
    for kind, nslots, shift in itertools.product(("rand", "select"), (1, 3, 1024), (0, 1)):
        g = (R.select_data(n) if kind == "select" else R.rand_data(n, 9, pad=False))["g"]
        blocks = R.flat_grid(n, nslots)
        res = []
        for _ in range(2):
            gb, out, part = Buf(g, shift), Buf([np.nan]), Buf(np.full(1024, np.nan, F32))
            assert L.lib.qfx_sumsq_det(gb.ptr, n, out.ptr, part.ptr, nslots, _stream()) == 0
            torch.cuda.synchronize()
            _STATS["launches"] += 1
            assert gb.unchanged()
            pt = part.get()
            assert np.isnan(pt[blocks:]).all() and np.isfinite(pt[:blocks]).all()      # slots past the launched blocks are not touched
            res.append((out.get(), pt))
        assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1])
        ref = R.sumsq_f64(g)
        if kind == "select":
            assert float(res[0][0][0]) == ref and float(res[0][1][:blocks].astype(F64).sum()) == ref
        else:
            _sum_check("sumsq_det", res[0][0][0], ref, R.sum_bound(R.sumsq_depth(n, True, nslots)))


# ---------------------------------------------------------------- Prodigy
ST_KEYS = ("d", "d_max", "num", "den", "d_hat", "k")


def launch_prodigy(d, st, h, clipargs, shift=0, expect=0, init=None):
    """init: the d0 (a double, as every caller holds it) that qfx_prodigy_init_state writes into a NaN-filled state; else st is uploaded."""
    L = _L()
    n = d["p"].size
    B = {k: Buf(d[k], shift) for k in ("p", "g", "m", "v", "s", "p0")}
    if init is None:
        sb = Buf(np.array([st[k] for k in ST_KEYS] + [0.0] * (L.PRODIGY_STATE - 6), F64), 0, F64)
    else:
        sb = Buf(np.full(L.PRODIGY_STATE, np.nan, F64), 0, F64)
        assert L.lib.qfx_prodigy_init_state(sb.ptr, init, _stream()) == 0
        w = sb.get()
        assert (w[[0, 1, 4]] == init).all() and not w[[2, 3, 5, 6, 7, 8, 9, 10, 11]].any() and [st[k] for k in ST_KEYS] == list(w[:6])
    gsq, mx, gs = clipargs
    gn = None if gsq is None else Buf([gsq])
    a = L.ProdigyArgs(B["p"].ptr, B["g"].ptr, B["m"].ptr, B["v"].ptr, B["s"].ptr, B["p0"].ptr, n, sb.ptr, h["lr"], h["b1"], h["b2"], h["beta3"],
                      h["eps"], h["wd"], h["d0"], h["d_coef"], h["growth"], h["use_bc"], h["safeguard"], 1, _ptr(gn), mx, gs)
    rc = L.lib.qfx_prodigy_step(C.byref(a), _stream())
    torch.cuda.synchronize()
    assert rc == expect
    _STATS["launches"] += 1
    assert B["g"].unchanged() and B["p0"].unchanged() and (gn is None or gn.unchanged())
    return {k: B[k].get() for k in "pmvs"}, dict(zip(ST_KEYS, sb.get()[:6])), B, sb


def prodigy_check(d, st, h, cn, shift, where, scalars_exact=False, init=None):
    c64, forms, exact, cargs = R.clips_of(cn, d["g"])
    got, gst, _, _ = launch_prodigy(d, st, h, cargs, shift, init=init)
    ema, acc_num, acc_den = R.prodigy_ema(d["p"], d["g"], d["m"], d["v"], d["s"], d["p0"], st, h, c64)
    n = d["p"].size
    trips = -(-n // (R.flat_grid(n, 2048) * 256))
    assert abs(gst["den"] - acc_den) <= R.prodigy_den_bound(ema["s"][1], trips), (where, gst["den"], acc_den)
    ref64, new, _, _ = R.prodigy_step(d["p"], d["g"], d["m"], d["v"], d["s"], d["p0"], st, h, c64, den=float(gst["den"]))
    for k in "pmvs":
        e = R.err_ulps(got[k], *ref64[k])
        record("prodigy", k, e)
        assert e <= R.BARS["prodigy"][k], (where, k, e)
    if not d["v"][100:128].any():
        pads_stay_zero(n, got, where)
    if scalars_exact:            # the numerator's sum is exact on select data, the rest is double arithmetic on the device's d_denom
        for k in ST_KEYS:
            assert abs(gst[k] - new[k]) <= R.SCALAR_RTOL * abs(new[k]), (where, k, gst[k], new[k])
    return new, gst


def test_prodigy_element_states_every_case_clip_and_length():
    for (name, cn, n, seed), shift in itertools.product(R.prodigy_element_cases(), (0, 1)):
        h, d, st = R.prodigy_inputs(name, n, seed)
        prodigy_check(d, st, h, cn, shift, (name, cn, n, shift))


def test_prodigy_scalars_on_select_data_through_every_branch_of_the_d_kernel():
    """The "fresh" states are the ones qfx_prodigy_init_state(1e-6) itself writes (the double 1e-6; the step sees (float)1e-6): the
    package's first jump, d = d_hat however small growth_rate is, must happen from them."""
    seen = {}
    for name, kw, st, n in R.prodigy_scalar_cases():
        h = R.prodigy_hp(**kw)
        d = R.select_prodigy(n, st["d"])
        fresh = name.startswith("fresh")
        assert not fresh or (st["d"] == R.PRODIGY_D0 != h["d0"])
        new, gst = prodigy_check(d, st, h, "max_norm_0", n % 2, (name, n), scalars_exact=True,      # clip = grad_scale = 0.5: exact products
                                 init=R.PRODIGY_D0 if fresh else None)
        s = seen.setdefault(n, set())
        if fresh and new["d_hat"] > st["d"]:
            assert gst["d"] == gst["d_hat"] == gst["d_max"], (name, n, gst)          # not capped at d0 growth_rate
            s.add("raised_from_d0_past_the_cap" if new["d_hat"] > st["d"] * h["growth"] else "raised_from_d0")
        if not fresh and new["d"] == st["d"] * h["growth"] < new["d_max"]:
            s.add("cap_binds")
        if math.isinf(h["growth"]) and new["d"] == new["d_max"]:
            s.add("cap_free")
        if new["d_max"] == st["d_max"] > new["d_hat"]:
            s.add("d_max_kept")
        assert new["k"] == st["k"] + 1 == gst["k"]
    for n in (N, R.N_SUM_TRIP2):
        assert seen[n] == {"raised_from_d0", "raised_from_d0_past_the_cap", "cap_binds", "cap_free", "d_max_kept"}, (n, seen[n])


def test_prodigy_first_jump_is_uncapped_through_ops_as_in_the_package():
    """ops.prodigy_init_state and ops.prodigy_step with their default d0 (the Python double 1e-6) and growth_rate = 1.02: the package
    (oracle/prodigy.py on the same fp32 tensors) raises d from d0 to d_hat in the first step, far past 1.02 d0."""
    from oracle import prodigy as OP
    from qflux_amd import ops
    d = R.select_prodigy(N, R.PRODIGY_D0)
    d["m"], d["v"], d["s"] = (np.zeros(N, F32) for _ in range(3))
    T = {k: torch.from_numpy(d[k].copy()).to(DEV) for k in ("p", "g", "m", "v", "s", "p0")}
    state = torch.full((_L().PRODIGY_STATE,), float("nan"), dtype=torch.float64, device=DEV)
    ops.prodigy_init_state(state)
    ops.prodigy_step(T["p"], T["g"], T["m"], T["v"], T["s"], T["p0"], state, growth_rate=1.02)
    torch.cuda.synchronize()
    _STATS["launches"] += 1
    w = state.cpu().numpy()
    p = torch.from_numpy(d["p"].copy())
    opt = OP.Prodigy([p], growth_rate=1.02)
    opt.state[0].update(step=0, s=torch.zeros(N), p0=torch.from_numpy(d["p0"].copy()), exp_avg=torch.zeros(N), exp_avg_sq=torch.zeros(N))
    opt.step([torch.from_numpy(d["g"].copy())])
    G = opt.group
    assert G["d"] == G["d_hat"] > 1000 * 1.02e-6
    assert w[0] == w[4] == w[1] and abs(w[0] - G["d"]) <= 1e-6 * G["d"] and w[5] == 1.0, (w[:6], G["d"])


def test_prodigy_skips_without_progress_and_returns_at_lr_zero():
    h, d, st = R.prodigy_inputs("decay")
    d = dict(d, g=np.zeros(N, F32), s=np.zeros(N, F32))
    got, gst, B, sb = launch_prodigy(d, st, h, (None, 0.0, 1.0))              # den == 0: the package returns before storing anything
    assert B["p"].unchanged() and all(gst[k] == st[k] for k in ST_KEYS)
    assert same_bits(got["m"], (d["m"] * F32(h["b1"])).astype(F32)) and same_bits(got["v"], (d["v"] * F32(h["b2"])).astype(F32))
    h, d, st = R.prodigy_inputs("decay")
    got, gst, B, sb = launch_prodigy(d, st, dict(h, lr=0.0), (None, 0.0, 1.0))          # lr == 0: nothing is written
    assert all(b.unchanged() for b in B.values()) and sb.unchanged()


# ---------------------------------------------------------------- refusals
def _refusal_bufs(n=257):
    d = R.case_data(n, 11)
    B = {k: Buf(d[k]) for k in ("p", "g", "m", "v", "buf", "s", "p0")}
    B["gn"], B["out"], B["part"] = Buf([4.0]), Buf([0.5]), Buf(np.zeros(8, F32))
    B["tg"] = Buf(np.zeros(2, np.uint32), 0, np.uint32)
    B["st"] = Buf(np.array([1e-6, 1e-6, 0, 0, 1e-6, 0] + [0.0] * 6, F64), 0, F64)
    return B, n


def _refused(B, rc, want, what):
    torch.cuda.synchronize()
    assert rc == want, (what, rc)
    assert all(b.unchanged() for b in B.values()), what


def test_refusals_of_the_sums_adamw_and_sgd():
    L, s = _L(), _stream()
    B, n = _refusal_bufs()
    P = {k: b.ptr for k, b in B.items()}
    ok = dict(sumsq=[P["g"], n, P["out"], s], det=[P["g"], n, P["out"], P["part"], 8, s],
              adamw=[P["p"], P["g"], P["m"], P["v"], n, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0.1, 0.001, P["gn"], 1.0, 1.0, s],
              sgd=[P["p"], P["g"], P["buf"], n, 0.05, 0.9, 0.0, 1e-4, 0, 0, P["gn"], 1.0, 1.0, s])
    fn = dict(sumsq=L.lib.qfx_sumsq, det=L.lib.qfx_sumsq_det, adamw=L.lib.qfx_adamw_step, sgd=L.lib.qfx_sgd_step)
    table = [("sumsq", 0, None), ("sumsq", 2, None), ("sumsq", 1, 0), ("sumsq", 1, -5),
             ("det", 0, None), ("det", 2, None), ("det", 3, None), ("det", 1, 0), ("det", 4, 0), ("det", 4, -1),
             ("adamw", 0, None), ("adamw", 1, None), ("adamw", 2, None), ("adamw", 3, None), ("adamw", 4, 0), ("adamw", 4, -1),
             ("sgd", 0, None), ("sgd", 1, None), ("sgd", 2, None), ("sgd", 3, 0), ("sgd", 3, -1)]
    for name, i, val in table:
        a = list(ok[name])
        a[i] = val
        _refused(B, fn[name](*a), EINVAL, (name, i, val))
    sgd = lambda **kw: [P["p"], P["g"], kw.get("buf", P["buf"]), n, 0.05, kw.get("mom", 0.9), kw.get("damp", 0.0), 1e-4, kw.get("nes", 0), 0,  # noqa: E731
                        P["gn"], 1.0, 1.0, s]
    for kw in (dict(nes=1, mom=0.0), dict(nes=1, mom=-0.5), dict(nes=1, damp=0.1), dict(buf=None, mom=0.5)):
        _refused(B, L.lib.qfx_sgd_step(*sgd(**kw)), EINVAL, kw)


def test_refusals_of_the_grouped_entries():
    L, s = _L(), _stream()
    B, n = _refusal_bufs()
    P = {k: b.ptr for k, b in B.items()}
    arow = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, bc1=0.1, bc2=0.001)
    srow = dict(lr=0.05, mom=0.9, damp=0.0, wd=1e-4, nes=0)
    A = lambda rows: (L.AdamwGroup * max(1, len(rows)))(*[L.AdamwGroup(*[r[k] for k in ("lr", "b1", "b2", "eps", "wd", "bc1", "bc2")]) for r in rows])  # noqa: E731
    S = lambda rows: (L.SgdGroup * max(1, len(rows)))(*[L.SgdGroup(*[r[k] for k in ("lr", "mom", "damp", "wd", "nes")]) for r in rows])  # noqa: E731

    def adamw(rows=None, ng=1, **kw):
        a = dict(p=P["p"], g=P["g"], m=P["m"], v=P["v"], n=n, tg=P["tg"], rows=A(rows or [arow]))
        a.update(kw)
        if a.pop("null_rows", False):
            a["rows"] = None
        return L.lib.qfx_adamw_step_grouped(a["p"], a["g"], a["m"], a["v"], a["n"], a["tg"], a["rows"], ng, P["gn"], 1.0, 1.0, s)

    def sgd(rows=None, ng=1, **kw):
        a = dict(p=P["p"], g=P["g"], buf=P["buf"], n=n, tg=P["tg"], rows=S(rows or [srow]))
        a.update(kw)
        if a.pop("null_rows", False):
            a["rows"] = None
        return L.lib.qfx_sgd_step_grouped(a["p"], a["g"], a["buf"], a["n"], a["tg"], a["rows"], ng, 0, P["gn"], 1.0, 1.0, s)
    nan = float("nan")
    for kw in [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(tg=None), dict(null_rows=True), dict(n=0), dict(n=-3), dict(ng=0), dict(ng=17),
               *[dict(rows=[dict(arow, **{k: x})]) for k, x in (("lr", -1e-3), ("lr", nan), ("b1", 1.0), ("b1", -0.1), ("b2", 1.0), ("b2", nan),
                                                               ("eps", -1e-8), ("wd", -0.01), ("bc1", 0.0), ("bc2", 0.0), ("bc2", -1.0))],
               dict(rows=[arow, dict(arow, lr=-1.0)], ng=2)]:
        _refused(B, adamw(**kw), EINVAL, ("adamw grouped", kw))
    for kw in [dict(p=None), dict(g=None), dict(tg=None), dict(null_rows=True), dict(n=0), dict(ng=0), dict(ng=17), dict(buf=None),
               *[dict(rows=[dict(srow, **r)]) for r in (dict(lr=-0.05), dict(mom=-0.9), dict(wd=-1e-4), dict(nes=1, mom=0.0), dict(nes=1, damp=0.1),
                                                       dict(lr=nan))],
               dict(rows=[dict(srow, mom=0.0), srow], ng=2, buf=None)]:
        _refused(B, sgd(**kw), EINVAL, ("sgd grouped", kw))
    assert sgd(rows=[dict(srow, mom=0.0)], buf=None) == 0          # NULL buf is fine when no group has momentum
    torch.cuda.synchronize()


def test_refusals_of_prodigy():
    L, s = _L(), _stream()
    B, n = _refusal_bufs()
    P = {k: b.ptr for k, b in B.items()}

    def step(**kw):
        f = dict(p=P["p"], g=P["g"], m=P["m"], v=P["v"], s=P["s"], p0=P["p0"], n=n, st=P["st"], lr=1.0, b1=0.9, b2=0.999, beta3=0.0, eps=1e-8,
                 wd=0.0, d0=1e-6, d_coef=1.0, growth=float("inf"), bc=0, sg=0, decouple=1)
        f.update(kw)
        a = L.ProdigyArgs(f["p"], f["g"], f["m"], f["v"], f["s"], f["p0"], f["n"], f["st"], f["lr"], f["b1"], f["b2"], f["beta3"], f["eps"], f["wd"],
                          f["d0"], f["d_coef"], f["growth"], f["bc"], f["sg"], f["decouple"], P["gn"], 1.0, 1.0)
        return L.lib.qfx_prodigy_step(C.byref(a), s)
    for kw in [*[{k: None} for k in ("p", "g", "m", "v", "s", "p0", "st")], dict(n=0), dict(n=-1), dict(b1=0.0), dict(b1=-0.5), dict(d0=0.0),
               dict(d0=-1e-6), dict(lr=-1.0), dict(b1=float("nan"))]:
        _refused(B, step(**kw), EINVAL, ("prodigy", kw))
    _refused(B, L.lib.qfx_prodigy_step(None, s), EINVAL, "NULL args")
    _refused(B, step(wd=0.01, decouple=0), EUNSUPPORTED, "coupled decay")
    _refused(B, step(lr=0.0), 0, "lr == 0 returns before any launch")
    for st, d0 in ((None, 1e-6), (P["st"], 0.0), (P["st"], -1.0), (P["st"], float("nan"))):
        _refused(B, L.lib.qfx_prodigy_init_state(st, d0, s), EINVAL, ("init", d0))
