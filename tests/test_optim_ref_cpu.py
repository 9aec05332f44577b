"""CPU: the yardstick of tests/test_optim_gpu.py (tests/optim_ref.py) checked on its own -- the fp64 restatements against torch.optim
and oracle/prodigy.py on fp64 tensors, the fmaf emulation against exact rationals, the bars against the fp32 restatement's own error,
`select` data exact in three summation orders, and every deliberate mistake (mutant) at least MUTANT_MARGIN bars away from the
reference on the data the GPU test uses.  Nothing here runs a kernel."""
import itertools
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import optim_ref as R
from oracle import prodigy as OP

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SEED = 1027, 3          # the GPU test's full-cross length and seed


def _rel(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---------------------------------------------------------------- fmaf
def _exact_fma(a, b, c):
    """Round the exact rational a b + c to fp32, ties to even, by hand."""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:
        return 0.0
    sgn, x = (-1 if x < 0 else 1), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    q = x / Fraction(2) ** (e - 23)               # in [2^23, 2^24)
    k, rem = divmod(q.numerator, q.denominator)
    twice = 2 * rem
    if twice > q.denominator or (twice == q.denominator and k & 1):
        k += 1
    return sgn * float(Fraction(k) * Fraction(2) ** (e - 23))


def test_fma32_matches_exact_rationals_on_random_and_near_tie_triples():
    r = np.random.default_rng(0)
    n = 1500
    a = (r.standard_normal(n) * 10.0 ** r.integers(-6, 6, n)).astype(F32)
    b = (r.standard_normal(n) * 10.0 ** r.integers(-6, 6, n)).astype(F32)
    c = (-(a.astype(F64) * b.astype(F64)) * (1 + r.standard_normal(n) * 10.0 ** r.integers(-9, 1, n))).astype(F32)      # cancelling too
    # near ties: c = 1 + odd 2^-23 (times 2^x), a b = +-(2^-24 - k^2 2^-70): half an ulp of c less a residue fp64 addition drops
    k = r.integers(1, 2000, n)
    m = r.integers(0, 1 << 22, n) * 2 + 1
    x = r.integers(-20, 20, n)
    sg = r.choice([-1.0, 1.0], n)
    ta = np.ldexp(1.0 + k * 2.0 ** -23, x).astype(F32)
    tb = (sg * np.ldexp(1.0 - k * 2.0 ** -23, -24)).astype(F32)
    tc = np.ldexp(1.0 + m * 2.0 ** -23, x).astype(F32)
    A, B, C = np.concatenate([a, ta, ta]), np.concatenate([b, tb, tb]), np.concatenate([c, tc, -tc])
    got = R.fma32(A, B, C)
    want = np.array([_exact_fma(*t) for t in zip(A, B, C)], dtype=F32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    naive = (A.astype(F64) * B.astype(F64) + C.astype(F64)).astype(F32)
    assert (naive != want).sum() > n // 4          # the triples do catch double rounding


# ---------------------------------------------------------------- fp64 tier against the installed packages
def _t64(x):
    return torch.tensor(np.asarray(x, F64))


@pytest.mark.parametrize("name", list(R.ADAMW_HP))
def test_fp64_adamw_is_torch_adamw_with_clip_grad_norm(name):
    hp = R.ADAMW_HP[name]
    d = R.case_data(257, 1, name)
    p = torch.nn.Parameter(_t64(d["p"]))
    opt = torch.optim.AdamW([p], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"])
    pr, m, v = d["p"].astype(F64), np.zeros(257), np.zeros(257)
    for t in range(1, 5):
        g = R.rand_data(257, 10 + t, pad=False)["g"].astype(F64)
        p.grad = _t64(g)
        torch.nn.utils.clip_grad_norm_([p], 0.5)
        opt.step()
        clip = min(1.0, 0.5 / (math.sqrt(float((g ** 2).sum())) + 1e-6))
        o = R.adamw_f64(pr, g, m, v, clip, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], 1 - hp["b1"] ** t, 1 - hp["b2"] ** t)
        pr, m, v = o["p"][0], o["m"][0], o["v"][0]
        st = opt.state[p]
        live = np.isfinite(pr)
        assert live.all() or name == "eps0"
        assert _rel(pr, p.detach().numpy()) < 1e-12 and _rel(m, st["exp_avg"].numpy()) < 1e-12 and _rel(v, st["exp_avg_sq"].numpy()) < 1e-12


@pytest.mark.parametrize("name", list(R.SGD_HP))
def test_fp64_sgd_is_torch_sgd_with_clip_grad_norm(name):
    hp = R.SGD_HP[name]
    d = R.case_data(257, 2)
    p = torch.nn.Parameter(_t64(d["p"]))
    opt = torch.optim.SGD([p], lr=hp["lr"], momentum=hp["mom"], dampening=hp["damp"], weight_decay=hp["wd"], nesterov=bool(hp["nesterov"]))
    pr, buf = d["p"].astype(F64), None
    for t in range(1, 5):
        g = R.rand_data(257, 20 + t, pad=False)["g"].astype(F64)
        p.grad = _t64(g)
        torch.nn.utils.clip_grad_norm_([p], 0.5)
        opt.step()
        clip = min(1.0, 0.5 / (math.sqrt(float((g ** 2).sum())) + 1e-6))
        o = R.sgd_f64(pr, g, buf, clip, hp["lr"], hp["mom"], hp["damp"], hp["wd"], hp["nesterov"], t == 1)
        pr, buf = o["p"][0], (o["buf"][0] if "buf" in o else None)
        assert _rel(pr, p.detach().numpy()) < 1e-12
        if hp["mom"]:
            assert _rel(buf, opt.state[p]["momentum_buffer"].numpy()) < 1e-12


@pytest.mark.parametrize("name", list(R.PRODIGY_CASES))
def test_fp64_prodigy_is_the_oracle_on_fp64_tensors(name):
    h = dict(R.PRODIGY_DEFAULTS, **R.PRODIGY_CASES[name])
    n = 257
    d = R.case_data(n, 4)
    p = _t64(d["p"]).clone()
    opt = OP.Prodigy([p], lr=h["lr"], betas=(h["b1"], h["b2"]), beta3=h["beta3"] or None, eps=h["eps"], weight_decay=h["wd"],
                     use_bias_correction=bool(h["use_bc"]), safeguard_warmup=bool(h["safeguard"]), d0=h["d0"], d_coef=h["d_coef"],
                     growth_rate=h["growth"])
    pr, p0 = d["p"].astype(F64), d["p"].astype(F64)
    m, v, s = np.zeros(n), np.zeros(n), np.zeros(n)
    st = R.prodigy_state(h["d0"])
    for t in range(6):
        g = R.rand_data(n, 30 + t, pad=False)["g"].astype(F64)
        opt.step([_t64(g)])
        out, new, _, _ = R.prodigy_step(pr, g, m, v, s, p0, st, h, 1.0, round_scalars=False)
        m, v, s, pr, st = out["m"][0], out["v"][0], out["s"][0], out["p"][0], new
        G, S = opt.group, opt.state[0]
        for key, want in (("d", G["d"]), ("d_max", G["d_max"]), ("num", G["d_numerator"]), ("den", G["d_denom"]), ("d_hat", G["d_hat"]), ("k", G["k"])):
            assert abs(st[key] - want) <= 1e-11 * abs(want), (t, key)
        assert _rel(pr, p.numpy()) < 1e-11 and _rel(m, S["exp_avg"].numpy()) < 1e-11 and _rel(v, S["exp_avg_sq"].numpy()) < 1e-11
        assert _rel(s, S["s"].numpy()) < 1e-11
    assert st["num"] != 0.0 and st["k"] == 6          # the estimate is live


def test_prodigy_scalar_branches():
    h = R.prodigy_hp(growth=2.0)
    d0 = h["d0"]
    first = R.prodigy_d(R.prodigy_state(d0), h, 1.0, 1e-3)                     # d == d0: raised to d_hat, the cap (2 d_hat) not binding
    as_held = R.prodigy_d(R.prodigy_state(1e-6), dict(h, growth=1.02), 1.0, 1e-3)      # the double 1e-6 against its float image: still `d == d0`
    assert 1e-6 != d0 and as_held["d"] == as_held["d_hat"] > 100 * d0
    assert first["d"] == first["d_hat"] == first["d_max"] > 100 * d0
    st = R.prodigy_state(d0, d=3 * d0, d_max=3 * d0)
    capped = R.prodigy_d(st, h, 1.0, 1e-3)                                      # d != d0: growth cap binds
    assert capped["d"] == 6 * d0 and capped["d_max"] == capped["d_hat"] > 6 * d0
    kept = R.prodigy_d(R.prodigy_state(d0, d=3 * d0, d_max=5 * d0), h, 1e-12, 1e3)      # d_hat tiny: d_max kept, d = min(d_max, 2 d)
    assert kept["d_max"] == 5 * d0 and kept["d"] == 5 * d0
    assert R.prodigy_d(st, h, 1.0, 0.0) is None
    assert R.prodigy_beta3(R.prodigy_hp()) == math.sqrt(R.f32img(0.999)) and R.prodigy_beta3(R.prodigy_hp(beta3=0.5)) == 0.5


# ---------------------------------------------------------------- floors, bars
def _floor_adamw():
    fl = {}
    for (hn, hp), cn, t in itertools.product(R.ADAMW_HP.items(), R.CLIPS, R.STEPS):
        d = R.case_data(N, SEED, hn)
        a = R.adamw_args(hp, t)
        c64, forms, _, _ = R.clips_of(cn, d["g"])
        ref = R.adamw_f64(d["p"], d["g"], d["m"], d["v"], c64, **a)
        for c in forms:
            got = dict(zip("pmv", R.adamw_f32(d["p"], d["g"], d["m"], d["v"], c, **a)))
            for k in "pmv":
                fl[k] = max(fl.get(k, 0.0), R.err_ulps(got[k], *ref[k]))
    return fl


def _floor_sgd():
    fl = {}
    for (hn, hp), cn, first in itertools.product(R.SGD_HP.items(), R.CLIPS, (0, 1)):
        d = R.case_data(N, SEED)
        a = R.sgd_args(hp)
        c64, forms, _, _ = R.clips_of(cn, d["g"])
        ref = R.sgd_f64(d["p"], d["g"], d["buf"], c64, first=first, **a)
        for c in forms:
            pn, bn = R.sgd_f32(d["p"], d["g"], d["buf"], c, first=first, **a)
            fl["p"] = max(fl.get("p", 0.0), R.err_ulps(pn, *ref["p"]))
            if bn is not None:
                fl["buf"] = max(fl.get("buf", 0.0), R.err_ulps(bn, *ref["buf"]))
    return fl


def _floor_prodigy():
    fl = {}

    def put(d, st, h, cn):
        c64, forms, _, _ = R.clips_of(cn, d["g"])
        ref, new, _, den = R.prodigy_step(d["p"], d["g"], d["m"], d["v"], d["s"], d["p0"], st, h, c64)
        for c in forms:
            got, _, _, _ = R.prodigy_step(d["p"], d["g"], d["m"], d["v"], d["s"], d["p0"], st, h, c, f32=True, den=den)
            for k in "pmvs":
                fl[k] = max(fl.get(k, 0.0), R.err_ulps(got[k][0], *ref[k]))
    for name, cn, n, seed in R.prodigy_element_cases():
        h, d, st = R.prodigy_inputs(name, n, seed)
        put(d, st, h, cn)
    for _, kw, st, n in R.prodigy_scalar_cases():
        put(R.select_prodigy(n, st["d"]), st, R.prodigy_hp(**kw), "max_norm_0")
    return fl


_FLOORS = {}


def floors():
    if not _FLOORS:
        _FLOORS.update(adamw=_floor_adamw(), sgd=_floor_sgd(), prodigy=_floor_prodigy())
    return _FLOORS


def test_bars_are_twice_the_floors():
    """FLOORS in optim_ref.py are the figures measured here, rounded up to 0.01 ulp; BARS are twice them; profiles/optim_parity.json
    records the same numbers."""
    got = floors()
    print("measured floors:", json.dumps(got))
    for line, fl in got.items():
        assert set(fl) == set(R.FLOORS[line])
        for k, x in fl.items():
            assert x <= R.FLOORS[line][k] <= x + 0.011, (line, k, x, R.FLOORS[line][k])
            assert R.BARS[line][k] == 2.0 * R.FLOORS[line][k]
    rec = json.load(open(os.path.join(ROOT, "profiles", "optim_parity.json")))
    assert rec["floors_ulps"] == R.FLOORS and rec["bars_ulps"] == R.BARS


# ---------------------------------------------------------------- select data
@pytest.mark.parametrize("n", [1027, R.N_SUM_TRIP2])
def test_select_data_sums_exactly_in_three_orders(n):
    d = R.select_data(n)
    for clip in (1.0, 0.5):
        gi = d["g"] * F32(clip)
        for terms in (gi * gi, gi * (d["p0"] - d["p"])):
            assert terms.dtype == F32
            exact = float(terms.astype(F64).sum())
            fwd = np.cumsum(terms, dtype=F32)[-1]                                   # one after the other
            rev = np.cumsum(terms[::-1], dtype=F32)[-1]
            k = -(-n // 256) * 256
            strided = np.cumsum(np.cumsum(np.pad(terms, (0, k - n)).reshape(-1, 256), axis=0, dtype=F32)[-1], dtype=F32)[-1]      # by lane, then across
            assert float(fwd) == float(rev) == float(strided) == exact
    g64, p64 = d["g"].astype(F64), (d["p0"].astype(F64) - d["p"].astype(F64))
    assert np.array_equal((d["g"] * d["g"]).astype(F64), g64 * g64) and np.array_equal((d["g"] * (d["p0"] - d["p"])).astype(F64), g64 * p64)


def test_sum_bounds_hold_for_an_fp32_sum_in_the_kernels_order():
    """The derived bound against a numpy fp32 re-enactment of qfx_sumsq_det's order (per-thread trips, butterfly, four-wave fold, fold kernel)."""
    for n, nslots in ((1027, 1024), (R.N_SUM_TRIP2, 1024), (R.N_SUM_TRIP2, 3), (5000, 1)):
        g = R.rand_data(n, 5, pad=False)["g"]
        blocks = R.flat_grid(n, nslots)
        t = blocks * 256
        sq = np.pad(g * g, (0, -(-n // t) * t - n)).reshape(-1, blocks, 256)
        acc = np.cumsum(sq, axis=0, dtype=F32)[-1]                                  # [blocks, 256]: the trips
        w = acc.reshape(blocks, 4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            w = w + w[:, :, np.arange(64) ^ o]
        part = (w[:, 0, 0] + w[:, 1, 0]) + (w[:, 2, 0] + w[:, 3, 0])
        a2 = np.cumsum(np.pad(part, (0, -(-blocks // 256) * 256 - blocks)).reshape(-1, 256), axis=0, dtype=F32)[-1].reshape(4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            a2 = a2 + a2[:, np.arange(64) ^ o]
        out = (a2[0, 0] + a2[1, 0]) + (a2[2, 0] + a2[3, 0])
        ref = R.sumsq_f64(g)
        assert out.dtype == F32 and abs(float(out) - ref) <= R.sum_bound(R.sumsq_depth(n, True, nslots)) * ref
    assert R.sumsq_depth(1, True, 1024) == 1 + 8 + 1 + 8 and R.sumsq_depth(R.N_SUM_TRIP2, False) == 2 + 9 + 2048


# ---------------------------------------------------------------- mutants
def test_every_mutant_misses_the_reference_by_four_bars_on_the_gpu_tests_data():
    need = R.MUTANT_MARGIN
    seen = {}

    def check(line, name, ref, mut, keys):
        miss = max(R.err_ulps(mut[k][0], *ref[k]) / R.BARS[line][k] for k in keys)
        seen[name] = min(seen.get(name, float("inf")), miss)
        assert miss >= need, (line, name, miss)

    for (hn, hp), cn, t in itertools.product(R.ADAMW_HP.items(), R.CLIPS, R.STEPS):
        d = R.case_data(N, SEED, hn)
        a = R.adamw_args(hp, t)
        c64 = R.clips_of(cn, d["g"])[0]
        x = (d["p"], d["g"], d["m"], d["v"], c64)
        ref = R.adamw_f64(*x, **a)
        if hp["eps"] > 0:
            live = d["v"] > 0                      # outside the zero slots, where dropping eps divides 0 by 0
            check("adamw", "no_eps", {"p": tuple(z[live] for z in ref["p"])}, {"p": (R.adamw_f64(*x, **a, mut="no_eps")["p"][0][live],)}, "p")
        if hp["wd"] > 0:
            check("adamw", "no_wd", ref, R.adamw_f64(*x, **a, mut="no_wd"), "p")
            check("adamw", "decay_after", ref, R.adamw_f64(*x, **a, mut="decay_after"), "p")
        check("adamw", "v_linear", ref, R.adamw_f64(*x, **a, mut="v_linear"), "v")
        for tn in (t + 1, max(t - 1, 1)):
            for key, b in (("bc1", "b1"), ("bc2", "b2")):
                a2 = dict(a, **{key: R.bias_corr(hp[b], tn)})
                if a2[key] != a[key]:              # beta1 = 0, or beta1^1000 = 0 in fp32: the neighbouring step's correction is this step's
                    check("adamw", key + "_neighbour", ref, R.adamw_f64(*x, **a2), "p")
    for (hn, hp), cn, first in itertools.product(R.SGD_HP.items(), R.CLIPS, (0, 1)):
        d = R.case_data(N, SEED)
        a = R.sgd_args(hp)
        c64 = R.clips_of(cn, d["g"])[0]
        x = (d["p"], d["g"], d["buf"], c64)
        ref = R.sgd_f64(*x, first=first, **a)
        keys = ("p", "buf") if hp["mom"] else ("p",)
        if hp["mom"] and first:
            check("sgd", "ignore_first", ref, R.sgd_f64(*x, first=first, **a, mut="ignore_first"), keys)
            if hp["damp"]:
                check("sgd", "damp_on_first", ref, R.sgd_f64(*x, first=first, **a, mut="damp_on_first"), keys)
        if hp["nesterov"]:
            check("sgd", "no_nesterov_sum", ref, R.sgd_f64(*x, first=first, **a, mut="no_nesterov_sum"), "p")
        if hp["wd"] and c64 != 1.0:
            check("sgd", "clip_after_decay", ref, R.sgd_f64(*x, first=first, **a, mut="clip_after_decay"), "p")
    for name in R.PRODIGY_CASES:
        h, d, st = R.prodigy_inputs(name)
        x = (d["p"], d["g"], d["m"], d["v"], d["s"], d["p0"], st, h, 0.5)
        ref, new, _, _ = R.prodigy_step(*x)
        if R.prodigy_begin(st, h) != st["d"]:          # lr bias_correction == 1: both branches of safeguard_warmup are one number
            check("prodigy", "safeguard_swapped", ref, R.prodigy_step(*x, mut="safeguard_swapped")[0], "s")
        check("prodigy", "eps_not_scaled", ref, R.prodigy_step(*x, mut="eps_not_scaled")[0], "p")
        if not h["beta3"] > 0:
            mut, mnew, _, _ = R.prodigy_step(*x, mut="beta3_is_beta2")
            check("prodigy", "beta3_is_beta2", ref, mut, "s")
            assert abs(mnew["num"] - new["num"]) > 1e6 * R.SCALAR_RTOL * abs(new["num"])
    print("mutants, smallest miss in bars:", json.dumps(seen))
    assert set(seen) == {"no_eps", "no_wd", "decay_after", "v_linear", "bc1_neighbour", "bc2_neighbour", "ignore_first", "damp_on_first",
                         "no_nesterov_sum", "clip_after_decay", "safeguard_swapped", "eps_not_scaled", "beta3_is_beta2"}
