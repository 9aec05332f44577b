"""CPU: the mask definition of the adapter dropout (include/qfx.h) through the library's host function against the independent
numpy restatement (tests/lora_dropout_ref.py), its statistics, argument validation, state-dict behaviour and the launch plans
(built in host memory by the dry run of tools/plan_fingerprint.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import lora_dropout_ref as R
from parity_util import ROOT


def _host(words, site, b, t, r):
    from qflux_amd import _lib as L
    st = (C.c_uint32 * 8)(*[int(w) for w in words])
    out = (C.c_float * r)()
    assert L.lib.qfx_lora_dropout_factors_host(st, site, b, t, r, out) == 0
    return np.frombuffer(out, dtype=np.float32).copy()


def test_philox_known_answers_and_agreement_on_random_counters():
    """Random123's known-answer vectors of philox4x32_10 (counter 0 / key 0 and all-ones), then the library's generator against the
    numpy one on 1000 random (counter, key) pairs: reached through the element draw, whose counter is (t * 32 + q, sample0 + b,
    step, site) under the key (seed_lo, seed_hi), with thr_elem = 1 << 31 (a word is kept iff its top bit is set) -- so each call
    exposes one bit of each of the four output words, and 1000 calls 4000 bits."""
    assert [int(v) for v in R.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = 0xFFFFFFFF
    assert [int(v) for v in R.philox4x32_10(ones, ones, ones, ones, ones, ones)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    rng = np.random.default_rng(7)
    for _ in range(1000):
        t, q = int(rng.integers(0, (1 << 27) - 2)), int(rng.integers(0, 32))
        sample0, b, step, site, k0, k1 = (int(rng.integers(0, 1 << 32)) for _ in range(6))
        b &= 0x7FFFFFFF
        words = [k0, k1, step, 1, 1 << 31, 0, 0x3F800000, sample0]
        got = _host(words, site, b, t, 4 * q + 4)[4 * q:]
        w = R.philox4x32_10(t * 32 + q, (sample0 + b) & ones, step, site, k0, k1)
        assert [float(x) for x in got] == [1.0 if int(v) >> 31 else 0.0 for v in w]


@pytest.mark.parametrize("r", [4, 16, 24, 64])
def test_host_factors_equal_the_reference_bit_for_bit(r):
    for seed, step, sample0, pe, pr in ((0, 1, 0, 0.25, 0.25), (0x1234567890ABCDEF, 77, 6, 0.1, 0.0), (5, 4000000000, 1, 0.0, 0.5),
                                        (9, 3, 0, 0.0, 0.0)):
        words = R.make_state(seed=seed, step=step, network_dropout=pe, rank_dropout=pr, sample0=sample0)
        for site in (0, R.site_key("transformer_blocks.3.attn.to_q"), 0xFFFFFFFF):
            ts = [0, 1, 31, 32, 4095, 123456]
            ref = R.factors(words, site, [0, 1, 5], ts, r)
            for bi, b in enumerate((0, 1, 5)):
                for ti, t in enumerate(ts):
                    assert np.array_equal(_host(words, site, b, t, r).view(np.uint32), ref[bi, ti].view(np.uint32)), (seed, site, b, t)


def test_host_words_match_the_reference_state():
    from qflux_amd import ops
    for kw in (dict(seed=3, step=9, network_dropout=0.25, rank_dropout=0.25, sample0=4), dict(seed=(1 << 63) + 5, rank_dropout=0.9)):
        assert ops.lora_dropout_state_words(active=1, **kw) == [int(v) for v in R.make_state(active=1, **kw)]
    assert ops.lora_dropout_threshold(0.25) == 1 << 30 and ops.lora_dropout_threshold(0.0) == 0


@pytest.mark.parametrize("option", ["network_dropout", "rank_dropout"])
def test_statistics_of_each_option(option):
    """n = 2^20 draws at p = 0.25: the kept fraction lies within 5 sigma of 0.75 (sigma = sqrt(p (1 - p) / n) = 4.2e-4), every
    kept factor is `scale` exactly; rank draws are constant over the tokens and differ over samples and steps."""
    p, r, n = 0.25, 64, 1 << 20
    scale = np.float32(1.0 / (1.0 - p))
    site = R.site_key("transformer_blocks.0.attn.to_k")
    calls = n // r
    rows = []
    if option == "network_dropout":      # tokens of two samples at one step
        words = R.make_state(seed=11, step=1, **{option: p})
        for i in range(calls):
            rows.append(_host(words, site, i % 2, i // 2, r))
    else:                                # one draw per (sample, step, rank): samples x steps
        for i in range(calls):
            words = R.make_state(seed=11, step=1 + i // 128, **{option: p})
            rows.append(_host(words, site, i % 128, 0, r))
    f = np.stack(rows)
    kept = f != 0
    sigma = (p * (1 - p) / n) ** 0.5
    assert abs(kept.mean() - (1 - p)) < 5 * sigma, (kept.mean(), sigma)
    assert np.all(f[kept].view(np.uint32) == scale.view(np.uint32))
    if option == "rank_dropout":
        words = R.make_state(seed=11, step=1, rank_dropout=p)
        base = _host(words, site, 0, 0, r)
        for t in (1, 2, 1000, 99999):
            assert np.array_equal(_host(words, site, 0, t, r), base)
        assert not np.array_equal(_host(words, site, 1, 0, r), base)
        assert not np.array_equal(_host(R.make_state(seed=11, step=2, rank_dropout=p), site, 0, 0, r), base)


def test_argument_validation():
    from qflux_amd import _lib as L
    from qflux_amd import dropout, ops
    from qflux_amd.trainer import FluxKontextTrainStep, QwenLoraTrainStep
    for bad in (-0.1, 1.0):
        for what in ("network_dropout", "rank_dropout"):
            with pytest.raises(ValueError):
                ops.lora_dropout_state_words(**{what: bad})
            with pytest.raises(ValueError):
                dropout.check_probability(bad, what)
            for cls in (QwenLoraTrainStep, FluxKontextTrainStep):
                with pytest.raises(ValueError):
                    cls(None, **{what: bad})      # refused before the model is touched
    # the C entry points reject before any launch (safe without a GPU)
    lib = L.lib
    st = (C.c_uint32 * 8)()
    out = (C.c_float * 4)()
    assert lib.qfx_lora_dropout_factors_host(None, 0, 0, 0, 4, out) == -1 and lib.qfx_lora_dropout_factors_host(st, 0, 0, 0, 129, out) == -1
    assert lib.qfx_lora_dropout_factors_host(st, 0, -1, 0, 4, out) == -1 and lib.qfx_lora_dropout_factors_host(st, 0, 0, 0, 0, out) == -1
    assert lib.qfx_lora_dropout_advance(None, None) == -1
    a = L.LoraDropoutArgs()
    arr = (L.LoraDropoutArgs * 1)(a)
    assert lib.qfx_lora_dropout_apply(arr, 1, None, None) == -1 and lib.qfx_lora_dropout_apply(None, 1, 0x1000, None) == -1
    a.Ut_hi, a.Ut_lo, a.ld_ut, a.M, a.R, a.group_R, a.rows_per_batch = 0x1000, 0x2000, 128, 70, 16, 16, 35
    for field, value in (("ld_ut", 69), ("R", 24), ("R", 112), ("group_R", 8), ("rows_per_batch", 0), ("Ut_lo", 0), ("M", 0)):
        b = L.LoraDropoutArgs.from_buffer_copy(a)
        setattr(b, field, value)
        assert lib.qfx_lora_dropout_apply((L.LoraDropoutArgs * 1)(b), 1, 0x3000, None) == -1, field
    a.ext, a.ld_ext = 0x4000, 44      # ld_ext short of the three images
    assert lib.qfx_lora_dropout_apply((L.LoraDropoutArgs * 1)(a), 1, 0x3000, None) == -1
    a.ext, a.ld_ext = 0x4002, 48      # ext not 8-byte aligned
    assert lib.qfx_lora_dropout_apply((L.LoraDropoutArgs * 1)(a), 1, 0x3000, None) == -1
    assert lib.qfx_lora_dropout_apply((L.LoraDropoutArgs * 9)(), 9, 0x3000, None) == -1


@pytest.fixture(scope="module")
def pf():
    from tools import plan_fingerprint
    return plan_fingerprint


def _calls(plan):
    return [e[0].__name__ if e[0] is not None else "py" for prog in (plan.fwd, plan.bwd) for e in prog.calls]


def test_state_dict_keys_and_round_trip(pf, monkeypatch):
    """No new key with the feature off; with it on the key round-trips through load_state_dict into a fresh step, step count
    included; eval() / train() / eval_mode() move the switch the forward programs follow."""
    from qflux_amd.trainer import QwenLoraTrainStep
    monkeypatch.setenv("QFX_MOD_TABLE", "0")      # (the table is built by launches: not in host memory)
    with pf.dry_run():
        m = pf._qwen()
        m.lora_store
        s = QwenLoraTrainStep(m)
        assert m.lora_dropout is None and "lora_dropout" not in s.state_dict()
        s0 = QwenLoraTrainStep(m, network_dropout=0.0, rank_dropout=0.0)
        assert m.lora_dropout is None and "lora_dropout" not in s0.state_dict()
        s1 = QwenLoraTrainStep(m, network_dropout=0.25, rank_dropout=0.5, dropout_seed=99)
        m.lora_dropout.set_step(17)
        sd = s1.state_dict()
        assert sd["lora_dropout"] == {"seed": 99, "step": 17, "network_dropout": 0.25, "rank_dropout": 0.5}
        assert set(sd) - {"lora_dropout"} == set(s.state_dict()) - {"lora_dropout"}
        m2 = pf._qwen()
        m2.lora_store
        s2 = QwenLoraTrainStep(m2)
        s2.load_state_dict(sd)
        assert s2.state_dict()["lora_dropout"] == sd["lora_dropout"]
        assert m2.lora_dropout.host_words()[:3] == [99, 0, 17] and m2.lora_dropout.host_words()[4:6] == [1 << 30, 1 << 31]
        st = m2.lora_dropout
        assert st.enabled
        s2.eval()
        assert not st.enabled
        s2.train()
        assert st.enabled
        with s2.eval_mode():
            assert not st.enabled
        assert st.enabled
        with m2.lora_dropout_off():
            assert not st.enabled
        assert st.enabled
        # the MX-FP8 trunk refuses the option, in either order
        with pytest.raises(NotImplementedError):
            m2.quantize_trunk("mxfp8")
        m3 = pf._qwen(quant="mxfp8")
        with pytest.raises(NotImplementedError):
            m3.set_lora_dropout(0.1, 0.0)


PLAN_CONFIGS = ["qwen_attn", "qwen_q_only", "qwen_ff", "qwen_embed", "qwen_head_lora", "qwen_multires", "flux_attn", "flux_q_only",
                "flux_all", "flux_multires"]


def test_plans_with_dropout_off_equal_the_committed_fingerprints(pf):
    """Off is part of the plan-cache key and emits today's launches: the digests of tests/golden/plan_fingerprints.json, also after
    the option was on and is switched off again on the same model."""
    with open(os.path.join(ROOT, "tests", "golden", "plan_fingerprints.json")) as f:
        recorded = json.load(f)["sha256"]
    with pf.dry_run():
        for name, build, plan in (("qwen_attn", pf._qwen, pf._qwen_plan), ("flux_all", lambda: pf._flux(targets=pf.FLUX_ALL), pf._flux_plan)):
            m = build()
            m.set_lora_dropout(0.0, 0.0)
            assert pf.digest(pf.fingerprint(plan(m))) == recorded[name]
            m.set_lora_dropout(0.25, 0.25, 1)
            on = plan(m)
            assert "qfx_lora_dropout_apply" in _calls(on)
            m.set_lora_dropout(0.0, 0.0)
            off = plan(m)
            assert off is not on and pf.digest(pf.fingerprint(off)) == recorded[name]


@pytest.mark.parametrize("name", PLAN_CONFIGS)
def test_plans_with_dropout_on_mask_every_rank_r_producer(pf, name, monkeypatch):
    """With the option on a plan is the plan without it plus: the advance as the first forward call, and behind every rank-r
    producer problem one dropout problem on the same Ut / ext buffers before the next GEMM or gradient launch; the site keys of a
    buffer's forward and backward problems name the same adapters."""
    import qflux_amd.models as M
    with pf.dry_run():
        off = pf.build(name)
        for cls in (M.QwenImageTransformer2DModel, M.FluxTransformer2DModel):
            orig = cls.add_adapter

            def add(self, *a, _orig=orig, **k):
                r = _orig(self, *a, **k)
                self.set_lora_dropout(0.25, 0.25, 7)
                return r
            monkeypatch.setattr(cls, "add_adapter", add)
        on = pf.build(name)
    assert on.fwd.calls[0][0].__name__ == "qfx_lora_dropout_advance"
    assert [c for c in _calls(on) if "dropout" not in c] == _calls(off)
    producers = {"qfx_lora_down": 1, "qfx_lora_down_batch": None, "qfx_ln_down_fwd": None, "qfx_lora_head_reduce": None}
    consumers = ("qfx_gemm_bf16", "qfx_gemm_grouped", "qfx_lora_grad", "qfx_lora_grad_batch")
    n_masked = 0
    for prog in (on.fwd, on.bwd):
        pending = {}
        for fn, args, *_ in prog.calls:
            fname = fn.__name__ if fn is not None else "py"
            if fname in producers:
                probs = [args[0]._obj] if fname == "qfx_lora_down" else [args[0][k] for k in range(args[1])]
                for a in probs:
                    if a.Ut_hi:
                        pending[a.Ut_hi] = (a.ext, a.R)
            elif fname == "qfx_lora_dropout_apply":
                for k in range(args[1]):
                    a = args[0][k]
                    assert pending.pop(a.Ut_hi) == (a.ext, a.R), "a dropout problem without its producer right before it"
                    assert a.rows_per_batch * on.B == a.M
                    assert "q_only" in name or all(a.site[g] for g in range(a.R // a.group_R))      # every group names its adapter
                    n_masked += 1
            elif fname in consumers:
                assert not pending, f"{fname} reads rank-r buffers that were not masked"
    assert n_masked > 0
