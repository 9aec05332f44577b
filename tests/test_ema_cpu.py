"""CPU: EMA of the adapter weights -- the decay schedule against hand-worked constants, the state-dict layout, the ABI of the two
entry points and their argument validation (no launch), the train steps' constructor refusals and the stock-loop class on plain
tensors against tests/ema_ref.py."""
import ctypes as C
import os
import re

import pytest
import torch

import ema_ref as R
from test_sgd_cpu import toy_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decay_schedule_hand_worked_constants():
    from qflux_amd.ema import get_decay
    plain = dict(decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3)
    # step = max(0, n - 0 - 1); (1 + step) / (10 + step)
    assert [get_decay(n, **plain) for n in (1, 2, 3, 11)] == [0.0, 2 / 11, 3 / 12, 11 / 20]
    assert get_decay(0, **plain) == 0.0
    # the clamp at `decay`: step 99 gives 100 / 109 > 0.9, step 10^6 gives the decay itself
    assert get_decay(100, **dict(plain, decay=0.9)) == 0.9 and get_decay(10 ** 6 + 1, **plain) == 0.9999
    assert get_decay(3, **dict(plain, decay=0.1)) == 0.1
    # the min_decay floor acts on positive steps only
    assert get_decay(2, **dict(plain, min_decay=0.5)) == 0.5 and get_decay(1, **dict(plain, min_decay=0.5)) == 0.0
    assert get_decay(11, **dict(plain, min_decay=0.5)) == 11 / 20
    # update_after_step = 3: 0 through step 4, then step 5 is the first averaged one
    late = dict(plain, update_after_step=3)
    assert [get_decay(n, **late) for n in (1, 2, 3, 4)] == [0.0] * 4 and get_decay(5, **late) == 2 / 11 and get_decay(6, **late) == 3 / 12
    # warm-up with inv_gamma = 1, power = 2/3 at step 2: 1 - (1 + 1)^(-2/3)
    warm = dict(plain, use_ema_warmup=True)
    assert get_decay(2, **warm) == pytest.approx(1 - 2 ** (-2 / 3), abs=1e-15) and abs(get_decay(2, **warm) - 0.3700394750525634) < 1e-15
    assert get_decay(1, **warm) == 0.0
    # inv_gamma = 2, power = 1 at step 5: step = 4, 1 - 1 / (1 + 4 / 2) = 2 / 3
    assert get_decay(5, **dict(warm, inv_gamma=2.0, power=1.0)) == pytest.approx(2 / 3, abs=1e-15)
    for n in range(0, 40):
        for kw in (plain, late, warm, dict(warm, min_decay=0.2, decay=0.6)):
            assert get_decay(n, **kw) == R.get_decay(n, **kw)


def test_state_dict_layout_and_reload():
    from qflux_amd.ema import EmaState, ensure_state
    toy = toy_model()
    st = toy.lora_store
    ema = EmaState(st, (0.5, 0.9, 0.999), update_after_step=2, use_ema_warmup=True, power=0.75)
    assert [n for n, _ in ema.buffers()] == ["ema0", "ema1", "ema2"] and EmaState.names((0.5, 0.9)) == ["ema0", "ema1"]
    assert all(t.shape == st.pflat.shape and t.data_ptr() != st.pflat.data_ptr() and torch.equal(t, st.pflat) for _, t in ema.buffers())
    ema.optimization_step = 7
    ema.shadows[1].mul_(2.0)
    sd = ema.state_dict(st)
    assert isinstance(sd, list) and len(sd) == 3
    names = [n for n, _ in toy.named_parameters() if "lora_" in n]
    for k, e in enumerate(sd):
        assert set(e) == R.KEYS
        assert (e["decay"], e["min_decay"], e["optimization_step"], e["update_after_step"], e["use_ema_warmup"], e["inv_gamma"],
                e["power"]) == ((0.5, 0.9, 0.999)[k], 0.0, 7, 2, True, 1.0, 0.75)
        assert len(e["shadow_params"]) == len(names) == len(st.entries)
        for t, (n, p, off, cnt), name in zip(e["shadow_params"], st.entries, names):
            assert n == name and t.shape == p.shape and t.dtype == torch.float32 and t.device.type == "cpu"
            assert torch.equal(t.reshape(-1), ema.shadows[k][off:off + cnt])
    other = EmaState(st, (0.1, 0.2, 0.3))
    other.load_state_dict(st, sd)
    assert other.decays == (0.5, 0.9, 0.999) and other.optimization_step == 7 and other.args == ema.args
    for k in range(3):
        for _, _, off, cnt in st.entries:
            assert R.same_bits(other.shadows[k][off:off + cnt], ema.shadows[k][off:off + cnt])
    with pytest.raises(ValueError, match="3 shadows"):
        EmaState(st, (0.5,)).load_state_dict(st, sd)
    bad = [dict(e) for e in sd]
    bad[2]["shadow_params"] = bad[2]["shadow_params"][:-1]
    with pytest.raises(ValueError, match="shadow 2"):
        other.load_state_dict(st, bad)
    # re-keying: the same layout keeps the state, another adapter set starts fresh shadows
    assert ensure_state(ema, st, ema.decays, ema.args) is ema
    bigger = toy_model(n_blocks=4).lora_store
    fresh = ensure_state(ema, bigger, ema.decays, ema.args)
    assert fresh is not ema and fresh.optimization_step == 0 and torch.equal(fresh.shadows[1], bigger.pflat)
    with pytest.raises(ValueError, match="shadows 0..2"):
        ema._index(3)


def test_abi_declarations_symbols_and_struct_layout(tmp_path):
    import subprocess
    from qflux_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "qfx.h")).read()
    assert re.search(r"^int qfx_ema_update\(const float\* p, int64_t n, const qfx_ema_args\* a, void\* stream\);", hdr, flags=re.M)
    assert re.search(r"^int qfx_ema_swap\(float\* p, float\* s, int64_t n, void\* stream\);", hdr, flags=re.M)
    assert "#define QFX_EMA_MAX_SHADOWS 4" in hdr and "#define QFX_ABI_VERSION 7" in hdr
    assert "qfx_ema_update" in L.SYMBOLS and "qfx_ema_swap" in L.SYMBOLS and L.ABI_VERSION == 7 and L.lib.qfx_abi_version() == 7
    assert hasattr(L.lib, "qfx_ema_update") and hasattr(L.lib, "qfx_ema_swap") and L.EMA_MAX_SHADOWS == 4
    fields = [f for f, _ in L.EmaArgs._fields_]
    src = tmp_path / "ema_abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qfx.h"\nint main(void) {\n  printf("%zu", sizeof(qfx_ema_args));\n' +
                   "".join(f'  printf(" %zu", offsetof(qfx_ema_args, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "ema_abi"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(L.EmaArgs)] + [getattr(L.EmaArgs, f).offset for f in fields] == [56, 0, 32, 48]


def _args(shadows, omds, n_shadows=None):
    from qflux_amd import _lib as L
    a = L.EmaArgs()
    for k, (s, o) in enumerate(zip(shadows, omds)):
        a.shadow[k], a.one_minus_decay[k] = s, o
    a.n_shadows = len(shadows) if n_shadows is None else n_shadows
    return a


def test_argument_validation_without_gpu():
    """Every rejected argument returns QFX_EINVAL before any launch; n == 0 returns 0 without one.  The pointers are never
    dereferenced on these paths."""
    from qflux_amd import _lib as L
    up, sw = L.lib.qfx_ema_update, L.lib.qfx_ema_swap
    P, S = 0x10000, [0x20000, 0x30000, 0x40000, 0x50000]
    ok = _args(S[:2], [0.5, 1e-4])
    assert up(P, 0, C.byref(ok), None) == 0
    assert up(P, 0, C.byref(_args(S, [0.0, 1.0, 0.5, 1e-4])), None) == 0
    assert up(None, 0, C.byref(ok), None) == L.QFX_EINVAL and up(None, 64, C.byref(ok), None) == L.QFX_EINVAL      # null p
    assert up(P, 64, None, None) == L.QFX_EINVAL and up(P, 0, None, None) == L.QFX_EINVAL                          # null a
    assert up(P, 64, C.byref(_args([S[0], None], [0.5, 0.5])), None) == L.QFX_EINVAL                               # null shadow below n_shadows
    assert up(P, 0, C.byref(_args([S[0], None], [0.5, 0.5], n_shadows=1)), None) == 0                              # ... above it: not read
    for ns in (0, -1, 5, 1 << 20):
        assert up(P, 64, C.byref(_args(S, [0.5] * 4, n_shadows=ns)), None) == L.QFX_EINVAL
    assert up(P, -1, C.byref(ok), None) == L.QFX_EINVAL and up(P, -(1 << 40), C.byref(ok), None) == L.QFX_EINVAL
    for omd in (-1e-6, 1.0001, 2.0, float("nan"), float("inf"), -float("inf")):
        assert up(P, 64, C.byref(_args(S[:2], [0.5, omd])), None) == L.QFX_EINVAL, omd
        assert up(P, 0, C.byref(_args(S[:1], [omd])), None) == L.QFX_EINVAL, omd
    assert up(P, 64, C.byref(_args([S[0], P], [0.5, 0.5])), None) == L.QFX_EINVAL                                  # a shadow equal to p
    assert up(P, 64, C.byref(_args([S[0], S[1], S[0]], [0.5] * 3)), None) == L.QFX_EINVAL                          # ... or to another shadow
    assert sw(P, S[0], 0, None) == 0
    assert sw(None, S[0], 64, None) == sw(P, None, 64, None) == sw(P, P, 64, None) == sw(P, S[0], -1, None) == L.QFX_EINVAL
    # the Python wrappers refuse before the library is asked
    from qflux_amd import ops
    t = torch.zeros(8)
    with pytest.raises(ValueError, match="1..4 shadows"):
        ops.ema_update(t, [], [])
    with pytest.raises(ValueError, match="1..4 shadows"):
        ops.ema_update(t, [t.clone()] * 5, [0.5] * 5)
    with pytest.raises(ValueError, match="p must be a contiguous float32 tensor"):
        ops.ema_update(t, [t.clone()], [0.5])


def test_train_step_constructor_refusals():
    from qflux_amd.trainer import FluxKontextTrainStep, QwenLoraTrainStep
    toy = toy_model()
    for cls in (QwenLoraTrainStep, FluxKontextTrainStep):
        for bad in (-0.1, 1.5, float("nan"), (0.9, 1.01)):
            with pytest.raises(ValueError, match=r"ema_decay must lie in \[0, 1\]"):
                cls(toy, ema_decay=bad)
        with pytest.raises(ValueError, match="1..4 decays"):
            cls(toy, ema_decay=(0.1, 0.2, 0.3, 0.4, 0.5))
        with pytest.raises(ValueError, match="1..4 decays"):
            cls(toy, ema_decay=())
        with pytest.raises(ValueError, match="adamw_schedulefree"):
            cls(toy, optimizer="adamw_schedulefree", ema_decay=0.999)
        with pytest.raises(ValueError, match="unknown .*decay_rate"):
            cls(toy, ema_decay=0.999, ema_args={"decay_rate": 1})
        with pytest.raises(ValueError, match="ema_args without ema_decay"):
            cls(toy, ema_args={"power": 0.75})
        step = cls(toy, ema_decay=(0.5, 0.9), ema_args={"update_after_step": 1})
        assert step.ema_decays == (0.5, 0.9) and step.ema_args["update_after_step"] == 1 and step.ema_args["power"] == 2 / 3
        assert step.ema is None and step.train_mode is True                           # nothing is allocated before the first use
        assert [n for n, _ in step._state_buffers()][-2:] == ["ema0", "ema1"]
        plain = cls(toy)
        assert plain.ema_decays is None and plain.ema is None and not any(n.startswith("ema") for n, _ in plain._state_buffers())
        assert cls(toy, ema_decay=0.999).ema_decays == (0.999,) and cls(toy, ema_decay=1).ema_decays == (1.0,)


def _plain_params(seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g) * 0.1) for s in ((4, 8), (12, 4), (5,), (1,))]


def test_stock_loop_class_on_plain_tensors_equals_the_restatement_bit_for_bit():
    from qflux_amd.ema import EMAModel
    params = _plain_params()
    kw = dict(decay=0.9, update_after_step=1, use_ema_warmup=True, inv_gamma=1.0, power=0.75)
    ema = EMAModel(params, **kw)
    assert ema._state is None                                                        # plain tensors: the per-tensor path
    ref = R.Ema(params, kw["decay"], **{n: v for n, v in kw.items() if n != "decay"})
    g = torch.Generator().manual_seed(9)
    decays = []
    for it in range(5):
        with torch.no_grad():
            for p in params:
                p.add_(torch.randn(p.shape, generator=g) * 0.01)
        ema.step(params)
        decays.append(ref.step(params))
        assert ema.optimization_step == it + 1 and ema.cur_decay_value == decays[-1]
        assert all(R.same_bits(a, b) for a, b in zip(ema.shadow_params, ref.shadow)), it
    assert decays[:2] == [0.0, 0.0] and 0 < decays[2] < decays[3] < decays[4] <= 0.9
    assert not any(torch.equal(s, p) for s, p in zip(ema.shadow_params, params))
    # store / copy_to / restore round trip
    trained = [p.detach().clone() for p in params]
    with pytest.raises(RuntimeError, match="no `store\\(\\)`ed weights"):
        ema.restore(params)
    ema.store(params)
    ema.copy_to(params)
    assert all(R.same_bits(p, s) for p, s in zip(params, ref.shadow))
    ema.restore(params)
    assert all(R.same_bits(p, t) for p, t in zip(params, trained)) and ema.temp_stored_params is None
    # state dict -> a new object -> same bits, same schedule
    sd = ema.state_dict()
    assert set(sd) == R.KEYS and sd["optimization_step"] == 5 and [t.shape for t in sd["shadow_params"]] == [p.shape for p in params]
    other = EMAModel(_plain_params(seed=4), decay=0.5)
    other.load_state_dict(sd)
    assert other.decay == 0.9 and other.optimization_step == 5 and other.power == 0.75 and other.use_ema_warmup is True
    ema.step(params); other.step(params); ref.step(params)
    assert all(R.same_bits(a, b) and R.same_bits(a, c) for a, b, c in zip(ema.shadow_params, other.shadow_params, ref.shadow))
    assert ema.to(device="cpu", dtype=torch.float32) is ema
    # a frozen parameter is copied, as in the package
    params[2].requires_grad_(False)
    ema.step(params)
    assert R.same_bits(ema.shadow_params[2], params[2]) and not R.same_bits(ema.shadow_params[0], params[0])
