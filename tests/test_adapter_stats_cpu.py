"""CPU: per-adapter telemetry (qfx_adapter_stats, qflux_amd.telemetry) without a device -- the restatement's kernel-order fp32
sums against its fp64 truth, the descriptor table of a LoraStore, the C ABI's refusals, the train steps' launch list with the
option off and on (models built in host memory by the dry run of tools/plan_fingerprint.py, launches recorded, none made) and
the host arithmetic of the summary."""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapter_stats_ref as R  # noqa: E402
from parity_util import ROOT  # noqa: E402

NUMELS = (1, 63, 64, 65, 255, 256, 257, 1024, 4097, 16 * 3072)


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("numel", NUMELS)
def test_kernel_order_sum_is_within_the_derived_bound_of_the_fp64_sum(numel):
    x = R.make_tensor(numel, seed=numel)
    got, want = float(R.ordered_sumsq(x)), R.sumsq64(x)
    print(f"numel {numel}: |ordered - fp64| = {abs(got - want):.3e}, bound {R.bound(numel, want):.3e}")
    assert want > 0 and abs(got - want) <= R.bound(numel, want)
    y = R.make_tensor(numel, seed=numel + 7, scale=1e-3)
    d32, d64 = float(R.ordered_sumsq((x - y).astype(np.float32))), R.sumsq64(x.astype(np.float64) - y.astype(np.float64))
    assert abs(d32 - d64) <= R.bound(numel, d64, update=True)


def test_kernel_order_is_what_the_docstring_says():
    """Written out by hand for 600 elements: three terms down lanes 0..87, two down the others, the tree, the wave fold."""
    x = R.make_tensor(600, seed=3)
    f = np.float32
    lanes = []
    for lane in range(256):
        acc = f(0)
        for i in range(lane, 600, 256):
            acc = f(acc + f(x[i] * x[i]))
        lanes.append(acc)
    waves = []
    for w in range(4):
        v = list(lanes[64 * w:64 * w + 64])
        for o in (32, 16, 8, 4, 2, 1):
            v = [f(v[l] + v[l ^ o]) for l in range(64)]
        waves.append(v[0])
    want = f(f(waves[0] + waves[1]) + f(waves[2] + waves[3]))
    assert R.ordered_sumsq(x) == want
    # non-finite elements add nothing and are counted; the maximum passes over them
    g = x.copy()
    g[5], g[300] = np.nan, np.inf
    r0 = R.phase0(g, 0, 600, np.float32(1.0))
    keep = np.delete(x, [5, 300])
    assert r0["grad_nonfinite"] == 2 and r0["grad_sq"] == R.sumsq64(keep) and r0["grad_absmax"] == float(np.abs(keep).max())
    assert R.phase0(g, -4, 600, 1.0) == dict(grad_sq=0.0, grad_absmax=0.0, grad_nonfinite=0)
    assert R.phase1(g, g, 0, 0) == dict(weight_sq=0.0, update_sq=0.0, weight_nonfinite=0)


def test_clip_factor_restates_the_optimizers_prologue():
    assert R.clip_factor(None, 1.0, 1.0) == np.float32(1.0) and R.clip_factor(9.0, 0.0, 0.5) == np.float32(0.5)
    c = R.clip_factor(16.0, 1.0, 0.5)      # norm 4 * 0.5 = 2 -> 0.5 * 1 / (2 + 1e-6)
    assert c == np.float32(np.float32(0.5) * np.float32(np.float32(1.0) / np.float32(np.float32(2.0) + np.float32(1e-6))))
    assert R.clip_factor(0.01, 1.0, 1.0) == np.float32(1.0)      # below the threshold: no clip


# ---------------------------------------------------------------- the descriptor table
@pytest.fixture(scope="module")
def pf():
    from tools import plan_fingerprint
    return plan_fingerprint


def test_stats_table_follows_the_store_and_names_tensors_as_the_weights_file_does(pf):
    import ctypes as C
    from qflux_amd import _lib as L
    from qflux_amd import ops
    from qflux_amd.lora_io import get_lora_state_dict
    with pf.dry_run():
        m = pf._qwen(targets=pf.FF)
        st = m.lora_store
        lay = ops.stats_table(st)
        params = st.params()
        assert lay.n_entries == len(params) == len(st.entries) and lay.table.numel() == 16 * lay.n_entries
        rows = (L.StatsEntry * lay.n_entries).from_buffer_copy(lay.table.numpy().tobytes())
        covered = np.zeros(st.pflat.numel(), bool)
        for (n, p), r, (off, k), kind in zip(params, rows, lay.entries, lay.kinds):
            assert (r.off, r.numel, r.pad) == (off, k, 0) and off % 64 == 0 and k == p.numel()
            assert p.data_ptr() == st.pflat.data_ptr() + 4 * off
            assert kind == ("A" if "lora_A" in n else "B")
            assert not covered[off:off + k].any()
            covered[off:off + k] = True
        # padding is never counted: exactly the parameters' elements are covered
        assert covered.sum() == sum(p.numel() for _, p in params)
        assert lay.extent == max(off + k for off, k in lay.entries) <= st.pflat.numel()
        sd = get_lora_state_dict(m)            # what save_lora_weights writes
        assert set(lay.names) == set(sd) and len(set(lay.names)) == lay.n_entries
        for name, (off, k), kind in zip(lay.names, lay.entries, lay.kinds):
            assert sd[name].numel() == k
            assert (".lora.down." in name or ".lora_A." in name) == (kind == "A")
        assert any(".lora.down.weight" in n for n in lay.names) and any(".lora_A.weight" in n for n in lay.names)


def test_raw_table_keeps_skipped_entries_out_of_the_extent():
    from qflux_amd import ops
    lay = ops.stats_table_entries([(128, 65), (0, 0), (-64, 10), (0, 63)])
    assert lay.extent == 193 and lay.n_entries == 4 and lay.names == ["entry0", "entry1", "entry2", "entry3"]
    with pytest.raises(ValueError):
        ops.stats_table_entries([])
    with pytest.raises(ValueError):
        ops.stats_table_entries([(0, 1 << 31)])


# ---------------------------------------------------------------- C ABI
def test_symbol_struct_sizes_and_refusals_without_a_device():
    import ctypes as C
    from qflux_amd import _lib as L
    assert L.ABI_VERSION == 7 and L.lib.qfx_abi_version() == 7 and "qfx_adapter_stats" in L.SYMBOLS      # appended: the version stays
    assert hasattr(L.lib, "qfx_adapter_stats")
    assert C.sizeof(L.StatsEntry) == 16 and C.sizeof(L.StatsRow) == 32
    assert [getattr(L.StatsRow, f).offset for f, _ in L.StatsRow._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]
    f = L.lib.qfx_adapter_stats
    ok = dict(p=0x1000, g=0x2000, prev=0x3000, table=0x4000, n=3, out=0x5000, phase=0, gnorm=None, max_norm=1.0, grad_scale=1.0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["p"], a["g"], a["prev"], a["table"], a["n"], a["out"], a["phase"], a["gnorm"], a["max_norm"], a["grad_scale"], None)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(p=None), dict(table=None), dict(out=None), dict(g=None), dict(prev=None), dict(prev=None, phase=1),
                dict(p=None, phase=1), dict(n=0), dict(n=-2), dict(phase=2), dict(phase=-1), dict(max_norm=-1.0), dict(max_norm=nan),
                dict(grad_scale=nan), dict(grad_scale=inf), dict(grad_scale=-inf)):
        assert call(**bad) == L.QFX_EINVAL, bad
    from qflux_amd import ops
    assert ops.STATS_ROW_FIELDS == ("grad_sq", "weight_sq", "update_sq", "grad_absmax", "grad_nonfinite", "weight_nonfinite", "r0", "r1")
    assert np.dtype(ops.STATS_ROW_DTYPE).itemsize == 32


def test_new_source_is_built_without_fma_contraction():
    import __graft_entry__ as g
    assert "qfx_adapter_stats.hip" in g.PLAIN_SOURCES and g.EXTRA_FLAGS["qfx_adapter_stats.hip"] == ["-ffp-contract=off"]
    assert os.path.exists(os.path.join(g.CSRC, "qfx_adapter_stats.hip"))


# ---------------------------------------------------------------- the train steps
class _Recorder:
    """Stands in for the loaded library: every qfx_ entry is recorded by name and reports success; nothing is launched."""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        if name.startswith("qfx_"):
            def entry(*args):
                self._log.append(name)
                return 0
            return entry
        return getattr(self._real, name)


def _recorded_steps(pf, monkeypatch, make, n_steps):
    """The library entries each of n_steps optimizer_step() calls reaches, models and buffers in host memory."""
    from qflux_amd import ops
    log = []
    monkeypatch.setenv("QFX_MOD_TABLE", "0")
    monkeypatch.setattr(ops, "lib", _Recorder(ops.lib, log))
    monkeypatch.setattr(ops, "stream_ptr", lambda: 0)
    monkeypatch.setattr(ops, "adapter_stats", lambda p, g, prev, table, out, phase, *a, **k: log.append(f"qfx_adapter_stats:{phase}"))
    out = []
    with pf.dry_run():
        m = pf._qwen()
        m.lora_store
        step = make(m)
        for _ in range(n_steps):
            del log[:]
            step.optimizer_step()
            out.append(list(log))
    return step, out


TODAY = ["qfx_sumsq_det", "qfx_adamw_step"]      # the optimizer-side launches of a step, as the parent emits them


def test_with_the_option_off_a_step_launches_what_it_launched_before(pf, monkeypatch):
    from qflux_amd.trainer import QwenLoraTrainStep
    step, calls = _recorded_steps(pf, monkeypatch, lambda m: QwenLoraTrainStep(m), 2)
    assert calls == [TODAY, TODAY]
    assert step.adapter_stats_every == 0 and step._adapter_stats is None
    assert step.last_adapter_stats is None and step.adapter_stats_summary() is None
    # the forward / backward programs are not touched by the option at all: the committed digest, with the option on
    with open(os.path.join(ROOT, "tests", "golden", "plan_fingerprints.json")) as f:
        recorded = json.load(f)["sha256"]
    with pf.dry_run():
        m = pf._qwen()
        QwenLoraTrainStep(m, adapter_stats_every=1)
        assert pf.digest(pf.fingerprint(pf._qwen_plan(m))) == recorded["qwen_attn"]


def test_with_the_option_on_the_two_launches_bracket_the_optimizer_on_every_nth_step(pf, monkeypatch):
    from qflux_amd.trainer import FluxKontextTrainStep, QwenLoraTrainStep
    on = ["qfx_sumsq_det", "qfx_adapter_stats:0", "qfx_adamw_step", "qfx_adapter_stats:1"]
    step, calls = _recorded_steps(pf, monkeypatch, lambda m: QwenLoraTrainStep(m, adapter_stats_every=2), 4)
    assert calls == [TODAY, on, TODAY, on]
    assert step._adapter_stats.collected == 2 and step._adapter_stats.prev.shape == step.dit.lora_store.pflat.shape
    _, calls = _recorded_steps(pf, monkeypatch, lambda m: FluxKontextTrainStep(m, adapter_stats_every=1, optimizer="sgd"), 1)
    assert calls == [["qfx_sumsq_det", "qfx_adapter_stats:0", "qfx_sgd_step", "qfx_adapter_stats:1"]]
    for bad in (-1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="adapter_stats_every"):
            QwenLoraTrainStep(step.dit, adapter_stats_every=bad)


def test_capture_graph_refuses_the_option_by_name(pf, monkeypatch):
    from qflux_amd.trainer import QwenLoraTrainStep
    monkeypatch.setenv("QFX_MOD_TABLE", "0")
    with pf.dry_run():
        m = pf._qwen()
        m.lora_store
        step = QwenLoraTrainStep(m, adapter_stats_every=3)
        with pytest.raises(NotImplementedError, match="adapter_stats_every"):
            step.capture_graph({})


def test_after_step_needs_a_before_step(pf, monkeypatch):
    from qflux_amd import ops
    from qflux_amd.telemetry import AdapterStats
    monkeypatch.setattr(ops, "adapter_stats", lambda *a, **k: None)
    with pf.dry_run():
        m = pf._qwen()
        s = AdapterStats(m)
        assert s.read() is None and s.summary() is None
        with pytest.raises(RuntimeError, match="before_step"):
            s.after_step()
        s.before_step()
        s.after_step()
        assert s.collected == 1 and set(s.read()) == set(s.names)
        with pytest.raises(ValueError):
            AdapterStats.from_optimizer(object())


# ---------------------------------------------------------------- host arithmetic
def test_summary_arithmetic_on_hand_made_rows():
    from qflux_amd import ops
    from qflux_amd.telemetry import rows_to_dict, summarize
    rows = np.zeros(6, dtype=np.dtype(ops.STATS_ROW_DTYPE))
    names = ["a0.lora.down.weight", "a0.lora.up.weight", "a1.lora_A.weight", "a1.lora_B.weight", "a2.lora_A.weight", "a2.lora_B.weight"]
    kinds = ["A", "B", "A", "B", "A", "B"]
    #            grad_sq weight_sq update_sq absmax gbad wbad
    vals = [(9.0, 4.0, 1.0, 2.0, 0, 0),        # A: ratio 1 / 2
            (16.0, 0.0, 0.0, 3.0, 0, 0),       # B: zero weight -> ratio 0
            (0.0, 16.0, 1.0, 0.0, 0, 1),       # A: ratio 1 / 4
            (144.0, 25.0, 4.0, 7.0, 2, 0),     # B: ratio 2 / 5, the first non-finite gradient
            (0.0, 1.0, 0.0625, 0.0, 1, 0),     # A: ratio 1 / 4
            (0.0, 100.0, 9.0, 0.0, 0, 0)]      # B: ratio 3 / 10
    for r, v in zip(rows, vals):
        r["grad_sq"], r["weight_sq"], r["update_sq"], r["grad_absmax"], r["grad_nonfinite"], r["weight_nonfinite"] = v
    d = rows_to_dict(rows, names)
    assert list(d) == names
    assert d[names[0]] == dict(grad_norm=3.0, weight_norm=2.0, update_norm=1.0, update_ratio=0.5, grad_absmax=2.0, grad_nonfinite=0,
                               weight_nonfinite=0)
    assert d[names[1]]["update_ratio"] == 0.0 and d[names[1]]["weight_norm"] == 0.0
    assert d[names[2]]["weight_nonfinite"] == 1 and isinstance(d[names[3]]["grad_nonfinite"], int)
    s = summarize(d, kinds)
    assert s["grad_norm"] == 13.0                                            # sqrt(9 + 16 + 144)
    assert (s["update_ratio_max_A"], s["update_ratio_median_A"]) == (0.5, 0.25)
    assert (s["update_ratio_max_B"], s["update_ratio_median_B"]) == (0.4, 0.3)
    assert s["first_nonfinite_grad"] == names[3]
    clean = {n: dict(v, grad_nonfinite=0) for n, v in d.items()}
    assert summarize(clean, kinds)["first_nonfinite_grad"] is None
    # an even count: the median is the mean of the two middle ratios; no tensor of a kind: None
    s4 = summarize({n: d[n] for n in names[:4]}, ["A", "A", "A", "A"])
    assert s4["update_ratio_median_A"] == 0.5 * (0.25 + 0.4) and s4["update_ratio_max_B"] is None and s4["update_ratio_median_B"] is None
    # host reductions run in fp64: a squared norm that fp32 holds exactly keeps its fp64 root
    rows[0]["grad_sq"] = np.float32(2.0)
    assert rows_to_dict(rows[:1], names[:1])[names[0]]["grad_norm"] == math.sqrt(2.0)
