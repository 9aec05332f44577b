"""CPU: max-norm regularisation of the adapters -- the restatement (tests/maxnorm_ref.py) against a literal transcription of kohya's
loop, the fp64 Gram identity against the direct product, pair discovery on tiny Qwen and FLUX models, the ABI of the two entry
points, their argument validation (no launch) and the train steps' constructor refusals."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest
import torch

import maxnorm_ref as R
from test_sgd_cpu import toy_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


def _random_pairs(seed, n=12):
    """n pairs of mixed shapes whose norms straddle 1.0 (about half above), scales of both signs."""
    g = torch.Generator().manual_seed(seed)
    shapes = [(1, 5, 3), (4, 64, 48), (16, 96, 40), (17, 100, 7), (8, 33, 65), (32, 48, 48)]
    pairs = []
    for i in range(n):
        r, nin, nout = shapes[i % len(shapes)]
        A, B = torch.randn(r, nin, generator=g), torch.randn(nout, r, generator=g)
        scale = (0.5, 2.0, -1.0)[i % 3]
        target = (0.3, 0.8, 1.3, 3.0)[i % 4]
        B = (B.double() * (target / float(R.norm_raw(A, B, scale)))).float()
        pairs.append((A, B, scale))
    return pairs


def test_restatement_against_the_literal_transcription():
    pairs = _random_pairs(1)
    ours, theirs = [(a.clone(), b.clone(), s) for a, b, s in pairs], [(a.clone(), b.clone(), s) for a, b, s in pairs]
    keys, mean, mx, norms, ratios, raw = R.apply(ours, 1.0)
    k_keys, k_mean, k_max = R.kohya_literal(theirs, 1.0)
    assert keys == k_keys and 0 < keys < len(pairs)
    assert all(abs(float(nr) - 1.0) > 1e-3 for nr in raw)                          # no decision hangs on the last bit
    assert R.ulps(mean, k_mean) <= 1 and R.ulps(mx, k_max) <= 1
    for (a, b, _), (ka, kb, _), (a0, b0, _), ratio in zip(ours, theirs, pairs, ratios):
        assert R.ulps(a.abs(), ka.abs()) <= 1 and R.ulps(b.abs(), kb.abs()) <= 1 and torch.equal(a.sign(), ka.sign())
        assert R.same_bits(a, a0) == R.same_bits(b, b0) == bool(ratio == 1)         # untouched exactly where the ratio is 1
    assert float(norms.max()) <= 1.0 * (1 + 1e-6)
    # measure only: nothing moves, the raw norms are reported
    free = [(a.clone(), b.clone(), s) for a, b, s in pairs]
    keys, mean, mx, norms, ratios, raw2 = R.apply(free, INF)
    assert keys == 0 and R.same_bits(norms, raw) and all(R.same_bits(a, a0) and R.same_bits(b, b0) for (a, b, _), (a0, b0, _) in zip(free, pairs))
    # B = 0 and a NaN: ratio 1, untouched, the NaN reported and kept by mean and max
    A = torch.randn(4, 8, generator=torch.Generator().manual_seed(2))
    bad = A.clone(); bad[1, 2] = NAN
    special = [(A.clone(), torch.zeros(6, 4), 1.0), (bad.clone(), torch.ones(6, 4), 1.0)]
    keys, mean, mx, norms, ratios, _ = R.apply(special, 0.5)
    assert keys == 0 and float(norms[0]) == 0.0 and math.isnan(float(norms[1])) and math.isnan(float(mean)) and math.isnan(float(mx))
    assert R.same_bits(special[0][0], A) and R.same_bits(special[1][0], bad) and ratios.tolist() == [1.0, 1.0]


@pytest.mark.parametrize("r,nin,nout", [(1, 5, 3), (4, 64, 48), (16, 256, 192), (17, 100, 7), (64, 300, 129), (16, 3072, 3072)])
def test_gram_identity_gives_the_norm_of_the_direct_product(r, nin, nout):
    g = torch.Generator().manual_seed(r * 1000 + nin)
    A, B = torch.randn(r, nin, generator=g) * 0.05, torch.randn(nout, r, generator=g) * 0.02
    want = R.norm_raw(A, B, 0.75)
    assert R.ulps(R.gram_norm(A, B, 0.75), want) <= 1 and R.ulps(R.gram_norm(A, B, 0.75, chunk=37), want) <= 1
    if r > 1:                                                                      # a rank-deficient B
        B[:, 1] = B[:, 0] * 0.5
        want = R.norm_raw(A, B, -2.0)
        assert R.ulps(R.gram_norm(A, B, -2.0), want) <= 1 and R.ulps(R.gram_norm(A, B, -2.0, chunk=37), want) <= 1


def _check_pairs(model, expect_n):
    from qflux_amd.modules import QfxLoraLinear
    from qflux_amd.regularize import adapter_pairs
    pairs = adapter_pairs(model)
    st = model.lora_store
    assert adapter_pairs(st) == pairs and len(pairs) == expect_n
    params = dict(model.named_parameters())
    mods = [(n, m) for n, m in model.named_modules() if isinstance(m, QfxLoraLinear)]
    assert [p[0] for p in pairs] == [n for n, _ in mods]
    offs = {n: off for n, _, off, _ in st.entries}
    for (name, off_a, off_b, r, nin, nout, scale), (_, m) in zip(pairs, mods):
        ad = m.active_adapter
        a, b = params[f"{name}.lora_A.{ad}.weight"], params[f"{name}.lora_B.{ad}.weight"]
        assert (off_a, off_b) == (offs[f"{name}.lora_A.{ad}.weight"], offs[f"{name}.lora_B.{ad}.weight"])
        assert tuple(a.shape) == (r, nin) and tuple(b.shape) == (nout, r) and (nin, nout) == (m.in_features, m.out_features)
        assert scale == m.lora_alpha[ad] / r
        assert a.data_ptr() == st.pflat.data_ptr() + 4 * off_a and b.data_ptr() == st.pflat.data_ptr() + 4 * off_b
    return pairs


@pytest.mark.parametrize("extra", [(), ("img_mod.1",)], ids=["default", "plus-img_mod"])
def test_pair_discovery_on_a_tiny_qwen_model(extra):
    from common import TINY
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.modules import LoraConfig
    m = QwenImageTransformer2DModel(**dict(TINY))
    cfg = LoraConfig(r=4, lora_alpha=6)
    names = m.add_adapter(LoraConfig(r=4, lora_alpha=6, target_modules=tuple(cfg.target_modules) + extra), "a")
    pairs = _check_pairs(m, len(names))
    assert sorted(p[0] for p in pairs) == sorted(names) and all(p[6] == 1.5 for p in pairs)
    assert bool(extra) == any(p[0].endswith("img_mod.1") for p in pairs)


@pytest.mark.parametrize("extra", [(), ("ff.net.2",)], ids=["default", "plus-ff"])
def test_pair_discovery_on_a_tiny_flux_model(extra):
    from common import FLUX_TINY
    from qflux_amd.models import FluxTransformer2DModel
    from qflux_amd.modules import LoraConfig
    m = FluxTransformer2DModel(**dict(FLUX_TINY))
    cfg = LoraConfig(r=4, lora_alpha=8)
    names = m.add_adapter(LoraConfig(r=4, lora_alpha=8, target_modules=tuple(cfg.target_modules) + extra), "a")
    pairs = _check_pairs(m, len(names))
    assert sorted(p[0] for p in pairs) == sorted(names) and all(p[6] == 2.0 for p in pairs)
    assert bool(extra) == any(p[0].endswith("ff.net.2") for p in pairs)


def test_state_names_rank_limit_and_rekeying():
    from qflux_amd.modules import QfxLinear, QfxLoraLinear
    from qflux_amd.regularize import MaxNorm, MaxNormState, ensure_state
    toy = toy_model()
    state = MaxNormState(toy)
    assert state.names == [f"transformer_blocks.{i}.{n}" for i in range(3) for n in ("to_q", "to_k")]
    assert state.layout.n_pairs == 6 and state.norms.shape == (6,) and state.ratios.shape == (6,) and state.summary.shape == (4,)
    assert ensure_state(state, toy) is state and ensure_state(state, toy.lora_store) is state
    bigger = toy_model(n_blocks=4)
    assert ensure_state(state, bigger) is not state
    toy.transformer_blocks[1].to_k = QfxLoraLinear(QfxLinear(200, 12), 129, 8, "ad")
    toy._store.rebuild("cpu")
    with pytest.raises(NotImplementedError, match=r"transformer_blocks\.1\.to_k.*rank 129"):
        MaxNormState(toy)
    with pytest.raises(NotImplementedError, match=r"transformer_blocks\.1\.to_k"):
        MaxNorm(toy, 1.0)
    for bad in (0.0, -1.0, NAN, None, "1"):
        with pytest.raises(ValueError, match="positive float or inf"):
            MaxNorm(toy_model(), bad)
    assert MaxNorm(toy_model(), INF).max_norm == INF and MaxNorm(toy_model(), 2).names == state.names


def _layout(struct, c_name, tmp_path):
    fields = [f for f, _ in struct._fields_]
    src = tmp_path / f"{c_name}.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qfx.h"\nint main(void) {\n  printf("%zu", sizeof(' + c_name + '));\n' +
                   "".join(f'  printf(" %zu", offsetof({c_name}, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / c_name
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(struct)] + [getattr(struct, f).offset for f in fields]
    return got


def test_abi_declarations_symbols_and_struct_layout(tmp_path):
    from qflux_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "qfx.h")).read()
    assert re.search(r"^int qfx_maxnorm_check_table\(const qfx_maxnorm_pair\* host_table, int32_t n_pairs, int64_t n_elems\);", hdr, flags=re.M)
    assert re.search(r"^int qfx_maxnorm_apply\(const qfx_maxnorm_args\* a, void\* stream\);", hdr, flags=re.M)
    assert "#define QFX_ABI_VERSION 7" in hdr and L.ABI_VERSION == 7 and L.lib.qfx_abi_version() == 7
    assert "qfx_maxnorm_check_table" in L.SYMBOLS and "qfx_maxnorm_apply" in L.SYMBOLS
    assert hasattr(L.lib, "qfx_maxnorm_check_table") and hasattr(L.lib, "qfx_maxnorm_apply")
    assert _layout(L.MaxnormPair, "qfx_maxnorm_pair", tmp_path) == [32, 0, 8, 16, 20, 24, 28]
    assert _layout(L.MaxnormArgs, "qfx_maxnorm_args", tmp_path) == [48, 0, 8, 16, 20, 24, 32, 40]


def _table(rows):
    from qflux_amd import _lib as L
    return (L.MaxnormPair * len(rows))(*[L.MaxnormPair(*r) for r in rows])


def test_table_validation_without_gpu():
    from qflux_amd import _lib as L
    from qflux_amd import ops
    chk = L.lib.qfx_maxnorm_check_table
    good = [(0, 64, 4, 16, 8, 2.0), (100, 132, 1, 5, 3, -0.5)]          # A [4,16] at 0, B [8,4] at 64; A [1,5] at 100, B [3,1] at 132
    assert chk(_table(good), 2, 135) == 0 and chk(_table(good), 2, 1 << 40) == 0 and chk(None, 0, 0) == 0
    assert chk(_table(good), 2, 134) == L.QFX_EINVAL                     # the last matrix reaches past n_elems
    assert chk(None, 2, 135) == chk(_table(good), -1, 135) == chk(_table(good), 2, -1) == L.QFX_EINVAL
    assert chk(_table([(0, 2048, 128, 16, 8, 1.0)]), 1, 4096) == 0       # the largest rank
    bad_rows = [(0, 64, 0, 16, 8, 1.0), (0, 64, -4, 16, 8, 1.0), (0, 4096, 129, 16, 8, 1.0),       # rank
                (0, 64, 4, 0, 8, 1.0), (0, 64, 4, 16, 0, 1.0), (0, 64, 4, -16, 8, 1.0), (0, 64, 4, 16, -8, 1.0),
                (0, 64, 1, (1 << 24) + 1, 8, 1.0), (0, 64, 1, 16, (1 << 24) + 1, 1.0),           # too large
                (-1, 64, 4, 16, 8, 1.0), (0, -64, 4, 16, 8, 1.0), (0, -(1 << 62), 4, 16, 8, 1.0),   # negative offsets
                (0, 63, 4, 16, 8, 1.0), (10, 0, 4, 16, 8, 1.0), (0, 0, 4, 16, 8, 1.0),               # A and B overlap
                ((1 << 62), 64, 4, 16, 8, 1.0),                                                    # far past n_elems
                (0, 64, 4, 16, 8, NAN), (0, 64, 4, 16, 8, INF), (0, 64, 4, 16, 8, -INF)]           # scale
    for row in bad_rows:
        assert chk(_table([row]), 1, 1 << 40) == L.QFX_EINVAL, row
        assert chk(_table([good[1], row]), 2, 1 << 40) == L.QFX_EINVAL, row
    # matrices of two pairs overlap
    assert chk(_table([good[0], (90, 60, 1, 5, 3, 1.0)]), 2, 1 << 20) == L.QFX_EINVAL
    assert chk(_table([good[0], (96, 200, 1, 5, 3, 1.0)]), 2, 1 << 20) == 0
    # the Python builder: refusals by name, the extent, the device table
    lay = ops.maxnorm_table(good)
    assert lay.n_pairs == 2 and lay.extent == 135 and lay.table.numel() == 64 and lay.table.dtype == torch.uint8
    with pytest.raises(ValueError, match="qfx_maxnorm_check_table"):
        ops.maxnorm_table(good, n_elems=134)
    with pytest.raises(ValueError, match="qfx_maxnorm_check_table"):
        ops.maxnorm_table([(0, 63, 4, 16, 8, 1.0)])
    with pytest.raises(NotImplementedError, match="rank 129"):
        ops.maxnorm_table([(0, 4096, 129, 16, 8, 1.0)])
    with pytest.raises(ValueError, match="no pairs"):
        ops.maxnorm_table([])
    t = torch.zeros(256)
    with pytest.raises(ValueError, match="max_norm must be positive"):
        ops.maxnorm_apply(t, lay, 0.0, t, t, t)
    with pytest.raises(ValueError, match="pflat must be a contiguous float32 tensor"):
        ops.maxnorm_apply(t, lay, 1.0, t, t, t)


def _args(p=0x10000, table=0x20000, n=3, m=1.0, norms=0x30000, ratios=0x40000, summary=0x50000):
    from qflux_amd import _lib as L
    return L.MaxnormArgs(p, table, n, m, norms, ratios, summary)


def test_apply_validation_without_gpu():
    """Every rejected argument returns QFX_EINVAL before any launch; n_pairs == 0 returns 0 without one.  The pointers are never
    dereferenced on these paths."""
    from qflux_amd import _lib as L
    ap = L.lib.qfx_maxnorm_apply
    assert ap(None, None) == L.QFX_EINVAL
    assert ap(C.byref(_args(n=0)), None) == 0 and ap(C.byref(_args(n=0, m=INF)), None) == 0
    assert ap(C.byref(_args(n=0, p=None, table=None, norms=None, ratios=None, summary=None)), None) == 0
    for name in ("p", "table", "norms", "ratios", "summary"):
        assert ap(C.byref(_args(**{name: None})), None) == L.QFX_EINVAL, name
    for n in (-1, -(1 << 31)):
        assert ap(C.byref(_args(n=n)), None) == L.QFX_EINVAL
    for m in (0.0, -0.0, -1.0, -INF, NAN):
        assert ap(C.byref(_args(m=m)), None) == L.QFX_EINVAL, m
        assert ap(C.byref(_args(m=m, n=0)), None) == L.QFX_EINVAL, m


def test_train_step_constructor_refusals():
    from qflux_amd.trainer import FluxKontextTrainStep, QwenLoraTrainStep
    toy = toy_model()
    for cls in (QwenLoraTrainStep, FluxKontextTrainStep):
        for bad in (0.0, -1.0, -INF, NAN, "2", True):
            with pytest.raises(ValueError, match="max_weight_norm must be a positive float or inf"):
                cls(toy, max_weight_norm=bad)
        with pytest.raises(ValueError, match="max_weight_norm with optimizer='adamw_schedulefree'"):
            cls(toy, optimizer="adamw_schedulefree", max_weight_norm=1.0)
        for fam in ("adamw", "adam8bit", "prodigy", "lion", "sgd", "muon", "adafactor"):
            kw = dict(lr=None) if fam == "adafactor" else {}
            assert cls(toy, optimizer=fam, max_weight_norm=2, **kw).max_weight_norm == 2.0
        step = cls(toy, max_weight_norm=INF, ema_decay=0.9)
        assert step.max_weight_norm == INF and step.last_weight_norms is None and step.weight_norm_stats() is None
        plain = cls(toy)
        assert plain.max_weight_norm is None and plain.last_weight_norms is None and plain.weight_norm_stats() is None
        assert [n for n, _ in step._state_buffers()] == [n for n, _ in cls(toy, ema_decay=0.9)._state_buffers()]      # no state
