"""CPU: the objective options of the train steps -- timestep densities, loss weighting and Huber thresholds against formulas written
out here, the steps' constructor refusals, the ABI of the general criterion entry and its argument validation (no launch)."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest
import torch

from test_sgd_cpu import toy_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_timestep_density_formulas_with_a_seeded_generator():
    from qflux_amd.schedules import timestep_density
    B = 64

    def gen():
        return torch.Generator().manual_seed(1234)

    u = torch.rand(size=(B,), generator=gen())
    for scheme in ("none", "sigma_sqrt", "cosmap"):
        assert torch.equal(timestep_density(scheme, B, generator=gen()), u), scheme
    z = torch.normal(mean=0.3, std=1.7, size=(B,), generator=gen())
    got = timestep_density("logit_normal", B, logit_mean=0.3, logit_std=1.7, generator=gen())
    assert torch.equal(got, 1 / (1 + torch.exp(-z))) or torch.allclose(got, 1 / (1 + torch.exp(-z)), rtol=0, atol=2 ** -23)
    assert got.min() > 0 and got.max() < 1 and abs(float(torch.logit(got.double()).mean()) - 0.3) < 1.0
    got = timestep_density("mode", B, mode_scale=1.29, generator=gen())
    want = torch.tensor([1 - x - 1.29 * (math.cos(math.pi * x / 2) ** 2 - 1 + x) for x in u.double().tolist()], dtype=torch.float64)
    assert got.dtype == torch.float32 and torch.allclose(got.double(), want, rtol=0, atol=1e-6)
    assert got.min() >= 0 and got.max() <= 1
    assert all(timestep_density(s, 3).shape == (3,) and timestep_density(s, 3).device.type == "cpu" for s in ("none", "logit_normal", "mode"))
    with pytest.raises(ValueError, match="weighting_scheme"):
        timestep_density("lognormal", 4)


def test_none_scheme_consumes_the_global_generator_like_torch_rand():
    """The default step draws what it drew before: same seed, same u, and the generator ends in the same state."""
    from qflux_amd.trainer import QwenLoraTrainStep
    step = QwenLoraTrainStep(toy_model())
    torch.manual_seed(77)
    u = torch.rand(size=(5,), device="cpu")
    after = torch.rand(3)
    torch.manual_seed(77)
    ts, sig = step.sample_timesteps(5)
    assert torch.equal(torch.rand(3), after)
    idx = (u * 1000).long()
    assert torch.equal(ts, step.timesteps_tbl[idx]) and torch.equal(sig, step.sigmas_tbl[idx])


def test_index_clamp_at_u_equal_one():
    from qflux_amd.trainer import QwenLoraTrainStep
    step = QwenLoraTrainStep(toy_model())
    ts, sig = step.sample_timesteps(3, u=torch.tensor([1.0, 0.9995, 0.0]))
    assert ts.tolist() == [1.0, 1.0, 1000.0] and torch.equal(sig, ts / 1000)
    # what makes the clamp necessary: the sigmoid of a far-out normal draw is 1.0 in fp32
    assert float(torch.sigmoid(torch.tensor(20.0))) == 1.0


def test_loss_weighting_and_huber_threshold_values():
    from qflux_amd.schedules import huber_threshold, loss_weighting
    sig = torch.tensor([0.001, 0.5, 1.0])
    w = loss_weighting("sigma_sqrt", sig)
    assert w.dtype == torch.float32 and torch.allclose(w.double(), torch.tensor([1e6, 4.0, 1.0], dtype=torch.float64), rtol=1e-6)
    w = loss_weighting("cosmap", sig)
    want = [2 / (math.pi * (1 - 2 * s + 2 * s * s)) for s in (0.001, 0.5, 1.0)]      # 0.6379..., 4 / pi, 2 / pi
    assert w.dtype == torch.float32 and torch.allclose(w.double(), torch.tensor(want, dtype=torch.float64), rtol=1e-6)
    assert abs(want[1] - 4 / math.pi) < 1e-15 and abs(want[2] - 2 / math.pi) < 1e-15
    for scheme in ("none", "logit_normal", "mode"):
        assert torch.equal(loss_weighting(scheme, sig), torch.ones(3))
    ts = sig * 1000
    c = huber_threshold("constant", 0.1, ts)
    assert c.dtype == torch.float32 and torch.equal(c, torch.full((3,), 0.1))
    c = huber_threshold("exponential", 0.1, ts)
    want = torch.tensor([0.1 ** 0.001, 0.1 ** 0.5, 0.1], dtype=torch.float64).float()
    assert c.dtype == torch.float32 and torch.equal(c, want)
    with pytest.raises(ValueError, match="huber_schedule"):
        huber_threshold("snr", 0.1, ts)


def test_shifted_tables_and_flux_time_shift():
    from qflux_amd.schedules import flowmatch_tables, shift_time
    from qflux_amd.trainer import QwenLoraTrainStep
    step = QwenLoraTrainStep(toy_model(), timestep_shift=3.0)
    ts, sig = flowmatch_tables(shift=3)
    assert torch.equal(step.timesteps_tbl, ts) and torch.equal(step.sigmas_tbl, sig)
    plain = QwenLoraTrainStep(toy_model())
    assert torch.equal(plain.sigmas_tbl, flowmatch_tables()[1]) and not torch.equal(plain.sigmas_tbl, sig)
    u = torch.tensor([0.0, 0.25, 0.5, 1.0])
    assert shift_time(u, 1.0) is u
    assert torch.allclose(shift_time(u, 3.0), torch.tensor([0.0, 0.5, 0.75, 1.0]), rtol=0, atol=1e-7)


def test_staged_objective_follows_the_injected_u():
    """Weighting and threshold follow from the (injected) timesteps; unit weights with l2 stage nothing (the MSE kernels' path)."""
    from qflux_amd.schedules import huber_threshold, loss_weighting
    from qflux_amd.trainer import QwenLoraTrainStep
    toy = toy_model()
    u = torch.tensor([0.7109, 0.1611])
    for kw in ({}, {"weighting_scheme": "logit_normal"}, {"weighting_scheme": "mode", "timestep_shift": 2.0}):
        s = QwenLoraTrainStep(toy, **kw)
        assert s._stage_objective(*s.sample_timesteps(2, u), "cpu") is None and s.last_sample_losses is None
    s = QwenLoraTrainStep(toy, weighting_scheme="cosmap", timestep_shift=3.0)
    ts, sig = s.sample_timesteps(2, u)
    sw, hc = s._stage_objective(ts, sig, "cpu")
    assert hc is None and torch.equal(sw, loss_weighting("cosmap", s.sigmas_tbl[(u * 1000).long()]))
    s = QwenLoraTrainStep(toy, weighting_scheme="logit_normal", loss_type="huber", huber_c=0.2, huber_schedule="exponential")
    ts, sig = s.sample_timesteps(2, u)
    sw, hc = s._stage_objective(ts, sig, "cpu")
    assert sw is None and torch.equal(hc, huber_threshold("exponential", 0.2, ts)) and hc.dtype == torch.float32
    assert torch.all(hc > 0) and torch.all(torch.isfinite(hc))


def test_constructor_refusals_and_defaults():
    from qflux_amd.trainer import FluxKontextTrainStep, QwenLoraTrainStep
    toy = toy_model()
    for cls in (QwenLoraTrainStep, FluxKontextTrainStep):
        s = cls(toy)
        assert (s.weighting_scheme, s.logit_mean, s.logit_std, s.mode_scale, s.timestep_shift, s.loss_type, s.huber_c,
                s.huber_schedule) == ("none", 0.0, 1.0, 1.29, 1.0, "l2", 0.1, "constant")
        for bad in (dict(weighting_scheme="lognormal"), dict(loss_type="l1"), dict(huber_schedule="snr"), dict(huber_c=0.0),
                    dict(huber_c=-1.0), dict(huber_c=float("nan")), dict(huber_c=float("inf")), dict(timestep_shift=0.0),
                    dict(timestep_shift=-2.0), dict(timestep_shift=float("nan"))):
            with pytest.raises(ValueError, match=next(iter(bad))):
                cls(toy, **bad)
        for scheme in ("none", "logit_normal", "mode", "sigma_sqrt", "cosmap"):
            for lt in ("l2", "huber", "smooth_l1"):
                s = cls(toy, weighting_scheme=scheme, loss_type=lt, huber_schedule="exponential")
                assert s._general_objective == (scheme in ("sigma_sqrt", "cosmap") or lt != "l2")


def test_header_declares_and_lib_binds_the_entries():
    from qflux_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "qfx.h")).read()
    assert re.search(r"^int64_t\s+qfx_criterion_workspace_bytes\s*\(", hdr, flags=re.M)
    assert re.search(r"^int\s+qfx_criterion_fwd_bwd\s*\(const qfx_criterion_args\* a, void\* stream\);", hdr, flags=re.M)
    for name, val in (("QFX_LOSS_L2", 0), ("QFX_LOSS_HUBER", 1), ("QFX_LOSS_SMOOTH_L1", 2)):
        assert re.search(rf"^#define {name} {val}$", hdr, flags=re.M)
    assert (_lib.LOSS_L2, _lib.LOSS_HUBER, _lib.LOSS_SMOOTH_L1) == (0, 1, 2)
    for name in ("qfx_criterion_workspace_bytes", "qfx_criterion_fwd_bwd"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib, name)
    assert _lib.lib.qfx_abi_version() == _lib.ABI_VERSION == 7 and re.search(r"^#define QFX_ABI_VERSION 7$", hdr, flags=re.M)
    # the three older criterion entries are still declared as they were
    for name in ("qfx_mse_loss_fwd_bwd", "qfx_mse_token_weighted_fwd_bwd", "qfx_flowmatch_prepare"):
        assert name in _lib.SYMBOLS and re.search(rf"^int {name}\(", hdr, flags=re.M)


def test_ctypes_struct_matches_the_header_layout(tmp_path):
    """As tests/test_abi_cpu.py does for the older argument structs: sizeof and every field offset through gcc."""
    from qflux_amd import _lib as L
    ct = L.CriterionArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "qfx.h"', "int main(void) {",
             '  printf("%zu", sizeof(qfx_criterion_args));']
    lines += [f'  printf(" %zu", offsetof(qfx_criterion_args, {f}));' for f, _ in ct._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(ct)] + [getattr(ct, f).offset for f, _ in ct._fields_]
    hdr = open(os.path.join(ROOT, "include", "qfx.h")).read()
    body = re.search(r"typedef struct qfx_criterion_args \{(.*?)\} qfx_criterion_args;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f for f, _ in ct._fields_]


def _valid_args():
    from qflux_amd import _lib as L
    a = L.CriterionArgs()
    a.pred, a.target, a.loss, a.workspace, a.huber_c = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    a.B, a.S_all, a.S_t, a.C, a.kind, a.inv_denom, a.gscale = 2, 70, 37, 64, L.LOSS_HUBER, 1.0 / 74, 1.0
    a.workspace_bytes = L.lib.qfx_criterion_workspace_bytes(2, 37, 64)
    return a


def test_argument_validation_without_gpu():
    """Every refusal of the header returns QFX_EINVAL before any launch: the pointers are never dereferenced."""
    from qflux_amd import _lib as L
    f, ws = L.lib.qfx_criterion_fwd_bwd, L.lib.qfx_criterion_workspace_bytes
    assert f(None, None) == L.QFX_EINVAL
    for field in ("pred", "target", "loss", "workspace"):
        a = _valid_args()
        setattr(a, field, None)
        assert f(C.byref(a), None) == L.QFX_EINVAL, field
    for field in ("B", "S_all", "S_t", "C"):
        for bad in (0, -3):
            a = _valid_args()
            setattr(a, field, bad)
            assert f(C.byref(a), None) == L.QFX_EINVAL, (field, bad)
    a = _valid_args()
    a.S_t = a.S_all + 1
    a.workspace_bytes = 1 << 20
    assert f(C.byref(a), None) == L.QFX_EINVAL
    for bad in (-1, 3, 17):
        a = _valid_args()
        a.kind = bad
        assert f(C.byref(a), None) == L.QFX_EINVAL, bad
    for kind in (L.LOSS_HUBER, L.LOSS_SMOOTH_L1):
        a = _valid_args()
        a.kind, a.huber_c = kind, None
        assert f(C.byref(a), None) == L.QFX_EINVAL, kind
    a = _valid_args()
    a.workspace_bytes -= 1
    assert f(C.byref(a), None) == L.QFX_EINVAL
    # the workspace query: one fp64 partial per sample and chunk of ~2048 elements' whole rows below S_t; 0 for a bad dimension
    assert ws(2, 37, 64) == 2 * 2 * 8 and ws(1, 4096, 64) == 128 * 8 and ws(1, 1, 8) == 8 and ws(2, 5, 12) == 2 * 8
    assert ws(3, 257, 64) == 3 * 9 * 8 and ws(1, 5, 4096) == 5 * 8 and ws(1, 5, 1) == 8
    assert ws(0, 4, 4) == 0 and ws(1, 0, 4) == 0 and ws(1, 4, -1) == 0
    assert L.QFX_EINVAL == -1


def test_ops_wrapper_refuses_on_the_host():
    from qflux_amd import ops
    pred = torch.zeros(1, 2, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="kind"):
        ops.criterion_fwd_bwd(pred, pred, 2, kind="l1")
    with pytest.raises(ValueError, match="huber_c"):
        ops.criterion_fwd_bwd(pred, pred, 2, kind="huber")
    assert ops.LOSS_KINDS == {"l2": 0, "huber": 1, "smooth_l1": 2}
