"""CPU: the fused RAdam / NAdam / Adamax families without a device -- the yardstick tests/adamx_ref.py against the real
torch.optim.RAdam / NAdam / Adamax in fp64, class_path resolution, defaults and refusals, torch's state-dict layout and its round trip
through torch.optim.*.load_state_dict, the group map, the ctypes mirror of the header and the refusals of qfx_adamx_step."""
import ctypes as C
import inspect
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adamx_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = ["to_q", "to_k", "to_v", "to_out.0", "img_mlp.net.2", "txt_mod.1"]
F32, F64 = np.float32, np.float64
T = 10
# every option of the issue: RAdam's decoupled_weight_decay, NAdam's momentum_decay and decoupled_weight_decay, Adamax (L2 only)
OPTIONS = {
    "radam": [dict(weight_decay=0.0), dict(weight_decay=0.0625), dict(weight_decay=0.0625, decoupled_weight_decay=True)],
    "nadam": [dict(weight_decay=0.0), dict(weight_decay=0.0625, momentum_decay=0.0), dict(weight_decay=0.0625, decoupled_weight_decay=True),
              dict(weight_decay=0.0, momentum_decay=0.05)],
    "adamax": [dict(weight_decay=0.0), dict(weight_decay=0.0625)],
}
BETAS = [(0.9, 0.999), (0.5, 0.9)]      # beta1 = 0.5: the other branch of lerp_; with either beta2 RAdam is rectified from step 6 on


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from qflux_amd import _lib
    return _lib


def int_data(n, seed, steps):
    """Small integers scaled by powers of two: p in [-32, 32] / 16, g[t] in [-64, 64] / 2^(4 + t % 3)."""
    rng = np.random.default_rng(seed)
    p = rng.integers(-32, 33, n).astype(F64) / 16
    g = [rng.integers(-64, 65, n).astype(F64) / 2 ** (4 + t % 3) for t in range(steps)]
    return p, g


def torch_run(family, p, grads, hp, dtype=torch.float64):
    """The real torch.optim class (single-tensor path) on one tensor: (param, state) as numpy."""
    q = torch.nn.Parameter(torch.tensor(p, dtype=dtype))
    kw = dict(hp)
    opt = getattr(torch.optim, R.TORCH[family])([q], lr=kw.pop("lr"), betas=(kw.pop("beta1"), kw.pop("beta2")), foreach=False, **kw)
    for g in grads:
        q.grad = torch.tensor(g, dtype=dtype)
        opt.step()
    st = {k: (v.numpy() if v.ndim else float(v)) for k, v in opt.state[q].items()}
    return q.detach().numpy(), st


def roundoff_bounds(p, grads, hp, steps):
    """Two evaluations of the same real-number recurrence in double, each rounding at most 16 operations per element and step
    (weight decay 2, lerp 3, second state 4, update 7), differ by at most steps * 32 * 2^-53 of the magnitudes involved, to
    first order: exp_avg is a convex combination of gradients (max |g'|), exp_avg_sq of their squares, and the parameter moves per
    step by at most lr * A with A = 1 / ((1 - beta1) sqrt(1 - beta2)) -- 1 / bias_correction1 <= 1 / (1 - beta1), |exp_avg| /
    sqrt(exp_avg_sq) <= 1 / sqrt(1 - beta2), the rectification, sqrt(bias_correction2), exp_avg / exp_inf and NAdam's two
    coefficients over lr / (1 - beta1) are all <= 1 -- which is also the factor a relative error of the states is amplified by."""
    u = 2.0 ** -53
    A = 1.0 / ((1.0 - hp["beta1"]) * np.sqrt(1.0 - hp["beta2"]))
    pmax = np.abs(p).max() + steps * hp["lr"] * A
    gmax = max(np.abs(g).max() for g in grads) + hp["weight_decay"] * pmax
    k = steps * 32 * u
    return {"p": k * A * pmax, "exp_avg": k * gmax, "second": k * max(gmax * gmax, gmax + hp["eps"])}


@pytest.mark.parametrize("family", list(OPTIONS))
def test_restatement_is_torch_in_fp64_over_ten_steps(family):
    worst = 0.0
    for (b1, b2), opt, eps in itertools.product(BETAS, OPTIONS[family], (1e-8, 0.25)):
        hp = dict(lr=0.0625, beta1=b1, beta2=b2, eps=eps, **opt)
        p, grads = int_data(257, 11, T)
        want_p, want = torch_run(family, p, grads, hp)
        got_p, got = R.run(family, p, grads, hp)
        bound = roundoff_bounds(p, grads, hp, T)
        assert got["step"] == want["step"] == T
        for name, a, b in (("p", got_p, want_p), ("exp_avg", got["exp_avg"], want["exp_avg"]),
                           ("second", got[R.SECOND[family]], want[R.SECOND[family]])):
            err = np.abs(a - b).max()
            worst = max(worst, err / bound[name])
            assert err <= bound[name], (family, hp, name, err, bound[name])
        if family == "nadam":
            assert got["mu_product"] == want["mu_product"], hp      # one fp32 rounding per step on both sides
    assert worst > 0 or family == "adamax"      # the bound is not vacuous: torch's fused multiply-adds do round differently


def exact_case(family, n=300, seed=2, option=0):
    """One step whose every operation is exact in fp32 (and so in fp64): p = odd integers / 8, g = +-2^k, beta1 = 0.5, beta2 = 0.75,
    lr = 2^-3, eps = 0, weight decay 0.5 or none.  RAdam is not rectified at step 1 (rho_1 = 1); NAdam with momentum_decay = 0 and
    beta1 = 0 has mu = 0 (c_grad = -lr, c_avg = 0) and sqrt(exp_avg_sq / bias_correction2) = |g|; Adamax divides g / 2 by |g|."""
    rng = np.random.default_rng(seed)
    p = (2 * rng.integers(-16, 16, n) + 1).astype(F64) / 8      # odd / 8: g + p / 2 is never 0, which eps = 0 could not divide by
    g = rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-2, 3, n)
    hp = dict(lr=0.125, beta1=0.5, beta2=0.75, eps=0.0, weight_decay=0.0)
    if family == "nadam":
        hp.update(beta1=0.0, momentum_decay=0.0)
    if option == 1 and family != "nadam":       # L2: g' = g + p / 2 is no power of two any more, which NAdam's square root needs
        hp["weight_decay"] = 0.5
    if option == 2 and family != "adamax":
        hp.update(weight_decay=0.5, decoupled_weight_decay=True)
    return p, [g], hp


@pytest.mark.parametrize("family,option", [(f, o) for f in OPTIONS for o in range(3)])
def test_exact_step_is_the_same_number_in_fp64_torch_fp64_and_torch_fp32(family, option):
    p, grads, hp = exact_case(family, option=option)
    got_p, got = R.run(family, p, grads, hp)
    for dtype in (torch.float64, torch.float32):
        want_p, want = torch_run(family, p, grads, hp, dtype)
        assert np.array_equal(got_p, want_p.astype(F64)), (family, hp, dtype)
        assert np.array_equal(got["exp_avg"], want["exp_avg"].astype(F64))
        assert np.array_equal(got[R.SECOND[family]], want[R.SECOND[family]].astype(F64))
    assert np.abs(got_p - p).max() > 0


def test_radam_crosses_the_rectification_switch_between_steps_five_and_six(lib):
    from qflux_amd import ops
    for b2 in (0.999, 0.9):
        flags = [ops.radam_scalars(t, 0.9, b2)[2] for t in range(1, 9)]
        assert flags == [False] * 5 + [True] * 3, (b2, flags)
    bc1, sq2, on, rect = ops.radam_scalars(6, 0.9, 0.999)
    assert on and 0 < rect < 1 and bc1 == 1 - 0.9 ** 6 and sq2 == (1 - 0.999 ** 6) ** 0.5
    assert ops.radam_scalars(2, 0.9, 0.999)[3] == 0.0


def test_nadam_scalars_follow_torch_and_compound(lib):
    from qflux_amd import ops
    mp = torch.tensor(1.0)
    want = 1.0
    for t in range(1, 5):
        bc2, cg, ca = ops.nadam_scalars(t, 0.0625, 0.9, 0.999, 4e-3, mp)
        mu, mu_next = ops.nadam_mu(t, 0.9, 4e-3)
        want = float(F32(want) * F32(mu))
        assert float(mp) == want and bc2 == 1 - 0.999 ** t
        assert cg == -0.0625 * (1.0 - mu) / (1.0 - want) and ca == (-0.0625 * mu_next) / (1.0 - want * mu_next)
    assert float(mp) < 0.9 ** 4 / 2 ** 3      # four factors of about beta1 / 2 ... beta1 (1 - 0.5 * 0.96^(t * 0.004))


# ---------------------------------------------------------------- resolution, defaults, refusals
def test_resolve_family_and_defaults(lib):
    from qflux_amd.trainer import optim_state as OS
    assert OS.resolve_family("radam") == (None, "radam", OS.RAdamState, 0.0, {"decoupled_weight_decay": False})
    assert OS.resolve_family("nadam") == (None, "nadam", OS.NAdamState, 0.0, {"momentum_decay": 4e-3, "decoupled_weight_decay": False})
    assert OS.resolve_family("adamax") == (None, "adamax", OS.AdamaxState, 0.0, {})
    assert OS.resolve_family("nadam", 0.1, {"momentum_decay": 0})[3:] == (0.1, {"momentum_decay": 0.0, "decoupled_weight_decay": False})
    for fam in ("radam", "nadam", "adamax"):
        assert OS.default_betas(fam) == (0.9, 0.999)
        assert OS.FAMILIES[fam][0].GROUPED
    for fam, bad in (("radam", {"momentum_decay": 0.1}), ("adamax", {"decoupled_weight_decay": True}), ("nadam", {"amsgrad": True})):
        with pytest.raises(ValueError):
            OS.resolve_family(fam, None, bad)
    with pytest.raises(ValueError):
        OS.resolve_family("nadam", None, {"momentum_decay": -1.0})


def test_class_paths_map_with_torchs_defaults_and_refuse_the_rest(lib):
    from qflux_amd.trainer import optimizer_kwargs_from_config as f
    lrs = {"RAdam": 1e-3, "NAdam": 2e-3, "Adamax": 2e-3}
    for name, lr in lrs.items():
        real = inspect.signature(getattr(torch.optim, name).__init__).parameters
        assert real["lr"].default == lr and real["weight_decay"].default == 0 and real["betas"].default == (0.9, 0.999)
        for path in (f"torch.optim.{name}", f"qflux_amd.optim.{name}"):
            kw = f(path, {})
            assert kw["optimizer"] == name.lower() and kw["lr"] == lr and kw["weight_decay"] == 0.0 and "betas" not in kw and "eps" not in kw
            assert kw.get("optimizer_args", {}) == {}
            kw = f(path, {"lr": 3e-4, "betas": [0.8, 0.95], "eps": 1e-6, "weight_decay": 0.01, "foreach": True, "maximize": False})
            assert kw == dict({"lr": 3e-4, "betas": (0.8, 0.95), "eps": 1e-6, "weight_decay": 0.01, "optimizer": name.lower()},
                              **({} if name == "Adamax" else {"optimizer_args": {}}))
            for bad in ({"maximize": True}, {"differentiable": True}, {"capturable": True}, {"amsgrad": False}, {"fused": True},
                        {"momentum": 0.9}, {"min_8bit_size": 4096}):
                with pytest.raises(NotImplementedError):
                    f(path, dict(lr=1e-3, **bad))
            for bad in ({"lr": -1.0}, {"eps": -1e-8}, {"betas": [1.0, 0.999]}, {"betas": [0.9, -0.1]}, {"weight_decay": -0.1}):
                with pytest.raises(ValueError):
                    f(path, bad)
    assert f("torch.optim.RAdam", {"decoupled_weight_decay": True})["optimizer_args"] == {"decoupled_weight_decay": True}
    assert f("torch.optim.NAdam", {"momentum_decay": 0.01, "decoupled_weight_decay": True})["optimizer_args"] == \
        {"momentum_decay": 0.01, "decoupled_weight_decay": True}
    with pytest.raises(NotImplementedError):
        f("torch.optim.Adamax", {"decoupled_weight_decay": True})      # not a keyword of torch.optim.Adamax
    with pytest.raises(NotImplementedError):
        f("torch.optim.RAdam", {"momentum_decay": 0.01})
    with pytest.raises(ValueError):
        f("torch.optim.NAdam", {"momentum_decay": -0.01})
    # what was refused before stays refused
    for path, init in (("torch.optim.AdamW", {"amsgrad": True, "maximize": True}), ("torch.optim.SGD", {"lr": 0.1}), ("torch.optim.Adagrad", {})):
        with pytest.raises(NotImplementedError):
            f(path, init)


def _tiny_model():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from common import TINY
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.modules import LoraConfig
    q = QwenImageTransformer2DModel(**TINY)
    q.add_adapter(LoraConfig(r=4, lora_alpha=8, target_modules=TARGETS), "lora_edit")
    return q


def test_train_steps_and_optim_classes_take_the_families(lib):
    from qflux_amd import optim as O
    from qflux_amd.trainer import FluxKontextTrainStep, QwenLoraTrainStep
    q = _tiny_model()
    for cls in (QwenLoraTrainStep, FluxKontextTrainStep):
        for fam in ("radam", "nadam", "adamax"):
            s = cls(q, optimizer=fam)
            assert s.betas == (0.9, 0.999) and s.weight_decay == 0.0 and s.eps == 1e-8 and s.optimizer == fam
        s = cls(q, optimizer="nadam", optimizer_args={"momentum_decay": 0.01}, loraplus_lr_ratio=4.0)
        assert s.optimizer_args == {"momentum_decay": 0.01, "decoupled_weight_decay": False} and len(s.group_rules) == 2
        with pytest.raises(ValueError):
            cls(q, optimizer="adamax", optimizer_args={"decoupled_weight_decay": True})
    assert {"RAdam", "NAdam", "Adamax"} <= set(O.__all__)
    params = [p for _, p in q.lora_store.params()]
    for name in ("RAdam", "NAdam", "Adamax"):
        mine, real = getattr(O, name), getattr(torch.optim, name)
        sig = lambda c: [(n, p.default, p.kind) for n, p in inspect.signature(c.__init__).parameters.items() if n != "self"]      # noqa: E731
        assert sig(mine) == sig(real), name
        o = mine(params)
        r = real([torch.nn.Parameter(torch.zeros(2))])
        assert isinstance(o, torch.optim.Optimizer) and o.family == name.lower()
        for k in ("lr", "betas", "eps", "weight_decay") + (("decoupled_weight_decay",) if name != "Adamax" else ()) + \
                (("momentum_decay",) if name == "NAdam" else ()):
            assert o.param_groups[0][k] == r.param_groups[0][k], (name, k)
        for bad in ("maximize", "differentiable", "capturable"):
            with pytest.raises(NotImplementedError):
                mine(params, **{bad: True})
        groups = O.loraplus_param_groups(q, 1e-3, 4.0)
        assert [g["lr"] for g in mine(groups).param_groups] == [1e-3, 4e-3]


# ---------------------------------------------------------------- state-dict layout and group map
KEYS = {"radam": {"step", "exp_avg", "exp_avg_sq"}, "nadam": {"step", "exp_avg", "exp_avg_sq", "mu_product"},
        "adamax": {"step", "exp_avg", "exp_inf"}}


def _real_file(q, family, steps=3, groups=False, **kw):
    """optimizer.bin of the real torch.optim class after `steps` steps on parameters shaped like the adapters (fp32, CPU)."""
    torch.manual_seed(7)
    named = [(n, torch.nn.Parameter(torch.randn(p.shape) * 0.1)) for n, p in q.lora_store.params()]
    ps = [p for _, p in named]
    if groups:
        params = [{"params": [p for n, p in named if "lora_A" in n], "lr": 1e-3},
                  {"params": [p for n, p in named if "lora_B" in n], "lr": 4e-3, "betas": (0.8, 0.99)}]
    else:
        params = ps
    opt = getattr(torch.optim, R.TORCH[family])(params, **kw)
    for _ in range(steps):
        for p in ps:
            p.grad = torch.randn(p.shape)
        opt.step()
    return opt, ps


@pytest.mark.parametrize("family", list(KEYS))
def test_state_dict_is_torchs_layout_and_round_trips_with_the_real_class(lib, family):
    from qflux_amd.trainer import QwenLoraTrainStep
    q = _tiny_model()
    kw = {"adamax": {}, "radam": {"decoupled_weight_decay": True}, "nadam": {"momentum_decay": 0.01}}[family]
    real, _ = _real_file(q, family, lr=2e-3, betas=(0.85, 0.98), eps=1e-6, weight_decay=0.01, **kw)
    sd = real.state_dict()
    assert {frozenset(e) for e in sd["state"].values()} == {frozenset(KEYS[family])}
    step = QwenLoraTrainStep(q, optimizer=family, lr=0.5)
    step.load_state_dict(sd)
    assert (step.lr, step.betas, step.eps, step.weight_decay, step.global_step) == (2e-3, (0.85, 0.98), 1e-6, 0.01, 3)
    assert all(step.optimizer_args[k] == v for k, v in kw.items())
    out = step.state_dict()
    assert set(out["state"]) == set(sd["state"]) and set(out["param_groups"][0]) >= set(sd["param_groups"][0])
    for i, e in sd["state"].items():
        assert set(out["state"][i]) == KEYS[family]
        for k, v in e.items():
            o = out["state"][i][k]
            assert torch.is_tensor(o) and o.dtype == v.dtype and o.shape == v.shape and torch.equal(o, v), (i, k)
    for k, v in sd["param_groups"][0].items():
        assert out["param_groups"][0][k] == v or k == "betas" and tuple(v) == out["param_groups"][0][k], k
    # and back into a fresh instance of the real class, which then holds the same state
    fresh, _ = _real_file(q, family, steps=0)
    fresh.load_state_dict({k: out[k] for k in ("state", "param_groups")})
    back = fresh.state_dict()
    for i, e in sd["state"].items():
        for k, v in e.items():
            assert torch.equal(back["state"][i][k], v), (i, k)
    assert back["param_groups"][0]["lr"] == 2e-3 and tuple(back["param_groups"][0]["betas"]) == (0.85, 0.98)
    # nothing before the first step, as in torch
    assert QwenLoraTrainStep(q, optimizer=family).state_dict()["state"] == {}
    for flag in ("maximize", "capturable", "differentiable"):
        bad = dict(sd, param_groups=[dict(sd["param_groups"][0], **{flag: True})])
        with pytest.raises(NotImplementedError):
            QwenLoraTrainStep(q, optimizer=family).load_state_dict(bad)
    short = {"state": {i: {k: v for k, v in e.items() if k != "exp_avg"} for i, e in sd["state"].items()}, "param_groups": sd["param_groups"]}
    with pytest.raises(ValueError):
        QwenLoraTrainStep(q, optimizer=family).load_state_dict(short)


def test_groups_build_the_tile_map_and_nadam_keeps_one_mu_product_per_group(lib):
    from qflux_amd import ops
    from qflux_amd.trainer import QwenLoraTrainStep
    from qflux_amd.trainer import optim_state as OS
    q = _tiny_model()
    st = q.lora_store
    names = [n for n, _, _, _ in st.entries]
    members = (tuple(i for i, n in enumerate(names) if "lora_A" in n), tuple(i for i, n in enumerate(names) if "lora_B" in n))
    for fam in ("radam", "nadam", "adamax"):
        cls = OS.FAMILIES[fam][0]
        args = dict(cls.DEFAULTS)
        state = OS.ensure_state(cls, None, st, args, members)
        assign = [0 if "lora_A" in n else 1 for n in names]
        want = ops.tile_group_map([(off, k) for _, _, off, k in st.entries], assign, 2, numel=st.pflat.numel())
        assert state.group_map.dtype == torch.uint8 and torch.equal(state.group_map.cpu(), want)
        for i, (_, _, off, k) in enumerate(st.entries):
            assert off % 64 == 0 and (state.group_map[off // 64:(off + k + 63) // 64] == assign[i]).all()
        same = OS.ensure_state(cls, state, st, args, members)
        assert same is state
        one = OS.ensure_state(cls, state, st, args, None)
        assert one is state and one.group_map is None      # the moments stay, the map goes
        with pytest.raises(ValueError):
            cls.check_groups(ops.MAX_PARAM_GROUPS + 1)
    # NAdam: the real class's per-parameter mu_product differs between two groups with different beta1; the file's values come back
    real, _ = _real_file(q, "nadam", steps=4, groups=True)
    sd = real.state_dict()
    step = QwenLoraTrainStep(q, optimizer="nadam", param_groups=[{"match": "lora_A", "lr": 1e-3}, {"match": "lora_B", "lr": 4e-3, "betas": (0.8, 0.99)}])
    step.load_state_dict(sd)
    mus = [float(m) for m in step.opt_state.mu]
    na = len(members[0])
    assert mus == [float(sd["state"][0]["mu_product"]), float(sd["state"][na]["mu_product"])] and mus[0] != mus[1]
    out = step.state_dict()
    assert [tuple(g["betas"]) for g in out["param_groups"]] == [(0.9, 0.999), (0.8, 0.99)] and [g["lr"] for g in out["param_groups"]] == [1e-3, 4e-3]
    for i, e in sd["state"].items():
        assert float(out["state"][i]["mu_product"]) == float(e["mu_product"]) and torch.equal(out["state"][i]["exp_avg"], e["exp_avg"])
    # the host image that travels with a broadcast
    step.opt_state.buffers()
    step.opt_state.mu = [torch.tensor(1.0), torch.tensor(1.0)]
    step.opt_state.sync_host()
    assert [float(m) for m in step.opt_state.mu] == mus


# ---------------------------------------------------------------- the C ABI without a device
def test_ctypes_layout_matches_header(tmp_path, lib):
    pairs = {"qfx_adamx_group": lib.AdamxGroup, "qfx_adamx_args": lib.AdamxArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "qfx.h"', "int main(void) {"]
    for cname, ct in pairs.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'  printf(" %zu", offsetof({cname}, {fname}));')
        lines.append('  printf("\\n");')
    lines += ['  printf("abi %d %d %d %d\\n", QFX_ABI_VERSION, QFX_ADAMX_RADAM, QFX_ADAMX_NADAM, QFX_ADAMX_ADAMAX);', "  return 0;", "}"]
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for line in out[:-1]:
        parts = line.split()
        ct = pairs[parts[0]]
        assert [int(v) for v in parts[1:]] == [C.sizeof(ct)] + [getattr(ct, f).offset for f, _ in ct._fields_], parts
    assert out[-1].split() == ["abi", "7", str(lib.ADAMX_RADAM), str(lib.ADAMX_NADAM), str(lib.ADAMX_ADAMAX)] and lib.ABI_VERSION == 7
    assert "qfx_adamx_step" in lib.SYMBOLS


def good_row(lib, **kw):
    from qflux_amd import ops
    row = ops.adamx_rows("radam", [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)], 6)[0]
    g = lib.AdamxGroup(*row)
    g.bias_corr2 = 0.5
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def check_refusals(lib):
    """Every QFX_EINVAL of include/qfx.h for qfx_adamx_step; none of them reaches a launch (the pointers are not memory)."""
    f = lib.lib.qfx_adamx_step
    assert f(None, None) == lib.QFX_EINVAL

    def call(rows=None, **kw):
        rows = [good_row(lib)] if rows is None else rows
        arr = (lib.AdamxGroup * max(1, len(rows)))(*rows)
        a = lib.AdamxArgs(0x1000, 0x2000, 0x3000, 0x4000, 64, lib.ADAMX_RADAM, len(rows), arr, None, None, 1.0, 1.0)
        for k, v in kw.items():
            setattr(a, k, v)
        return f(C.byref(a), None)
    for bad in (dict(p=None), dict(g=None), dict(exp_avg=None), dict(state2=None), dict(n=0), dict(n=-64), dict(variant=3), dict(variant=-1),
                dict(n_groups=0), dict(n_groups=17), dict(n_groups=2), dict(groups=None)):
        assert call(**bad) == lib.QFX_EINVAL, bad
    for bad in (dict(lr=-1e-3), dict(lr=float("nan")), dict(eps=-1e-8), dict(weight_decay=-0.01), dict(beta1=1.0), dict(beta1=-0.1),
                dict(beta2=1.0), dict(beta2=-0.5), dict(beta2=float("nan")), dict(bias_corr1=0.0)):
        assert call([good_row(lib, **bad)]) == lib.QFX_EINVAL, bad
        assert call([good_row(lib), good_row(lib, **bad)], tile_group=0x5000) == lib.QFX_EINVAL, bad      # in a later row too
    assert call([good_row(lib, bias_corr2=0.0)], variant=lib.ADAMX_NADAM) == lib.QFX_EINVAL
    assert call([good_row(lib)] * 17, tile_group=0x5000) == lib.QFX_EINVAL


def test_bad_arguments_are_rejected_without_a_device(lib):
    check_refusals(lib)
