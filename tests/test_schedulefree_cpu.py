"""CPU: Schedule-Free AdamW -- the restatement (tests/schedulefree_ref.py) against the paper's invariants and, where it is installed,
against the package; the family name, the config mapping and its refusals, the torch.optim class, the file layout, the mode
handling that needs no launch, and the C ABI of qfx_sfadamw_step / qfx_sf_swap (no device needed)."""
import importlib.util
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import schedulefree_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = ["to_q", "to_k", "to_v", "to_out.0", "img_mlp.net.2", "txt_mod.1"]
EPS32, EPS64 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from qflux_amd import _lib
    return _lib


def _tiny_model():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from common import TINY
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.modules import LoraConfig
    q = QwenImageTransformer2DModel(**TINY)
    q.add_adapter(LoraConfig(r=4, lora_alpha=8, target_modules=TARGETS), "lora_edit")
    return q


# ---------------------------------------------------------------- the restatement against the published method
def _invariant_runs(steps, n=257, **kw):
    """The restatement in fp64 and fp32 on the same inputs (no clip), stepping both; yields (k, opt64, opt32) after every step."""
    y, grads, _ = R.make_inputs(n, steps, seed=9)
    opts = [R.SFRef([y.to(dt).clone()], **kw) for dt in (torch.float64, torch.float32)]
    for k, g in enumerate(grads):
        for o in opts:
            o.step([g])
        yield k, opts[0], opts[1]


def _x_of(opt):
    """The averaged point the eval() lerp recovers from y and z, without touching the optimizer."""
    return R.lerp(opt.params[0], opt.state[0]["z"], 1 - 1 / opt.group["betas"][0])


def _bounds(o64, o32, res64):
    """Tolerances of an invariant residual, derived from the fp64 run.  In fp64 the residual is rounding alone: a few roundings
    per step, amplified by at most 1 / beta1 in the recovery of x, on values of magnitude max|y|, |z| -- 64 eps64 of that per
    step taken.  The fp32 run's y and z sit within `own` = its largest error against the fp64 run; x = z + (y - z) / beta1 moves
    by at most (1 + 2 / beta1) own, an average of z's by at most own, y itself by own: (3 + 2 / beta1) own on top of the fp64
    residual, plus one fp32 ulp of the magnitude for the recovery's own last rounding."""
    mag = max(o64.params[0].abs().max().item(), o64.state[0]["z"].abs().max().item())
    own = max((o32.params[0].double() - o64.params[0]).abs().max().item(),
              (o32.state[0]["z"].double() - o64.state[0]["z"]).abs().max().item())
    b1 = o64.group["betas"][0]
    return 64 * EPS64 * mag * (o64.group["k"] + 1), res64 + (3 + 2 / b1) * own + EPS32 * mag


def test_ckp1_is_one_over_k_and_x_is_the_uniform_mean_of_z():
    """Constant lr, no warm-up, r = 0, no weight decay: every averaging weight is lr^2, so ckp1 = 1 / (k + 1) and the x that
    eval() recovers after k steps is the uniform mean of z_1 .. z_k (Defazio et al., eq. 5 with c_{t+1} = 1 / (t + 1))."""
    g = dict(R.DEFAULTS, lr=2.0 ** -9, k=0, weight_sum=0.0, lr_max=-1.0)
    for k in range(40):
        g["k"] = k
        assert R.host_scalars(g)[2] == 1.0 / (k + 1)            # lr^2 a power of two: the running sum is exact, the quotient correctly rounded
    g = dict(R.DEFAULTS, k=0, weight_sum=0.0, lr_max=-1.0)
    for k in range(40):
        g["k"] = k
        assert abs(R.host_scalars(g)[2] * (k + 1) - 1.0) <= 4 * EPS64      # the default lr: up to the rounding of the running sum
    zs = []
    for k, o64, o32 in _invariant_runs(12, lr=0.0025):
        zs.append(o64.state[0]["z"].clone())
        mean = torch.stack(zs).mean(dim=0)
        res64 = (_x_of(o64) - mean).abs().max().item()
        res32 = (_x_of(o32).double() - mean).abs().max().item()
        tol64, tol32 = _bounds(o64, o32, res64)
        print(f"uniform mean, step {k}: residual fp64 {res64:.3e} (tol {tol64:.3e}), fp32 {res32:.3e} (tol {tol32:.3e})")
        assert res64 <= tol64 and res32 <= tol32, (k, res64, tol64, res32, tol32)
    assert (zs[-1] - zs[0]).abs().max() > 1e-3                   # the sequence did move


@pytest.mark.parametrize("kw", [dict(lr=0.0025), dict(lr=0.01, betas=(0.8, 0.99), warmup_steps=3, r=0.5, weight_decay=0.01)],
                         ids=["defaults", "warmup_r_decay"])
def test_y_is_the_interpolation_of_z_and_x_after_every_step(kw):
    """y = (1 - beta1) z + beta1 x after every step, with x tracked independently of the restatement's lerps as the paper's running
    average x_{t+1} = (1 - c_{t+1}) x_t + c_{t+1} z_{t+1} of the fp64 run's own z (c from the host scalars of a second group)."""
    side = dict(R.DEFAULTS, **kw)
    side.update(k=0, weight_sum=0.0, lr_max=-1.0)
    b1, x = side["betas"][0], None
    for k, o64, o32 in _invariant_runs(10, **kw):
        side["k"] = k
        c = R.host_scalars(side)[2]
        z = o64.state[0]["z"]
        x = z.clone() if x is None else (1 - c) * x + c * z
        want = (1 - b1) * z + b1 * x
        res64 = (o64.params[0] - want).abs().max().item()
        res32 = (o32.params[0].double() - want).abs().max().item()
        tol64, tol32 = _bounds(o64, o32, res64)
        print(f"y = (1 - b1) z + b1 x, step {k}: residual fp64 {res64:.3e} (tol {tol64:.3e}), fp32 {res32:.3e} (tol {tol32:.3e})")
        assert res64 <= tol64 and res32 <= tol32, (k, res64, tol64, res32, tol32)
        assert (_x_of(o64) - x).abs().max().item() <= tol64      # and eval() recovers that x


def test_mode_swap_of_the_restatement():
    y, grads, _ = R.make_inputs(100, 2)
    p = y.clone()
    opt = R.SFRef([p], betas=(0.5, 0.75))
    opt.eval()
    assert torch.equal(p, y) and opt.group["train_mode"] is False        # before the first step there is nothing to move
    with pytest.raises(RuntimeError):
        opt.step([grads[0]])
    opt.train()
    opt.step([grads[0]])
    assert torch.equal(p, opt.state[0]["z"])                             # ckp1 = 1 on the first step: y = z = x
    opt.step([grads[1]])
    y1, z1 = p.clone(), opt.state[0]["z"].clone()
    opt.train()
    assert torch.equal(p, y1)                                            # a no-op in its own mode
    opt.eval()
    assert torch.equal(p, z1 - (z1 - y1) * 2.0) and not torch.equal(p, y1)      # weight 1 - 1 / 0.5 = -1: the |w| >= 0.5 branch
    opt.eval()
    assert torch.equal(p, z1 - (z1 - y1) * 2.0)
    opt.train()
    assert torch.allclose(p, y1, rtol=0, atol=4 * EPS32 * float(y1.abs().max())) and opt.group["train_mode"] is True
    assert set(opt.state_dict()["state"][0]) == R.PARAM_KEYS
    assert set(opt.state_dict()["param_groups"][0]) == R.GROUP_KEYS | {"params"}


@pytest.mark.skipif(importlib.util.find_spec("schedulefree") is None, reason="the schedulefree package is not installed")
def test_restatement_matches_the_package():
    """betas that fp32 represents exactly: the restatement is then the package's arithmetic (see schedulefree_ref)."""
    import schedulefree
    kw = dict(lr=0.0025, betas=(0.875, 1 - 2.0 ** -10), weight_decay=0.01, warmup_steps=3, r=0.5)
    y, grads, gsq = R.make_inputs(1027, 6)
    r64 = R.run(y, grads, gsq, torch.float64, max_norm=0.0, grad_scale=1.0, **kw)
    r32 = R.run(y, grads, gsq, torch.float32, max_norm=0.0, grad_scale=1.0, **kw)
    p = torch.nn.Parameter(y.clone())
    opt = schedulefree.AdamWScheduleFree([p], **kw)
    opt.train()
    for it, g in enumerate(grads):
        p.grad = g.clone()
        opt.step()
        st = opt.state[p]
        for name, got, i in (("y", p.detach(), 0), ("z", st["z"], 1), ("v", st["exp_avg_sq"], 2)):
            R.check(name, got, r32[it][i], r64[it][i], f"package step {it}")
    assert set(opt.state[p]) == R.PARAM_KEYS and set(opt.state_dict()["param_groups"][0]) >= R.GROUP_KEYS
    opt.eval()
    b1 = kw["betas"][0]
    R.check("x", p.detach(), R.lerp(r32[-1][0], r32[-1][1], 1 - 1 / b1), R.lerp(r64[-1][0], r64[-1][1], 1 - 1 / b1), "package eval")
    with pytest.raises(Exception):
        opt.step()


# ---------------------------------------------------------------- family, mapping, class
def test_resolve_family_and_defaults(lib):
    from qflux_amd.trainer import optim_state as OS
    S = OS.ScheduleFreeAdamWState
    assert OS.resolve_family("adamw_schedulefree") == (None, "adamw_schedulefree", S, 0.0, dict(warmup_steps=0, r=0.0, weight_lr_power=2.0))
    _, _, _, wd, args = OS.resolve_family("adamw_schedulefree", 0.05, {"warmup_steps": 100, "r": 1})
    assert wd == 0.05 and args == dict(warmup_steps=100, r=1.0, weight_lr_power=2.0) and isinstance(args["r"], float)
    assert OS.default_betas("adamw_schedulefree") == (0.9, 0.999)
    assert S.DEFAULTS == dict(warmup_steps=0, r=0.0, weight_lr_power=2.0) and S.LAYOUT_ARGS == ()
    for bad in ({"blocksize": 256}, {"momentum": 0.9}, {"warmup_steps": -1}, {"warmup_steps": 2.5}):
        with pytest.raises(ValueError):
            OS.resolve_family("adamw_schedulefree", None, bad)
    assert OS.resolve_family("adamw")[1:3] == ("adamw", OS.AdamWState) and OS.resolve_family("lion")[2] is OS.LionState


def test_config_mapping(lib):
    from qflux_amd.trainer import optimizer_kwargs_from_config as f
    for path in ("schedulefree.AdamWScheduleFree", "qflux_amd.optim.AdamWScheduleFree"):
        for bits in (32, 8):
            assert f(path, {}, state_bits=bits) == {"optimizer": "adamw_schedulefree", "lr": 0.0025, "weight_decay": 0.0, "optimizer_args": {}}
        assert f(path, None) == f(path, {})
        got = f(path, {"lr": 1e-3, "betas": [0.95, 0.99], "eps": 1e-6, "weight_decay": 0.01, "warmup_steps": 50, "r": 0.5,
                       "weight_lr_power": 1.0, "foreach": False})
        assert got == {"optimizer": "adamw_schedulefree", "lr": 1e-3, "betas": (0.95, 0.99), "eps": 1e-6, "weight_decay": 0.01,
                       "optimizer_args": {"warmup_steps": 50, "r": 0.5, "weight_lr_power": 1.0}}          # foreach dropped
        assert f(path, {"foreach": True}) == f(path, {})
        for bad in ({"momentum": 0.9}, {"amsgrad_like": 1}, {"d0": 1e-6}):
            with pytest.raises(NotImplementedError) as e:
                f(path, dict(lr=1e-3, **bad))
            assert "unsupported optimizer init_args" in str(e.value) and list(bad)[0] in str(e.value)
        with pytest.raises(ValueError):
            f(path, {"warmup_steps": -5})
    for path in ("schedulefree.SGDScheduleFree", "schedulefree.RAdamScheduleFree", "schedulefree.AdamWScheduleFreeClosure"):
        with pytest.raises(NotImplementedError):
            f(path, {"lr": 1e-3})
    assert f("torch.optim.AdamW", {"lr": 1e-4})["optimizer"] == "adamw"                                  # what was mapped before stays so


def test_train_steps_take_the_family(lib):
    from qflux_amd.trainer import FluxKontextTrainStep, QwenLoraTrainStep
    q = _tiny_model()
    for cls in (QwenLoraTrainStep, FluxKontextTrainStep):
        s = cls(q, lr=0.0025, optimizer="adamw_schedulefree")
        assert (s.optimizer, s.betas, s.weight_decay, s.train_mode) == ("adamw_schedulefree", (0.9, 0.999), 0.0, True)
        assert s.optimizer_args == dict(warmup_steps=0, r=0.0, weight_lr_power=2.0)
        s = cls(q, optimizer="adamw_schedulefree", weight_decay=0.01, optimizer_args={"warmup_steps": 10, "weight_lr_power": 0.0})
        assert s.weight_decay == 0.01 and s.optimizer_args == dict(warmup_steps=10, r=0.0, weight_lr_power=0.0)
        with pytest.raises(ValueError):
            cls(q, optimizer="adamw_schedulefree", optimizer_args={"min_8bit_size": 100})
        # every other family: the mode calls exist and do nothing
        a = cls(q)
        before = q.lora_store.pflat.clone()
        a.eval(); a.train()
        with a.eval_mode():
            assert a.train_mode is True
        assert a.opt_state is None and torch.equal(q.lora_store.pflat, before)


def test_mode_handling_without_a_launch(lib):
    """Before the first step a swap moves nothing (the package's eval() skips parameters without z), so the flag logic runs here."""
    from qflux_amd import optim as O
    from qflux_amd.trainer import QwenLoraTrainStep
    from qflux_amd.trainer import optim_state as OS
    q = _tiny_model()
    before = q.lora_store.pflat.clone()
    s = QwenLoraTrainStep(q, optimizer="adamw_schedulefree")
    s.train()
    assert s.train_mode is True
    with s.eval_mode():
        assert s.train_mode is False
        with pytest.raises(RuntimeError, match=r"train\(\) first"):
            s.optimizer_step()
        with s.eval_mode():                                              # nested: the inner one leaves the mode it found
            pass
        assert s.train_mode is False
    assert s.train_mode is True and s.global_step == 0 and torch.equal(q.lora_store.pflat, before)
    s.eval()
    sd = s.state_dict()
    assert sd["param_groups"][0]["train_mode"] is False and sd["state"] == {}
    s.eval()
    assert s.train_mode is False
    # the class
    params = [p for _, p in q.lora_store.params()]
    opt = O.AdamWScheduleFree(params)
    opt.train()
    opt.eval()
    with pytest.raises(RuntimeError, match=r"train\(\) first"):
        opt.step()
    assert opt._step_count_fused == 0 and opt.state_dict()["param_groups"][0]["train_mode"] is False
    opt.train()
    assert opt.state_dict()["param_groups"][0]["train_mode"] is True
    # a file saved in eval mode loads in eval mode: stepping it is refused until train() (which needs the device)
    sd = _file(q, eval_mode=True)
    for o in (O.AdamWScheduleFree(params), QwenLoraTrainStep(q, optimizer="adamw_schedulefree")):
        o.load_state_dict(sd)
        with pytest.raises(RuntimeError, match=r"train\(\) first"):
            (o.step if hasattr(o, "step") else o.optimizer_step)()
    assert OS.ScheduleFreeAdamWState.EVAL_STEP.endswith("call train() first")


def test_constructor_signature_of_the_class(lib):
    from qflux_amd import optim as O
    assert "AdamWScheduleFree" in O.__all__ and issubclass(O.AdamWScheduleFree, torch.optim.Optimizer)
    sig = {n: p.default for n, p in inspect.signature(O.AdamWScheduleFree.__init__).parameters.items() if n not in ("self", "params")}
    assert list(sig) == ["lr", "betas", "eps", "weight_decay", "warmup_steps", "r", "weight_lr_power", "foreach"]
    assert [sig[n] for n in list(sig)[:7]] == [0.0025, (0.9, 0.999), 1e-8, 0, 0, 0.0, 2.0]
    q = _tiny_model()
    params = [p for _, p in q.lora_store.params()]
    o = O.AdamWScheduleFree(params)
    g = o.param_groups[0]
    assert o.family == "adamw_schedulefree" and (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (0.0025, (0.9, 0.999), 1e-8, 0.0)
    assert (g["warmup_steps"], g["r"], g["weight_lr_power"]) == (0, 0.0, 2.0)
    o = O.AdamWScheduleFree(params, lr=1e-3, warmup_steps=20, r=0.5, foreach=False)
    assert o._args == dict(warmup_steps=20, r=0.5, weight_lr_power=2.0) and o.param_groups[0]["warmup_steps"] == 20
    with pytest.raises(ValueError):
        O.AdamWScheduleFree(params, warmup_steps=-1)


# ---------------------------------------------------------------- state object and file layout
def _file(q, steps=3, eval_mode=False, **kw):
    torch.manual_seed(4)
    ps = [torch.randn(p.shape) * 0.1 for _, p in q.lora_store.params()]
    opt = R.SFRef(ps, **dict(dict(lr=1e-3, betas=(0.95, 0.98), weight_decay=0.01, warmup_steps=2, r=0.5), **kw))
    for _ in range(steps):
        opt.step([torch.randn(p.shape) for p in ps])
    if eval_mode:
        opt.eval()
    return opt.state_dict()


def _same(out, sd):
    assert set(out["state"]) == set(sd["state"])
    for i, e in sd["state"].items():
        o = out["state"][i]
        assert set(o) == set(e) == R.PARAM_KEYS, (i, sorted(o), sorted(e))
        for k, v in e.items():
            assert o[k].dtype == v.dtype and o[k].shape == v.shape and torch.equal(o[k], v), (i, k)
    g, h = out["param_groups"][0], sd["param_groups"][0]
    assert set(g) - {"params"} == R.GROUP_KEYS
    for n in R.GROUP_KEYS:
        assert g[n] == h[n] and type(g[n]) is type(h[n]), (n, g[n], h[n])


def test_state_names_buffers_and_host_scalars(lib):
    from qflux_amd.trainer import optim_state as OS
    S = OS.ScheduleFreeAdamWState
    q = _tiny_model()
    args = dict(S.DEFAULTS)
    st = S(q.lora_store, args)
    assert S.names(args) == ("z", "v", "sched") == tuple(n for n, _ in st.buffers()) and len(S.names(args)) == len(st.buffers())
    assert st.z.shape == st.v.shape == q.lora_store.pflat.shape and st.key == S.layout_key(q.lora_store, args)
    assert (st.k, st.weight_sum, st.lr_max, st.train_mode, st.scheduled_lr) == (0, 0.0, -1.0, True, 0.0)
    # the host scalars ride in the fp64 buffer: what a broadcast or a replica check sees, and what the receiver reads back
    st.k, st.weight_sum, st.lr_max, st.train_mode, st.scheduled_lr = 7, 4.375e-5, 0.0025, False, 0.00125
    sched = dict(st.buffers())["sched"]
    assert sched.dtype == torch.float64 and sched.tolist() == [7.0, 4.375e-5, 0.0025, 0.0, 0.00125]
    other = S(q.lora_store, args)
    for (_, src), (_, dst) in zip(st.buffers(), other.buffers()):
        dst.copy_(src)
    other.sync_host()
    assert (other.k, other.weight_sum, other.lr_max, other.train_mode, other.scheduled_lr) == (7, 4.375e-5, 0.0025, False, 0.00125)
    assert type(other.k) is int and type(other.train_mode) is bool


def test_layout_round_trip(lib):
    from qflux_amd import optim as O
    from qflux_amd.trainer import QwenLoraTrainStep
    from qflux_amd.trainer import optim_state as OS
    S = OS.ScheduleFreeAdamWState
    q = _tiny_model()
    sd = _file(q)
    assert {frozenset(e) for e in sd["state"].values()} == {frozenset(R.PARAM_KEYS)} and sd["param_groups"][0]["k"] == 3
    args = dict(S.DEFAULTS)
    state, n = S.load(q.lora_store, sd, args)
    assert n == 0 and args == dict(warmup_steps=2, r=0.5, weight_lr_power=2.0) and state.k == 3 and state.train_mode is True
    extra, per = S.save(state, q.lora_store.entries, 3, args)
    assert set(extra) == R.GROUP_KEYS - {"lr", "betas", "eps", "weight_decay"}
    assert set(per) == set(sd["state"]) and all(set(e) == R.PARAM_KEYS for e in per.values())
    extra0, per0 = S.save(None, q.lora_store.entries, 0, dict(S.DEFAULTS))
    assert per0 == {} and (extra0["k"], extra0["train_mode"], extra0["weight_sum"], extra0["lr_max"], extra0["scheduled_lr"]) == \
        (0, True, 0.0, -1.0, 0.0)
    for make in (lambda: QwenLoraTrainStep(q, optimizer="adamw_schedulefree", lr=0.5), lambda: O.AdamWScheduleFree([p for _, p in q.lora_store.params()])):
        o = make()
        o.load_state_dict(sd)
        _same(o.state_dict(), sd)
        assert o.state_dict()["global_step"] == 3                        # the package's file counts in its group's k
    step = QwenLoraTrainStep(q, optimizer="adamw_schedulefree", lr=0.5)
    step.load_state_dict(sd)
    assert (step.lr, step.betas, step.weight_decay, step.global_step) == (1e-3, (0.95, 0.98), 0.01, 3)
    sde = _file(q, eval_mode=True)
    step.load_state_dict(sde)
    assert step.train_mode is False
    _same(step.state_dict(), sde)
    bad = {"state": {i: dict(e) for i, e in sd["state"].items()}, "param_groups": sd["param_groups"]}
    del bad["state"][0]["z"]
    with pytest.raises(ValueError):
        S.load(q.lora_store, bad, dict(S.DEFAULTS))


# ---------------------------------------------------------------- C ABI
def test_bad_arguments_are_rejected_without_a_device(lib):
    assert lib.ABI_VERSION == 7 and {"qfx_sfadamw_step", "qfx_sf_swap"} <= set(lib.SYMBOLS)      # append-only: the version stays
    f = lib.lib.qfx_sfadamw_step
    ok = dict(p=0x1000, g=0x2000, z=0x3000, v=0x4000, n=16, lr_t=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
              bias_corr2=0.001, ckp1=0.5, first=0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["p"], a["g"], a["z"], a["v"], a["n"], a["lr_t"], a["beta1"], a["beta2"], a["eps"], a["weight_decay"], a["bias_corr2"],
                 a["ckp1"], a["first"], None, 1.0, 1.0, None)
    nan = float("nan")
    for bad in (dict(p=None), dict(g=None), dict(z=None), dict(v=None), dict(z=None, first=1), dict(n=0), dict(n=-4), dict(lr_t=-1e-4),
                dict(lr_t=nan), dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=nan), dict(beta2=1.0), dict(beta2=-0.5), dict(beta2=nan),
                dict(weight_decay=-0.01), dict(eps=-1e-8), dict(eps=nan), dict(bias_corr2=0.0), dict(bias_corr2=-0.5), dict(bias_corr2=nan),
                dict(ckp1=-0.01), dict(ckp1=1.5), dict(ckp1=nan)):
        assert call(**bad) == lib.QFX_EINVAL, bad
    s = lib.lib.qfx_sf_swap
    for bad in ((None, 0x2000, 16, 0.1), (0x1000, None, 16, 0.1), (0x1000, 0x2000, 0, 0.1), (0x1000, 0x2000, -1, 0.1),
                (0x1000, 0x2000, 16, float("-inf")), (0x1000, 0x2000, 16, nan)):
        assert s(*bad, None) == lib.QFX_EINVAL, bad
    # beta1 == 0 would make the eval weight 1 - 1 / beta1 a division by zero: the swap's caller refuses it
    from qflux_amd import ops
    t = torch.zeros(4)
    for b1 in (0.0, 1.0, -0.5):
        for to_eval in (True, False):
            with pytest.raises(ValueError):
                ops.sf_swap(t, t, b1, to_eval)


def test_schedule_on_the_host_matches_the_restatement(lib):
    from qflux_amd import ops
    for kw in (dict(lr=0.0025), dict(lr=0.01, betas=(0.8, 0.99), warmup_steps=3, r=0.5, weight_lr_power=1.0), dict(lr=0.0)):
        g = dict(R.DEFAULTS, **kw)
        g.update(k=0, weight_sum=0.0, lr_max=-1.0)
        lr_max, wsum = -1.0, 0.0
        for k in range(8):
            g["k"] = k
            lr_t, bc2, ckp1, _ = R.host_scalars(g)
            got = ops.sfadamw_schedule(k, g["lr"], g["betas"][1], g["warmup_steps"], g["r"], g["weight_lr_power"], lr_max, wsum)
            assert got == (lr_t, bc2, ckp1, g["lr_max"], g["weight_sum"])
            lr_max, wsum = got[3], got[4]
