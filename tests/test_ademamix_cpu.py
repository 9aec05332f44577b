"""CPU-side tests of the fused AdEMAMix family: the schedules, the restatement tests/ademamix_ref.py (reduction to AdamW at alpha = 0,
the fp32 form against the fp64 one), the class-path mapping, the state classes (registration, group rows and maps, the file layout
and a bit-for-bit round trip on CPU tensors), the qflux_amd.optim classes and the C ABI's refusals (no launch, so no device)."""
import ctypes as C
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ademamix_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = ["to_q", "to_k", "to_v", "to_out.0", "img_mlp.net.2", "txt_mod.1"]
F32, F64 = np.float32, np.float64
FP32_PATHS = ("bitsandbytes.optim.AdEMAMix", "bitsandbytes.optim.AdEMAMix32bit", "bitsandbytes.optim.PagedAdEMAMix",
              "bitsandbytes.optim.PagedAdEMAMix32bit", "qflux_amd.optim.AdEMAMix")
BNB_8BIT_PATHS = ("bitsandbytes.optim.AdEMAMix8bit", "bitsandbytes.optim.PagedAdEMAMix8bit")
KEYS32 = {"step", "m1_m2", "nu"}
KEYS8 = {"step", "state1", "state2", "absmax1", "absmax2", "qmap1", "qmap2"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from qflux_amd import _lib
    return _lib


def hp_of(**kw):
    return dict(dict(lr=0.01, betas=R.BETAS, eps=1e-8, weight_decay=0.0, alpha=5.0, t_alpha=None, t_beta3=None), **kw)


# ---------------------------------------------------------------- schedules
def test_schedules_ramp_saturate_and_stand_still_without_a_length(lib):
    from qflux_amd import ops
    for mod in (R, ops):      # the restatement and the host side state the same two functions
        a_of = mod.alpha_t if mod is R else mod.ademamix_alpha
        b_of = mod.beta3_t if mod is R else mod.ademamix_beta3
        assert [a_of(t, 5.0, None) for t in (1, 10, 10 ** 6)] == [5.0] * 3
        assert [b_of(t, 0.9, 0.9999, None) for t in (1, 10, 10 ** 6)] == [0.9999] * 3
        al = [a_of(t, 5.0, 100) for t in range(1, 301)]
        assert al[0] == 0.05 and all(x < y for x, y in zip(al[:99], al[1:100])) and all(x == 5.0 for x in al[99:])
        for b1, b3, T in ((0.9, 0.9999, 100), (0.5, 0.999, 7), (0.9, 0.99, 4)):
            bs = [b_of(t, b1, b3, T) for t in range(1, 3 * T + 1)]
            assert b1 < bs[0] < b3 and all(x < y for x, y in zip(bs[:T - 1], bs[1:T])), (b1, b3, T)
            assert abs(bs[T - 1] - b3) <= 4 * 2.0 ** -53 and F32(bs[T - 1]) == F32(b3)      # s = 1: ln b1 ln b3 / ln b1, one rounding off at most
            assert all(x == b3 for x in bs[T:]), (b1, b3, T)                              # past it the min() holds beta3 exactly
            # the warm-up is linear in the half-life ln 0.5 / ln beta - 1 ... up to the constant: 1 / ln(beta3_t) is linear in t
            inv = [1 / math.log(x) for x in bs[:T]]
            d = np.diff(inv)
            assert np.allclose(d, d[0], rtol=1e-6)
    for t in (1, 2, 3, 4, 5, 9):
        assert ops.ademamix_alpha(t, 5.0, 3) == R.alpha_t(t, 5.0, 3) and ops.ademamix_beta3(t, 0.9, 0.9999, 4) == R.beta3_t(t, 0.9, 0.9999, 4)


def test_rows_are_the_restatements_scalars_rounded_once(lib):
    from qflux_amd import ops
    hp = hp_of(lr=3e-3, weight_decay=0.01, t_alpha=3, t_beta3=4, betas=(0.9, 0.99, 0.999))
    names = [n for n, _ in lib.AdemamixGroup._fields_][:13]
    mine = dict(lr="lr", beta1="beta1", beta2="beta2", eps="eps", weight_decay="weight_decay", one_minus_beta1="omb1", one_minus_beta2="omb2",
                beta3_t="beta3_t", one_minus_beta3_t="omb3", alpha_t="alpha_t", bias_corr1="bc1", sqrt_bias_corr2="sbc2", decay="decay")
    for t in (1, 2, 3, 4, 5, 50):
        got = ops.ademamix_rows([hp], t)[0]
        want = R.row(hp, t)
        assert len(got) == 13 and [got[i] for i in range(13)] == [want[mine[n]] for n in names], t
        g = lib.AdemamixGroup(*got)
        assert all(F32(getattr(g, n)) == R.row32(hp, t)[mine[n]] for n in names)


# ---------------------------------------------------------------- the restatement
def data(n, seed, steps):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 0.5).astype(F32), [(rng.standard_normal(n) * (0.1 + 0.05 * t)).astype(F32) for t in range(steps)]


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_alpha_zero_is_bnb_style_adamw_in_fp64(wd):
    """With alpha = 0 the slow average leaves the update: p, m1 and nu are those of AdamW with the decay after the update, to the
    last bit in double (the same operations in the same order; 0 * m2 adds an exact zero)."""
    p, grads = data(500, 3, 6)
    for sched in (dict(), dict(t_alpha=3, t_beta3=4)):
        hp = hp_of(alpha=0.0, weight_decay=wd, **sched)
        got = R.run64(p, grads, [1.0] * 6, hp)
        wp, wm, wv = R.adamw64(p, grads, hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], wd)
        assert np.array_equal(got["p"], wp) and np.array_equal(got["m1"], wm) and np.array_equal(got["nu"], wv)
        assert np.abs(got["m2"]).max() > 0      # it is still kept


def test_fp32_restatement_stays_within_roundoff_of_the_fp64_one_and_skips_non_finite_elements():
    p, grads = data(1000, 5, 5)
    hp = hp_of(weight_decay=0.01, t_alpha=3, t_beta3=4)
    r64, r32 = R.run64(p, grads, [0.5] * 5, hp), R.run32(p, grads, [F32(0.5)] * 5, hp)
    for k in ("p",) + R.STATES:
        assert r32[k].dtype == F32 and np.abs(r32[k] - r64[k]).max() < 1e-5 * max(1.0, np.abs(r64[k]).max()), k
    assert np.abs(r64["p"] - p).max() > 1e-3
    bad = [g.copy() for g in grads]
    bad[2][[3, 77]] = [np.inf, np.nan]
    for run, dt in ((R.run64, F64), (R.run32, F32)):
        full, two = run(p, bad[:3], [dt(1)] * 3, hp), run(p, bad[:2], [dt(1)] * 2, hp)
        for k in ("p",) + R.STATES:
            assert np.array_equal(full[k][[3, 77]], two[k][[3, 77]]) and np.isfinite(full[k]).all(), k
            assert (full[k][[2, 4, 76, 78]] != two[k][[2, 4, 76, 78]]).all(), k


def test_8bit_restatement_from_zero_state_zero_block_and_small_tensor():
    torch.manual_seed(0)
    sizes, bs = [700, 100], 256
    params = [torch.randn(k) * 0.5 for k in sizes]
    g = [torch.randn(k) * 0.1 for k in sizes]
    g[0][256:512] = 0
    ref = R.AdEMAMix8bitRef([p.clone() for p in params], hp_of(weight_decay=0.01), min_8bit_size=200, blocksize=bs)
    ref.step(g)
    sd = ref.state_dict()
    assert set(sd[0]) == KEYS8 and set(sd[1]) == {"step", "state1", "state2"} and sd[1]["state1"].dtype == torch.float32
    assert sd[0]["state1"].shape == (2, 700) and sd[0]["state1"].dtype == torch.uint8 and sd[0]["absmax1"].shape == (2, 3)
    assert (sd[0]["absmax1"][:, 1] == 0).all() and sd[0]["absmax2"][1] == 0
    zero = int(torch.searchsorted(ref.qmap1, torch.tensor(0.0)))
    assert ref.qmap1[zero] == 0 and (sd[0]["state1"][:, 256:512] == zero).all() and (sd[0]["state2"][256:512] == 0).all()
    # the update used the fp32 states: p equals the fp32 restatement's from zero states
    want = R.run32(params[0].numpy(), [g[0].numpy()], [F32(1)], ref.hp)["p"]
    assert np.array_equal(ref.params[0].numpy(), want)
    # both planes decode to within one code step of the fp32 averages
    dec, last = ref.decoded(0), ref.last[0]["after"]
    for k in R.STATES:
        assert np.abs(dec[k] - last[k]).max() <= 0.04 * np.abs(last[k]).max(), k


# ---------------------------------------------------------------- configuration
def test_class_paths_map_with_the_defaults_and_refuse_the_rest(lib):
    from qflux_amd.trainer import optimizer_kwargs_from_config as f
    for path in FP32_PATHS:
        for bits in (8, 32):
            assert f(path, {}, state_bits=bits) == dict(optimizer="ademamix", lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999, 0.9999),
                                                        optimizer_args={}), path
    for path in BNB_8BIT_PATHS:
        assert f(path, {}, state_bits=32)["optimizer"] == "ademamix" and f(path, {}, state_bits=8)["optimizer"] == "ademamix8bit_blockwise"
        assert f(path, {"min_8bit_size": 1024}, state_bits=8)["optimizer_args"] == {"min_8bit_size": 1024}
        assert f(path, {"min_8bit_size": 1024}, state_bits=32)["optimizer_args"] == {}
    for bits in (8, 32):
        assert f("qflux_amd.optim.AdEMAMix8bit", {}, state_bits=bits)["optimizer"] == "ademamix8bit_blockwise"
    init = dict(lr=2e-4, betas=[0.8, 0.99, 0.999], eps=1e-6, weight_decay=0.0, alpha=8, t_alpha=1000, t_beta3=2000, is_paged=True, optim_bits=32,
                min_8bit_size=64, percentile_clipping=100, max_unorm=0.0, block_wise=True)
    got = f("bitsandbytes.optim.PagedAdEMAMix8bit", init, state_bits=8)
    assert got == dict(optimizer="ademamix8bit_blockwise", lr=2e-4, betas=(0.8, 0.99, 0.999), eps=1e-6, weight_decay=0.0,
                       optimizer_args=dict(alpha=8, t_alpha=1000, t_beta3=2000, min_8bit_size=64))
    for path in FP32_PATHS + BNB_8BIT_PATHS + ("qflux_amd.optim.AdEMAMix8bit",):
        for bad in (dict(percentile_clipping=5), dict(max_unorm=1.0), dict(block_wise=False), dict(amsgrad=True), dict(foreach=True),
                    dict(fused=True), dict(cautious=True), dict(momentum=0.9)):
            with pytest.raises(NotImplementedError):
                f(path, bad, state_bits=8)
        for bad in (dict(lr=-1.0), dict(eps=-1e-8), dict(weight_decay=-0.1), dict(alpha=-1.0), dict(betas=(0.9, 0.999)), dict(betas=(0.9, 0.999, 1.0)),
                    dict(betas=(-0.1, 0.9, 0.9)), dict(betas=(0.9, 1.0, 0.9)), dict(t_alpha=0), dict(t_beta3=-5), dict(t_beta3=10, betas=(0.0, 0.9, 0.9))):
            with pytest.raises(ValueError):
                f(path, bad, state_bits=8)
    with pytest.raises(NotImplementedError, match="no fused counterpart"):
        f("bitsandbytes.optim.AdEMAMixScheduleFree", {})


def test_families_are_registered_and_the_train_steps_take_them(lib):
    from qflux_amd.trainer import FluxKontextTrainStep, QwenLoraTrainStep
    from qflux_amd.trainer import adam8bit as A8
    from qflux_amd.trainer import optim_state as OS
    assert OS.FAMILIES["ademamix"] == (OS.AdEMAMixState, 0.01) and OS.FAMILIES["ademamix8bit_blockwise"] == (OS.AdEMAMixBlockwiseState, 0.01)
    assert A8.ADEMAMIX_BLOCKWISE == ("ademamix8bit_blockwise",) and set(OS.ADEMAMIX) == {"ademamix", "ademamix8bit_blockwise"}
    assert issubclass(OS.AdEMAMixState, OS.FlatState) and OS.AdEMAMixState.GROUPED and OS.AdEMAMixState.NAMES == ("m1", "m2", "nu")
    assert OS.AdEMAMixState.DEFAULTS == dict(alpha=5.0, t_alpha=None, t_beta3=None) and OS.AdEMAMixState.BETAS == (0.9, 0.999, 0.9999)
    assert issubclass(OS.AdEMAMixBlockwiseState, OS._BlockwiseBase) and OS.AdEMAMixBlockwiseState.GROUPED
    assert OS.AdEMAMixBlockwiseState.NAMES == ("q1", "q2", "absmax1", "absmax2", "m32", "v32", "qmap1", "qmap2")
    assert OS.AdEMAMixBlockwiseState.DEFAULTS == dict(min_8bit_size=4096, blocksize=256, alpha=5.0, t_alpha=None, t_beta3=None)
    for fam in OS.ADEMAMIX:
        assert OS.default_betas(fam) == (0.9, 0.999, 0.9999)
    q = _tiny_model()
    for cls in (QwenLoraTrainStep, FluxKontextTrainStep):
        for fam in OS.ADEMAMIX:
            s = cls(q, optimizer=fam)
            assert s.betas == (0.9, 0.999, 0.9999) and s.weight_decay == 0.01 and s.optimizer == fam and s.optimizer_args["alpha"] == 5.0
            s = cls(q, optimizer=fam, optimizer_args={"t_alpha": 100, "alpha": 2}, loraplus_lr_ratio=4.0, ema_decay=0.9, max_weight_norm=1.0)
            assert s.optimizer_args["t_alpha"] == 100 and s.optimizer_args["alpha"] == 2.0 and len(s.group_rules) == 2
            for bad in ({"alpha": -1}, {"t_alpha": 0}, {"t_beta3": -1}, {"beta3": 0.9}):
                with pytest.raises(ValueError):
                    cls(q, optimizer=fam, optimizer_args=bad)
        with pytest.raises(ValueError):
            cls(q, optimizer="ademamix", optimizer_args={"blocksize": 256})
        with pytest.raises(ValueError):
            cls(q, optimizer="ademamix8bit_blockwise", optimizer_args={"blocksize": 512})


def _tiny_model():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from common import TINY
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.modules import LoraConfig
    q = QwenImageTransformer2DModel(**TINY)
    q.add_adapter(LoraConfig(r=4, lora_alpha=8, target_modules=TARGETS), "lora_edit")
    return q


def test_optim_classes_constructor_checks_and_groups(lib):
    from qflux_amd import optim as O
    assert {"AdEMAMix", "AdEMAMix8bit"} <= set(O.__all__)
    q = _tiny_model()
    params = [p for _, p in q.lora_store.params()]
    for name, fam in (("AdEMAMix", "ademamix"), ("AdEMAMix8bit", "ademamix8bit_blockwise")):
        cls = getattr(O, name)
        sig = {n: p.default for n, p in inspect.signature(cls.__init__).parameters.items() if n not in ("self", "params")}
        assert (sig["lr"], sig["betas"], sig["alpha"], sig["t_alpha"], sig["t_beta3"], sig["eps"], sig["weight_decay"]) == \
            (1e-3, (0.9, 0.999, 0.9999), 5.0, None, None, 1e-8, 1e-2)
        o = cls(params)
        g = o.param_groups[0]
        assert isinstance(o, torch.optim.Optimizer) and o.family == fam
        assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"], g["alpha"], g["t_alpha"], g["t_beta3"]) == \
            (1e-3, (0.9, 0.999, 0.9999), 1e-8, 1e-2, 5.0, None, None)
        o = cls(params, lr=2e-3, alpha=3.0, t_alpha=10, t_beta3=20, weight_decay=0.0)
        assert (o.param_groups[0]["alpha"], o.param_groups[0]["t_alpha"], o.param_groups[0]["t_beta3"]) == (3.0, 10, 20)
        for bad in (dict(lr=-1e-3), dict(eps=-1.0), dict(weight_decay=-1.0), dict(alpha=-0.5), dict(betas=(0.9, 0.999)), dict(betas=(0.9, 0.999, 1.0)),
                    dict(betas=(1.0, 0.999, 0.9)), dict(t_alpha=0), dict(t_beta3=0)):
            with pytest.raises(ValueError):
                cls(params, **bad)
        groups = O.loraplus_param_groups(q, 1e-3, 4.0)
        o = cls(groups)
        assert [g["lr"] for g in o.param_groups] == [1e-3, 4e-3] and all(g["alpha"] == 5.0 for g in o.param_groups)
    assert O.AdEMAMix8bit(params, blocksize=2048)._args["blocksize"] == 2048
    with pytest.raises(ValueError):
        O.AdEMAMix8bit(params, blocksize=512)


# ---------------------------------------------------------------- state classes on CPU tensors
def _members(st):
    names = [n for n, _, _, _ in st.entries]
    return (tuple(i for i, n in enumerate(names) if "lora_A" in n), tuple(i for i, n in enumerate(names) if "lora_B" in n)), names


def test_group_rows_and_maps(lib):
    from qflux_amd import ops
    from qflux_amd.trainer import optim_state as OS
    q = _tiny_model()
    st = q.lora_store
    members, names = _members(st)
    assign = [0 if "lora_A" in n else 1 for n in names]
    for fam in OS.ADEMAMIX:
        cls = OS.FAMILIES[fam][0]
        args = dict(cls.DEFAULTS, min_8bit_size=64) if fam.endswith("blockwise") else dict(cls.DEFAULTS)
        state = OS.ensure_state(cls, None, st, args, members)
        if fam == "ademamix":
            want = ops.tile_group_map([(off, k) for _, _, off, k in st.entries], assign, 2, numel=st.pflat.numel())
        else:
            want = ops.block_group_map(state.layout, assign, 2)
        assert state.group_map.dtype == torch.uint8 and torch.equal(state.group_map, want)
        assert OS.ensure_state(cls, state, st, args, members) is state
        one = OS.ensure_state(cls, state, st, args, None)
        assert one is state and one.group_map is None
        cls.check_groups(ops.MAX_PARAM_GROUPS)
        with pytest.raises(ValueError):
            cls.check_groups(ops.MAX_PARAM_GROUPS + 1)
        # a row without the family's own fields takes them from the optimizer_args; a row that carries them keeps them
        a = dict(args, alpha=2.0, t_alpha=7)
        rows = state._group_rows(1e-3, R.BETAS, 1e-8, 0.01, a, [dict(lr=1e-3, betas=R.BETAS, eps=1e-8, weight_decay=0.0),
                                                                dict(lr=4e-3, betas=(0.8, 0.99, 0.999), eps=1e-8, weight_decay=0.01, alpha=9.0)])
        assert [(r["alpha"], r["t_alpha"], r["t_beta3"], r["lr"]) for r in rows] == [(2.0, 7, None, 1e-3), (9.0, 7, None, 4e-3)]
        assert state._group_rows(1e-3, R.BETAS, 1e-8, 0.01, a, None) == [dict(lr=1e-3, betas=R.BETAS, eps=1e-8, weight_decay=0.01, alpha=2.0,
                                                                              t_alpha=7, t_beta3=None)]
        assert [n for n, _ in state.buffers()] == list(cls.NAMES) and cls.names(args) == cls.NAMES


def _fill(state, seed):
    g = torch.Generator().manual_seed(seed)
    for n, t in state.buffers():
        if n.startswith("qmap"):
            continue
        if t.dtype == torch.uint8:
            t.copy_(torch.randint(0, 256, t.shape, generator=g, dtype=torch.uint8))
        else:
            t.copy_(torch.rand(t.shape, generator=g) + 0.25)


@pytest.mark.parametrize("fam,bs", [("ademamix", None), ("ademamix8bit_blockwise", 256), ("ademamix8bit_blockwise", 2048)])
def test_file_layout_and_bit_for_bit_round_trip(lib, fam, bs, tmp_path):
    """state_dict -> torch.save -> load_state_dict into a fresh step -> state_dict: every tensor the same bits, the step count (the
    schedules' only input) and the family's fields included; the per-parameter keys and shapes are the documented ones."""
    from qflux_amd.trainer import QwenLoraTrainStep
    q = _tiny_model()
    st = q.lora_store
    args = dict(alpha=3.0, t_alpha=50, t_beta3=70, **({"blocksize": bs, "min_8bit_size": 64} if bs else {}))
    rules = [{"match": "lora_A", "lr": 1e-3}, {"match": "lora_B", "lr": 4e-3, "betas": (0.8, 0.99, 0.999), "weight_decay": 0.0}]
    for groups in (None, rules):
        a = QwenLoraTrainStep(q, optimizer=fam, lr=1e-3, optimizer_args=dict(args), param_groups=groups)
        assert a.state_dict()["state"] == {}      # nothing before the first step
        a._ensure_opt_state()
        _fill(a.opt_state, 5)
        a.global_step = 37
        sd = a.state_dict()
        assert sd["global_step"] == 37 and len(sd["param_groups"]) == (2 if groups else 1)
        for g in sd["param_groups"]:
            assert (g["alpha"], g["t_alpha"], g["t_beta3"]) == (3.0, 50, 70) and len(g["betas"]) == 3
        eight = 0
        shapes = {}
        members = a.param_groups_of(st)[1]
        order = [i for m in members for i in m] if members else list(range(len(st.entries)))
        for num, i in enumerate(order):
            p, e = st.entries[i][1], sd["state"][num]
            shapes[num] = tuple(p.shape)
            assert e["step"] == 37
            if fam == "ademamix":
                assert set(e) == KEYS32 and e["m1_m2"].shape == (2,) + tuple(p.shape) and e["nu"].shape == p.shape and e["m1_m2"].dtype == torch.float32
            elif p.numel() >= 64:
                nb = (p.numel() + bs - 1) // bs
                eight += 1
                assert set(e) == KEYS8 and e["state1"].shape == (2,) + tuple(p.shape) and e["state1"].dtype == torch.uint8
                assert e["state2"].shape == p.shape and e["absmax1"].shape == (2, nb) and e["absmax2"].shape == (nb,) and e["qmap1"].shape == (256,)
            else:
                assert set(e) == {"step", "state1", "state2"} and e["state1"].shape == (2,) + tuple(p.shape) and e["state1"].dtype == torch.float32
        assert fam == "ademamix" or eight > 0
        path = tmp_path / "optimizer.bin"
        torch.save(sd, path)
        # min_8bit_size is the run's own setting (a file does not carry it); everything else comes from the file
        b = QwenLoraTrainStep(_tiny_model(), optimizer=fam, lr=0.5, param_groups=groups, optimizer_args={"min_8bit_size": 64} if bs else None)
        b.load_state_dict(torch.load(path, map_location="cpu", weights_only=False))
        assert b.global_step == 37 and all(b.optimizer_args[k] == v for k, v in args.items() if k != "min_8bit_size")
        for (n, x), (_, y) in zip(a.opt_state.buffers(), b.opt_state.buffers()):
            if fam == "ademamix":
                assert torch.equal(x, y), n
        out = b.state_dict()
        assert set(out["state"]) == set(sd["state"])
        for i, e in sd["state"].items():
            for k, v in e.items():
                o = out["state"][i][k]
                assert (o == v) if not torch.is_tensor(v) else (o.dtype == v.dtype and o.shape == v.shape and
                                                               torch.equal(o.view(torch.uint8), v.view(torch.uint8))), (i, k)
        if groups:
            assert [g["lr"] for g in out["param_groups"]] == [1e-3, 4e-3] and tuple(out["param_groups"][1]["betas"]) == (0.8, 0.99, 0.999)
        # a file with a missing key or a wrong shape is refused
        if fam == "ademamix":
            for bad in ({i: {k: v for k, v in e.items() if k != "nu"} for i, e in sd["state"].items()},
                        {i: dict(e, m1_m2=e["m1_m2"][0]) for i, e in sd["state"].items()}):
                with pytest.raises(ValueError):
                    QwenLoraTrainStep(_tiny_model(), optimizer=fam, param_groups=groups).load_state_dict(dict(sd, state=bad))


# ---------------------------------------------------------------- the C ABI without a device
def test_ctypes_layout_matches_header(tmp_path, lib):
    pairs = {"qfx_ademamix_group": lib.AdemamixGroup, "qfx_ademamix_args": lib.AdemamixArgs, "qfx_ademamix8bit_args": lib.Ademamix8bitArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "qfx.h"', "int main(void) {"]
    for cname, ct in pairs.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'  printf(" %zu", offsetof({cname}, {fname}));')
        lines.append('  printf("\\n");')
    lines += ['  printf("abi %d\\n", QFX_ABI_VERSION);', "  return 0;", "}"]
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for line in out[:-1]:
        parts = line.split()
        ct = pairs[parts[0]]
        assert [int(v) for v in parts[1:]] == [C.sizeof(ct)] + [getattr(ct, f).offset for f, _ in ct._fields_], parts
    assert out[-1].split() == ["abi", "7"] and lib.ABI_VERSION == 7 and C.sizeof(lib.AdemamixGroup) == 64
    assert {"qfx_ademamix_step", "qfx_ademamix8bit_step", "qfx_ademamix8bit_step_grouped"} <= set(lib.SYMBOLS)


def good_row(lib, **kw):
    from qflux_amd import ops
    g = lib.AdemamixGroup(*ops.ademamix_rows([hp_of(weight_decay=0.01, t_alpha=3, t_beta3=4)], 2)[0])
    for k, v in kw.items():
        setattr(g, k, v)
    return g


BAD_ROWS = (dict(lr=-1e-3), dict(lr=float("nan")), dict(eps=-1e-8), dict(weight_decay=-0.01), dict(alpha_t=-1.0), dict(alpha_t=float("nan")),
            dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=-0.5), dict(beta2=float("nan")), dict(beta3_t=1.0), dict(beta3_t=-0.1),
            dict(bias_corr1=0.0), dict(bias_corr1=-0.5))


def check_refusals(lib):
    """Every QFX_EINVAL of include/qfx.h for the three AdEMAMix entries; none of them reaches a launch (the pointers are not memory)."""
    f = lib.lib.qfx_ademamix_step
    assert f(None, None) == lib.QFX_EINVAL

    def call(rows=None, **kw):
        rows = [good_row(lib)] if rows is None else rows
        arr = (lib.AdemamixGroup * max(1, len(rows)))(*rows)
        a = lib.AdemamixArgs(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 64, len(rows), 0, arr, None, None, 1.0, 1.0)
        for k, v in kw.items():
            setattr(a, k, v)
        return f(C.byref(a), None)
    for bad in (dict(p=None), dict(g=None), dict(m1=None), dict(m2=None), dict(nu=None), dict(n=0), dict(n=-64), dict(n_groups=0), dict(n_groups=17),
                dict(n_groups=2), dict(groups=None)):
        assert call(**bad) == lib.QFX_EINVAL, bad
    for bad in BAD_ROWS:
        assert call([good_row(lib, **bad)]) == lib.QFX_EINVAL, bad
        assert call([good_row(lib), good_row(lib, **bad)], tile_group=0x6000) == lib.QFX_EINVAL, bad      # in a later row too
    assert call([good_row(lib)] * 17, tile_group=0x6000) == lib.QFX_EINVAL

    f8, f8g = lib.lib.qfx_ademamix8bit_step, lib.lib.qfx_ademamix8bit_step_grouped
    assert f8(None, None) == lib.QFX_EINVAL and f8g(None, 0x6000, (lib.AdemamixGroup * 1)(good_row(lib)), 1, None) == lib.QFX_EINVAL

    def args8(**kw):
        a = lib.Ademamix8bitArgs(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 4096, 16, 64, 0x9000, 4, 256, 0xa000, 0xb000,
                                 good_row(lib), None, 1.0, 1.0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def grouped8(rows=None, bg=0xc000, n=None, **kw):
        """The grouped entry's answer.  ONLY the grouped entry is called: what makes these cases bad lies outside the args struct."""
        rows = [good_row(lib)] if rows is None else rows
        arr = (lib.AdemamixGroup * max(1, len(rows)))(*rows)
        return f8g(C.byref(args8(**kw)), bg, arr, len(rows) if n is None else n, None)

    def both8(row=None, **kw):
        """(the ungrouped entry's answer with `row` in a->hp, the grouped entry's with [row]): the struct or the row is bad for both."""
        row = good_row(lib) if row is None else row
        return f8(C.byref(args8(hp=row, **kw)), None), grouped8([row], **kw)
    for bad in [{k: None} for k in ("p", "g", "q1", "q2", "absmax1", "absmax2", "m32", "v32", "table", "qmap1", "qmap2")] + \
            [dict(blocksize=512), dict(blocksize=0), dict(n_blocks=0), dict(n_blocks=-1), dict(q1_plane=0), dict(q1_plane=4098), dict(m32_plane=62),
             dict(m32_plane=0), dict(absmax1_plane=0)]:
        assert both8(**bad) == (lib.QFX_EINVAL, lib.QFX_EINVAL), bad
    for bad in BAD_ROWS:
        assert both8(good_row(lib, **bad)) == (lib.QFX_EINVAL, lib.QFX_EINVAL), bad
        assert grouped8([good_row(lib), good_row(lib, **bad)]) == lib.QFX_EINVAL, bad      # in a later row too
    assert grouped8(bg=None) == lib.QFX_EINVAL and grouped8(n=0) == lib.QFX_EINVAL and grouped8([good_row(lib)] * 17) == lib.QFX_EINVAL
    assert f8g(C.byref(args8()), 0xc000, None, 1, None) == lib.QFX_EINVAL


def test_bad_arguments_are_rejected_without_a_device(lib):
    check_refusals(lib)


def test_host_wrappers_refuse_bad_groups_and_planes(lib):
    from qflux_amd import ops
    z = torch.zeros(64)
    with pytest.raises(ValueError):      # not on a device: refused on the host, before the library is asked
        ops.ademamix_step(z, z, z, z, z, [hp_of()], 1)
    with pytest.raises(ValueError, match="group map"):
        ops.ademamix_step(z, z, z, z, z, [hp_of(), hp_of()], 1)
    with pytest.raises(ValueError, match="triple"):
        ops.ademamix_step(z, z, z, z, z, [hp_of(betas=(0.9, 0.999))], 1)
    with pytest.raises(ValueError):
        ops.ademamix_step(z, z, z, z, z, [hp_of()] * 17, 1, tile_group=torch.zeros(1, dtype=torch.uint8))
    lay = ops.adam8bit_block_table([(0, 300)], 256, 64)
    q1, q2, a1, a2, m32, v32 = torch.zeros(2, 300, dtype=torch.uint8), torch.zeros(300, dtype=torch.uint8), torch.zeros(2, 2), torch.zeros(2), \
        torch.zeros(2, 4), torch.zeros(4)
    p = torch.zeros(300)
    qm = torch.zeros(256)
    with pytest.raises(ValueError, match="q1"):
        ops.ademamix8bit_step(p, p, q1[:, :298].contiguous(), q2, a1, a2, m32, v32, lay, qm, qm, [hp_of()], 1)
    with pytest.raises(ValueError, match="q1"):
        ops.ademamix8bit_step(p, p, q1[0], q2, a1, a2, m32, v32, lay, qm, qm, [hp_of()], 1)
    with pytest.raises(ValueError, match="absmax1"):
        ops.ademamix8bit_step(p, p, q1, q2, a1[:, :1].contiguous(), a2, m32, v32, lay, qm, qm, [hp_of()], 1)
    with pytest.raises(ValueError, match="m32"):
        ops.ademamix8bit_step(p, p, q1, q2, a1, a2, m32[:, :3].contiguous(), v32, lay, qm, qm, [hp_of()], 1)
