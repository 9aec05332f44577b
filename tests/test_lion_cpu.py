"""CPU: Lion with an fp32 and a blockwise 8-bit moment -- the restatement (tests/lion_ref.py) against a hand-computed example, the
family names, the config mapping and its refusals, the constructor signatures of the torch.optim classes, the two file layouts,
the C ABI of qfx_lion_step / qfx_lion8bit_step (no device needed), and the census of near-cancelling signs in the inputs the GPU
tests share."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnb8_ref as B  # noqa: E402
import lion_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = ["to_q", "to_k", "to_v", "to_out.0", "img_mlp.net.2", "txt_mod.1"]
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from qflux_amd import _lib
    return _lib


def test_restatement_matches_a_hand_computed_example():
    """Three elements, b1 = 0.5, b2 = 0.75, lr = 0.25, wd = 0.5 (every product exact in fp32), no clip:
      0: m = 1, g = -1:   c = 0.5 - 0.5 = 0  -> sgn 0: p = 2 * 0.875 = 1.75;         m = 0.75 - 0.25 = 0.5
      1: m = 0.5, g = 2:  c = 0.25 + 1 > 0   -> p = 4 * 0.875 - 0.25 = 3.25;        m = 0.375 + 0.5 = 0.875
      2: m = -3, g = inf: not finite          -> p = -8 and m = -3 stay
    and with g = (-4, 2, 1): element 0 has c = 0.5 - 2 < 0 -> p = 1.75 + 0.25 = 2."""
    p = torch.tensor([2.0, 4.0, -8.0])
    opt = R.LionRef([p], lr=0.25, betas=(0.5, 0.75), weight_decay=0.5)
    opt.state[0]["exp_avg"] = torch.tensor([1.0, 0.5, -3.0])
    opt.step([torch.tensor([-1.0, 2.0, float("inf")])])
    assert p.tolist() == [1.75, 3.25, -8.0]
    assert opt.state[0]["exp_avg"].tolist() == [0.5, 0.875, -3.0]
    assert opt.undecided[0].tolist() == [True, False, False]           # c == 0 from two non-zero products: the sign is undecided
    p = torch.tensor([2.0, 4.0, -8.0])
    opt = R.LionRef([p], lr=0.25, betas=(0.5, 0.75), weight_decay=0.5)
    opt.state[0]["exp_avg"] = torch.tensor([1.0, 0.5, -3.0])
    opt.step([torch.tensor([-4.0, 2.0, 1.0])])
    assert p.tolist() == [2.0, 3.25, -8.0 * 0.875 + 0.25]
    # no decay: p only moves by lr; the clip scales g' before anything else (grad_scale 0.5 turns g = -2 into the -1 of above)
    p = torch.tensor([2.0, 4.0])
    opt = R.LionRef([p], lr=0.25, betas=(0.5, 0.75))
    opt.state[0]["exp_avg"] = torch.tensor([1.0, 0.5])
    opt.step([torch.tensor([-2.0, 4.0])], grad_scale=0.5)
    assert p.tolist() == [2.0, 3.75] and opt.state[0]["exp_avg"].tolist() == [0.5, 0.875]
    # a zero gradient over a zero moment is decided: sgn(0) = 0
    p = torch.tensor([1.0])
    opt = R.LionRef([p], lr=0.25)
    opt.step([torch.tensor([0.0])])
    assert p.tolist() == [1.0] and opt.undecided[0].tolist() == [False]


def test_restatement_eight_bit_state_from_zero_and_non_finite_elements():
    """Step 1 from zero state: p' = p decay - lr sgn(g), m = (1 - b2) g quantised blockwise; a zero block stores the code of 0.0."""
    torch.manual_seed(0)
    n, lr, wd = 5000, 1e-3, 0.1
    p = torch.randn(n)
    g = torch.randn(n) * torch.logspace(-3, 1, n)
    g[:256] = 0.0
    p0 = p.clone()
    opt = R.LionRef([p], lr=lr, weight_decay=wd, min_8bit_size=4096)
    opt.step([g.clone()])
    K = R.step_scalars(lr, 0.9, 0.99, wd)
    assert torch.equal(p, p0 * K["decay"] - K["lr"] * torch.sign(g))
    st = opt.state[0]
    assert set(st) - {"_m"} == {"step", "state1", "qmap1", "absmax1"} and st["step"] == 1
    assert st["state1"].dtype == torch.uint8 and st["absmax1"].numel() == (n + 255) // 256
    assert st["absmax1"][0] == 0 and (st["state1"].view(-1)[:256] == 127).all()
    assert torch.equal(st["absmax1"], B.blocks_absmax(K["omb2"] * g, 256))
    m = B.dequant(st["state1"], st["qmap1"], st["absmax1"], 256)
    assert torch.allclose(m, K["omb2"] * g, rtol=0.1, atol=float(st["absmax1"].max()) * 2e-2)
    c1, a1, p1 = st["state1"].clone(), st["absmax1"].clone(), p.clone()
    g2 = torch.randn(n)
    g2[7], g2[260] = float("nan"), float("inf")
    opt.step([g2])
    m_old = B.dequant(c1, st["qmap1"], a1, 256)
    assert p[7] == p1[7] and p[260] == p1[260] and torch.isfinite(p).all()
    assert st["_m"][260] == m_old[260] and torch.isfinite(st["absmax1"]).all() and st["step"] == 2
    small = R.LionRef([torch.zeros(4095)], min_8bit_size=4096)
    small.step([torch.ones(4095)])
    assert set(small.state[0]) == {"step", "state1"} and small.state[0]["state1"].dtype == torch.float32


def test_resolve_family_and_default_betas(lib):
    from qflux_amd.trainer import optim_state as OS
    alias, fam, cls, wd, args = OS.resolve_family("lion")
    assert (alias, fam, cls, wd, args) == (None, "lion", OS.LionState, 0.0, {})
    alias, fam, cls, wd, args = OS.resolve_family("lion8bit_blockwise", 0.05, {"blocksize": 2048})
    assert (alias, fam, cls, wd, args) == (None, "lion8bit_blockwise", OS.LionBlockwiseState, 0.05, {"min_8bit_size": 4096, "blocksize": 2048})
    assert OS.LionState.NAMES == ("exp_avg",) and OS.LionBlockwiseState.NAMES == ("q1", "absmax1", "m32", "qmap1")
    assert OS.LionBlockwiseState.LAYOUT_ARGS == ("blocksize", "min_8bit_size")
    with pytest.raises(ValueError):
        OS.resolve_family("lion", None, {"blocksize": 256})
    with pytest.raises(ValueError):
        OS.resolve_family("lion8bit_blockwise", None, {"blocksize": 512})
    with pytest.raises(ValueError):
        OS.resolve_family("lion8bit_blockwise", None, {"d0": 1e-6})
    assert OS.default_betas("lion") == OS.default_betas("lion8bit_blockwise") == (0.9, 0.99)
    for other in ("adamw", "prodigy", "sgd", "adafactor", "adam8bit_blockwise", "adamw8bit_blockwise"):
        assert OS.default_betas(other) == (0.9, 0.999)


def test_train_step_betas_default_per_family(lib):
    from qflux_amd.trainer import FluxKontextTrainStep, QwenLoraTrainStep
    q = _tiny_model()
    for cls in (QwenLoraTrainStep, FluxKontextTrainStep):
        assert cls(q, optimizer="lion").betas == (0.9, 0.99) and cls(q, optimizer="lion").weight_decay == 0.0
        assert cls(q, optimizer="lion8bit_blockwise").betas == (0.9, 0.99)
        assert cls(q, optimizer="lion", betas=(0.9, 0.999)).betas == (0.9, 0.999)          # an explicit value is never reinterpreted
        assert cls(q, optimizer="lion", betas=[0.95, 0.98]).betas == (0.95, 0.98)
        assert cls(q).betas == (0.9, 0.999) and cls(q, optimizer="adamw8bit_blockwise").betas == (0.9, 0.999)
        assert cls(q, optimizer="sgd").betas == (0.9, 0.999) and cls(q, optimizer="prodigy", betas=(0.8, 0.9)).betas == (0.8, 0.9)
    s = QwenLoraTrainStep(q, optimizer="lion8bit_blockwise", weight_decay=0.02, optimizer_args={"blocksize": 2048, "min_8bit_size": 100})
    assert s.weight_decay == 0.02 and s.optimizer_args == {"blocksize": 2048, "min_8bit_size": 100}
    with pytest.raises(ValueError):
        QwenLoraTrainStep(q, optimizer="lion", optimizer_args={"min_8bit_size": 100})


def test_config_mapping(lib):
    from qflux_amd.trainer import optimizer_kwargs_from_config as f
    for path in ("lion_pytorch.Lion", "bitsandbytes.optim.Lion", "bitsandbytes.optim.Lion32bit"):
        for bits in (32, 8):
            assert f(path, {"lr": 1e-4, "betas": [0.95, 0.98], "weight_decay": 0.1}, state_bits=bits) == \
                {"lr": 1e-4, "betas": (0.95, 0.98), "weight_decay": 0.1, "optimizer": "lion"}
        assert f(path, {"lr": 3e-5}) == {"lr": 3e-5, "optimizer": "lion", "weight_decay": 0.0}       # betas left to the family
    assert f("lion_pytorch.Lion", {"lr": 1e-4, "use_triton": True, "decoupled_weight_decay": False, "cautious_factor": 1.0}) == \
        {"lr": 1e-4, "optimizer": "lion", "weight_decay": 0.0}
    for bad in ({"decoupled_weight_decay": True}, {"cautious_factor": 0.5}, {"momentum": 0.9}):
        with pytest.raises(NotImplementedError):
            f("lion_pytorch.Lion", dict(lr=1e-4, **bad))
    for cls in ("Lion8bit", "PagedLion8bit"):
        init = {"lr": 1e-4, "betas": [0.9, 0.99], "is_paged": True, "percentile_clipping": 100, "block_wise": True, "min_8bit_size": 2048}
        assert f("bitsandbytes.optim." + cls, init, state_bits=8) == \
            {"lr": 1e-4, "betas": (0.9, 0.99), "optimizer": "lion8bit_blockwise", "weight_decay": 0.0, "optimizer_args": {"min_8bit_size": 2048}}
        assert f("bitsandbytes.optim." + cls, init) == {"lr": 1e-4, "betas": (0.9, 0.99), "optimizer": "lion", "weight_decay": 0.0}
        assert f("bitsandbytes.optim." + cls, {"lr": 1e-4, "weight_decay": 0.05}, state_bits=8)["weight_decay"] == 0.05
        for bits in (32, 8):                                             # the project's own classes are named for their state
            assert f("qflux_amd.optim." + cls, {"lr": 1e-4}, state_bits=bits) == \
                {"lr": 1e-4, "optimizer": "lion8bit_blockwise", "weight_decay": 0.0}
        for path in ("bitsandbytes.optim." + cls, "qflux_amd.optim." + cls):
            for bad in ({"percentile_clipping": 5}, {"max_unorm": 1.0}, {"block_wise": False}, {"skip_zeros": True}, {"amsgrad": True}):
                with pytest.raises(NotImplementedError):
                    f(path, dict(lr=1e-4, **bad), state_bits=8)
    # what was mapped or refused before stays so; that includes the path qflux_amd.optim.Lion, whose refusal tests/test_optim_classes_cpu.py
    # pins (the class itself exists and maps as lion_pytorch.Lion: test_constructor_signatures)
    with pytest.raises(NotImplementedError):
        f("qflux_amd.optim.Lion", {"lr": 0.1})
    assert f("bitsandbytes.optim.Adam8bit", {"lr": 1e-4, "betas": [0.9, 0.999]}) == \
        {"lr": 1e-4, "betas": (0.9, 0.999), "optimizer": "adam8bit", "weight_decay": 0.0}
    assert f("bitsandbytes.optim.AdamW8bit", {"lr": 1e-4}, state_bits=8)["optimizer"] == "adamw8bit_blockwise"
    for path in ("torch.optim.SGD", "lion_pytorch.LionW", "bitsandbytes.optim.Lion4bit", "torch.optim.RMSprop"):
        with pytest.raises(NotImplementedError):
            f(path, {"lr": 1e-4})


def test_constructor_signatures(lib):
    from qflux_amd import optim as O
    assert {"Lion", "Lion8bit", "PagedLion8bit"} <= set(O.__all__)

    def sig(cls):
        return {n: p.default for n, p in inspect.signature(cls.__init__).parameters.items() if n not in ("self", "params")}
    lion = sig(O.Lion)
    assert list(lion)[:3] == ["lr", "betas", "weight_decay"]
    assert (lion["lr"], lion["betas"], lion["weight_decay"]) == (1e-4, (0.9, 0.99), 0.0)
    assert lion["use_triton"] is False and lion["decoupled_weight_decay"] is False and lion["cautious_factor"] == 1.0
    for cls in (O.Lion8bit, O.PagedLion8bit):
        s = sig(cls)
        assert list(s)[:9] == ["lr", "betas", "weight_decay", "optim_bits", "args", "min_8bit_size", "percentile_clipping", "block_wise",
                               "is_paged"]
        assert [s[n] for n in list(s)[:9]] == [1e-4, (0.9, 0.99), 0, 32, None, 4096, 100, True, False]
        assert s["blocksize"] == 256
    assert issubclass(O.PagedLion8bit, O.Lion8bit) and issubclass(O.Lion, torch.optim.Optimizer)
    q = _tiny_model()
    params = [p for _, p in q.lora_store.params()]
    o = O.Lion(params)
    assert o.family == "lion" and o.param_groups[0]["betas"] == (0.9, 0.99) and o.param_groups[0]["weight_decay"] == 0.0
    assert O.Lion(params, use_triton=True, decoupled_weight_decay=False).param_groups[0]["lr"] == 1e-4
    o8 = O.PagedLion8bit(params, lr=3e-4, is_paged=True, min_8bit_size=2048, blocksize=2048)
    assert o8.family == "lion8bit_blockwise" and o8._args == {"min_8bit_size": 2048, "blocksize": 2048}
    for cls, bad in ((O.Lion, {"decoupled_weight_decay": True}), (O.Lion, {"cautious_factor": 0.5}), (O.Lion8bit, {"percentile_clipping": 5}),
                     (O.Lion8bit, {"block_wise": False}), (O.Lion8bit, {"args": object()})):
        with pytest.raises(NotImplementedError):
            cls(params, **bad)


def _tiny_model():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from common import TINY
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.modules import LoraConfig
    q = QwenImageTransformer2DModel(**TINY)
    q.add_adapter(LoraConfig(r=4, lora_alpha=8, target_modules=TARGETS), "lora_edit")
    return q


def _file(q, min_8bit_size, bs=256, steps=3, wd=0.0):
    torch.manual_seed(4)
    ps = [torch.randn(p.shape) * 0.1 for _, p in q.lora_store.params()]
    opt = R.LionRef(ps, lr=1e-3, betas=(0.95, 0.98), weight_decay=wd, min_8bit_size=min_8bit_size, blocksize=bs)
    for _ in range(steps):
        opt.step([torch.randn(p.shape) for p in ps])
    return opt.state_dict()


def _same(out, sd):
    assert set(out["state"]) == set(sd["state"])
    for i, e in sd["state"].items():
        o = out["state"][i]
        assert set(o) == set(e), (i, sorted(o), sorted(e))
        for k, v in e.items():
            if torch.is_tensor(v):
                assert o[k].dtype == v.dtype and o[k].shape == v.shape and torch.equal(o[k], v), (i, k)
            else:
                assert o[k] == v, (i, k)


@pytest.mark.parametrize("bs", [256, 2048])
def test_bnb_one_state_layout_round_trip(lib, bs):
    """bnb's Optimizer1State keys through LionBlockwiseState.load / .save; the block size (2048 too) comes from the file."""
    from qflux_amd.trainer import QwenLoraTrainStep
    from qflux_amd.trainer import optim_state as OS
    q = _tiny_model()
    sd = _file(q, 4096, bs, wd=0.01)
    assert {frozenset(e) for e in sd["state"].values()} == {frozenset({"step", "state1"}), frozenset({"step", "state1", "qmap1", "absmax1"})}
    args = dict(min_8bit_size=4096, blocksize=256)
    state, n = OS.LionBlockwiseState.load(q.lora_store, sd, args)
    assert n == 3 and args["blocksize"] == bs and state.layout.blocksize == bs
    extra, per = OS.LionBlockwiseState.save(state, q.lora_store.entries, n, args)
    assert extra == {}
    _same({"state": per}, sd)
    assert OS.LionBlockwiseState.save(None, q.lora_store.entries, 0, args) == ({}, {})
    # and through the train step
    step = QwenLoraTrainStep(q, optimizer="lion8bit_blockwise")
    step.load_state_dict(sd)
    assert step.optimizer_args["blocksize"] == bs and step.global_step == 3 and step.betas == (0.95, 0.98)
    out = step.state_dict()
    assert out["param_groups"][0]["weight_decay"] == 0.01 and out["param_groups"][0]["lr"] == 1e-3
    _same(out, sd)
    bad = {"state": {i: dict(e) for i, e in sd["state"].items()}, "param_groups": sd["param_groups"]}
    with pytest.raises(ValueError):
        OS.LionBlockwiseState.load(q.lora_store, bad, dict(min_8bit_size=1 << 20, blocksize=256))      # another min_8bit_size


def test_lion_pytorch_layout_round_trip_and_bnb_32bit_file(lib):
    from qflux_amd.trainer import QwenLoraTrainStep
    from qflux_amd.trainer import optim_state as OS
    q = _tiny_model()
    sd = _file(q, None, wd=0.01)
    assert {frozenset(e) for e in sd["state"].values()} == {frozenset({"exp_avg"})}
    state, n = OS.LionState.load(q.lora_store, sd, {})
    assert n == 0                                                         # lion_pytorch counts no steps
    extra, per = OS.LionState.save(state, q.lora_store.entries, n, {})
    assert extra == {}
    _same({"state": per}, sd)
    assert OS.LionState.save(None, q.lora_store.entries, 0, {}) == ({}, {})
    step = QwenLoraTrainStep(q, optimizer="lion", lr=0.5)
    step.load_state_dict(sd)
    assert step.lr == 1e-3 and step.betas == (0.95, 0.98) and step.weight_decay == 0.01
    out = step.state_dict()
    assert set(out["param_groups"][0]) >= {"lr", "betas", "weight_decay", "params"}
    _same(out, sd)
    # a bitsandbytes 32-bit Lion file (every state1 in fp32) loads into "lion" with the same moments
    sd32 = _file(q, 1 << 30)
    assert {frozenset(e) for e in sd32["state"].values()} == {frozenset({"step", "state1"})}
    step = QwenLoraTrainStep(q, optimizer="lion")
    step.load_state_dict(sd32)
    assert step.global_step == 3
    for i, (_, p, off, k) in enumerate(q.lora_store.entries):
        assert torch.equal(step.opt_state.exp_avg[off:off + k], sd32["state"][i]["state1"].reshape(-1))
    assert {frozenset(e) for e in step.state_dict()["state"].values()} == {frozenset({"exp_avg"})}
    # and an 8-bit one with its moment dequantised
    sd8 = _file(q, 4096, 2048)
    step = QwenLoraTrainStep(q, optimizer="lion")
    step.load_state_dict(sd8)
    for i, (_, p, off, k) in enumerate(q.lora_store.entries):
        e = sd8["state"][i]
        want = B.dequant(e["state1"], e["qmap1"], e["absmax1"], 2048) if e["state1"].dtype == torch.uint8 else e["state1"].reshape(-1)
        assert torch.equal(step.opt_state.exp_avg[off:off + k], want)


def test_ctypes_layout_matches_header(tmp_path, lib):
    pairs = {"qfx_lion8bit_args": lib.Lion8bitArgs, "qfx_adam8bit_block": lib.Adam8bitBlock}
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
    assert out[-1].split() == ["abi", str(lib.ABI_VERSION)] and lib.ABI_VERSION == 7       # append-only: the version stays
    assert [f for f, _ in lib.Lion8bitArgs._fields_] == [f for f, _ in lib.Adam8bitArgs._fields_
                                                        if f not in ("q2", "absmax2", "v32", "qmap2", "eps", "step")]
    assert "qfx_lion_step" in lib.SYMBOLS and "qfx_lion8bit_step" in lib.SYMBOLS


def test_bad_arguments_are_rejected_without_a_device(lib):
    f = lib.lib.qfx_lion_step
    ok = dict(p=0x1000, g=0x2000, m=0x3000, n=16, lr=1e-4, beta1=0.9, beta2=0.99, weight_decay=0.0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["p"], a["g"], a["m"], a["n"], a["lr"], a["beta1"], a["beta2"], a["weight_decay"], None, 1.0, 1.0, None)
    for bad in (dict(p=None), dict(g=None), dict(m=None), dict(n=0), dict(n=-4), dict(lr=-1e-4), dict(lr=float("nan")), dict(beta1=1.0),
                dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=-0.5), dict(weight_decay=-0.01)):
        assert call(**bad) == lib.QFX_EINVAL, bad
    f8 = lib.lib.qfx_lion8bit_step
    assert f8(None, None) == lib.QFX_EINVAL
    a = lib.Lion8bitArgs()
    assert f8(C.byref(a), None) == lib.QFX_EINVAL                       # NULL pointers
    ptrs = ("p", "g", "q1", "absmax1", "m32", "table", "qmap1")

    def fresh(**kw):
        a = lib.Lion8bitArgs()
        for name in ptrs:
            setattr(a, name, 0x1000)
        a.n_blocks, a.blocksize, a.lr, a.beta1, a.beta2, a.weight_decay, a.max_norm, a.grad_scale = 1, 256, 1e-4, 0.9, 0.99, 0.0, 1.0, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for name in ptrs:
        assert f8(C.byref(fresh(**{name: None})), None) == lib.QFX_EINVAL, name
    for bad in (dict(blocksize=512), dict(blocksize=0), dict(n_blocks=0), dict(n_blocks=-1), dict(lr=-1.0), dict(beta1=1.0),
                dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=-0.1), dict(weight_decay=-0.5)):
        assert f8(C.byref(fresh(**bad)), None) == lib.QFX_EINVAL, bad


@pytest.mark.parametrize("bs,wd", [(None, 0.0), (256, 0.01), (2048, 0.01)])
def test_near_cancellation_census_of_the_shared_inputs(bs, wd):
    """The GPU tests exempt an element from the parameter comparison only where the restatement itself calls the sign of c undecided
    (lion_ref.update), and cap the share of such elements per step.  With the seeds and sizes they use, that share must be within
    the cap -- counted outside the deliberately zeroed block, where both products are exactly zero and the sign is decided."""
    total = sum(R.SIZES)
    zero_lo, zero_n = 0, (bs or 256)
    for it, rec in enumerate(R.run_reference(bs, wd)):
        und = rec["undecided"]
        assert not und[4][zero_lo:zero_lo + zero_n].any()               # c == 0 from 0 + 0: decided
        m4 = rec["after"][1][4]
        moment = m4["exp_avg"] if "exp_avg" in m4 else m4["_m"]
        assert (moment.reshape(-1)[:zero_n] == 0).all() and torch.equal(rec["after"][0][4][:zero_n], rec["before"][0][4][:zero_n] *
                                                                       R.step_scalars(R.KW["lr"], *R.KW["betas"], wd)["decay"])
        n_und = sum(int(u.sum()) for u in und)
        print(f"lion census bs={bs} step {it}: {n_und} undecided of {total}")
        assert n_und <= R.UNDECIDED_CAP * total, (bs, it, n_und)
