"""CPU: optimizer="adafactor" -- the restatement tests/adafactor_ref.py against a hand derivation (and against the transformers
package where it is installed), the config mapping and its refusals, resolve_family, the struct layouts against include/qfx.h, the
descriptor table, argument validation of qfx_adafactor_step without a launch, and transformers' checkpoint layout in both directions
with shape validation on load."""
import ctypes as C
import math
import os
import subprocess

import pytest
import torch

import adafactor_ref as R
from test_sgd_cpu import toy_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_matches_a_hand_derivation_of_one_step():
    """Step t = 1 on a 2 x 3 matrix with external lr, beta1 and weight decay, every formula of the issue written out on Python floats
    (float64): beta2_1 = 0, so the statistics are the plain means."""
    p0 = [[0.5, -1.0, 2.0], [1.5, 0.25, -0.75]]
    g0 = [[0.1, -0.2, 0.3], [-0.4, 0.5, 0.6]]
    eps1, eps2, thr, lr_ext, beta1, wd, gs = 1e-30, 1e-3, 0.5, 1e-2, 0.9, 0.1, 0.5
    g = [[x * gs for x in r] for r in g0]                                  # no gnorm_sq: clip = grad_scale
    rms = math.sqrt(sum(x * x for r in p0 for x in r)) / math.sqrt(6)
    lr = lr_ext * max(eps2, rms)
    b2 = 1.0 - 1.0 ** -0.8
    assert b2 == 0.0
    u = [[x * x + eps1 for x in r] for r in g]
    row = [b2 * 0.0 + (1 - b2) * (sum(r) / 3) for r in u]
    col = [b2 * 0.0 + (1 - b2) * ((u[0][c] + u[1][c]) / 2) for c in range(3)]
    rmean = (row[0] + row[1]) / 2
    upd = [[g[r][c] / math.sqrt(row[r] / rmean) / math.sqrt(col[c]) for c in range(3)] for r in range(2)]
    urms = math.sqrt(sum(x * x for r in upd for x in r) / 6)
    den = max(1.0, urms / thr)
    assert den > 1.0                       # the update clip is active in this example
    upd = [[x / den * lr for x in r] for r in upd]
    m = [[beta1 * 0.0 + (1 - beta1) * x for x in r] for r in upd]
    want_p = [[p0[r][c] - wd * lr * p0[r][c] - m[r][c] for c in range(3)] for r in range(2)]

    p = [torch.tensor(p0, dtype=torch.float64)]
    st = R.new_state([(2, 3)], beta1=beta1, dtype=torch.float64)
    R.step(p, [torch.tensor(g0, dtype=torch.float64)], st, 1, dtype=torch.float64, grad_scale=gs, lr=lr_ext, relative_step=False,
           beta1=beta1, weight_decay=wd, eps=(eps1, eps2), clip_threshold=thr)
    D = torch.float64
    tight = dict(rtol=1e-13, atol=0)
    torch.testing.assert_close(p[0], torch.tensor(want_p, dtype=D), **tight)
    torch.testing.assert_close(st[0]["exp_avg_sq_row"], torch.tensor(row, dtype=D), **tight)
    torch.testing.assert_close(st[0]["exp_avg_sq_col"], torch.tensor(col, dtype=D), **tight)
    torch.testing.assert_close(st[0]["exp_avg"], torch.tensor(m, dtype=D), **tight)
    torch.testing.assert_close(st[0]["RMS"], torch.tensor(rms, dtype=D), **tight)
    # the relative step and the unfactored path, second step: lr = min(1e-2, 1 / sqrt(2)) * max(eps2, RMS), beta2_2 = 1 - 2^-0.8
    pv, gv, v1 = [0.3, -0.4], [0.02, 0.05], [1e-4, 4e-4]
    b2 = 1.0 - 2.0 ** -0.8
    v = [b2 * v1[i] + (1 - b2) * (gv[i] ** 2 + eps1) for i in range(2)]
    uu = [gv[i] / math.sqrt(v[i]) for i in range(2)]
    den = max(1.0, math.sqrt((uu[0] ** 2 + uu[1] ** 2) / 2) / 1.0)
    lr = min(1e-2, 1 / math.sqrt(2)) * max(eps2, math.sqrt((0.09 + 0.16) / 2))
    want = [pv[i] - uu[i] / den * lr for i in range(2)]
    p = [torch.tensor(pv, dtype=D)]
    st = R.new_state([(2,)], dtype=D)
    st[0]["exp_avg_sq"] = torch.tensor(v1, dtype=D)
    R.step(p, [torch.tensor(gv, dtype=D)], st, 2, dtype=D)
    torch.testing.assert_close(p[0], torch.tensor(want, dtype=D), **tight)
    torch.testing.assert_close(st[0]["exp_avg_sq"], torch.tensor(v, dtype=D), **tight)
    # warm-up: 1e-6 t
    assert R.host_scalars(7, warmup_init=True)[0] == 7e-6 and R.host_scalars(10 ** 6, warmup_init=False)[0] == 1e-3


def test_restatement_skips_a_tensor_with_a_non_finite_gradient():
    g = torch.Generator().manual_seed(3)
    ps = [torch.randn(3, 4, generator=g), torch.randn(5, generator=g)]
    gs = [torch.randn(3, 4, generator=g), torch.randn(5, generator=g)]
    gs[0][1, 2] = float("inf")
    st = R.new_state([(3, 4), (5,)])
    before = [p.clone() for p in ps]
    R.step(ps, gs, st, 1)
    assert torch.equal(ps[0], before[0]) and not st[0]["exp_avg_sq_row"].any() and st[0]["RMS"] == 0
    assert not torch.equal(ps[1], before[1]) and st[1]["exp_avg_sq"].all()


CONFIGS = [dict(), dict(lr=1e-3, relative_step=False, beta1=0.9, weight_decay=1e-2), dict(warmup_init=True),
           dict(scale_parameter=False, clip_threshold=0.5, decay_rate=-0.5)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=["defaults", "external_lr", "warmup", "unscaled"])
def test_restatement_matches_transformers(cfg):
    T = pytest.importorskip("transformers.optimization")
    g = torch.Generator().manual_seed(11)
    shapes = [(3, 40), (130, 5), (7,)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g) * 0.1) for s in shapes]
    mine = [p.detach().clone() for p in ps]
    st = R.new_state(shapes, beta1=cfg.get("beta1"))
    opt = T.Adafactor(ps, **dict(dict(lr=None), **cfg))
    for t in range(1, 6):
        grads = [torch.randn(s, generator=g) * 1e-2 for s in shapes]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt.step()
        R.step(mine, grads, st, t, **cfg)
    # bar: 1e-5 of the tensor's maximum, what test_kernels_gpu.py::test_adamw_matches_torch grants two fp32 statements of one
    # optimizer (the package multiplies in place and takes rsqrt / mean where the kernel divides: a few roundings per element and step)
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    for p, q, e in zip(ps, mine, st):
        assert rel(q, p.detach()) <= 1e-5
        for k, v in opt.state[p].items():
            if torch.is_tensor(v):
                assert v.abs().max() > 0 and rel(e[k], v) <= 1e-5, (k, rel(e[k], v))


def test_config_mapping_and_its_refusals():
    from qflux_amd.trainer import optimizer_kwargs_from_config as f
    for path in ("transformers.optimization.Adafactor", "transformers.Adafactor", "qflux_amd.optim.Adafactor"):
        assert f(path, {}) == {"optimizer": "adafactor", "lr": None, "optimizer_args": {}}
        kw = f(path, {"lr": 1e-3, "relative_step": False, "scale_parameter": False, "beta1": 0.9, "weight_decay": 0.01,
                      "eps": [1e-30, 1e-3], "clip_threshold": 1.0, "decay_rate": -0.8, "warmup_init": False})
        assert kw == {"optimizer": "adafactor", "lr": 1e-3, "weight_decay": 0.01,
                      "optimizer_args": {"relative_step": False, "scale_parameter": False, "beta1": 0.9, "eps": (1e-30, 1e-3),
                                         "clip_threshold": 1.0, "decay_rate": -0.8, "warmup_init": False}}
        with pytest.raises(ValueError, match="relative_step"):
            f(path, {"lr": 1e-3})                                        # lr with the default relative_step=True
        with pytest.raises(ValueError, match="warmup_init"):
            f(path, {"lr": 1e-3, "relative_step": False, "warmup_init": True})
        with pytest.raises(ValueError, match="learning rate"):
            f(path, {"relative_step": False})
        with pytest.raises(NotImplementedError, match="momentum"):
            f(path, {"momentum": 0.9})
        with pytest.raises(NotImplementedError, match="betas"):
            f(path, {"betas": [0.9, 0.99]})
    with pytest.raises(NotImplementedError):
        f("torch.optim.Adafactor", {})                                   # another class with other semantics: not mapped
    with pytest.raises(NotImplementedError):
        f("torch.optim.SGD", {"lr": 0.1})


def test_resolve_family_and_the_train_steps_accept_adafactor():
    from qflux_amd.trainer import FluxKontextTrainStep, QwenLoraTrainStep
    from qflux_amd.trainer.optim_state import AdafactorState, resolve_family
    alias, fam, cls, wd, args = resolve_family("adafactor")
    assert (alias, fam, cls, wd) == (None, "adafactor", AdafactorState, 0.0)
    assert args == dict(eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, scale_parameter=True, relative_step=True,
                        warmup_init=False)
    assert resolve_family("adafactor", 0.01, {"beta1": 0.9, "eps": [1e-20, 1e-2]})[3:] == (0.01, dict(args, beta1=0.9, eps=(1e-20, 1e-2)))
    assert AdafactorState.names(args) == ("row", "col", "v", "rms") and AdafactorState.names(dict(args, beta1=0.9))[-1] == "m"
    with pytest.raises(ValueError, match="unsupported optimizer_args"):
        resolve_family("adafactor", None, {"momentum": 0.9})
    with pytest.raises(ValueError, match="warmup_init"):
        resolve_family("adafactor", None, {"warmup_init": True, "relative_step": False})
    with pytest.raises(ValueError, match="pair"):
        resolve_family("adafactor", None, {"eps": 1e-8})
    with pytest.raises(ValueError, match="unknown optimizer"):
        resolve_family("adafactor8bit")
    toy = toy_model()
    s = QwenLoraTrainStep(toy, lr=None, optimizer="adafactor")
    assert s.lr is None and s.weight_decay == 0.0 and s.optimizer_args == args
    s = FluxKontextTrainStep(toy, lr=1e-3, weight_decay=0.01, optimizer="adafactor", optimizer_args={"relative_step": False, "beta1": 0.9})
    assert s.lr == 1e-3 and s.weight_decay == 0.01 and s.optimizer_args["beta1"] == 0.9
    with pytest.raises(ValueError, match="relative_step"):
        QwenLoraTrainStep(toy, lr=1e-4, optimizer="adafactor")
    with pytest.raises(ValueError, match="learning rate"):
        QwenLoraTrainStep(toy, lr=None, optimizer="adafactor", optimizer_args={"relative_step": False})
    # before the first step: transformers' empty state, its options in the group
    sd = QwenLoraTrainStep(toy, lr=None, optimizer="adafactor").state_dict()
    g = sd["param_groups"][0]
    assert sd["state"] == {} and g["lr"] is None and g["eps"] == (1e-30, 1e-3) and g["relative_step"] is True and g["beta1"] is None


def test_torch_optim_class_refuses_what_the_others_refuse():
    from qflux_amd import optim as O
    toy = toy_model()
    ps = [p for _, p in toy.lora_store.params()]
    opt = O.Adafactor(ps)
    g = opt.param_groups[0]
    assert isinstance(opt, torch.optim.Optimizer) and opt.family == "adafactor"
    assert g["lr"] is None and g["eps"] == (1e-30, 1e-3) and g["relative_step"] is True and g["weight_decay"] == 0.0
    assert opt.state_dict()["state"] == {}
    with pytest.raises(ValueError, match="missing"):
        O.Adafactor(ps[:-1])
    with pytest.raises(ValueError, match="not an adapter parameter"):
        O.Adafactor(ps + [torch.nn.Parameter(torch.zeros(3))])
    with pytest.raises(ValueError, match="parameter groups"):
        O.Adafactor([{"params": ps[:2]}, {"params": ps[2:]}])
    with pytest.raises(ValueError, match="relative_step"):
        O.Adafactor(ps, lr=1e-3)
    with pytest.raises(ValueError, match="warmup_init"):
        O.Adafactor(ps, lr=1e-3, relative_step=False, warmup_init=True)


def test_ctypes_structs_match_the_c_header_layout(tmp_path):
    from qflux_amd import _lib as L
    pairs = {"qfx_adafactor_tensor": L.AdafactorTensor, "qfx_adafactor_args": L.AdafactorArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "qfx.h"', "int main(void) {"]
    for cname, ct in pairs.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'  printf(" %zu", offsetof({cname}, {fname}));')
        lines.append('  printf("\\n");')
    lines += ["  return 0;", "}"]
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(out) == len(pairs)
    for line in out:
        parts = line.split()
        ct = pairs[parts[0]]
        want = [C.sizeof(ct)] + [getattr(ct, f).offset for f, _ in ct._fields_]
        assert [int(v) for v in parts[1:]] == want, (parts[0], parts[1:], want)
    assert L.ABI_VERSION == 7 and "qfx_adafactor_step" in L.SYMBOLS


def test_descriptor_table_layout_and_refusals():
    from qflux_amd import _lib as L
    from qflux_amd import ops
    lay = ops.adafactor_table([(0, (1, 32)), (32, (130, 5)), (700, (7,)), (710, (16, 3072))])
    assert (lay.n_tensors, lay.n_row, lay.n_col, lay.n_v, lay.extent) == (4, 1 + 130 + 16, 32 + 5 + 3072, 7, 710 + 16 * 3072)
    assert lay.tensors[1] == (32, 130, 5, True, 1, 32, -1) and lay.tensors[2] == (700, 1, 7, False, -1, -1, 0)
    arr = (L.AdafactorTensor * 4).from_buffer_copy(lay.table.numpy().tobytes())
    assert [(d.off, d.row, d.col, d.v, d.m, d.rows, d.cols, d.rms, d.factored) for d in arr] == [
        (0, 0, 0, 0, 0, 1, 32, 0, 1), (32, 1, 32, 0, 32, 130, 5, 1, 1), (700, 0, 0, 0, 700, 1, 7, 2, 0),
        (710, 131, 37, 0, 710, 16, 3072, 3, 1)]
    for bad in ([], [(0, (2, 3, 4))], [(-4, (2, 3))], [(0, (0, 3))], [(0, (1 << 16, 1 << 15))]):
        with pytest.raises(ValueError):
            ops.adafactor_table(bad)


def test_adafactor_step_rejects_bad_arguments_before_any_launch():
    from qflux_amd import _lib as L
    f = L.lib.qfx_adafactor_step

    def args(**kw):
        a = L.AdafactorArgs(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, None, 0x6000, 0x7000, 3, 1, 0, 1e-2, 0.5, 0.5, 1e-30, 1e-3, 1.0,
                            0.0, 1.0, 0.0, None, 0.0, 1.0)     # never dereferenced: every call below is rejected on the host
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert f(None, None) == L.QFX_EINVAL
    assert f(args(n_tensors=0, table=None), None) == L.QFX_OK            # nothing to do, nothing launched
    for kw in (dict(n_tensors=-1), dict(table=None), dict(p=None), dict(g=None), dict(row=None), dict(col=None), dict(v=None),
               dict(rms=None), dict(use_beta1=1), dict(use_beta1=1, m=0x8000, beta1=1.0), dict(lr=-1.0), dict(beta2t=1.0),
               dict(beta2t=-0.1), dict(one_minus_beta2t=0.0), dict(clip_threshold=0.0), dict(eps1=-1.0), dict(weight_decay=-0.1),
               dict(lr=float("nan"))):
        assert f(args(**kw), None) == L.QFX_EINVAL, kw


def _filled_state(toy, beta1):
    from qflux_amd.trainer import QwenLoraTrainStep
    args = {"beta1": beta1} if beta1 is not None else None
    step = QwenLoraTrainStep(toy, lr=None, optimizer="adafactor", optimizer_args=args)
    st = toy.lora_store
    step.opt_state = step._opt_cls(st, step.optimizer_args)
    g = torch.Generator().manual_seed(5)
    for n, t in step.opt_state.buffers():
        if n != "v":                        # no unfactored tensor in the toy: the placeholder element is not part of any file
            t.copy_(torch.rand(t.shape, generator=g) + 0.5)
    step.global_step = 4
    return step


@pytest.mark.parametrize("beta1", [None, 0.9])
def test_state_dict_has_transformers_layout_and_round_trips(beta1, tmp_path):
    from qflux_amd.trainer import QwenLoraTrainStep
    toy = toy_model()
    st = toy.lora_store
    step = _filled_state(toy, beta1)
    assert [n for n, _ in step._state_buffers()] == ["lora", "row", "col", "v", "rms"] + (["m"] if beta1 else [])
    torch.save(step.state_dict(), str(tmp_path / "optimizer.bin"))
    sd = torch.load(str(tmp_path / "optimizer.bin"), map_location="cpu", weights_only=False)
    g = sd["param_groups"][0]
    assert g["params"] == list(range(len(st.entries))) and g["beta1"] == beta1 and g["eps"] == (1e-30, 1e-3) and g["lr"] is None
    assert {"clip_threshold", "decay_rate", "scale_parameter", "relative_step", "warmup_init", "weight_decay"} <= set(g)
    lay = step.opt_state.layout
    for i, (_, p, off, k) in enumerate(st.entries):
        e = sd["state"][i]
        assert set(e) == {"step", "RMS", "exp_avg_sq_row", "exp_avg_sq_col"} | ({"exp_avg"} if beta1 else set())
        assert e["step"] == 4 and e["RMS"].shape == () and e["RMS"] == step.opt_state.rms[i]
        assert e["exp_avg_sq_row"].shape == p.shape[:-1] and e["exp_avg_sq_col"].shape == p.shape[-1:]
        r0, c0 = lay.tensors[i][4], lay.tensors[i][5]
        assert torch.equal(e["exp_avg_sq_row"], step.opt_state.row[r0:r0 + p.shape[0]])
        assert torch.equal(e["exp_avg_sq_col"], step.opt_state.col[c0:c0 + p.shape[1]])
        if beta1:
            assert torch.equal(e["exp_avg"], step.opt_state.m[off:off + k].view(p.shape))
    fresh = QwenLoraTrainStep(toy, lr=None, eps=1e-6, optimizer="adafactor")
    fresh.load_state_dict(sd)
    assert fresh.global_step == 4 and fresh.optimizer_args["beta1"] == beta1 and fresh.lr is None and fresh.eps == 1e-6
    for (n, x), (_, y) in zip(step.opt_state.buffers(), fresh.opt_state.buffers()):
        if n == "m":                        # indexed like pflat: the padding between two parameters is in no file
            assert all(torch.equal(x[off:off + k], y[off:off + k]) for _, _, off, k in st.entries)
        else:
            assert torch.equal(x, y), n
    # the torch.optim class reads and writes the same file
    from qflux_amd import optim as O
    opt = O.Adafactor([p for _, p in st.params()])
    opt.load_state_dict(sd)
    assert opt._step_count_fused == 4 and opt.param_groups[0]["beta1"] == beta1
    back = opt.state_dict()
    for i, e in sd["state"].items():
        for key, v in e.items():
            assert torch.equal(back["state"][i][key], v) if torch.is_tensor(v) else back["state"][i][key] == v


def test_load_validates_shapes():
    from qflux_amd.trainer import QwenLoraTrainStep
    toy = toy_model()
    sd = _filled_state(toy, 0.9).state_dict()
    fresh = lambda: QwenLoraTrainStep(toy, lr=None, optimizer="adafactor")

    def broken(fn):
        bad = {"state": {i: dict(e) for i, e in sd["state"].items()}, "param_groups": [dict(sd["param_groups"][0])], "global_step": 4}
        fn(bad)
        return bad
    with pytest.raises(ValueError, match="exp_avg_sq_row has shape"):
        fresh().load_state_dict(broken(lambda b: b["state"][1].update(exp_avg_sq_row=torch.zeros(5))))
    with pytest.raises(ValueError, match="exp_avg_sq_col has shape"):
        fresh().load_state_dict(broken(lambda b: b["state"][0].update(exp_avg_sq_col=torch.zeros(1, 8))))
    with pytest.raises(ValueError, match="exp_avg has shape"):
        fresh().load_state_dict(broken(lambda b: b["state"][2].update(exp_avg=torch.zeros(3, 3))))
    with pytest.raises(ValueError, match="no 'exp_avg_sq_row'"):     # an unfactored file for a matrix
        fresh().load_state_dict(broken(lambda b: b["state"][0].pop("exp_avg_sq_row")))
    with pytest.raises(ValueError, match="no 'exp_avg'"):            # the group says beta1, the state has no first moment
        fresh().load_state_dict(broken(lambda b: b["state"][3].pop("exp_avg")))
    s = fresh()
    s.load_state_dict(broken(lambda b: b["state"].clear()))         # a file written before the first step
    assert s.opt_state is None and s.global_step == 4
