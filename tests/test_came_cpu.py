"""CPU: optimizer="came" -- the restatement tests/came_ref.py against a hand derivation of two steps (and against the came_pytorch
package where it is installed), the config mapping and its refusals, resolve_family, the struct layouts against include/qfx.h, the
descriptor table, argument validation of qfx_came_step without a launch, and came_pytorch's checkpoint layout in both directions
with shape validation on load."""
import ctypes as C
import math
import os
import subprocess

import pytest
import torch

import came_ref as R
from test_sgd_cpu import toy_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.float64


def _hand_step(p, g0, st, lr, b1, b2, b3, eps1, eps2, thr, wd, gs):
    """One CAME step on a 2 x 3 matrix, every formula of include/qfx.h written out on Python floats (float64).  st: row[2], col[3],
    rrow[2], rcol[3], m[2][3], changed in place; returns the new parameters."""
    g = [[x * gs for x in r] for r in g0]                                  # no gnorm_sq: clip = grad_scale
    u = [[x * x + eps1 for x in r] for r in g]
    st["row"] = [b2 * st["row"][r] + (1 - b2) * (sum(u[r]) / 3) for r in range(2)]
    st["col"] = [b2 * st["col"][c] + (1 - b2) * ((u[0][c] + u[1][c]) / 2) for c in range(3)]
    rmean = (st["row"][0] + st["row"][1]) / 2
    upd = [[g[r][c] / math.sqrt(st["row"][r] / rmean) / math.sqrt(st["col"][c]) for c in range(3)] for r in range(2)]
    urms = math.sqrt(sum(x * x for r in upd for x in r) / 6)
    den = max(1.0, urms / thr)
    upd = [[x / den for x in r] for r in upd]                              # NOT times lr: lr multiplies `out` at the end
    st["m"] = [[b1 * st["m"][r][c] + (1 - b1) * upd[r][c] for c in range(3)] for r in range(2)]
    res = [[(upd[r][c] - st["m"][r][c]) ** 2 + eps2 for c in range(3)] for r in range(2)]
    st["rrow"] = [b3 * st["rrow"][r] + (1 - b3) * (sum(res[r]) / 3) for r in range(2)]
    st["rcol"] = [b3 * st["rcol"][c] + (1 - b3) * ((res[0][c] + res[1][c]) / 2) for c in range(3)]
    rrmean = (st["rrow"][0] + st["rrow"][1]) / 2
    out = [[st["m"][r][c] / math.sqrt(st["rrow"][r] / rrmean) / math.sqrt(st["rcol"][c]) for c in range(3)] for r in range(2)]
    return [[p[r][c] - wd * lr * p[r][c] - lr * out[r][c] for c in range(3)] for r in range(2)], den


def test_restatement_matches_a_hand_derivation_of_two_steps():
    """Step 1 from zero state and step 2 from the state step 1 left (m and the instability statistics are non-zero then), with weight
    decay, a grad_scale and an update clip that engages."""
    p0 = [[0.5, -1.0, 2.0], [1.5, 0.25, -0.75]]
    grads = [[[0.1, -0.2, 0.3], [-0.4, 0.5, 0.6]], [[-0.3, 0.1, 0.2], [0.05, -0.6, 0.4]]]
    hyper = dict(lr=1e-2, b1=0.9, b2=0.999, b3=0.9999, eps1=1e-30, eps2=1e-16, thr=0.5, wd=0.1, gs=0.5)
    hand = dict(row=[0.0] * 2, col=[0.0] * 3, rrow=[0.0] * 2, rcol=[0.0] * 3, m=[[0.0] * 3, [0.0] * 3])
    p = [torch.tensor(p0, dtype=D)]
    st = R.new_state([(2, 3)], dtype=D)
    want, tight = p0, dict(rtol=1e-12, atol=0)
    for s, g0 in enumerate(grads):
        rms = math.sqrt(sum(x * x for r in want for x in r) / 6)
        want, den = _hand_step(want, g0, hand, **hyper)
        assert den > 1.0                               # beta2 = 0.999 from zero state: |upd| ~ 30, the update clip is active
        R.step(p, [torch.tensor(g0, dtype=D)], st, dtype=D, grad_scale=0.5, lr=1e-2, betas=(0.9, 0.999, 0.9999), eps=(1e-30, 1e-16),
               clip_threshold=0.5, weight_decay=0.1)
        torch.testing.assert_close(p[0], torch.tensor(want, dtype=D), **tight)
        for key, name in (("exp_avg_sq_row", "row"), ("exp_avg_sq_col", "col"), ("exp_avg_res_row", "rrow"),
                          ("exp_avg_res_col", "rcol"), ("exp_avg", "m")):
            torch.testing.assert_close(st[0][key], torch.tensor(hand[name], dtype=D), **tight)
        torch.testing.assert_close(st[0]["RMS"], torch.tensor(rms, dtype=D), **tight)
    # step 1 alone: m = (1 - b1) upd, so the instability is (b1 upd)^2 and out is a multiple of upd, not upd itself
    assert hand["rrow"][0] > 1e-6 and hand["m"][0][0] != 0
    # the unfactored path from non-zero state: out = m
    pv, gv, v1, m1 = [0.3, -0.4], [0.02, 0.05], [1e-4, 4e-4], [0.5, -0.25]
    v = [0.999 * v1[i] + (1 - 0.999) * (gv[i] ** 2 + 1e-30) for i in range(2)]
    uu = [gv[i] / math.sqrt(v[i]) for i in range(2)]
    den = max(1.0, math.sqrt((uu[0] ** 2 + uu[1] ** 2) / 2) / 1.0)
    m = [0.9 * m1[i] + (1 - 0.9) * uu[i] / den for i in range(2)]
    p = [torch.tensor(pv, dtype=D)]
    st = R.new_state([(2,)], dtype=D)
    st[0]["exp_avg_sq"], st[0]["exp_avg"] = torch.tensor(v1, dtype=D), torch.tensor(m1, dtype=D)
    R.step(p, [torch.tensor(gv, dtype=D)], st, dtype=D, lr=1e-3)
    torch.testing.assert_close(p[0], torch.tensor([pv[i] - 1e-3 * m[i] for i in range(2)], dtype=D), **tight)
    torch.testing.assert_close(st[0]["exp_avg_sq"], torch.tensor(v, dtype=D), **tight)
    torch.testing.assert_close(st[0]["exp_avg"], torch.tensor(m, dtype=D), **tight)


def test_restatement_skips_a_tensor_with_a_non_finite_gradient():
    g = torch.Generator().manual_seed(3)
    ps = [torch.randn(3, 4, generator=g), torch.randn(5, generator=g)]
    gs = [torch.randn(3, 4, generator=g), torch.randn(5, generator=g)]
    gs[0][1, 2] = float("inf")
    st = R.new_state([(3, 4), (5,)])
    before = [p.clone() for p in ps]
    R.step(ps, gs, st, lr=1e-3)
    assert torch.equal(ps[0], before[0]) and st[0]["RMS"] == 0 and not st[0]["exp_avg"].any()
    assert not any(st[0][k].any() for k in R.FACTORED)
    assert not torch.equal(ps[1], before[1]) and st[1]["exp_avg_sq"].all() and st[1]["exp_avg"].all()


CONFIGS = [dict(lr=1e-3), dict(lr=1e-3, weight_decay=1e-2), dict(lr=2e-4, clip_threshold=0.5, betas=(0.8, 0.99, 0.999)),
           dict(lr=1e-3, betas=(0.0, 0.9, 0.9))]


@pytest.mark.parametrize("cfg", CONFIGS, ids=["defaults", "decay", "clip", "no_momentum"])
def test_restatement_matches_came_pytorch(cfg):
    """Skipped where came_pytorch is not installed (it is not a dependency): the package comparison has then NOT been made."""
    P = pytest.importorskip("came_pytorch")
    g = torch.Generator().manual_seed(11)
    shapes = [(3, 40), (130, 5), (7,)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g) * 0.1) for s in shapes]
    mine = [p.detach().clone() for p in ps]
    st = R.new_state(shapes)
    opt = P.CAME(ps, **cfg)
    for t in range(1, 6):
        grads = [torch.randn(s, generator=g) * 1e-2 for s in shapes]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt.step()
        R.step(mine, grads, st, **cfg)
    # bar: 1e-5 of the tensor's maximum, what test_adafactor_cpu.py grants two fp32 statements of one optimizer
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    for p, q, e in zip(ps, mine, st):
        assert rel(q, p.detach()) <= 1e-5
        assert set(opt.state[p]) == set(e) | {"step"}
        for k, v in opt.state[p].items():
            if torch.is_tensor(v) and k != "step":
                assert v.abs().max() > 0 and rel(e[k], v) <= 1e-5, (k, rel(e[k], v))


def test_config_mapping_and_its_refusals():
    from qflux_amd.trainer import optimizer_kwargs_from_config as f
    for path in ("came_pytorch.CAME", "came_pytorch.CAME.CAME", "qflux_amd.optim.CAME"):
        assert f(path, {"lr": 2e-4}) == {"optimizer": "came", "lr": 2e-4, "optimizer_args": {}}
        kw = f(path, {"lr": 1e-3, "weight_decay": 0.01, "eps": [1e-30, 1e-16], "clip_threshold": 1.0, "betas": [0.9, 0.999, 0.9999]})
        assert kw == {"optimizer": "came", "lr": 1e-3, "weight_decay": 0.01, "betas": (0.9, 0.999, 0.9999),
                      "optimizer_args": {"eps": (1e-30, 1e-16), "clip_threshold": 1.0}}
        with pytest.raises(ValueError, match="learning rate"):
            f(path, {})                                                  # lr is required
        with pytest.raises(ValueError, match="learning rate"):
            f(path, {"lr": 0.0})
        with pytest.raises(ValueError, match="triple"):
            f(path, {"lr": 1e-3, "betas": [0.9, 0.999]})
        with pytest.raises(ValueError, match="betas"):
            f(path, {"lr": 1e-3, "betas": [0.9, 0.999, 1.5]})
        with pytest.raises(ValueError, match="pair"):
            f(path, {"lr": 1e-3, "eps": 1e-8})
        with pytest.raises(ValueError, match="clip_threshold"):
            f(path, {"lr": 1e-3, "clip_threshold": 0.0})
        for unknown in ({"momentum": 0.9}, {"relative_step": False}, {"beta1": 0.9}, {"decay_rate": -0.8}):
            with pytest.raises(NotImplementedError, match=next(iter(unknown))):
                f(path, dict({"lr": 1e-3}, **unknown))
    with pytest.raises(NotImplementedError):
        f("came_pytorch.Came", {"lr": 1e-3})                             # not a class path of the package


def test_resolve_family_and_the_train_steps_accept_came():
    from qflux_amd.trainer import FluxKontextTrainStep, QwenLoraTrainStep
    from qflux_amd.trainer.optim_state import FAMILIES, CameState, default_betas, resolve_family
    alias, fam, cls, wd, args = resolve_family("came")
    assert (alias, fam, cls, wd) == (None, "came", CameState, 0.0) and FAMILIES["came"] == (CameState, 0.0)
    assert args == dict(eps=(1e-30, 1e-16), clip_threshold=1.0) and default_betas("came") == (0.9, 0.999, 0.9999)
    assert default_betas("adamw") == (0.9, 0.999) and default_betas("lion") == (0.9, 0.99)
    assert resolve_family("came", 0.01, {"eps": [1e-20, 1e-12]})[3:] == (0.01, dict(args, eps=(1e-20, 1e-12)))
    assert CameState.names(args) == ("row", "col", "rrow", "rcol", "v", "rms", "m") and CameState.FAMILY == "CAME"
    with pytest.raises(ValueError, match="unsupported optimizer_args"):
        resolve_family("came", None, {"beta1": 0.9})
    with pytest.raises(ValueError, match="pair"):
        resolve_family("came", None, {"eps": 1e-8})
    with pytest.raises(ValueError, match="clip_threshold"):
        resolve_family("came", None, {"clip_threshold": -1.0})
    toy = toy_model()
    s = QwenLoraTrainStep(toy, lr=2e-4, optimizer="came")
    assert s.lr == 2e-4 and s.weight_decay == 0.0 and s.optimizer_args == args and s.betas == (0.9, 0.999, 0.9999)
    s = FluxKontextTrainStep(toy, lr=1e-3, weight_decay=0.01, betas=(0.8, 0.99, 0.999), optimizer="came", optimizer_args={"clip_threshold": 0.5})
    assert s.betas == (0.8, 0.99, 0.999) and s.weight_decay == 0.01 and s.optimizer_args["clip_threshold"] == 0.5
    for ctor in (QwenLoraTrainStep, FluxKontextTrainStep):
        with pytest.raises(ValueError, match="learning rate"):
            ctor(toy, lr=None, optimizer="came")
        with pytest.raises(ValueError, match="triple"):
            ctor(toy, lr=1e-4, betas=(0.9, 0.999), optimizer="came")
    with pytest.raises(ValueError, match="CAME: 2 parameter groups"):
        CameState.check_groups(2)
    # before the first step: the package's empty state, its options in the group
    sd = QwenLoraTrainStep(toy, lr=2e-4, optimizer="came").state_dict()
    g = sd["param_groups"][0]
    assert sd["state"] == {} and g["lr"] == 2e-4 and g["eps"] == (1e-30, 1e-16) and g["betas"] == (0.9, 0.999, 0.9999)
    assert g["clip_threshold"] == 1.0 and g["weight_decay"] == 0.0


def test_torch_optim_class_refuses_what_the_others_refuse():
    from qflux_amd import optim as O
    toy = toy_model()
    ps = [p for _, p in toy.lora_store.params()]
    opt = O.CAME(ps, lr=2e-4)
    g = opt.param_groups[0]
    assert isinstance(opt, torch.optim.Optimizer) and opt.family == "came" and "CAME" in O.__all__
    assert g["lr"] == 2e-4 and g["eps"] == (1e-30, 1e-16) and g["betas"] == (0.9, 0.999, 0.9999) and g["weight_decay"] == 0.0
    assert g["clip_threshold"] == 1.0 and opt.state_dict()["state"] == {}
    with pytest.raises(ValueError, match="missing"):
        O.CAME(ps[:-1], lr=2e-4)
    with pytest.raises(ValueError, match="not an adapter parameter"):
        O.CAME(ps + [torch.nn.Parameter(torch.zeros(3))], lr=2e-4)
    with pytest.raises(ValueError, match="CAME: 2 parameter groups"):
        O.CAME([{"params": ps[:2]}, {"params": ps[2:]}], lr=2e-4)
    with pytest.raises(ValueError, match="learning rate"):
        O.CAME(ps)
    with pytest.raises(ValueError, match="triple"):
        O.CAME(ps, lr=2e-4, betas=(0.9, 0.999))
    with pytest.raises(TypeError):
        O.CAME(ps, lr=2e-4, relative_step=False)                         # Adafactor's keyword, not CAME's


def test_ctypes_structs_match_the_c_header_layout(tmp_path):
    from qflux_amd import _lib as L
    pairs = {"qfx_came_tensor": L.CameTensor, "qfx_came_args": L.CameArgs}
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
    assert L.ABI_VERSION == 7 and "qfx_came_step" in L.SYMBOLS
    assert [f for f, _ in L.CameArgs._fields_][11:22] == ["lr", "beta1", "one_minus_beta1", "beta2", "one_minus_beta2", "beta3",
                                                          "one_minus_beta3", "eps1", "eps2", "clip_threshold", "weight_decay"]


def test_descriptor_table_layout_and_refusals():
    from qflux_amd import _lib as L
    from qflux_amd import ops
    lay = ops.came_table([(0, (1, 32)), (32, (130, 5)), (700, (7,)), (710, (16, 3072))])
    assert (lay.n_tensors, lay.n_row, lay.n_col, lay.n_v, lay.extent) == (4, 1 + 130 + 16, 32 + 5 + 3072, 7, 710 + 16 * 3072)
    assert lay.tensors[1] == (32, 130, 5, True, 1, 32, -1) and lay.tensors[2] == (700, 1, 7, False, -1, -1, 0)
    arr = (L.CameTensor * 4).from_buffer_copy(lay.table.numpy().tobytes())
    assert [(d.off, d.row, d.col, d.rrow, d.rcol, d.v, d.rows, d.cols, d.rms, d.factored) for d in arr] == [
        (0, 0, 0, 0, 0, 0, 1, 32, 0, 1), (32, 1, 32, 1, 32, 0, 130, 5, 1, 1), (700, 0, 0, 0, 0, 0, 1, 7, 2, 0),
        (710, 131, 37, 131, 37, 0, 16, 3072, 3, 1)]
    # every offset stays inside the buffer its count sizes
    for d in arr:
        assert d.off + d.rows * d.cols <= lay.extent
        if d.factored:
            assert d.row + d.rows <= lay.n_row and d.rrow + d.rows <= lay.n_row and d.col + d.cols <= lay.n_col and d.rcol + d.cols <= lay.n_col
        else:
            assert d.v + d.cols <= lay.n_v
    for bad in ([], [(0, (2, 3, 4))], [(0, ())], [(-4, (2, 3))], [(0, (0, 3))], [(0, (1 << 16, 1 << 15))]):
        with pytest.raises(ValueError):
            ops.came_table(bad)


def test_came_step_rejects_bad_arguments_before_any_launch():
    from qflux_amd import _lib as L
    f = L.lib.qfx_came_step

    def args(**kw):
        a = L.CameArgs(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000, 0xa000, 3, 1e-3, 0.9, 0.1, 0.999, 0.001,
                       0.9999, 0.0001, 1e-30, 1e-16, 1.0, 0.0, None, 0.0, 1.0)     # never dereferenced: every call below is rejected on the host
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert f(None, None) == L.QFX_EINVAL
    assert f(args(n_tensors=0, table=None), None) == L.QFX_OK            # nothing to do, nothing launched
    nan = float("nan")
    for kw in (dict(n_tensors=-1), dict(table=None), dict(p=None), dict(g=None), dict(row=None), dict(col=None), dict(rrow=None),
               dict(rcol=None), dict(v=None), dict(m=None), dict(rms=None), dict(lr=-1.0), dict(lr=nan), dict(beta1=1.5), dict(beta1=-0.1),
               dict(beta2=1.01), dict(beta2=-0.1), dict(beta3=2.0), dict(beta3=nan), dict(one_minus_beta1=-0.5), dict(one_minus_beta2=1.5),
               dict(one_minus_beta3=nan), dict(clip_threshold=0.0), dict(clip_threshold=-1.0), dict(eps1=-1.0), dict(eps2=-1e-16),
               dict(weight_decay=-0.1)):
        assert f(args(**kw), None) == L.QFX_EINVAL, kw


def _filled_state(toy):
    from qflux_amd.trainer import QwenLoraTrainStep
    step = QwenLoraTrainStep(toy, lr=2e-4, optimizer="came")
    st = toy.lora_store
    step.opt_state = step._opt_cls(st, step.optimizer_args)
    g = torch.Generator().manual_seed(5)
    for n, t in step.opt_state.buffers():
        if n != "v":                        # no unfactored tensor in the toy: the placeholder element is not part of any file
            t.copy_(torch.rand(t.shape, generator=g) + 0.5)
    step.global_step = 4
    return step


def test_state_dict_has_came_pytorch_layout_and_round_trips(tmp_path):
    from qflux_amd.trainer import QwenLoraTrainStep
    from qflux_amd.trainer.optim_state import CameState
    toy = toy_model()
    st = toy.lora_store
    step = _filled_state(toy)
    assert [n for n, _ in step._state_buffers()] == ["lora", "row", "col", "rrow", "rcol", "v", "rms", "m"]
    torch.save(step.state_dict(), str(tmp_path / "optimizer.bin"))
    sd = torch.load(str(tmp_path / "optimizer.bin"), map_location="cpu", weights_only=False)
    g = sd["param_groups"][0]
    assert g["params"] == list(range(len(st.entries))) and g["eps"] == (1e-30, 1e-16) and g["lr"] == 2e-4
    assert g["betas"] == (0.9, 0.999, 0.9999) and g["clip_threshold"] == 1.0 and g["weight_decay"] == 0.0
    lay, o = step.opt_state.layout, step.opt_state
    assert set(CameState.FACTORED_KEYS) == {"step", "RMS", "exp_avg", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_res_row", "exp_avg_res_col"}
    assert set(CameState.UNFACTORED_KEYS) == {"step", "RMS", "exp_avg", "exp_avg_sq"}
    for i, (_, p, off, k) in enumerate(st.entries):
        e = sd["state"][i]
        assert set(e) == set(CameState.FACTORED_KEYS)
        assert e["step"] == 4 and e["RMS"].shape == () and e["RMS"] == o.rms[i]
        r0, c0 = lay.tensors[i][4], lay.tensors[i][5]
        for key, buf, a0, cnt in (("exp_avg_sq_row", o.row, r0, p.shape[0]), ("exp_avg_sq_col", o.col, c0, p.shape[1]),
                                  ("exp_avg_res_row", o.rrow, r0, p.shape[0]), ("exp_avg_res_col", o.rcol, c0, p.shape[1])):
            assert e[key].shape == (cnt,) and torch.equal(e[key], buf[a0:a0 + cnt]), key
        assert torch.equal(e["exp_avg"], o.m[off:off + k].view(p.shape))
    fresh = QwenLoraTrainStep(toy, lr=1e-3, eps=1e-6, betas=(0.5, 0.5, 0.5), optimizer="came", optimizer_args={"clip_threshold": 2.0})
    fresh.load_state_dict(sd)
    assert fresh.global_step == 4 and fresh.lr == 2e-4 and fresh.eps == 1e-6 and fresh.betas == (0.9, 0.999, 0.9999)
    assert fresh.optimizer_args == dict(eps=(1e-30, 1e-16), clip_threshold=1.0)
    for (n, x), (_, y) in zip(step.opt_state.buffers(), fresh.opt_state.buffers()):
        if n == "m":                        # indexed like pflat: the padding between two parameters is in no file
            assert all(torch.equal(x[off:off + k], y[off:off + k]) for _, _, off, k in st.entries)
        else:
            assert torch.equal(x, y), n
    # the torch.optim class reads and writes the same file
    from qflux_amd import optim as O
    opt = O.CAME([p for _, p in st.params()], lr=1e-3)
    opt.load_state_dict(sd)
    assert opt._step_count_fused == 4 and opt.param_groups[0]["lr"] == 2e-4 and opt.param_groups[0]["betas"] == (0.9, 0.999, 0.9999)
    back = opt.state_dict()
    for i, e in sd["state"].items():
        for key, v in e.items():
            assert torch.equal(back["state"][i][key], v) if torch.is_tensor(v) else back["state"][i][key] == v


def test_unfactored_entries_use_the_elementwise_keys():
    """A store with a 1-D tensor (the toy has none): exp_avg_sq replaces the four factored statistics, in both directions."""
    import types
    from qflux_amd.trainer import optim_state as OS
    p = torch.arange(20, dtype=torch.float32)
    store = types.SimpleNamespace(pflat=p, gflat=torch.zeros_like(p), entries=[("a", p[1:13].view(3, 4), 1, 12), ("b", p[14:19], 14, 5)])
    _, _, cls, wd, args = OS.resolve_family("came")
    state = cls(store, args)
    for n, t in state.buffers():
        t.copy_(torch.arange(t.numel(), dtype=torch.float32) + 1)
    sd = OS.state_dict(cls, state, store, 3, args, 1e-3, (0.9, 0.999, 0.9999), 1e-8, wd)
    assert set(sd["state"][0]) == set(cls.FACTORED_KEYS) and set(sd["state"][1]) == set(cls.UNFACTORED_KEYS)
    assert sd["state"][1]["exp_avg_sq"].shape == (5,) and torch.equal(sd["state"][1]["exp_avg_sq"], state.v[:5])
    hyper = dict(lr=1.0, betas=(0.0, 0.0, 0.0), eps=1e-8, weight_decay=0.5)
    back, t = OS.load_state_dict(cls, store, sd, dict(args), hyper)
    assert t == 3 and hyper == dict(lr=1e-3, betas=(0.9, 0.999, 0.9999), eps=1e-8, weight_decay=0.0)
    assert torch.equal(back.v, state.v) and torch.equal(back.rcol, state.rcol) and torch.equal(back.m[14:19], state.m[14:19])
    sd["state"][1]["exp_avg_sq"] = torch.zeros(4)
    with pytest.raises(ValueError, match="exp_avg_sq has shape"):
        OS.load_state_dict(cls, store, sd, dict(args), dict(hyper))


def test_load_validates_shapes():
    from qflux_amd.trainer import QwenLoraTrainStep
    toy = toy_model()
    sd = _filled_state(toy).state_dict()
    fresh = lambda: QwenLoraTrainStep(toy, lr=2e-4, optimizer="came")

    def broken(fn):
        bad = {"state": {i: dict(e) for i, e in sd["state"].items()}, "param_groups": [dict(sd["param_groups"][0])], "global_step": 4}
        fn(bad)
        return bad
    with pytest.raises(ValueError, match="exp_avg_sq_row has shape"):
        fresh().load_state_dict(broken(lambda b: b["state"][1].update(exp_avg_sq_row=torch.zeros(5))))
    with pytest.raises(ValueError, match="exp_avg_res_col has shape"):
        fresh().load_state_dict(broken(lambda b: b["state"][0].update(exp_avg_res_col=torch.zeros(1, 8))))
    with pytest.raises(ValueError, match="exp_avg has shape"):
        fresh().load_state_dict(broken(lambda b: b["state"][2].update(exp_avg=torch.zeros(3, 3))))
    with pytest.raises(ValueError, match="no 'exp_avg_res_row'"):    # an Adafactor file for a CAME run
        fresh().load_state_dict(broken(lambda b: b["state"][0].pop("exp_avg_res_row")))
    with pytest.raises(ValueError, match="no 'exp_avg'"):
        fresh().load_state_dict(broken(lambda b: b["state"][3].pop("exp_avg")))
    with pytest.raises(ValueError, match="pair"):
        fresh().load_state_dict(broken(lambda b: b["param_groups"][0].update(eps=1e-8)))
    s = fresh()
    s.load_state_dict(broken(lambda b: b["state"].clear()))         # a file written before the first step
    assert s.opt_state is None and s.global_step == 4
