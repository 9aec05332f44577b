"""CPU: the scaled AdamW family (Riemannian-preconditioned AdamW for LoRA pairs) without a GPU -- the restatement
tests/scaled_adamw_ref.py against exact statements, the bar of the GPU test as twice the restatement's own order noise, the config
mapping and its refusals, the pair table against the store layout, qfx_scaled_adamw_check_table through the host entry point, and
the ctypes structs against the header."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import optim_ref as OR
import scaled_adamw_ref as R
from test_sgd_cpu import toy_model

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("r,nout", [(4, 96), (16, 33), (64, 64), (1, 1)])
def test_inverse_times_gram_is_the_identity_to_fp64_rounding(r, nout):
    """P_B (B^T B + reg I) = I: the residual of an inverse computed backward-stably is of order cond * 2^-53."""
    rng = np.random.default_rng(r)
    B = (rng.standard_normal((nout, r)) * 0.2).astype(F32)
    G = R.gram(B.T, R.REG)
    P = R.inverse(G)
    res = float((P @ G - torch.eye(r, dtype=torch.float64)).abs().max())
    cond = float(torch.linalg.cond(G))
    assert res <= 64 * r * cond * 2.0 ** -53, (res, cond)
    assert float((G - G.T).abs().max()) == 0.0 and float(G[0, 0]) > float(F32(R.REG))


def test_precondition_off_is_the_adamw_reference_bit_for_bit():
    pairs, n = R.pack(R.SHAPES, ratios=(1.0, 1.0), wds=(1e-2, 1e-2))
    st, grads = R.gaussian_state(pairs, n)
    hp = R.hyper()
    clip = float(F32(0.37))
    got, _, skipped = R.run(st, grads, pairs, hp, clip=clip, precondition=False)
    want = {k: v.copy() for k, v in st.items()}
    for t, g in enumerate(grads, 1):
        want["p"], want["m"], want["v"] = OR.adamw_f32(want["p"], g, want["m"], want["v"], clip, **OR.adamw_args(hp, t))
    mask = R.covered(pairs, n)
    assert skipped == 0 and bool(mask.any()) and not mask.all()
    for q in R.QUANTITIES:
        assert np.array_equal(got[q][mask], want[q][mask]), q
        assert np.array_equal(got[q][~mask], st[q][~mask]), q          # the slots between the tensors are nobody's


def test_preconditioning_makes_the_step_invariant_to_the_pairs_parametrisation():
    """What the method is for: B Q and Q^-1 A are the same adapter, and the preconditioned gradients move the PRODUCT the same way
    for both: d(B A) = B dA + dB A with dA = P_B gA, dB = gB P_A is invariant under Q (reg -> 0).  Plain gradients are not."""
    rng = np.random.default_rng(5)
    r, nin, nout = 4, 12, 10
    A, B = rng.standard_normal((r, nin)), rng.standard_normal((nout, r))
    gW = rng.standard_normal((nout, nin))                     # gradient of the product
    Q = rng.standard_normal((r, r)) + 3 * np.eye(r)

    def move(A, B, pre):
        gA, gB = (B.T @ gW).astype(F32), (gW @ A.T).astype(F32)
        if pre:
            gA, gB = R.preconditioned(A.astype(F32), B.astype(F32), gA, gB, reg=1e-12)
        return B @ gA.astype(np.float64) + gB.astype(np.float64) @ A
    a, b = move(A, B, True), move(np.linalg.inv(Q) @ A, B @ Q, True)
    assert np.abs(a - b).max() <= 1e-4 * np.abs(a).max()
    a, b = move(A, B, False), move(np.linalg.inv(Q) @ A, B @ Q, False)
    assert np.abs(a - b).max() > 0.1 * np.abs(a).max()


def test_bar_is_twice_the_references_own_order_noise():
    """The floor of the GPU test: forward against reversed fp64 sums on the very inputs the kernel is held on, three steps, in fp32
    ulps of each quantity's scale.  Also on the rank-deficient input (condition number about 1e5 against fp64's 1e-16): its two
    orders stay within the same bar."""
    hp = R.hyper()
    pairs, n = R.pack(R.SHAPES)
    st, grads = R.gaussian_state(pairs, n)
    noise = R.order_noise(st, grads, pairs, hp)
    print("ORDER_NOISE gaussian", noise)
    assert noise == R.FLOORS and R.BARS == {q: 2.0 * x for q, x in R.FLOORS.items()}
    dpairs, dn, dst, dgrads = R.rank_deficient_state()
    off_a, _, r, nin, *_ = dpairs[0]
    GA = R.gram(dst["p"][off_a:off_a + r * nin].reshape(r, nin), R.RANK_DEFICIENT["reg"])
    cond = float(torch.linalg.cond(GA))
    deficient = R.order_noise(dst, dgrads, dpairs, hp, reg=R.RANK_DEFICIENT["reg"])
    print("ORDER_NOISE rank-deficient", deficient, "cond", cond)
    assert 1e4 < cond < 1e7
    assert all(deficient[q] <= R.BARS[q] for q in R.QUANTITIES)
    fpairs, fn = R.pack(R.SHAPES)
    fst, fgrads = R.fresh_lora_state(fpairs, fn)
    fresh = R.order_noise(fst, fgrads, fpairs, hp)
    assert all(fresh[q] <= R.BARS[q] for q in R.QUANTITIES)


def test_reference_skip_rule_and_fresh_lora():
    hp = R.hyper()
    pairs, n = R.pack(R.SHAPES)
    st, grads = R.gaussian_state(pairs, n)
    grads[0][pairs[1][1] + 3] = np.nan
    got, _, skipped = R.run(st, grads[:1], pairs, hp)
    assert skipped == 1
    s = slice(pairs[1][0], pairs[1][1] + pairs[1][4] * pairs[1][2])
    assert all(np.array_equal(got[q][s], st[q][s]) for q in R.QUANTITIES) and not np.array_equal(got["p"], st["p"])
    fst, fgrads = R.fresh_lora_state(pairs, n)
    got, _, skipped = R.run(fst, fgrads, pairs, hp)
    decay = OR.fma32(-F32(hp["lr"]), F32(hp["wd"]), F32(1.0))
    for off_a, off_b, r, nin, nout, *_ in pairs:
        a = fst["p"][off_a:off_a + r * nin]
        for _ in range(R.STEPS):
            a = a * decay
        assert np.array_equal(got["p"][off_a:off_a + r * nin], a) and not got["m"][off_a:off_a + r * nin].any()
        assert got["p"][off_b:off_b + nout * r].any()
    assert skipped == 0


# ---------------------------------------------------------------- config mapping and refusals
def test_config_mapping_and_its_refusals():
    from qflux_amd.trainer import optimizer_kwargs_from_config as f
    path = "qflux_amd.optim.ScaledAdamW"
    assert f(path, {}) == {"optimizer": "scaled_adamw", "lr": 1e-3, "weight_decay": 1e-2, "optimizer_args": {}}
    kw = f(path, {"lr": 2e-4, "betas": [0.8, 0.99], "eps": 1e-6, "weight_decay": 0.0, "reg": 1e-4, "precondition": False})
    assert kw == {"optimizer": "scaled_adamw", "lr": 2e-4, "betas": (0.8, 0.99), "eps": 1e-6, "weight_decay": 0.0,
                  "optimizer_args": {"reg": 1e-4, "precondition": False}}
    for unknown in ({"amsgrad": True}, {"momentum": 0.9}, {"foreach": None}):
        with pytest.raises(NotImplementedError, match=next(iter(unknown))):
            f(path, dict({"lr": 1e-3}, **unknown))
    for reg in (0.0, -1e-6, float("inf"), float("nan"), True, "1e-6"):
        with pytest.raises(ValueError, match="reg"):
            f(path, {"reg": reg})
    with pytest.raises(ValueError, match="precondition"):
        f(path, {"precondition": 1})
    with pytest.raises(ValueError, match="beta"):
        f(path, {"betas": [0.9, 1.0]})
    with pytest.raises(NotImplementedError):
        f("riemannian_lora.ScaledAdamW", {})                 # no class path of the authors' is mapped


def test_resolve_family_the_train_steps_and_the_class():
    from qflux_amd import optim as O
    from qflux_amd.trainer import FluxKontextTrainStep, QwenLoraTrainStep
    from qflux_amd.trainer import optim_state as OS
    alias, fam, cls, wd, args = OS.resolve_family("scaled_adamw")
    assert (alias, fam, cls, wd) == (None, "scaled_adamw", OS.ScaledAdamWState, 0.01) and cls.FAMILY == "scaled_adamw"
    assert args == dict(reg=1e-6, precondition=True) and OS.default_betas("scaled_adamw") == (0.9, 0.999)
    assert OS.resolve_family("scaled_adamw", 0.0, {"reg": 1e-4})[3:] == (0.0, dict(reg=1e-4, precondition=True))
    with pytest.raises(ValueError, match="unsupported optimizer_args"):
        OS.resolve_family("scaled_adamw", None, {"alpha": 5.0})
    for reg in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError, match="reg"):
            OS.resolve_family("scaled_adamw", None, {"reg": reg})
    toy = toy_model()
    for ctor in (QwenLoraTrainStep, FluxKontextTrainStep):
        s = ctor(toy, lr=2e-4, optimizer="scaled_adamw", loraplus_lr_ratio=4, ema_decay=0.99, max_weight_norm=1.0, adapter_stats_every=2)
        assert s.weight_decay == 0.01 and s.optimizer_args == args and len(s.group_rules) == 2
        with pytest.raises(OS.ParamGroupsNotImplemented, match="betas"):
            ctor(toy, lr=2e-4, optimizer="scaled_adamw", param_groups=[{"match": "lora_B", "betas": (0.8, 0.9)}])
        with pytest.raises(OS.ParamGroupsNotImplemented, match="eps"):
            ctor(toy, lr=2e-4, optimizer="scaled_adamw", param_groups=[{"match": "lora_B", "eps": 1e-6}])
        ctor(toy, lr=2e-4, optimizer="adamw", param_groups=[{"match": "lora_B", "betas": (0.8, 0.9)}])      # AdamW still takes them
    sd = QwenLoraTrainStep(toy, lr=2e-4, optimizer="scaled_adamw").state_dict()
    g = sd["param_groups"][0]
    assert sd["state"] == {} and g["reg"] == 1e-6 and g["precondition"] is True and g["weight_decay"] == 0.01
    ps = [p for _, p in toy.lora_store.params()]
    opt = O.ScaledAdamW(ps)
    g = opt.param_groups[0]
    assert isinstance(opt, torch.optim.Optimizer) and opt.family == "scaled_adamw" and "ScaledAdamW" in O.__all__
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["reg"], g["precondition"]) == (1e-3, (0.9, 0.999), 1e-8, 1e-2, 1e-6, True)
    assert opt.skipped is None and opt.state_dict()["state"] == {}
    two = O.ScaledAdamW(O.loraplus_param_groups(toy, 1e-3, 4.0, weight_decay=0.01, b_weight_decay=0.0))
    assert len(two.param_groups) == 2 and two.param_groups[1]["lr"] == 4e-3
    with pytest.raises(ValueError, match="missing"):
        O.ScaledAdamW(ps[:-1])
    with pytest.raises(ValueError, match="reg"):
        O.ScaledAdamW(ps, reg=0.0)
    with pytest.raises(TypeError):
        O.ScaledAdamW(ps, amsgrad=True)


# ---------------------------------------------------------------- the pair table against the store layout
def _entries(store):
    return [(n, p, off, k) for n, p, off, k in store.entries]


def test_pairs_follow_the_store_layout_of_a_tiny_model():
    from qflux_amd.trainer import optim_state as OS
    from qflux_amd import ops
    toy = toy_model(n_blocks=2)
    st = toy.lora_store
    pairs = OS.ScaledAdamWState.adapter_pairs(st.entries)
    mods = [n for n, m in toy.named_modules() if type(m).__name__ == "QfxLoraLinear"]
    assert [p[0] for p in pairs] == mods and len(pairs) == 4
    for (mod, i, j, r, nin, nout), name in zip(pairs, mods):
        m = toy.get_submodule(name)
        assert st.entries[i][1] is m.A and st.entries[j][1] is m.B
        assert (r, nin, nout) == (4, 8, m.B.shape[0]) and st.entries[i][3] == r * nin and st.entries[j][3] == nout * r
    # per-tensor fields from LoRA+ groups: lora_A in group 0, lora_B in group 1 with four times the rate and no decay
    state = OS.ScaledAdamWState.__new__(OS.ScaledAdamWState)
    state.pairs = pairs
    names = [n for n, _, _, _ in st.entries]
    state.group_map = tuple(int("lora_B" in n) for n in names)
    rows = [dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01), dict(lr=8e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)]
    lr, fields = state.table_fields(123.0, (0.9, 0.999), 1e-8, 0.01, rows)          # with groups the rows alone decide
    assert lr == 2e-4 and fields == [(1.0, 4.0, float(F32(0.01)), 0.0)] * 4
    assert state.table_fields(2e-4, (0.9, 0.999), 1e-8, 0.01, None) == (2e-4, [(1.0, 1.0, float(F32(0.01)), float(F32(0.01)))] * 4)
    with pytest.raises(OS.ParamGroupsNotImplemented, match="betas / eps"):
        state.table_fields(2e-4, (0.9, 0.999), 1e-8, 0.01, [rows[0], dict(rows[1], betas=(0.8, 0.999))])
    with pytest.raises(OS.ParamGroupsNotImplemented, match="betas / eps"):
        state.table_fields(2e-4, (0.9, 0.999), 1e-8, 0.01, [rows[0], dict(rows[1], eps=1e-6)])
    # and the table the launch would read: offsets, shapes and fields of every pair, checked on the host against the flat buffer
    off = [o for _, _, o, _ in st.entries]
    lay = ops.scaled_adamw_table([(off[i], off[j], r, nin, nout) + f for (_, i, j, r, nin, nout), f in zip(pairs, fields)],
                                 n_elems=st.pflat.numel())
    assert lay.n_pairs == 4 and lay.extent <= st.pflat.numel() and lay.table.numel() == 4 * C.sizeof(_lib().ScaledAdamwPair)
    raw = (_lib().ScaledAdamwPair * 4).from_buffer_copy(lay.table.numpy().tobytes())
    for t, (_, i, j, r, nin, nout) in zip(raw, pairs):
        assert (t.off_a, t.off_b, t.r, t.in_features, t.out_features) == (off[i], off[j], r, nin, nout)
        assert (t.lr_ratio_a, t.lr_ratio_b, t.wd_b) == (1.0, 4.0, 0.0) and t.wd_a == F32(0.01)


def test_a_tensor_without_its_partner_and_a_rank_above_64_are_refused_by_module_name():
    from qflux_amd.trainer import optim_state as OS
    f = OS.ScaledAdamWState.adapter_pairs
    z = lambda *s: torch.zeros(*s)
    good = [("blk.to_q.lora_A.ad.weight", z(4, 8), 0, 32), ("blk.to_q.lora_B.ad.weight", z(6, 4), 64, 24)]
    assert f(good) == [("blk.to_q", 0, 1, 4, 8, 6)]
    with pytest.raises(NotImplementedError, match="blk.to_q"):
        f(good[:1])
    with pytest.raises(NotImplementedError, match="blk.to_q"):
        f(good[1:])
    with pytest.raises(NotImplementedError, match="blk.norm"):
        f(good + [("blk.norm.weight", z(8), 128, 8)])
    with pytest.raises(NotImplementedError, match="blk.to_q.*no pair"):
        f([good[0], ("blk.to_q.lora_B.ad.weight", z(6, 5), 64, 30)])
    big = [("blk.to_k.lora_A.ad.weight", z(65, 8), 0, 520), ("blk.to_k.lora_B.ad.weight", z(6, 65), 576, 390)]
    with pytest.raises(NotImplementedError, match="blk.to_k.*rank 65"):
        f(big)
    from qflux_amd import ops
    with pytest.raises(NotImplementedError, match="rank 65"):
        ops.scaled_adamw_table([(0, 576, 65, 8, 6, 1.0, 1.0, 0.0, 0.0)])


# ---------------------------------------------------------------- the C ABI without a GPU
def _lib():
    from qflux_amd import _lib as L
    return L


def _check(rows, n_elems, n=None):
    L = _lib()
    arr = (L.ScaledAdamwPair * max(1, len(rows)))(*[L.ScaledAdamwPair(*r, 0) for r in rows])
    return L.lib.qfx_scaled_adamw_check_table(arr, len(rows) if n is None else n, n_elems)


def test_check_table_rejects_every_malformed_table():
    L = _lib()
    ok = (0, 64, 4, 8, 6, 1.0, 4.0, 0.01, 0.0)            # A [4, 8] at 0, B [6, 4] at 64
    assert _check([ok], 88) == 0 and _check([ok, (100, 200, 64, 1, 1, 1.0, 1.0, 0.0, 0.0)], 264) == 0
    assert _check([], 0, n=0) == 0
    assert L.lib.qfx_scaled_adamw_check_table(None, 0, 0) == 0
    assert L.lib.qfx_scaled_adamw_check_table(None, 1, 100) == L.QFX_EINVAL        # a NULL table with pairs
    assert _check([ok], 88, n=-1) == L.QFX_EINVAL and _check([ok], -1) == L.QFX_EINVAL
    bad = {
        "r = 0": (0, 64, 0, 8, 6, 1.0, 1.0, 0.0, 0.0), "r = 65": (0, 1000, 65, 8, 6, 1.0, 1.0, 0.0, 0.0),
        "in = 0": (0, 64, 4, 0, 6, 1.0, 1.0, 0.0, 0.0), "in > 2^24": (0, 64, 4, (1 << 24) + 1, 6, 1.0, 1.0, 0.0, 0.0),
        "out = 0": (0, 64, 4, 8, 0, 1.0, 1.0, 0.0, 0.0), "out > 2^24": (0, 64, 4, 8, (1 << 24) + 1, 1.0, 1.0, 0.0, 0.0),
        "off_a < 0": (-1, 64, 4, 8, 6, 1.0, 1.0, 0.0, 0.0), "off_b < 0": (0, -64, 4, 8, 6, 1.0, 1.0, 0.0, 0.0),
        "A and B overlap": (0, 31, 4, 8, 6, 1.0, 1.0, 0.0, 0.0),
        "lr ratio NaN": (0, 64, 4, 8, 6, float("nan"), 1.0, 0.0, 0.0), "lr ratio inf": (0, 64, 4, 8, 6, 1.0, float("inf"), 0.0, 0.0),
        "lr ratio < 0": (0, 64, 4, 8, 6, -1.0, 1.0, 0.0, 0.0), "wd NaN": (0, 64, 4, 8, 6, 1.0, 1.0, float("nan"), 0.0),
        "wd < 0": (0, 64, 4, 8, 6, 1.0, 1.0, 0.0, -0.1),
    }
    for what, row in bad.items():
        assert _check([row], 1 << 40) == L.QFX_EINVAL, what
    assert _check([ok], 87) == L.QFX_EINVAL                                          # B reaches past n_elems
    assert _check([ok], 31) == L.QFX_EINVAL                                          # A does
    assert _check([ok, (80, 200, 4, 8, 6, 1.0, 1.0, 0.0, 0.0)], 1000) == L.QFX_EINVAL      # two pairs overlap
    from qflux_amd import ops
    with pytest.raises(ValueError, match="qfx_scaled_adamw_check_table"):
        ops.scaled_adamw_table([ok], n_elems=87)
    with pytest.raises(ValueError, match="no pairs"):
        ops.scaled_adamw_table([])


def test_step_argument_checks_return_einval_before_any_launch():
    L = _lib()
    step = L.lib.qfx_scaled_adamw_step
    assert step(None, None) == L.QFX_EINVAL

    def args(**kw):
        a = L.ScaledAdamwArgs(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 1e-6, 0.1, 0.001, None, 0.0, 1.0, 0x6000)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    bad = [dict(n_pairs=-1), dict(lr=-1.0), dict(lr=float("nan")), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=-1e-8), dict(reg=0.0),
           dict(reg=float("inf")), dict(reg=float("nan")), dict(bias_corr1=0.0), dict(bias_corr2=float("nan")), dict(precondition=2),
           dict(max_norm=float("nan")), dict(grad_scale=float("inf")), dict(p=None), dict(g=None), dict(exp_avg=None),
           dict(exp_avg_sq=None), dict(table=None), dict(skipped=None)]
    for kw in bad:
        assert step(C.byref(args(**kw)), None) == L.QFX_EINVAL, kw
    assert step(C.byref(args(n_pairs=0, p=None, table=None, skipped=None)), None) == L.QFX_OK      # nothing to do: no launch
    assert step(C.byref(args(n_pairs=0, precondition=0, reg=0.0)), None) == L.QFX_OK               # reg is not read without the preconditioner
    assert step(C.byref(args(n_pairs=0, reg=0.0)), None) == L.QFX_EINVAL


def test_ctypes_structs_match_the_header(tmp_path):
    """sizeof and every field offset of the two new structs, compiled from include/qfx.h (the manner of tests/test_abi_cpu.py)."""
    L = _lib()
    pairs = {"qfx_scaled_adamw_pair": L.ScaledAdamwPair, "qfx_scaled_adamw_args": L.ScaledAdamwArgs}
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
    assert C.sizeof(L.ScaledAdamwPair) == 48
    hdr = open(os.path.join(ROOT, "include", "qfx.h")).read()
    assert "THIS LISTING IS THE SPECIFICATION" in hdr and "qfx_scaled_adamw_step" in L.SYMBOLS and math.isclose(R.REG, 1e-6)
