"""GPU: qfx_lora_fold bit for bit against the numpy restatement of its listing (tests/pissa_ref.py), at any placement and in any
table order, then the PiSSA initialisation of the tiny Qwen DiT through the public interface: the factorisation against
numpy.linalg.svd on planted weights, the identity W = W_res + s B0 A0 on every adapted linear, reproducibility, no stale derived
state (bf16 and MX-FP8 trunk), the conversion to a LoRA of the original weights, and the refusals.  The 64 x 64 tile of the fold
sets the shapes: edges on both sides, several tiles, a single element, the widest rank."""
import ast
import json
import os

import numpy as np
import pytest
import torch

from parity_util import ROOT  # noqa: F401  (puts the repository root and the package on sys.path)

import pissa_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SENT32, SENT16 = 12345.0, -7.0
# (out, in, r, dtype, c, ld - in, elements off the allocation)
FOLD_CASES = [(65, 65, 3, BF, -0.5, 0, 0), (65, 65, 3, torch.float32, 1.0, 0, 0), (64, 128, 16, BF, 1.0, 8, 0),       # vector path, padded
              (64, 128, 16, torch.float32, -3.25, 0, 0), (1, 1, 1, BF, -3.25, 0, 0), (1, 1, 1, torch.float32, -0.5, 0, 0),
              (130, 67, 64, BF, -3.25, 3, 1),                                                                           # scalar path
              (130, 67, 64, torch.float32, 0.0, 0, 0), (96, 64, 4, BF, 0.0, 0, 0), (96, 64, 4, torch.float32, 1.0, 4, 0),
              (70, 67, 5, BF, -0.5, 5, 0), (70, 67, 5, torch.float32, 1.0, 5, 0)]     # ld = 72: vector path with a ragged last column tile
PLANTED = ("transformer_blocks.0.attn.to_q", "transformer_blocks.1.attn.to_out.0")
_FIX = {}


def _bits(x):
    return x.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()])


def _same(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y))


def _fold_inputs():
    """The cases' W (as stored), A, B on the host, once."""
    if "inputs" not in _FIX:
        rng = np.random.default_rng(7)
        out = []
        for nout, nin, r, dt, c, pad, shift in FOLD_CASES:
            W = torch.from_numpy(rng.standard_normal((nout, nin)).astype(np.float32)).to(dt)
            A = torch.from_numpy((rng.standard_normal((r, nin)) * 0.3).astype(np.float32))
            B = torch.from_numpy((rng.standard_normal((nout, r)) * 0.3).astype(np.float32))
            out.append((W, A, B))
        _FIX["inputs"] = out
    return _FIX["inputs"]


def _fold_reference():
    if "ref" not in _FIX:
        ref = []
        for (W, A, B), (_, _, _, dt, c, _, _) in zip(_fold_inputs(), FOLD_CASES):
            if dt == BF:
                bits = P.fold(W.view(torch.int16).numpy().view(np.uint16), A.numpy(), B.numpy(), c, P.BF16)
                ref.append(torch.from_numpy(bits.view(np.int16)).view(BF))
            else:
                ref.append(torch.from_numpy(P.fold(W.numpy(), A.numpy(), B.numpy(), c, P.FP32)))
        _FIX["ref"] = ref
    return _FIX["ref"]


def _run_fold(extra_shift=0, reverse=False):
    """One launch over the mixed table.  Every W sits in a sentinel-filled allocation of its own, `shift` elements in, with
    leading dimension in + pad; A and B sit in one sentinel-filled flat buffer.  -> per case (W region after, whole allocation
    after, allocation before), and p before / after."""
    from qflux_amd import ops
    cases = list(zip(_fold_inputs(), FOLD_CASES))
    allocs, views, off, places = [], [], 5 + extra_shift, []
    for (W, A, B), (nout, nin, r, dt, c, pad, shift) in cases:
        ld, sh = nin + pad, shift + extra_shift
        buf = torch.full((sh + nout * ld + 9,), SENT16 if dt == BF else SENT32, dtype=dt)
        v = buf[sh:sh + nout * ld].view(nout, ld)[:, :nin]
        v.copy_(W)
        allocs.append(buf)
        oa, ob = off, off + r * nin + 3
        off = ob + nout * r + 2
        places.append((oa, ob))
    p = torch.full((off + 7,), SENT32)
    for ((W, A, B), _), (oa, ob) in zip(cases, places):
        p[oa:oa + A.numel()] = A.reshape(-1)
        p[ob:ob + B.numel()] = B.reshape(-1)
    dev_allocs = [b.to(DEV) for b in allocs]
    for buf, (_, (nout, nin, r, dt, c, pad, shift)) in zip(dev_allocs, cases):
        ld, sh = nin + pad, shift + extra_shift
        views.append(buf[sh:sh + nout * ld].view(nout, ld)[:, :nin])
    rows = [(v, oa, ob, r, c) for v, (oa, ob), (_, (_, _, r, _, c, _, _)) in zip(views, places, cases)]
    order = list(range(len(rows)))[::-1] if reverse else list(range(len(rows)))
    pd = p.to(DEV)
    table = ops.lora_fold_table([rows[i] for i in order], device=DEV, n_elems=pd.numel())
    ops.lora_fold(table, pd)
    torch.cuda.synchronize()
    return [(v.cpu().contiguous(), b.cpu(), a) for v, b, a in zip(views, dev_allocs, allocs)], p, pd.cpu(), table


def _fold_result(key):
    if key not in _FIX:
        _FIX[key] = _run_fold(extra_shift=key[1], reverse=key[2])
    return _FIX[key]


def test_fold_bit_parity_with_the_restatement_and_sentinels():
    res, p0, p1, table = _fold_result(("fold", 0, False))
    starts = table.tile_start.cpu().tolist()
    tiles = [((c[0] + 63) // 64) * ((c[1] + 63) // 64) for c in FOLD_CASES]
    assert starts == [sum(tiles[:i]) for i in range(len(tiles) + 1)]
    for (got, after, before), want, case in zip(res, _fold_reference(), FOLD_CASES):
        nout, nin, r, dt, c, pad, shift = case
        assert _same(got, want), (case, int((_bits(got) != _bits(want)).sum()))
        ld = nin + pad
        mask = torch.ones(after.numel(), dtype=torch.bool)                 # everything but W[:, :in] keeps its bits: the ld padding,
        mask[shift:shift + nout * ld].view(nout, ld)[:, :nin] = False      # the elements around W
        assert torch.equal(_bits(after)[mask], _bits(before)[mask]), case
        if c == 0.0:
            assert _same(got, before[shift:shift + nout * ld].view(nout, ld)[:, :nin].contiguous())
    assert _same(p0, p1)                                                   # A, B and the sentinels between them


@pytest.mark.parametrize("shift,reverse", [(1, False), (3, True), (0, True)])
def test_fold_same_bits_at_any_address_and_in_any_table_order(shift, reverse):
    base, _, _, _ = _fold_result(("fold", 0, False))
    res, p0, p1, _ = _fold_result(("fold", shift, reverse))
    for (got, _, _), (want, _, _), case in zip(res, base, FOLD_CASES):
        assert _same(got, want), case
    assert _same(p0, p1)


def test_fold_nonfinite_values_propagate_and_nothing_else_changes():
    from qflux_amd import ops
    W = torch.ones(70, 70, device=DEV, dtype=BF)
    p = torch.zeros(4 * 70 + 70 * 4, device=DEV)
    p[:280] = 0.5
    p[280:] = 0.25
    p[280 + 4 * 3] = float("inf")                                          # B[3, 0]
    ops.lora_fold(ops.lora_fold_table([(W, 0, 280, 4, 1.0)], device=DEV), p)
    W = W.float().cpu()
    assert bool(torch.isinf(W[3]).all()) and bool((W[:3] == 1.5).all()) and bool((W[4:] == 1.5).all())


# ------------------------------------------------------------------ the model

STEP_TARGETS = ("to_k", "to_q", "to_v", "to_out.0", "img_in")
ALL_TARGETS = STEP_TARGETS + ("proj_out", "img_mlp.net.2", "img_mod.1", "timestep_embedder.linear_1")      # + feed-forward, conditioning head


def _fresh(targets=STEP_TARGETS, init=None, quant=None, r=4, alpha=8):
    """The tiny Qwen DiT of the GPU tests with deterministic weights, two of them planted; init: the adapter's init string."""
    from common import TINY, fill_weights
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.modules import LoraConfig
    with torch.device(DEV):
        m = QwenImageTransformer2DModel(**dict(TINY))
    fill_weights(m, seed=2)
    rng = np.random.default_rng(21)
    with torch.no_grad():
        for name in PLANTED:
            w = m.get_submodule(name).weight
            w.copy_(torch.from_numpy(P.planted(rng, *w.shape)).to(BF))
    m._invalidate()
    if quant:
        m.quantize_trunk(quant)
    if init is not None:
        m.add_adapter(LoraConfig(r=r, lora_alpha=alpha, init_lora_weights=init, target_modules=list(targets)), "lora_edit")
    return m


def _adapted(m):
    from qflux_amd.modules import QfxLoraLinear
    return {n: x for n, x in m.named_modules() if isinstance(x, QfxLoraLinear)}


def _initialised():
    """One model: the original weights, the model after add_adapter(pissa_niter_2)... via pissa_init_, and its report."""
    if "model" not in _FIX:
        m = _fresh(ALL_TARGETS, init="gaussian")
        W = {n: x.base_layer.weight.detach().clone() for n, x in _adapted(m).items()}
        report = m.pissa_init_(niter=2, oversample=8, seed=0)
        torch.cuda.synchronize()
        _FIX["model"] = (m, W, report)
    return _FIX["model"]


def test_init_against_the_restatement_on_planted_weights():
    m, W, report = _initialised()
    with open(os.path.join(ROOT, "profiles", "lora_extract_accuracy.json")) as f:
        tol = json.load(f)["tolerance"]
    s, measured = 2.0, {}
    for name in PLANTED:
        x = _adapted(m)[name]
        Wd = W[name].double().cpu().numpy()
        B0r, A0r, sig = P.split(Wd, 4, s)
        A0, B0 = x.A.detach().double().cpu().numpy(), x.B.detach().double().cpu().numpy()
        prod = float(np.abs(s * B0 @ A0 - s * B0r @ A0r).max() / np.linalg.norm(Wd))
        bal = float(np.abs(B0.T @ B0 - A0 @ A0.T).max() / (sig[0] / s))
        share = abs(report[name]["fro_retained"] - P.retained(sig, 4))
        measured[name] = dict(product=prod, balance=bal, retained_share=share)
        print(f"{name}: product {prod:.3e} (tolerance {tol['product']:.1e}) balance {bal:.3e} (tolerance {tol['orth']:.1e}) share {share:.3e}")
        assert prod <= tol["product"] and bal <= tol["orth"] and share <= 1e-6
        assert report[name]["sketch_converged"] and 4 <= report[name]["sketch_kept"] <= 12
    dest = os.environ.get("QFX_WRITE_PISSA_ACCURACY")                      # "1": profiles/pissa_accuracy.json; else a path
    if dest:
        dest = os.path.join(ROOT, "profiles", "pissa_accuracy.json") if dest == "1" else dest
        with open(dest, "w") as f:
            json.dump({"rule": "the tiny Qwen DiT of tests/test_pissa_gpu.py, r = 4, planted weights: s B0 A0 against numpy.linalg.svd "
                               "elementwise / ||W||_F, max |B0^T B0 - A0 A0^T| / (sigma_0 / s), the report's retained share against the "
                               "restatement's; tolerances: product and orth of profiles/lora_extract_accuracy.json, 1e-6",
                       "measured": measured}, f, indent=1)


def test_identity_bound_on_every_adapted_linear():
    m, W, report = _initialised()
    mods = _adapted(m)
    assert sorted(report) == sorted(mods) == sorted(m._pissa["A0"]) and len(mods) >= 10
    for name, x in mods.items():
        s = x.scaling[x.active_adapter]
        w, res = W[name].double(), x.base_layer.weight.detach().double()
        low = s * (x.B.detach().double() @ x.A.detach().double())
        bound = 2.0 ** -8 * res.abs() + 2.0 ** -22 * (w.abs() + low.abs())
        assert bool(((w - (res + low)).abs() <= bound).all()), name
        assert _same(x.A.detach().cpu(), m._pissa["A0"][name]) and _same(x.B.detach().cpu(), m._pissa["B0"][name])
        assert bool(x.B.detach().any()) and float(res.norm()) < float(w.norm())
    assert (m._pissa["niter"], m._pissa["oversample"], m._pissa["seed"]) == (2, 8, 0)


def test_reproducible_and_independent_of_the_grouping():
    m, _, _ = _initialised()
    other = _fresh(ALL_TARGETS, init="pissa_niter_2")                       # through add_adapter
    third = _fresh(ALL_TARGETS, init="gaussian")
    third.pissa_init_(group_bytes=1)                                        # one matrix per group
    for name, x in _adapted(m).items():
        for y in (_adapted(other)[name], _adapted(third)[name]):
            assert _same(x.base_layer.weight.detach(), y.base_layer.weight.detach()), name
            assert _same(x.A.detach(), y.A.detach()) and _same(x.B.detach(), y.B.detach()), name
    moved = _fresh(ALL_TARGETS, init="gaussian")
    moved.pissa_init_(seed=1)
    assert not _same(_adapted(m)[PLANTED[0]].A.detach(), _adapted(moved)[PLANTED[0]].A.detach())


def _one_step(m):
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    e, noise, u = tiny_embeddings(B=2, shapes=((1, 4, 4), (1, 4, 4)), seed=5)
    step = QwenLoraTrainStep(m, lr=1e-3)
    loss = step.forward_backward(e, noise=noise, u=u)
    torch.cuda.synchronize()
    return step, loss.detach().clone(), m.lora_store.gflat.detach().clone(), (e, noise, u)


@pytest.mark.parametrize("quant", [None, "mxfp8"])
def test_no_stale_state(quant, tmp_path):
    """X: PiSSA through add_adapter (for MX-FP8: quantised before the init).  Y: a fresh model that is GIVEN X's residual weights
    and adapters (quantised after).  One train step on each: the same loss and adapter gradients, bit for bit."""
    X = _fresh(init="pissa_niter_2", quant=quant)
    X.save_lora_weights(str(tmp_path / "x"))
    Y = _fresh()
    with torch.no_grad():
        for name, x in _adapted(X).items():
            Y.get_submodule(name).weight.copy_(x.base_layer.weight)
    Y.load_lora_adapter(str(tmp_path / "x"), adapter_name="lora_edit", lora_alpha=8)
    if quant:
        Y.quantize_trunk(quant)
    assert sorted(_adapted(Y)) == sorted(_adapted(X))
    _, lx, gx, _ = _one_step(X)
    _, ly, gy, _ = _one_step(Y)
    assert bool(torch.isfinite(lx)) and bool(gx.any())
    assert _same(lx, ly) and _same(gx, gy)


def test_export_applies_to_the_original_weights(tmp_path):
    from qflux_amd.lora_io import _normalise
    from safetensors import safe_open
    from safetensors.torch import load_file
    X = _fresh(init="pissa")
    step, _, _, (e, noise, u) = _one_step(X)
    step.zero_grad()
    for _ in range(2):
        step.train_step(e, noise=noise, u=u)
    torch.cuda.synchronize()
    path = X.save_lora_weights(str(tmp_path / "conv"), convert_pissa=True)
    with safe_open(path, framework="pt") as f:
        alphas = {n: float(v) for n, v in ast.literal_eval(f.metadata()["lora_alpha"]).items()}
    assert set(alphas.values()) == {16.0}
    O = _fresh()                                                            # the ORIGINAL weights
    O.load_lora_adapter(str(tmp_path / "conv"), adapter_name="lora_edit", lora_alpha=16.0)
    mx, mo = _adapted(X), _adapted(O)
    assert sorted(mx) == sorted(mo)
    for name, x in mx.items():
        o = mo[name]
        assert o.A.shape[0] == 8 and o.scaling[o.active_adapter] == x.scaling[x.active_adapter] == 2.0
        A0, B0 = X._pissa["A0"][name], X._pissa["B0"][name]
        assert _same(o.A.detach().cpu(), torch.cat([x.A.detach().cpu(), -A0], 0)) and _same(o.B.detach().cpu(), torch.cat([x.B.detach().cpu(), B0], 1))
        assert not _same(x.A.detach().cpu(), A0)                            # it trained
    small = _normalise(load_file(X.save_lora_weights(str(tmp_path / "small"), convert_pissa=True, rank=4)))
    from qflux_amd.resize import resize_pairs
    pairs, chunks, off = [], [], 0                                          # the resize tests' standard: the file is what resize_pairs
    for name, o in mo.items():                                              # makes of the rank-2r pairs, bit for bit
        pairs.append((name, off, off + 8 * o.in_features + 64, 8, o.in_features, o.out_features, 2.0))
        chunks += [o.A.detach().reshape(-1), torch.zeros(64, device=DEV), o.B.detach().reshape(-1), torch.zeros(32, device=DEV)]
        off += 8 * o.in_features + 64 + o.out_features * 8 + 32
    direct, direct_alphas, rep = resize_pairs(torch.cat(chunks), pairs, 4)
    for name, x in mx.items():
        assert _same(small[name]["A"], direct[name][0].cpu()) and _same(small[name]["B"], direct[name][1].cpu()) and direct_alphas[name] == 8.0
        A, B = x.A.detach().double().cpu(), x.B.detach().double().cpu()
        want = 2.0 * (B @ A - X._pissa["B0"][name].double() @ X._pissa["A0"][name].double())
        got = 2.0 * (small[name]["B"].double() @ small[name]["A"].double())
        assert small[name]["A"].shape[0] == 4
        sv, k = torch.linalg.svdvals(want).numpy(), rep[name]["kept"]
        best = float(np.sqrt((sv[k:] ** 2).sum()))                          # Eckart-Young at the k components kept
        err, bound = float((got - want).norm()), 4 * np.sqrt(k) * 2.0 ** -24 * float(want.norm())      # the resize tests' bound
        print(f"{name}: k {k} |s B'A' - s (BA - B0A0)| {err:.6e} Eckart-Young {best:.6e} bound {bound:.3e}")      # (test_project_below_the_numeric_rank)
        assert abs(err - best) <= bound, (name, err, best, bound)


def test_resume_rebuilds_the_residual_trunk_from_the_checkpoint(tmp_path):
    """save_checkpoint on an initialised, trained model; load_checkpoint on a fresh model with the ORIGINAL weights and a plain
    adapter: the same base weights and A, B bit for bit, and the next step matches."""
    import json
    X = _fresh(init="pissa_niter_2")
    sx, _, _, (e, noise, u) = _one_step(X)
    sx.zero_grad()
    sx.train_step(e, noise=noise, u=u)
    sx.save_checkpoint(str(tmp_path / "ck"))
    with open(tmp_path / "ck" / "state.json") as f:
        assert json.load(f)["pissa"] == dict(niter=2, oversample=8, seed=0)
    from qflux_amd.trainer import QwenLoraTrainStep
    Y = _fresh(init="gaussian")
    sy = QwenLoraTrainStep(Y, lr=1e-3)
    with pytest.raises(ValueError, match="adapter_name"):
        sy.load_checkpoint(str(tmp_path / "ck"))
    assert Y._pissa is None
    sy.load_checkpoint(str(tmp_path / "ck"), adapter_name="lora_edit")
    assert (Y._pissa["niter"], Y._pissa["oversample"], Y._pissa["seed"]) == (2, 8, 0) and sy.global_step == sx.global_step
    for name, x in _adapted(X).items():
        y = _adapted(Y)[name]
        assert _same(x.base_layer.weight.detach(), y.base_layer.weight.detach()), name
        assert _same(x.A.detach(), y.A.detach()) and _same(x.B.detach(), y.B.detach()), name
        assert _same(X._pissa["A0"][name], Y._pissa["A0"][name]) and _same(X._pissa["B0"][name], Y._pissa["B0"][name])
    lx, ly = sx.train_step(e, noise=noise, u=u), sy.train_step(e, noise=noise, u=u)
    torch.cuda.synchronize()
    assert _same(torch.as_tensor(float(lx)), torch.as_tensor(float(ly))) and _same(X.lora_store.pflat, Y.lora_store.pflat)
    Z = _fresh(init="gaussian")
    Z.pissa_init_(seed=3)
    with pytest.raises(ValueError, match="another"):
        QwenLoraTrainStep(Z, lr=1e-3).load_checkpoint(str(tmp_path / "ck"), adapter_name="lora_edit")


def test_refusals():
    from qflux_amd.modules import LoraConfig
    m, _, _ = _initialised()
    with pytest.raises(ValueError, match="already"):
        m.pissa_init_()
    with pytest.raises(ValueError, match="already"):
        m.add_adapter(LoraConfig(r=4, lora_alpha=8, init_lora_weights="pissa", target_modules=["txt_in"]), "lora_edit")
    merged = _fresh(init="gaussian")
    merged.merge_adapter()
    with pytest.raises(ValueError, match="merged"):
        merged.pissa_init_()
    with pytest.raises(ValueError, match="scaling"):
        _fresh(init="pissa", alpha=0)
    with pytest.raises(ValueError, match="scaling"):
        _fresh(init="gaussian", alpha=-8).pissa_init_()
    cpu = _fresh(init="gaussian").to("cpu")
    with pytest.raises(RuntimeError, match="not on a GPU"):
        cpu.pissa_init_()
    bad = _fresh(init="gaussian")
    before = bad.get_submodule(PLANTED[1]).base_layer.weight.detach().clone()
    with torch.no_grad():
        bad.get_submodule(PLANTED[0]).base_layer.weight[3, 5] = float("nan")
    with pytest.raises(ValueError, match="to_q"):
        bad.pissa_init_(group_bytes=1)
    assert bad._pissa is None and _same(bad.get_submodule(PLANTED[1]).base_layer.weight.detach(), before)
    # through add_adapter no plain LoRA is left behind: refused before anything is wrapped, or unwrapped again
    from qflux_amd.modules import QfxLoraLinear
    for kw in (dict(alpha=0), dict(r=65, alpha=65)):
        m = _fresh()
        with pytest.raises((ValueError, NotImplementedError)):
            m.add_adapter(LoraConfig(r=kw.get("r", 4), lora_alpha=kw["alpha"], init_lora_weights="pissa", target_modules=list(STEP_TARGETS)), "lora_edit")
        assert not _adapted(m) and not getattr(m, "peft_config", None)
    m = _fresh()
    with torch.no_grad():
        m.get_submodule(PLANTED[0]).weight[3, 5] = float("nan")
    with pytest.raises(ValueError, match="to_q"):
        m.add_adapter(LoraConfig(r=4, lora_alpha=8, init_lora_weights="pissa", target_modules=list(STEP_TARGETS)), "lora_edit")
    assert not any(isinstance(x, QfxLoraLinear) for x in m.modules()) and "lora_edit" not in m.peft_config and m._pissa is None
    assert type(m.get_submodule(PLANTED[0])).__name__ == "QfxLinear"
