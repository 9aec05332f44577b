"""GPU: qfx_lowrank_sketch against the fp64 restatement (tests/lora_extract_ref.py) with the same seed, on quantities that do not
hang on an ill-conditioned basis: (a) the residual, (b) the leading singular values of C, (c) the orthonormality of Q, (d) normsq,
(e) Q C elementwise where it is well determined.  The tolerances are committed in profiles/lora_extract_accuracy.json: 8 x the
deviation of the restatement's fp32 mode from its fp64 mode (tests/test_lora_extract_cpu.py), floored at 1e-6.  Then
extract_pairs on a tiny Qwen DiT with a merged adapter, and the file it saves loaded into a fresh model.

The D X launch owns ROW_CHUNK = 64 rows of D per workgroup, the D^T X launch COL_CHUNK = 64 columns: the case list holds one
shape with out = 65 and one with in = 65.  QFX_LORA_EXTRACT_MEASURED_OUT=<file> writes the kernel's measured deviations there."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lora_extract_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("residual", "sv", "orth", "normsq", "product")
SEED = 0x5EED0000BEEF
_FIX = {}


def _tol():
    with open(os.path.join(ROOT, "profiles", "lora_extract_accuracy.json")) as f:
        return json.load(f)["tolerance"]


def _cases():
    """The case list with the fp64 restatement's metrics at q = 2 (table index = position in the list), once."""
    if "cases" not in _FIX:
        cases = R.make_cases()
        for i, c in enumerate(cases):
            c["index"] = i
            c["D"] = R.difference(c["W1"], c["W0"])
            ref = R.sketch(c["W1"], c["W0"], c["k"], 2, SEED, i)
            c["ref"] = dict(R.metrics(c["D"], ref["Q"], ref["C"], c["rank"], ref["kept"]), normsq=ref["normsq"], kept=ref["kept"])
            c["well"] = R.well_determined(c["D"], c["k"])
        _FIX["cases"] = cases
    return _FIX["cases"]


def _place(x, dtype, odd):
    """A device matrix holding x: contiguous, or (odd) 1 element off its allocation with a leading dimension of in + 3."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    if not odd:
        return t.to(DEV)
    nout, nin = t.shape
    buf = torch.zeros(nout * (nin + 3) + 1, dtype=dtype, device=DEV)
    v = buf[1:].view(nout, nin + 3)[:, :nin]
    v.copy_(t)
    return v


def _run(cases, q=2, shift=0, seed=SEED):
    """One table over `cases` in the given order -> per case (Q, C, normsq, info) on the host, and skipped.  shift: floats ahead
    of every buffer, so that each lands at another address."""
    from qflux_amd import ops
    rows, off = [], 0
    for c in cases:
        dt = torch.bfloat16 if c["dtype"] == "bf16" else torch.float32
        W1 = _place(c["W1"], dt, c["odd"])
        W0 = None if c["W0"] is None else (W1 if c.get("same") else _place(c["W0"], dt, c["odd"]))
        nout, nin = W1.shape
        oa = off + 4 + (1 if c["odd"] else 0)
        ob = (oa + c["k"] * nin + 3) // 4 * 4 + 4 + (3 if c["odd"] else 0)
        off = (ob + nout * c["k"] + 3) // 4 * 4
        rows.append((W1, W0, c["k"], oa, ob, c["index"]))
    n = len(rows)
    pfull = torch.full((shift + off + 8,), 12345.0, device=DEV)
    p = pfull[shift:]
    lay = ops.lowrank_table(rows, device=DEV, n_elems=p.numel())
    normsq = torch.full((shift + n,), -7.0, dtype=torch.float64, device=DEV)[shift:]
    info = torch.full((shift + n, 2), -7, dtype=torch.int32, device=DEV)[shift:]
    skipped = torch.full((shift + 1,), -7, dtype=torch.int32, device=DEV)[shift:]
    ws = torch.full((16 * shift + lay.ws_bytes,), 0xAB, dtype=torch.uint8, device=DEV)[16 * shift:]
    ops.lowrank_sketch(lay, p, normsq, info, skipped, ws, power_iters=q, seed=seed)
    ph, out = p.cpu(), {}
    used = torch.zeros(ph.numel(), dtype=torch.bool)
    for c, row, (_, _, k, nin, nout), ns, inf in zip(cases, rows, lay.rows, normsq.cpu().tolist(), info.cpu().tolist()):
        oa, ob = row[3:5]
        out[c["label"]] = (ph[ob:ob + nout * k].view(nout, k).clone(), ph[oa:oa + k * nin].view(k, nin).clone(), ns, inf)
        used[oa:oa + k * nin] = True
        used[ob:ob + nout * k] = True
    assert bool((ph[~used] == 12345.0).all())          # nothing written outside the outputs
    return out, int(skipped.item())


def _fixture(name):
    if name not in _FIX:
        cases = _cases()
        _FIX[name] = _run(cases if name == "forward" else cases[::-1])
    return _FIX[name]


def _bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _deviation(c, Q, C, ns, ref=None):
    kept = int((Q != 0).any(dim=0).sum())
    m = R.metrics(c["D"], Q.numpy(), C.numpy(), c["rank"], kept)
    return R.deviations(c["ref"] if ref is None else ref, m, ns), kept


def test_mixed_table_against_the_restatement():
    out, skipped = _fixture("forward")
    tol, worst, per = _tol(), {k: 0.0 for k in KEYS}, {}
    assert skipped == 0
    for c in _cases():
        Q, C, ns, info = out[c["label"]]
        d, kept = _deviation(c, Q, C, ns)
        if not c["well"]:
            d["product"] = 0.0
        per[c["label"]] = d
        print(c["label"], {k: f"{v:.2e}" for k, v in d.items()}, "kept", info[0], "ref kept", c["ref"]["kept"], "residual", f"{c['ref']['residual']:.3e}")
        for k in KEYS:
            worst[k] = max(worst[k], d[k])
        assert info[1] == 1 and info[0] == kept <= min(c["k"], *c["D"].shape), (c["label"], info, kept)
        # the dropped columns of Q and rows of C: +0.0 bit for bit
        assert bool((Q[:, kept:].contiguous().view(torch.int32) == 0).all()) and bool((C[kept:].contiguous().view(torch.int32) == 0).all())
    print("worst", worst, "tolerance", tol)
    if os.environ.get("QFX_LORA_EXTRACT_MEASURED_OUT"):
        with open(os.environ["QFX_LORA_EXTRACT_MEASURED_OUT"], "w") as f:
            json.dump({"kernel_deviation_worst": worst, "kernel_deviation": per}, f, indent=1)
    for c in _cases():
        for k in KEYS:
            assert per[c["label"]][k] <= tol[k], (c["label"], k, per[c["label"]][k], tol[k])
    assert sum(c["well"] for c in _cases()) >= 6 and _cases()[5]["ref"]["kept"] == 8          # k > out keeps out columns


def test_same_bits_in_another_order_twice_and_at_other_addresses():
    a, _ = _fixture("forward")
    for other in (_fixture("reversed")[0], _run(_cases())[0], _run(_cases(), shift=3)[0]):
        for c in _cases():
            (Q, C, ns, info), (Q2, C2, ns2, info2) = a[c["label"]], other[c["label"]]
            assert _bits(Q, Q2) and _bits(C, C2) and ns == ns2 and info == info2, c["label"]
    # the table index feeds Omega, the seed too
    c = dict(_cases()[0])
    base = a[c["label"]]
    for change in (dict(index=7), dict()):
        got = _run([dict(c, **change)], seed=SEED if change else SEED + 1)[0][c["label"]]
        assert not _bits(base[1], got[1]) and got[2] == base[2]


def test_no_power_iterations():
    """q = 0 on two cases; the tolerance by the same rule, over these two."""
    cases = [dict(c) for c in _cases()[:2]]
    out, _ = _run(cases, q=0)
    for c in cases:
        r64, r32 = R.sketch(c["W1"], c["W0"], c["k"], 0, SEED, c["index"]), R.sketch(c["W1"], c["W0"], c["k"], 0, SEED, c["index"], fp32=True)
        m64 = dict(R.metrics(c["D"], r64["Q"], r64["C"], c["rank"], r64["kept"]), normsq=r64["normsq"])
        d32 = R.deviations(m64, R.metrics(c["D"], r32["Q"], r32["C"], c["rank"], r32["kept"]), r32["normsq"])
        Q, C, ns, info = out[c["label"]]
        d, kept = _deviation(c, Q, C, ns, m64)
        print(c["label"], "q=0", {k: f"{v:.2e}" for k, v in d.items()}, "residual", m64["residual"])
        assert m64["residual"] > c["ref"]["residual"]               # it is the q = 0 answer
        for k in KEYS:
            assert d[k] <= max(8.0 * d32[k], 1e-6), (c["label"], k, d[k], d32[k])


def test_zero_difference_and_a_nan():
    cases = _cases()
    zero = dict(cases[0], label="same", same=True, W0=cases[0]["W1"], index=0)
    nan = dict(cases[2], label="nan", W1=cases[2]["W1"].copy())
    nan["W1"][5, 700] = np.nan
    inf = dict(cases[8], label="inf", W1=cases[8]["W1"].copy())
    inf["W1"][0, 0] = np.inf
    keep = [cases[1], cases[3]]
    out, skipped = _run([keep[0], zero, nan, keep[1], inf])
    assert skipped == 2
    for lab in ("same", "nan", "inf"):
        Q, C, ns, info = out[lab]
        assert bool((Q.view(torch.int32) == 0).all()) and bool((C.view(torch.int32) == 0).all()) and ns == 0.0 and info[0] == 0, lab
    assert out["same"][3] == [0, 1] and out["nan"][3] == [0, 0] and out["inf"][3] == [0, 0]
    a, _ = _fixture("forward")
    for c in keep:
        assert _bits(a[c["label"]][0], out[c["label"]][0]) and _bits(a[c["label"]][1], out[c["label"]][1])


# ------------------------------------------------------------------ end to end on the tiny Qwen DiT

def _pred(dit, batch):
    emb = batch[0]
    x = torch.cat([emb["image_latents"], emb["control_latents"]], dim=1).to(torch.bfloat16)
    pe = emb["prompt_embeds"].to(torch.bfloat16)
    with torch.no_grad():
        return dit(hidden_states=x.to(DEV), encoder_hidden_states=pe.to(DEV), encoder_hidden_states_mask=emb["prompt_embeds_mask"],
                   timestep=torch.tensor([0.3]).to(DEV), img_shapes=emb["img_shapes"], txt_seq_lens=[pe.shape[1]], return_dict=False)[0].float().cpu()


def _model():
    from common import TINY
    from parity_util import build_pair
    from test_maxnorm_gpu import TARGETS
    return build_pair(dict(TINY), r=8, lora_alpha=8, device=DEV, targets=TARGETS, seed=2)[1]


def test_extract_from_a_merged_model_and_load_the_file(tmp_path):
    from parity_util import relmax, tiny_embeddings
    from qflux_amd.extract import extract_lora, extract_pairs
    from qflux_amd.lora_io import load_lora_adapter
    from qflux_amd.modules import QfxLoraLinear
    batch = tiny_embeddings(B=1, seed=5)
    dit = _model()
    mods = {n: m for n, m in dit.named_modules() if isinstance(m, QfxLoraLinear)}
    g = torch.Generator().manual_seed(17)
    base = {}
    with torch.no_grad():
        for n, m in mods.items():
            m.B.copy_((torch.randn(m.B.shape, generator=g) * 0.05).to(DEV))
            base[n] = m.base_layer.weight.detach().clone()
    dit.merge_adapter()
    want = _pred(dit, batch)
    mats = [(n, m.base_layer.weight.detach(), base[n]) for n, m in mods.items()]
    tensors, alphas, report = extract_pairs(mats, 8)
    optimal, worst = {}, 0.0
    for n, W1, W0 in mats:
        D = (W1.float() - W0.float()).double().cpu()
        U, S, Vh = torch.linalg.svd(D, full_matrices=False)
        best = float(S[8:].pow(2).sum().sqrt())
        A2, B2 = tensors[n]
        err = float(torch.linalg.norm(B2.double().cpu() @ A2.double().cpu() - D))
        worst = max(worst, err / best)
        assert err <= 1.01 * best, (n, err, best)
        assert A2.shape == (8, D.shape[1]) and B2.shape == (D.shape[0], 8) and alphas[n] == 8.0
        assert abs(report[n]["diff_norm"] - float(torch.linalg.norm(D))) <= 1e-6 * report[n]["diff_norm"]
        assert abs(report[n]["fro_retained_of_diff"] - float(S[:8].pow(2).sum().sqrt() / S.pow(2).sum().sqrt())) <= 1e-4
        optimal[n] = ((Vh[:8]).float(), (U[:, :8] * S[:8]).float())
    print("worst error ratio to the rank-8 optimum", worst)
    # the fp64-optimal factors in a fresh model: how far a perfect rank-8 extraction is from the merged model
    fresh = _model()
    with torch.no_grad():
        for n, m in fresh.named_modules():
            if isinstance(m, QfxLoraLinear):
                m.A.copy_(optimal[n][0].to(DEV))
                m.B.copy_(optimal[n][1].to(DEV))
    dev_opt = relmax(_pred(fresh, batch), want)
    sd_base = {n + ".weight": w for n, w in base.items()}
    sd_tuned = {n + ".weight": m.base_layer.weight.detach() for n, m in mods.items()}
    _, _, rep = extract_lora(sd_base, sd_tuned, save_to=str(tmp_path / "lora"), rank=8, device=DEV, group_bytes=1 << 16)
    assert sorted(rep) == sorted(mods) and not any(v["unchanged"] for v in rep.values())
    load_lora_adapter(fresh, str(tmp_path / "lora"))
    dev = relmax(_pred(fresh, batch), want)
    print("forward deviation from the merged model: extracted", dev, "fp64-optimal factors", dev_opt)
    assert dev <= 8.0 * dev_opt, (dev, dev_opt)
