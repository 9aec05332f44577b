"""GPU: qfx_lora_spectrum / qfx_lora_project against LAPACK (torch.linalg.svdvals of the fp64 product) on the case list of
tests/lora_svd_ref.py, laid out once with aligned and once with odd offsets, then through spectrum.py / resize.py on a tiny Qwen DiT
and through safetensors files.  The spectrum tolerance hangs on the restatement's own error against LAPACK, measured on the CPU and
committed in profiles/lora_svd_accuracy.json (tests/test_lora_svd_cpu.py), times 16 for the kernel's other Gram summation order."""
import ast
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lora_svd_ref as R  # noqa: E402
from test_maxnorm_gpu import _batch, _lay_out, _qwen  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24
SCALE = -1.5          # the scale of the max-norm cross-check
_FIX = {}


def _tol():
    with open(os.path.join(ROOT, "profiles", "lora_svd_accuracy.json")) as f:
        return 16.0 * float(json.load(f)["worst_sq_error"])


def _cases():
    """The case list with LAPACK's singular values, once."""
    if "cases" not in _FIX:
        _FIX["cases"] = [(lab, A, B, R.lapack_sv(A, B)) for lab, A, B in R.make_cases()]
    return _FIX["cases"]


def _many():
    """300 tiny pairs: more pairs than workgroups of one wave of the chip."""
    if "many_cases" not in _FIX:
        rng = np.random.default_rng(3)
        raw = [(f"tiny{i}", (rng.standard_normal((4, 64)) * 0.1).astype(np.float32),
                (rng.standard_normal((48, 4)) * 0.1).astype(np.float32)) for i in range(300)]
        _FIX["many_cases"] = [(lab, A, B, R.lapack_sv(A, B)) for lab, A, B in raw]
    return _FIX["many_cases"]


def _rho_ref(ref):
    return int((ref > R.RANK_TOL * ref[0]).sum()) if ref[0] > 0 else 0


def _run(cases, odd, ks=None, pad=2, nan_in=None):
    """Spectrum with a workspace, then project with k = ks[i] (default: the numeric rank, at least 1) into r_dst = min(k + pad, 64)
    rows.  Everything comes back on the host."""
    from qflux_amd import ops
    pairs = [(torch.from_numpy(A), torch.from_numpy(B), 1.0) for _, A, B, _ in cases]
    rows, buf, _ = _lay_out(pairs, odd)
    if nan_in is not None:
        buf[rows[nan_in][1] + 1] = float("nan")
    p = buf.to(DEV)
    lay = ops.lora_svd_table([r[:5] for r in rows], device=DEV, n_elems=p.numel())
    n = lay.n_pairs
    sv = torch.full((n, 64), -7.0, dtype=torch.float64, device=DEV)
    info = torch.full((n, 4), -7, dtype=torch.int32, device=DEV)
    skipped = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    ws = torch.full((n * ops.LORA_SVD_WS_DOUBLES,), -7.0, dtype=torch.float64, device=DEV)
    ops.lora_spectrum(p, lay, sv, info, skipped, ws=ws)
    info_h = info.cpu()
    dst, off = [], 0
    for i, (_, _, r, nin, nout) in enumerate(lay.pairs):
        k = max(int(info_h[i, 0]), 1) if ks is None else ks[i]
        r_dst = min(k + pad, 64)
        oa = off + (3 if odd else 0)
        ob = (oa + r_dst * nin + 3) // 4 * 4 + (1 if odd else 0)
        dst.append((oa, ob, k, r_dst))
        off = (ob + nout * r_dst + 3) // 4 * 4
    q = torch.full((off + 4,), 12345.0, device=DEV)
    tab = ops.lora_project_table(lay, dst, device=DEV, n_elems=q.numel())
    ops.lora_project(p, q, lay, tab, ws)
    qh = q.cpu()
    out = []
    for (oa, ob, k, r_dst), (_, _, r, nin, nout) in zip(dst, lay.pairs):
        out.append((qh[oa:oa + r_dst * nin].view(r_dst, nin).clone(), qh[ob:ob + nout * r_dst].view(nout, r_dst).clone(), k, r_dst))
    return dict(sv=sv.cpu(), info=info_h, skipped=int(skipped.item()), ws=ws.cpu().view(n, 2, 64, 64), out=out, rows=rows, buf=buf)


def _fixture(name):
    if name not in _FIX:
        _FIX[name] = _run(_many() if name == "many" else _cases(), odd=name == "odd")
    return _FIX[name]


def _bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.view(torch.int64 if x.element_size() == 8 else torch.int32),
                                                                     y.view(torch.int64 if y.element_size() == 8 else torch.int32))


@pytest.mark.parametrize("name", ["aligned", "odd", "many"])
def test_spectrum_against_lapack(name):
    fx, cases = _fixture(name), (_many() if name == "many" else _cases())
    tol = _tol()
    if name != "many":
        assert all(((off % 4) in (1, 3)) == (name == "odd") for row in fx["rows"] for off in row[:2])
    assert fx["skipped"] == 0
    worst = 0.0
    for i, (lab, A, B, ref) in enumerate(cases):
        r = A.shape[0]
        assert R.unambiguous(ref), lab
        sv = fx["sv"][i].numpy()
        err = R.sq_error(sv[:r], ref)
        worst = max(worst, err)
        if name != "many":
            print(f"{name} {lab}: sq_error {err:.3e} (tolerance {tol:.3e}) rho {int(fx['info'][i, 0])} sweeps {fx['info'][i, 1:3].tolist()}")
        assert err <= tol, (lab, err, tol)
        assert bool((sv[r:] == 0.0).all()) and bool((np.diff(sv[:r]) <= 0).all()), lab
        assert int(fx["info"][i, 3]) == 1, (lab, fx["info"][i].tolist())
        assert int(fx["info"][i, 0]) == _rho_ref(ref), (lab, fx["info"][i].tolist(), _rho_ref(ref))
    print(f"{name}: worst sq_error {worst:.3e}")


def test_frobenius_norm_agrees_with_the_max_norm_launch():
    from qflux_amd import ops
    fx = _fixture("aligned")
    rows = [tuple(r[:5]) + (SCALE,) for r in fx["rows"]]
    p = fx["buf"].to(DEV)
    lay = ops.maxnorm_table(rows, device=DEV, n_elems=p.numel())
    norms, ratios, summary = (torch.zeros(k, device=DEV) for k in (lay.n_pairs, lay.n_pairs, 4))
    ops.maxnorm_apply(p, lay, float("inf"), norms, ratios, summary)
    mine = (abs(SCALE) * fx["sv"].pow(2).sum(dim=1).sqrt()).to(torch.float32)
    d = (mine.view(torch.int32).long() - norms.cpu().view(torch.int32).long()).abs()
    assert int(d.max()) <= 2, d.tolist()


def _products(A, B, A2, B2):
    P = B.astype(np.float64) @ A.astype(np.float64)
    P2 = B2.numpy().astype(np.float64) @ A2.numpy().astype(np.float64)
    return P, P2


@pytest.mark.parametrize("name", ["aligned", "odd"])
def test_project_at_the_numeric_rank(name):
    fx = _fixture(name)
    for i, (lab, A, B, ref) in enumerate(_cases()):
        A2, B2, k, r_dst = fx["out"][i]
        assert k == max(_rho_ref(ref), 1) and r_dst == min(k + 2, 64)
        P, P2 = _products(A, B, A2, B2)
        err, bound = np.linalg.norm(P2 - P), 4 * np.sqrt(k) * EPS32 * np.linalg.norm(P)
        print(f"{name} {lab}: k {k} |B'A' - BA| {err:.3e} bound {bound:.3e}")
        assert err <= bound, (lab, err, bound)
        # rows / columns k <= j < r_dst: +0.0 bit for bit
        assert bool((A2[k:].view(torch.int32) == 0).all()) and bool((B2[:, k:].contiguous().view(torch.int32) == 0).all()), lab
        if lab == "b_zero":
            assert k == 1 and bool((A2.view(torch.int32) == 0).all()) and bool((B2.contiguous().view(torch.int32) == 0).all())


def test_project_below_the_numeric_rank():
    cases = _cases()
    ks = [max(_rho_ref(ref) // 2, 1) for _, _, _, ref in cases]
    fx = _run(cases, odd=False, ks=ks, pad=0)
    seen = 0
    for i, (lab, A, B, ref) in enumerate(cases):
        A2, B2, k, r_dst = fx["out"][i]
        if k >= _rho_ref(ref):
            continue
        seen += 1
        P, P2 = _products(A, B, A2, B2)
        err, want = np.linalg.norm(P2 - P), float(np.sqrt((ref[k:] ** 2).sum()))
        bound = 4 * np.sqrt(k) * EPS32 * np.linalg.norm(P)
        print(f"{lab}: k {k} |B'A' - BA| {err:.6e} Eckart-Young {want:.6e} bound {bound:.3e}")
        assert abs(err - want) <= bound, (lab, err, want, bound)
        gram = A2.numpy().astype(np.float64) @ A2.numpy().astype(np.float64).T
        assert np.abs(gram - np.eye(k)).max() <= 8 * A.shape[0] * EPS32, (lab, np.abs(gram - np.eye(k)).max())
    assert seen >= 6


def test_same_bits_twice_and_at_any_offset():
    a, b = _fixture("aligned"), _fixture("odd")
    again = _run(_cases(), odd=False)
    for other in (again, b):
        assert _bits(a["sv"], other["sv"]) and _bits(a["ws"], other["ws"]) and torch.equal(a["info"], other["info"])
        for (A2, B2, k, rd), (A3, B3, k3, rd3) in zip(a["out"], other["out"]):
            assert (k, rd) == (k3, rd3) and _bits(A2, A3) and _bits(B2, B3)


def test_a_nan_skips_its_pair_only():
    cases = _cases()
    bad = 2
    a, fx = _fixture("aligned"), _run(cases, odd=False, nan_in=bad)
    assert fx["skipped"] == 1 and fx["info"][bad].tolist() == [0, 0, 0, 0]
    assert bool((fx["sv"][bad] == 0).all()) and bool((fx["ws"][bad] == 0).all())
    keep = [i for i in range(len(cases)) if i != bad]
    assert _bits(a["sv"][keep], fx["sv"][keep]) and _bits(a["ws"][keep], fx["ws"][keep]) and torch.equal(a["info"][keep], fx["info"][keep])
    for i in keep:
        assert _bits(a["out"][i][0], fx["out"][i][0]) and _bits(a["out"][i][1], fx["out"][i][1])


# ------------------------------------------------------------------ through the public interface

def _trained(steps=2):
    """A tiny Qwen DiT whose adapters have left their B = 0 start, and its train step."""
    from qflux_amd.trainer import QwenLoraTrainStep
    dit = _qwen()
    step = QwenLoraTrainStep(dit, lr=1e-2, weight_decay=0.0)
    e, nz, u = _batch()
    for _ in range(steps):
        step.train_step(e, noise=nz, u=u)
    return dit, step, (e, nz, u)


def _lapack_of(m, name=None):
    name = m.active_adapter if name is None else name
    P = m.lora_B[name].weight.detach().double().cpu() @ m.lora_A[name].weight.detach().double().cpu()
    return torch.linalg.svdvals(P * m.scaling[name])


def _pred(dit, step, batch):
    e, nz, u = batch
    loss = step.forward_backward(e, noise=nz, u=u)
    step.zero_grad()
    plan = list(dit._plans.values())[0]
    return float(loss), plan.A["out"].detach().float().cpu().clone()


def test_adapter_spectrum_of_a_model():
    from qflux_amd.modules import QfxLoraLinear
    from qflux_amd.spectrum import adapter_spectrum, spectrum_summary
    dit, _, _ = _trained()
    mods = {n: m for n, m in dit.named_modules() if isinstance(m, QfxLoraLinear)}
    sv = adapter_spectrum(dit)
    assert sorted(sv) == sorted(mods) and len(sv) > 0
    tol = _tol()
    for n, m in mods.items():
        ref = _lapack_of(m).numpy()
        assert sv[n].dtype == torch.float64 and sv[n].shape == (m.r[m.active_adapter],)
        assert R.sq_error(sv[n].numpy(), ref[:len(sv[n])]) <= tol, n
    summ = spectrum_summary(dit)
    for n, s in summ.items():
        assert s["converged"] and 1.0 - 1e-12 <= s["stable_rank"] <= len(sv[n]) and s["effective_rank"] <= len(sv[n]) + 1e-9
        assert abs(s["fro"] - float(sv[n].pow(2).sum().sqrt())) <= 1e-12 * s["fro"] and s["spectral"] == float(sv[n][0])


def test_resize_adapter_at_full_rank_keeps_the_forward():
    from parity_util import QWEN_BARS, relmax
    from qflux_amd.modules import QfxLoraLinear
    from qflux_amd.resize import resize_adapter
    from qflux_amd.trainer import QwenLoraTrainStep
    dit, step, batch = _trained()
    _, before = _pred(dit, step, batch)
    old = {n: (m.A.detach().clone(), m.B.detach().clone(), m.active_adapter) for n, m in dit.named_modules() if isinstance(m, QfxLoraLinear)}
    report = resize_adapter(dit, 4)
    assert sorted(report) == sorted(old) and all(v["new_rank"] == 4 and v["old_rank"] == 4 for v in report.values())
    for n, m in dit.named_modules():
        if isinstance(m, QfxLoraLinear):
            A, B, name = old[n]
            assert m.active_adapter == "resized" and _bits(m.lora_A[name].weight.detach(), A) and _bits(m.lora_B[name].weight.detach(), B)
            assert m.scaling["resized"] == m.scaling[name]
    _, after = _pred(dit, QwenLoraTrainStep(dit, lr=1e-2), batch)
    assert relmax(after, before) < QWEN_BARS[1], relmax(after, before)


def test_resize_adapter_to_half_rank_trains_on():
    from qflux_amd.modules import QfxLoraLinear
    from qflux_amd.resize import resize_adapter
    from qflux_amd.trainer import QwenLoraTrainStep
    dit, _, (e, nz, u) = _trained()
    report = resize_adapter(dit, 2)
    assert all(v["new_rank"] == 2 and v["kept"] <= 2 and 0 < v["fro_retained"] <= 1 for v in report.values())
    assert all(m.A.shape[0] == 2 and m.B.shape[1] == 2 for m in dit.modules() if isinstance(m, QfxLoraLinear))
    step = QwenLoraTrainStep(dit, lr=1e-2, weight_decay=0.0)
    losses = [float(step.train_step(e, noise=nz, u=u)) for _ in range(3)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_step_adapter_spectrum_leaves_the_step_alone():
    from tools import plan_fingerprint as pf
    (da, sa, (e, nz, u)), (db, sb, _) = _trained(), _trained()
    plans = list(da._plans.values())
    digest = pf.digest(pf.fingerprint(plans[0]))
    sv = sa.adapter_spectrum()
    assert len(sv) == len(sa.adapter_spectrum()) > 0
    la, lb = sa.train_step(e, noise=nz, u=u), sb.train_step(e, noise=nz, u=u)
    assert _bits(torch.as_tensor(float(la)), torch.as_tensor(float(lb)))
    assert _bits(da.lora_store.pflat.cpu(), db.lora_store.pflat.cpu())
    after = list(da._plans.values())
    assert len(after) == len(plans) and after[0] is plans[0] and pf.digest(pf.fingerprint(after[0])) == digest


# ------------------------------------------------------------------ files

def _direct(dit, new_rank, **kw):
    from qflux_amd.regularize import adapter_pairs
    from qflux_amd.resize import resize_pairs
    store = dit.lora_store
    return resize_pairs(store.pflat, adapter_pairs(store), new_rank, **kw)


def test_resize_lora_file_uniform_round_trip(tmp_path):
    from qflux_amd.lora_io import load_lora_adapter, save_lora_weights
    from qflux_amd.modules import QfxLoraLinear
    from qflux_amd.resize import resize_lora_file
    from safetensors import safe_open
    dit, _, _ = _trained()
    save_lora_weights(dit, str(tmp_path / "src"))
    report = resize_lora_file(str(tmp_path / "src"), str(tmp_path / "dst"), 2, dynamic_method="sv_fro", dynamic_param=0.9)
    tensors, alphas, direct = _direct(dit, 2, dynamic_method="sv_fro", dynamic_param=0.9)
    assert {n: v["new_rank"] for n, v in report.items()} == {n: v["new_rank"] for n, v in direct.items()}
    with safe_open(str(tmp_path / "dst" / "pytorch_lora_weights.safetensors"), framework="pt") as f:
        written = ast.literal_eval(f.metadata()["lora_alpha"])
    assert {n: float(a) for n, a in written.items()} == alphas and len(set(alphas.values())) == 1
    fresh = _qwen()
    fresh_plain = {n for n, m in fresh.named_modules() if isinstance(m, QfxLoraLinear)}
    assert fresh_plain == set(tensors)
    # a model without adapters takes the file's rank and the written alpha
    from common import TINY
    from qflux_amd.models import QwenImageTransformer2DModel
    with torch.device(DEV):
        bare = QwenImageTransformer2DModel(**dict(TINY))
    load_lora_adapter(bare, str(tmp_path / "dst"), lora_alpha=next(iter(alphas.values())))
    for n, m in bare.named_modules():
        if isinstance(m, QfxLoraLinear):
            A2, B2 = tensors[n]
            got = (m.B.detach() @ m.A.detach()) * m.scaling[m.active_adapter]
            want = (B2 @ A2) * (alphas[n] / A2.shape[0])
            assert _bits(got.cpu(), want.cpu()), n


def test_resize_lora_file_per_module_ranks_keep_the_key_style(tmp_path):
    from qflux_amd.lora_io import _normalise, save_lora_weights
    from qflux_amd.resize import resize_lora_file
    from safetensors import safe_open
    from safetensors.torch import load_file
    dit, _, _ = _trained()
    for style in ("diffusers", "peft"):
        src, dst = tmp_path / f"src_{style}", tmp_path / f"dst_{style}.safetensors"
        save_lora_weights(dit, str(src), style=style)
        report = resize_lora_file(str(src), str(dst), 4, dynamic_method="sv_ratio", dynamic_param=2.0, uniform=False)
        before, after = load_file(str(src / "pytorch_lora_weights.safetensors")), load_file(str(dst))
        assert sorted(before) == sorted(after)
        with safe_open(str(dst), framework="pt") as f:
            alphas = ast.literal_eval(f.metadata()["lora_alpha"])
        mods = _normalise(after)
        assert sorted(mods) == sorted(report)
        for n, ab in mods.items():
            k = report[n]["new_rank"]
            assert k == report[n]["kept"] and ab["A"].shape[0] == k and ab["B"].shape[1] == k
            assert float(alphas[n]) == 2.0 * k          # scaling = 8 / 4 stays
        assert len({v["new_rank"] for v in report.values()}) > 1 or all(v["new_rank"] == 4 for v in report.values())
