"""CPU: the numpy restatement of the qfx_lowrank_sketch listing (tests/lora_extract_ref.py) -- its sign matrix against the Philox
restatement of the dropout masks, the algorithm against numpy.linalg.svd, exact recovery -- the host-side refusals of the library,
and the plumbing of qflux_amd.extract with the device part replaced by the restatement.

    QFX_WRITE_LORA_EXTRACT_ACCURACY=1 python -m pytest tests/test_lora_extract_cpu.py -k tolerances

rewrites the tolerances in profiles/lora_extract_accuracy.json: 8 x the largest deviation of the restatement's fp32 mode from its
fp64 mode over the case list, floored at 1e-6 -- the numbers the GPU tests hang on."""
import ast
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lora_extract_ref as R  # noqa: E402
from lora_dropout_ref import philox4x32_10  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "lora_extract_accuracy.json")
EINVAL = -1
KEYS = ("residual", "sv", "orth", "normsq", "product")


def test_sign_matrix_agrees_with_the_philox_restatement():
    for nin, k, index, seed in ((7, 5, 0, 0), (70, 64, 3, 0x1234567890), (33, 33, 65535, 1)):
        om = R.omega(nin, k, index, seed)
        assert om.shape == (nin, k) and set(np.unique(om)) <= {-1.0, 1.0}
        for i in (0, nin // 2, nin - 1):
            w = [int(x) for x in philox4x32_10(i, index, R.OMEGA_TAG, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)]
            for j in range(k):
                assert om[i, j] == (-1.0 if (w[j >> 5] >> (j & 31)) & 1 else 1.0), (i, j)
    assert 0.4 < (R.omega(4096, 64) > 0).mean() < 0.6
    assert not np.array_equal(R.omega(64, 16, 0), R.omega(64, 16, 1)) and not np.array_equal(R.omega(64, 16, 0, 0), R.omega(64, 16, 0, 1))


SPECTRA = {"0.8^i": lambda n: 0.8 ** np.arange(n), "1/(1+i)": lambda n: 1.0 / (1.0 + np.arange(n)),
           "plateau": lambda n: np.where(np.arange(n) < 8, 1.0, 0.05)}


@pytest.mark.parametrize("name", list(SPECTRA))
def test_near_optimality_against_numpy_svd(name):
    """Measured with the Philox stream (seed 0, index 0), rank 8, k = 16: ratio to the Eckart-Young optimum at q = 2
    1.00000 (0.8^i), 1.00003 (1/(1+i)), 1.00000 (plateau), at q = 0 1.04, 1.20, 1.38; largest singular value error
    1.1e-5 sigma_0 (1/(1+i)).  The run prints the figures."""
    rng = np.random.default_rng(5)
    D = R.with_spectrum(rng, 160, 224, SPECTRA[name](160))
    s = np.linalg.svd(D, compute_uv=False)
    best = float(np.sqrt((s[8:] ** 2).sum()))
    ratios = {}
    for q in (0, 2):
        out = R.sketch(D, None, 16, q=q)
        up, down, sv = R.truncate(out["Q"], out["C"], 8)
        ratios[q] = float(np.linalg.norm(D - up @ down)) / best
        if q == 2:
            sv_err = float(np.abs(sv[:8] - s[:8]).max() / s[0])
    print(f"{name}: ratio q=0 {ratios[0]:.5f} q=2 {ratios[2]:.5f} sv error {sv_err:.3e} sigma_0")
    assert out["converged"] and out["kept"] == 16
    assert ratios[2] <= 1.01 and sv_err <= 1e-3


def test_exact_recovery_and_degenerate_inputs():
    rng = np.random.default_rng(6)
    D = R.with_spectrum(rng, 120, 90, np.linspace(2.0, 1.0, 8))
    out = R.sketch(D, None, 16)
    assert out["kept"] == 8 and np.linalg.norm(D - out["Q"] @ out["C"]) <= 1e-12 * np.linalg.norm(D)
    assert not out["Q"][:, 8:].any() and not out["C"][8:].any()
    W0 = rng.standard_normal((120, 90))
    out = R.sketch(W0 + D, W0, 16)
    Dx = (W0 + D) - W0
    assert np.linalg.norm(Dx - out["Q"] @ out["C"]) <= 1e-12 * np.linalg.norm(Dx) or out["kept"] > 8
    D = rng.standard_normal((6, 40))                           # k > min(out, in)
    out = R.sketch(D, None, 16)
    assert out["kept"] == 6 and np.linalg.norm(D - out["Q"] @ out["C"]) <= 1e-12 * np.linalg.norm(D)
    assert abs(out["normsq"] - (D * D).sum()) <= 1e-12 * out["normsq"]
    out = R.sketch(np.zeros((12, 9)), None, 4)
    assert out["kept"] == 0 and not out["Q"].any() and not out["C"].any() and out["normsq"] == 0.0 and out["converged"] and not out["skipped"]
    D[2, 3] = np.nan
    out = R.sketch(D, None, 4)
    assert out["skipped"] and not out["Q"].any() and not out["C"].any() and out["kept"] == 0 and not out["converged"]


def _tolerances():
    worst, per = {k: 0.0 for k in KEYS}, {}
    for c in R.make_cases():
        D = R.difference(c["W1"], c["W0"])
        r64, r32 = R.sketch(c["W1"], c["W0"], c["k"]), R.sketch(c["W1"], c["W0"], c["k"], fp32=True)
        m64, m32 = R.metrics(D, r64["Q"], r64["C"], c["rank"], r64["kept"]), R.metrics(D, r32["Q"], r32["C"], c["rank"], r32["kept"])
        m64["normsq"] = r64["normsq"]
        d = R.deviations(m64, m32, r32["normsq"])
        if not R.well_determined(D, c["k"]):
            d["product"] = 0.0
        per[c["label"]] = d
        for k in KEYS:
            worst[k] = max(worst[k], d[k])
    return {k: max(8.0 * worst[k], 1e-6) for k in KEYS}, per


def test_tolerances_of_the_gpu_tests():
    tol, per = _tolerances()
    if os.environ.get("QFX_WRITE_LORA_EXTRACT_ACCURACY") == "1":
        doc = {}
        if os.path.exists(PROFILE):
            with open(PROFILE) as f:
                doc = json.load(f)
        doc.update({"rule": "tolerance = max(8 x the largest deviation of tests/lora_extract_ref.py fp32=True from its fp64 mode over "
                            "make_cases(), 1e-6); (a) residual, (b) leading singular values of C / sigma_0, (c) max |Q^T Q - I|, "
                            "(d) normsq relative, (e) Q C elementwise / ||D||_F on the well-determined cases",
                    "tolerance": tol, "restatement_fp32_deviation": per})
        with open(PROFILE, "w") as f:
            json.dump(doc, f, indent=1)
    with open(PROFILE) as f:
        committed = json.load(f)["tolerance"]
    print("now", tol, "committed", committed)
    for k in KEYS:
        assert 1e-6 <= committed[k] <= 1e-4, (k, committed[k])              # above 1e-4 a case is ill-posed: replace the case
        assert tol[k] <= 2.0 * committed[k] and committed[k] <= 2.0 * tol[k], (k, tol[k], committed[k])


# ------------------------------------------------------------------ the library's host side

def _mats(rows):
    from qflux_amd import _lib as L
    return (L.LowrankMat * len(rows))(*[L.LowrankMat(*r) for r in rows])


def _row(**kw):
    d = dict(w1=0x10000, w0=0x90000, ld1=16, ld0=16, off_a=0, off_b=64, k=4, nin=16, nout=8, dtype=0, index=0)
    d.update(kw)
    return (d["w1"], d["w0"], d["ld1"], d["ld0"], d["off_a"], d["off_b"], d["k"], d["nin"], d["nout"], d["dtype"], d["index"])


def test_check_table_and_workspace():
    from qflux_amd import _lib as L
    chk, wsb = L.lib.qfx_lowrank_check_table, L.lib.qfx_lowrank_sketch_workspace
    good = [_row(), _row(off_a=100, off_b=200, k=64, nin=1, nout=1, w0=None, ld0=0, dtype=1)]
    assert chk(_mats(good), 2, 264) == 0 and chk(_mats(good), 2, 263) == EINVAL
    assert chk(None, 0, 0) == 0 and chk(None, 1, 10) == EINVAL and chk(_mats(good), -1, 264) == EINVAL and chk(_mats(good), 2, -1) == EINVAL
    for bad in (dict(k=0), dict(k=65), dict(nin=0), dict(nin=(1 << 24) + 1, ld1=1 << 25, ld0=1 << 25), dict(nout=0), dict(nout=(1 << 24) + 1),
                dict(ld1=15), dict(ld0=15), dict(dtype=2), dict(dtype=-1), dict(w1=None), dict(off_a=-1), dict(off_b=-64), dict(off_b=63)):
        assert chk(_mats([_row(**bad)]), 1, 1 << 40) == EINVAL, bad
    assert chk(_mats([_row(w0=None, ld0=0)]), 1, 96) == 0                                              # W0 == NULL: its ld is not read
    assert chk(_mats([_row(), _row(off_a=95, off_b=200)]), 2, 1 << 20) == EINVAL                      # outputs of two matrices overlap
    assert wsb(None, 0) == 0 and wsb(None, 1) == EINVAL and wsb(_mats([_row(k=65)]), 1) == EINVAL
    small, big = wsb(_mats([_row()]), 1), wsb(_mats([_row(nin=3072, nout=3072, ld1=3072, ld0=3072, k=64)]), 1)
    assert 64 * 64 * 8 < small < big and big >= 2 * 3072 * 64 * 4 + 48 * 64 * 64 * 8 and small % 256 == 0


def test_sketch_refusals_without_a_gpu():
    from qflux_amd import _lib as L
    sk = L.lib.qfx_lowrank_sketch
    host = _mats([_row()])

    def args(**kw):
        d = dict(table=0x2000, host_table=C.cast(host, C.c_void_p), n_mats=1, q=2, seed_lo=0, seed_hi=0, orth_tol=1e-12, max_sweeps=30,
                 reserved=0, p=0x40000, n_elems=96, normsq=0x3000, info=0x4000, skipped=0x5000, ws=0x100000, ws_bytes=1 << 30)
        d.update(kw)
        return L.LowrankArgs(**d)

    assert sk(None, None) == EINVAL
    for kw in (dict(n_mats=-1), dict(n_mats=65536), dict(q=-1), dict(q=5), dict(max_sweeps=0), dict(max_sweeps=65), dict(orth_tol=-1e-3),
               dict(orth_tol=1.0), dict(orth_tol=float("nan")), dict(table=None), dict(host_table=None), dict(p=None), dict(normsq=None),
               dict(info=None), dict(skipped=None), dict(ws=None), dict(ws=0x100008), dict(ws_bytes=1024), dict(n_elems=95),
               dict(host_table=C.cast(_mats([_row(k=65)]), C.c_void_p)), dict(host_table=C.cast(_mats([_row(ld1=15)]), C.c_void_p)),
               dict(host_table=C.cast(_mats([_row(off_b=10)]), C.c_void_p))):
        assert sk(C.byref(args(**kw)), None) == EINVAL, kw
    assert sk(C.byref(args(n_mats=0, table=None, host_table=None, p=None, normsq=None, info=None, skipped=None, ws=None)), None) == 0


def test_header_build_entry_and_abi():
    import __graft_entry__ as g
    from qflux_amd import _lib as L
    from qflux_amd import ops
    hdr = open(os.path.join(ROOT, "include", "qfx.h")).read()
    for name in ("qfx_lowrank_check_table", "qfx_lowrank_sketch_workspace", "qfx_lowrank_sketch"):
        assert name in L.SYMBOLS and f" {name}(" in hdr
    assert L.ABI_VERSION == 7 and L.lib.qfx_abi_version() == 7 and "#define QFX_ABI_VERSION 7" in hdr
    assert hdr.rindex("qfx_lora_project(") < hdr.index("qfx_lowrank_mat")
    assert "THIS LISTING IS THE SPECIFICATION (tests/lora_extract_ref.py" in hdr and f"0x{R.OMEGA_TAG:08X}" in hdr
    assert C.sizeof(L.LowrankMat) == 80 and C.sizeof(L.LowrankArgs) == 104
    assert "qfx_lora_extract.hip" in g.PLAIN_SOURCES and "qfx_lora_extract.hip" not in g.SOURCES
    assert g.EXTRA_FLAGS["qfx_lora_extract.hip"] == ["-ffp-contract=off"]
    assert ops.LOWRANK_MAX_K == R.MAX_K == 64 and ops.LOWRANK_ORTH_TOL == R.ORTH_TOL


# ------------------------------------------------------------------ plumbing, the device part replaced by the restatement

@pytest.fixture()
def standins(monkeypatch):
    from qflux_amd import extract
    calls = []

    def sketch(mats, k, power_iters, seed):
        calls.append([m[0] for m in mats])
        return R.sketch_standin(mats, k, power_iters, seed)

    monkeypatch.setattr(extract, "_sketch", sketch)
    monkeypatch.setattr(extract, "_resize", R.resize_standin)
    return calls


def _checkpoints(seed=9):
    rng = np.random.default_rng(seed)
    base, tuned = {}, {}
    for name, (nout, nin) in {"blocks.0.attn.to_q": (24, 16), "blocks.0.attn.to_out.0": (16, 24), "blocks.0.mlp.fc1": (40, 16),
                              "blocks.1.attn.to_q": (24, 16)}.items():
        W = torch.from_numpy(rng.standard_normal((nout, nin)).astype(np.float32))
        D = torch.from_numpy(R.with_spectrum(rng, nout, nin, [1.0, 0.5, 0.25]).astype(np.float32))
        base[name + ".weight"], tuned[name + ".weight"] = W, W + (0.0 if name == "blocks.1.attn.to_q" else 1.0) * D
        base[name + ".bias"] = tuned[name + ".bias"] = torch.zeros(nout)
    base["norm.weight"] = tuned["norm.weight"] = torch.ones(16)                       # 1-D: not a linear
    base["only_in_base.weight"] = torch.zeros(4, 4)
    tuned["blocks.0.attn.to_q.lora_A.default.weight"] = base["blocks.0.attn.to_q.lora_A.default.weight"] = torch.zeros(2, 16)
    return base, tuned


def test_pairing_target_modules_and_groups():
    from qflux_amd.extract import byte_groups, pair_weights
    base, tuned = _checkpoints()
    bk, tk = {k: tuple(v.shape) for k, v in base.items()}, {k: tuple(v.shape) for k, v in tuned.items()}
    every = pair_weights(bk, tk)
    assert every == ["blocks.0.attn.to_q", "blocks.0.attn.to_out.0", "blocks.0.mlp.fc1", "blocks.1.attn.to_q"]
    assert pair_weights(bk, tk, r"attn\.to_q$") == ["blocks.0.attn.to_q", "blocks.1.attn.to_q"]
    assert pair_weights(bk, tk, ["fc1", "to_out.0"]) == ["blocks.0.attn.to_out.0", "blocks.0.mlp.fc1"]
    assert pair_weights(bk, dict(tk, **{"blocks.0.mlp.fc1.weight": (40, 17)})) == [n for n in every if "fc1" not in n]
    assert byte_groups([4, 4, 4, 9, 1, 1], 8) == [[0, 1], [2], [3], [4, 5]] and byte_groups([], 8) == [] and byte_groups([3], 1) == [[0]]


def test_extract_lora_round_trip_min_diff_and_budget(standins, tmp_path):
    from qflux_amd.extract import extract_lora, extract_pairs
    from qflux_amd.lora_io import _normalise
    from safetensors import safe_open
    from safetensors.torch import load_file, save_file
    base, tuned = _checkpoints()
    save_file({k: v.contiguous() for k, v in tuned.items()}, str(tmp_path / "tuned.safetensors"))
    dst = tmp_path / "out"
    one = 2 * 24 * 16 * 4
    tensors, alphas, report = extract_lora(base, str(tmp_path / "tuned.safetensors"), save_to=str(dst), rank=3, oversample=3, min_diff=1e-6,
                                           device="cpu", group_bytes=2 * one)
    assert standins == [["blocks.0.attn.to_q", "blocks.0.attn.to_out.0"], ["blocks.0.mlp.fc1"], ["blocks.1.attn.to_q"]]
    assert report["blocks.1.attn.to_q"]["unchanged"] and report["blocks.1.attn.to_q"]["diff_norm"] == 0.0
    assert sorted(tensors) == sorted(alphas) == ["blocks.0.attn.to_out.0", "blocks.0.attn.to_q", "blocks.0.mlp.fc1"]
    mods = _normalise(load_file(str(dst / "pytorch_lora_weights.safetensors")))
    with safe_open(str(dst / "pytorch_lora_weights.safetensors"), framework="pt") as f:
        written = ast.literal_eval(f.metadata()["lora_alpha"])
        assert any(k.endswith("to_q.lora.down.weight") for k in f.keys()) and any(k.endswith("fc1.lora_A.weight") for k in f.keys())
    assert sorted(mods) == sorted(tensors) and {n: float(a) for n, a in written.items()} == alphas
    for n, ab in mods.items():
        D = (tuned[n + ".weight"] - base[n + ".weight"]).double()
        assert ab["A"].shape == (3, D.shape[1]) and ab["B"].shape == (D.shape[0], 3) and alphas[n] == 3.0
        err = float(torch.linalg.norm(ab["B"].double() @ ab["A"].double() - D) / torch.linalg.norm(D))
        assert err <= 1e-5, (n, err)                                                # exact rank 3
        assert not report[n]["unchanged"] and abs(report[n]["fro_retained_of_diff"] - 1.0) <= 1e-5
        assert abs(report[n]["diff_norm"] - float(torch.linalg.norm(D))) <= 1e-5 * report[n]["diff_norm"]
    t2, _, r2 = extract_lora(base, tuned, rank=2, oversample=4, target_modules=r"fc1", device="cpu")
    assert list(t2) == ["blocks.0.mlp.fc1"] and t2["blocks.0.mlp.fc1"][0].shape[0] == 2
    want = (1.0 + 0.25) ** 0.5 / (1.0 + 0.25 + 0.0625) ** 0.5
    assert abs(r2["blocks.0.mlp.fc1"]["fro_retained_of_diff"] - want) <= 1e-4
    for bad in (dict(rank=65), dict(rank=0), dict(rank=2, oversample=-1), dict(rank=2, power_iters=5), dict(rank=2, dynamic_method="sv_nope")):
        with pytest.raises((ValueError, NotImplementedError)):
            extract_pairs([("m", torch.zeros(4, 4), None)], **bad)
    with pytest.raises(ValueError):
        extract_pairs([], 2)
    with pytest.raises(ValueError):
        extract_lora(base, tuned, rank=2, target_modules=r"nothing_matches", device="cpu")


def test_ops_refusals():
    from qflux_amd import ops
    W = torch.zeros(8, 16)
    with pytest.raises(NotImplementedError, match="k = 65"):
        ops.lowrank_table([(W, None, 65, 0, 2048)])
    for bad in ([], [(W.double(), None, 4, 0, 64)], [(W, torch.zeros(8, 15), 4, 0, 64)], [(W.t(), None, 4, 0, 64)], [(W, None, 4, 0, 10)],
                [(W, W.bfloat16(), 4, 0, 64)]):
        with pytest.raises(ValueError):
            ops.lowrank_table(bad)
    lay = ops.lowrank_table([(W, None, 4, 0, 64), (W[:, :9], W[:, 1:10], 3, 96, 128)])
    assert lay.rows == [(0, 64, 4, 16, 8), (96, 128, 3, 9, 8)] and lay.extent == 152 and lay.ws_bytes > 0
    assert lay.host[1].ld1 == 16 and lay.host[1].index == 1 and lay.host[0].w0 is None
