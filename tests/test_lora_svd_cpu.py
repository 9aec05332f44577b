"""CPU: the numpy restatement of the qfx_lora_spectrum / qfx_lora_project listing (tests/lora_svd_ref.py) against LAPACK, select_rank
on hand-made spectra, the host-side refusals of the library and of the Python layer, the header.

    QFX_WRITE_LORA_SVD_ACCURACY=1 python -m pytest tests/test_lora_svd_cpu.py -k lapack

rewrites profiles/lora_svd_accuracy.json with the restatement's measured error: the number the GPU tolerance hangs on."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lora_svd_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "lora_svd_accuracy.json")
EINVAL = -1


def _measure():
    per, worst = {}, 0.0
    for lab, A, B in R.make_cases():
        out, ref = R.spectrum(A, B, transforms=False), R.lapack_sv(A, B)
        per[lab] = R.sq_error(out["sv"], ref)
        worst = max(worst, per[lab])
    return worst, per


def test_restatement_against_lapack():
    worst, per = _measure()
    if os.environ.get("QFX_WRITE_LORA_SVD_ACCURACY") == "1":
        with open(PROFILE, "w") as f:
            json.dump({"metric": "max_i |sv_i^2 - ref_i^2| / ref_0^2, tests/lora_svd_ref.py against torch.linalg.svdvals of the fp64 product",
                       "worst_sq_error": worst, "per_case": per}, f, indent=1)
    with open(PROFILE) as f:
        committed = json.load(f)["worst_sq_error"]
    print("worst", worst, "committed", committed, per)
    assert 0.0 < committed < 1e-12 and worst <= 2.0 * committed      # BLAS builds sum the fp64 Gram matrices in their own order


def test_restatement_ranks_transforms_and_projection():
    for lab, A, B in R.make_cases(full=False):
        out, ref = R.spectrum(A, B), R.lapack_sv(A, B)
        assert R.unambiguous(ref) and out["converged"], lab
        rho = int((ref > R.RANK_TOL * ref[0]).sum()) if ref[0] > 0 else 0
        assert out["rho"] == rho, (lab, out["rho"], rho)
        k = max(rho, 1)
        A2, B2 = R.project(A, B, out["T_B"], out["T_A"], k, k + 1)
        P = B.astype(np.float64) @ A.astype(np.float64)
        err = np.linalg.norm(B2.astype(np.float64) @ A2.astype(np.float64) - P)
        assert err <= 4 * np.sqrt(k) * 2.0 ** -24 * np.linalg.norm(P), lab
        assert not A2[k:].any() and not B2[:, k:].any()
        if rho:
            G = A2[:k].astype(np.float64) @ A2[:k].astype(np.float64).T
            assert np.abs(G - np.eye(k)).max() <= 8 * A.shape[0] * 2.0 ** -24, lab
    # a sweep cap that is too low: what it has is reported, unconverged; a NaN is skipped
    _, A, B = R.make_cases(full=False)[3]
    assert not R.spectrum(A, B, max_sweeps=1)["converged"]
    A = A.copy()
    A[0, 0] = np.nan
    out = R.spectrum(A, B)
    assert out["skipped"] and out["rho"] == 0 and not out["sv"].any() and not out["converged"]


def test_round_robin_visits_every_pair_once():
    for n in (1, 2, 3, 7, 16, 63, 64):
        m = (n + 1) & ~1
        seen = [pq for rd in range(m - 1) for pq in R.round_pairs(n, rd)]
        assert sorted(seen) == [(p, q) for p in range(n) for q in range(p + 1, n)]
        for rd in range(m - 1):
            flat = [i for pq in R.round_pairs(n, rd) for i in pq]
            assert len(flat) == len(set(flat))


def test_select_rank():
    from qflux_amd.resize import select_rank
    sv = [8.0, 4.0, 2.0, 1.0, 1.0]          # sum 16, squares 64 16 4 1 1 = 86
    cases = [((sv, 3), 3), ((sv, 9), 5),
             ((sv, 5, "sv_ratio", 2.0), 2),                   # equality with the threshold counts: 4 >= 8 / 2
             ((sv, 5, "sv_ratio", 1.0), 1), ((sv, 5, "sv_ratio", 8.0), 5), ((sv, 2, "sv_ratio", 8.0), 2),
             ((sv, 5, "sv_cumulative", 0.75), 2),             # (8 + 4) / 16 == 0.75 exactly
             ((sv, 5, "sv_cumulative", 0.76), 3), ((sv, 5, "sv_cumulative", 1.0), 5),
             ((sv, 5, "sv_fro", (80.0 / 86.0) ** 0.5), 2),    # equality
             ((sv, 5, "sv_fro", 0.99), 4), ((sv, 5, "sv_fro", 1.0), 5),
             (([3.0], 4, "sv_fro", 0.5), 1), (([3.0], 1), 1), (([3.0], 4, "sv_ratio", 1.0), 1), (([3.0], 4, "sv_cumulative", 1.0), 1),
             (([0.0, 0.0, 0.0], 3), 3), (([0.0, 0.0, 0.0], 3, "sv_fro", 0.9), 1), (([0.0, 0.0, 0.0], 3, "sv_cumulative", 1.0), 1)]
    for args, want in cases:
        got, ref = select_rank(*args), R.select_rank(*args)
        assert got == ref and got[0] == want, (args, got, ref, want)
        assert 0.0 <= got[1] <= 1.0 and 0.0 <= got[2] <= 1.0
    assert select_rank([0.0, 0.0, 0.0], 3, numeric_rank=0) == (1, 1.0, 1.0)          # B = 0: rank 1
    assert select_rank(sv, 5, numeric_rank=2)[0] == 2 and select_rank(sv, 5, "sv_fro", 1.0, numeric_rank=3)[0] == 3
    k, fro, cum = select_rank(sv, 2)
    assert k == 2 and fro == (80.0 / 86.0) ** 0.5 and cum == 0.75
    for bad in ((sv, 3, "sv_nope", 0.5), (sv, 3, "sv_ratio", 0.5), (sv, 3, "sv_ratio", None), (sv, 3, "sv_fro", 0.0), (sv, 3, "sv_fro", 1.5),
                (sv, 3, "sv_cumulative", -0.1), (sv, 3, "sv_cumulative", float("nan")), (sv, 0), ([], 3)):
        with pytest.raises(ValueError):
            select_rank(*bad)


def _pairs(rows):
    from qflux_amd import _lib as L
    return (L.LoraSvdPair * len(rows))(*[L.LoraSvdPair(*r, 0) for r in rows])


def _dsts(rows):
    from qflux_amd import _lib as L
    return (L.LoraSvdDst * len(rows))(*[L.LoraSvdDst(*r) for r in rows])


def test_check_tables():
    from qflux_amd import _lib as L
    chk, pchk = L.lib.qfx_lora_svd_check_table, L.lib.qfx_lora_project_check_table
    good = [(0, 64, 4, 16, 8), (100, 200, 64, 1, 1)]
    assert chk(_pairs(good), 2, 264) == 0 and chk(_pairs(good), 2, 263) == EINVAL
    assert chk(None, 0, 0) == 0 and chk(None, 1, 10) == EINVAL and chk(_pairs(good), -1, 264) == EINVAL and chk(_pairs(good), 2, -1) == EINVAL
    for bad in ((0, 64, 0, 16, 8), (0, 64, 65, 16, 8), (0, 64, 4, 0, 8), (0, 64, 4, (1 << 24) + 1, 8), (0, 64, 4, 16, 0),
                (0, 64, 4, 16, (1 << 24) + 1), (-1, 64, 4, 16, 8), (0, -64, 4, 16, 8), (0, 63, 4, 16, 8)):
        assert chk(_pairs([bad]), 1, 1 << 40) == EINVAL, bad
    assert chk(_pairs([(0, 64, 4, 16, 8), (95, 200, 4, 16, 8)]), 2, 1 << 20) == EINVAL          # two pairs overlap
    assert chk(_pairs([(0, 0, 64, 1 << 24, 1 << 24)]), 1, 1 << 31) == EINVAL and chk(_pairs([(0, 1 << 30, 64, 1 << 24, 1 << 24)]), 1, 1 << 31) == 0
    src = [(0, 64, 4, 16, 8)]
    assert pchk(_pairs(src), _dsts([(0, 64, 2, 3)]), 1, 88) == 0 and pchk(_pairs(src), _dsts([(0, 64, 2, 3)]), 1, 87) == EINVAL
    assert pchk(None, None, 0, 0) == 0 and pchk(_pairs(src), None, 1, 88) == EINVAL and pchk(None, _dsts([(0, 64, 2, 3)]), 1, 88) == EINVAL
    for bad in ((0, 64, 0, 3), (0, 64, 5, 5), (0, 64, 2, 1), (0, 64, 2, 65), (-1, 64, 2, 3), (0, -1, 2, 3), (0, 47, 2, 3)):
        assert pchk(_pairs(src), _dsts([bad]), 1, 1 << 20) == EINVAL, bad
    assert pchk(_pairs(src), _dsts([(0, 1024, 4, 64)]), 1, 1 << 20) == 0
    assert pchk(_pairs([(0, 64, 65, 16, 8)]), _dsts([(0, 64, 2, 3)]), 1, 1 << 20) == EINVAL
    assert pchk(_pairs(src * 2), _dsts([(0, 64, 2, 3), (80, 200, 2, 3)]), 2, 1 << 20) == EINVAL     # destinations overlap


def test_launch_refusals_without_a_gpu():
    from qflux_amd import _lib as L
    spec, proj = L.lib.qfx_lora_spectrum, L.lib.qfx_lora_project

    def sargs(**kw):
        d = dict(p=0x1000, table=0x2000, n_pairs=1, max_sweeps=30, rank_tol=1e-6, sv=0x3000, ld_sv=64, info=0x4000, ws=None, skipped=0x5000)
        d.update(kw)
        return L.LoraSpectrumArgs(**d)

    assert spec(None, None) == EINVAL
    for kw in (dict(n_pairs=-1), dict(rank_tol=0.0), dict(rank_tol=1.0), dict(rank_tol=-1e-6), dict(rank_tol=float("nan")),
               dict(max_sweeps=0), dict(max_sweeps=65), dict(ld_sv=63), dict(p=None), dict(table=None), dict(sv=None), dict(info=None),
               dict(skipped=None)):
        assert spec(C.byref(sargs(**kw)), None) == EINVAL, kw
    assert spec(C.byref(sargs(n_pairs=0, p=None, table=None, sv=None, info=None, skipped=None)), None) == 0
    assert spec(C.byref(sargs(n_pairs=0, max_sweeps=64, rank_tol=0.5)), None) == 0

    def pargs(**kw):
        d = dict(p=0x1000, q=0x9000, table=0x2000, dst=0x3000, n_pairs=1, reserved=0, ws=0x4000)
        d.update(kw)
        return L.LoraProjectArgs(**d)

    assert proj(None, None) == EINVAL
    for kw in (dict(n_pairs=-1), dict(q=0x1000), dict(p=None), dict(q=None), dict(table=None), dict(dst=None), dict(ws=None),
               dict(n_pairs=0, q=0x1000)):
        assert proj(C.byref(pargs(**kw)), None) == EINVAL, kw
    assert proj(C.byref(pargs(n_pairs=0, p=None, q=None, table=None, dst=None, ws=None)), None) == 0


def test_header_build_entry_and_abi():
    import __graft_entry__ as g
    from qflux_amd import _lib as L
    from qflux_amd import ops
    hdr = open(os.path.join(ROOT, "include", "qfx.h")).read()
    for name in ("qfx_lora_svd_check_table", "qfx_lora_project_check_table", "qfx_lora_spectrum", "qfx_lora_project"):
        assert name in L.SYMBOLS and f"int {name}(" in hdr
    assert L.ABI_VERSION == 7 and L.lib.qfx_abi_version() == 7 and "#define QFX_ABI_VERSION 7" in hdr      # appended: the version stays
    assert hdr.rindex("qfx_scaled_adamw_step(") < hdr.index("qfx_lora_svd_pair")                           # ... behind the last feature
    assert "THIS LISTING IS THE SPECIFICATION (tests/lora_svd_ref.py" in hdr
    assert C.sizeof(L.LoraSvdPair) == 32 and C.sizeof(L.LoraSvdDst) == 24
    assert "qfx_lora_svd.hip" in g.PLAIN_SOURCES and g.EXTRA_FLAGS["qfx_lora_svd.hip"] == ["-ffp-contract=off"]
    assert ops.LORA_SVD_MAX_RANK == 64 == R.MAX_RANK and ops.LORA_SVD_RANK_TOL == R.RANK_TOL and ops.LORA_SVD_MAX_SWEEPS == R.MAX_SWEEPS


def test_python_refusals():
    from qflux_amd import ops
    from qflux_amd.resize import resize_pairs
    from qflux_amd.spectrum import SpectrumState, summarize
    p = torch.zeros(65 * 70)
    with pytest.raises(NotImplementedError, match="blocks.3.attn.to_q"):
        SpectrumState.for_pairs(p, [("blocks.3.attn.to_q", 0, 65 * 64, 65, 64, 4, 1.0)])
    with pytest.raises(NotImplementedError, match="rank 65"):
        ops.lora_svd_table([(0, 65 * 64, 65, 64, 4)])
    with pytest.raises(ValueError):
        ops.lora_svd_table([(0, 10, 4, 16, 8)])                  # overlap
    with pytest.raises(ValueError):
        ops.lora_svd_table([])
    lay = ops.lora_svd_table([(0, 64, 4, 16, 8)])
    with pytest.raises(ValueError):
        ops.lora_project_table(lay, [(0, 64, 5, 5)])             # k > r
    with pytest.raises(ValueError):
        ops.lora_project_table(lay, [])
    pairs = [("m", 0, 64, 4, 16, 8, 1.0)]
    for bad in (dict(dynamic_method="sv_nope", dynamic_param=0.5), dict(dynamic_method="sv_fro", dynamic_param=2.0),
                dict(dynamic_method="sv_ratio", dynamic_param=0.5), dict(dynamic_method="sv_cumulative")):
        with pytest.raises(ValueError):
            resize_pairs(p, pairs, 2, **bad)                     # refused before anything is launched
    with pytest.raises(ValueError):
        resize_pairs(p, pairs, 65)
    s = summarize([3.0, 4.0])
    assert s["fro"] == 5.0 and s["spectral"] == 3.0 and abs(s["stable_rank"] - 25.0 / 9.0) < 1e-15
    assert abs(summarize([2.0, 2.0, 2.0, 2.0])["effective_rank"] - 4.0) < 1e-12 and summarize([0.0, 0.0])["effective_rank"] == 0.0
