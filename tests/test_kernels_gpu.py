"""GPU parity tests, one per C-ABI entry point: HIP kernel vs a plain fp32 torch restatement of the same op
(with the reference's bf16 rounding points) on the same seeded inputs.  All calls go through the C ABI."""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda:0"
_STATS = {}


def _ops():
    from qflux_amd import ops
    return ops


def rel_err(got, ref):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = (got - ref).abs()
    denom = ref.abs().max().item() + 1e-12
    return d.max().item() / denom, d


def check(name, got, ref, tol):
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite output"
    e, d = rel_err(got, ref)
    bad = (d > tol * (ref.abs().max().item() + 1e-12)).float().mean().item()
    _STATS[name] = dict(rel=e, tol=tol, bad_frac=bad)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "kernel_parity.json"), "w") as f:
        json.dump(_STATS, f, indent=1)
    if e > tol:
        idx = torch.nonzero(d == d.max())[0].tolist()
        raise AssertionError(f"{name}: rel err {e:.3e} > {tol:.1e}; worst at {idx}; bad fraction {bad:.3f}")


def rb(x):  # round through bf16
    return x.to(BF).float()


def randn(*s, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*s, generator=g) * scale


# ------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 256, 128), (384, 768, 256), (130, 64, 64), (2432, 1024, 3072)])
def test_gemm_plain(M, N, K):
    ops = _ops()
    a = randn(M, K, seed=1).to(BF)
    b = randn(N, K, seed=2).to(BF)
    bias = randn(N, seed=3).to(BF)
    ref = rb(a.float() @ b.float().t() + bias.float())
    out = ops.gemm(a.to(DEV), b.to(DEV), bias=bias.to(DEV))
    check(f"gemm_plain_{M}x{N}x{K}", out, ref, 1e-2)


@pytest.mark.parametrize("M,N,K", [(2432, 3072, 3072), (2048, 3072, 128), (2000, 3080, 192), (4096, 2048, 64)])
def test_gemm_large_tile_kernel(M, N, K):
    """shapes that select the 256x128 / 3-stage kernel (>= 160 tiles); odd M/N edges, K = 1..3 stages."""
    ops = _ops()
    a = randn(M, K, seed=1).to(BF)
    b = randn(N, K, seed=2, scale=0.1).to(BF)
    bias = randn(N, seed=3).to(BF)
    ref = rb(a.float() @ b.float().t() + bias.float())
    out = ops.gemm(a.to(DEV), b.to(DEV), bias=bias.to(DEV))
    check(f"gemm256_{M}x{N}x{K}", out, ref, 1e-2)


def test_gemm_grouped_six_problems():
    ops = _ops()
    K, N = 256, 384
    Ms = [300, 300, 300, 70, 70, 70]
    items, refs = [], []
    for i, M in enumerate(Ms):
        a = randn(M, K, seed=10 + i).to(BF)
        b = randn(N, K, seed=20 + i, scale=0.1).to(BF)
        bias = randn(N, seed=30 + i).to(BF)
        out = torch.zeros(M, N, dtype=BF, device=DEV)
        items.append((a.to(DEV), b.to(DEV), out, dict(bias=bias.to(DEV))))
        refs.append(rb(a.float() @ b.float().t() + bias.float()))
    ops.gemm_grouped(items)
    for i, (it, ref) in enumerate(zip(items, refs)):
        check(f"gemm_grouped_{i}", it[2], ref, 1e-2)


def test_gemm_transpose_detect():
    """A = I-like asymmetric check: catches swapped row/col in the MFMA C layout."""
    ops = _ops()
    M = N = K = 128
    a = torch.eye(M, K).to(BF)
    b = (torch.arange(N * K).reshape(N, K) % 61).float().to(BF)
    out = ops.gemm(a.to(DEV), b.to(DEV))
    check("gemm_identity", out, b.float().t()[:M, :N], 1e-3)


def test_gemm_lora_segment_and_gelu():
    ops = _ops()
    M, N, K, K2 = 200, 256, 128, 64
    a, b = randn(M, K, seed=1).to(BF), randn(N, K, seed=2, scale=0.2).to(BF)
    a2, b2 = randn(M, K2, seed=3).to(BF), randn(N, K2, seed=4, scale=0.1).to(BF)
    bias = randn(N, seed=5).to(BF)
    base = rb(a.float() @ b.float().t() + bias.float())
    h = rb(base + a2.float() @ b2.float().t())
    g = rb(F.gelu(h, approximate="tanh"))
    out2 = torch.empty(M, N, dtype=BF, device=DEV)
    out = ops.gemm(a.to(DEV), b.to(DEV), bias=bias.to(DEV), a2=a2.to(DEV), b2=b2.to(DEV), epi=1, out2=out2)
    check("gemm_seg2_pre", out, h, 1e-2)
    check("gemm_seg2_gelu", out2, g, 1e-2)


def test_gemm_gate_res_and_remap():
    ops = _ops()
    Bn, rpb, T, N, K = 2, 100, 28, 128, 64
    S = T + rpb
    M = Bn * rpb
    a_joint = randn(Bn * S, K, seed=1).to(BF)     # A rows live in a joint [B, S] buffer at offset T
    b = randn(N, K, seed=2, scale=0.3).to(BF)
    gate = randn(Bn, N, seed=3).to(BF)
    res = randn(M, N, seed=4).to(BF)
    a = a_joint.view(Bn, S, K)[:, T:].reshape(M, K)
    y = rb(a.float() @ b.float().t())
    ref = rb(res.float() + rb(gate.float().repeat_interleave(rpb, 0) * y))
    out = ops.gemm(a_joint.to(DEV), b.to(DEV), epi=2, aux=res.to(DEV), gate=gate.to(DEV), rows_per_batch=rpb,
                   a_map=(S, T), M=M)
    check("gemm_gate_res_amap", out, ref, 1e-2)
    # C remap: write into a joint buffer
    cj = torch.zeros(Bn * S, N, dtype=BF, device=DEV)
    ops.gemm(a.contiguous().to(DEV), b.to(DEV), out=cj, rows_per_batch=rpb, c_map=(S, T))
    got = cj.view(Bn, S, N)[:, T:].reshape(M, N)
    check("gemm_cmap", got, y, 1e-2)
    assert cj.view(Bn, S, N)[:, :T].abs().max().item() == 0.0


def test_gemm_dgelu():
    ops = _ops()
    M, N, K = 192, 256, 128
    a, b = randn(M, K, seed=1).to(BF), randn(N, K, seed=2, scale=0.2).to(BF)
    h = randn(M, N, seed=3).to(BF)
    hh = h.float().requires_grad_(True)
    F.gelu(hh, approximate="tanh").sum().backward()
    ref = rb(rb(a.float() @ b.float().t()) * hh.grad)
    out = ops.gemm(a.to(DEV), b.to(DEV), epi=3, aux=h.to(DEV))
    check("gemm_dgelu", out, ref, 1.5e-2)


def test_gemm_wide_tile_all_epilogues():
    """Shapes whose tile count selects the 256x256 tile (N % 256 == 0 and fewer weighted rounds): every epilogue, the LoRA
    K segment with bf16 mid-rounding, a row remap, ragged M, a grouped launch and a row mask."""
    ops = _ops()
    M, N, K, K2 = 2000, 6144, 192, 64
    a, b = randn(M, K, seed=1).to(BF), randn(N, K, seed=2, scale=0.2).to(BF)
    a2, b2 = randn(M, K2, seed=3).to(BF), randn(N, K2, seed=4, scale=0.1).to(BF)
    bias = randn(N, seed=5).to(BF)
    base = rb(a.float() @ b.float().t() + bias.float())
    h = rb(base + a2.float() @ b2.float().t())
    g = rb(F.gelu(h, approximate="tanh"))
    out2 = torch.empty(M, N, dtype=BF, device=DEV)
    out = ops.gemm(a.to(DEV), b.to(DEV), bias=bias.to(DEV), a2=a2.to(DEV), b2=b2.to(DEV), epi=1, out2=out2)
    check("gemm_wide_seg2_pre", out, h, 1e-2)
    check("gemm_wide_seg2_gelu", out2, g, 1e-2)
    # plain + bias
    check("gemm_wide_plain", ops.gemm(a.to(DEV), b.to(DEV), bias=bias.to(DEV)), base, 1e-2)
    # dgelu
    hx = randn(M, N, seed=6).to(BF)
    hh = hx.float().requires_grad_(True)
    F.gelu(hh, approximate="tanh").sum().backward()
    ref = rb(rb(a.float() @ b.float().t()) * hh.grad)
    check("gemm_wide_dgelu", ops.gemm(a.to(DEV), b.to(DEV), epi=3, aux=hx.to(DEV)), ref, 1.5e-2)
    # gate + residual with a C remap into a joint buffer and a row mask
    Bn, rpb, T = 2, 1000, 24
    S = T + rpb
    gate = randn(Bn, N, seed=7).to(BF)
    res = randn(M, N, seed=8).to(BF)
    y = rb(a.float() @ b.float().t())
    refg = rb(res.float() + rb(gate.float().repeat_interleave(rpb, 0) * y))
    mask = torch.ones(M)
    mask[777:1000] = 0
    refg[mask == 0] = 0
    cj = torch.zeros(Bn * S, N, dtype=BF, device=DEV)
    resj = torch.zeros(Bn, S, N, dtype=BF)            # the residual lives in the same joint layout as C (aux is indexed like C)
    resj[:, T:] = res.view(Bn, rpb, N)
    ops.gemm(a.to(DEV), b.to(DEV), out=cj, epi=2, aux=resj.view(Bn * S, N).to(DEV), gate=gate.to(DEV), rows_per_batch=rpb, c_map=(S, T),
             row_mask=mask.to(DEV))
    check("gemm_wide_gate_res_cmap_mask", cj.view(Bn, S, N)[:, T:].reshape(M, N), refg, 1e-2)
    assert cj.view(Bn, S, N)[:, :T].abs().max().item() == 0.0
    # grouped: image-like + text-like problem in one launch
    items, refs = [], []
    for i, Mi in enumerate((2048, 384)):
        ai = randn(Mi, K, seed=40 + i).to(BF)
        bi = randn(N, K, seed=50 + i, scale=0.1).to(BF)
        bs = randn(N, seed=60 + i).to(BF)
        o = torch.zeros(Mi, N, dtype=BF, device=DEV)
        items.append((ai.to(DEV), bi.to(DEV), o, dict(bias=bs.to(DEV))))
        refs.append(rb(ai.float() @ bi.float().t() + bs.float()))
    ops.gemm_grouped(items)
    for i, (it, rf) in enumerate(zip(items, refs)):
        check(f"gemm_wide_grouped_{i}", it[2], rf, 1e-2)


def test_gemm_same_xcd_split_k_lever():
    """Round 5 lever (default off, profiles/r05_gemm_splitk.json): 256x256 tiles as two work items per tile on CUs of one XCD, fp32 partial
    tiles handed over through the L2.  Forced on for the step's deep-K launch shape (image + text group, 240 work items): the LoRA
    K extension with the bf16 mid-rounding after BOTH halves, gate + residual, ragged M; against the fp32 reference, against the
    unsplit launch, and twice for bit-reproducibility.  A shape outside the policy (K < 9216) must not change."""
    import ctypes as C
    from qflux_amd import _lib as L
    ops = _ops()
    lib = L.lib
    N, K, K2 = 3072, 9216, 192
    st = torch.cuda.current_stream().cuda_stream

    def launch(epi):
        gs, keep, outs, refs = [], [], [], []
        for i, Mi in enumerate((2040, 384)):
            ai, bi, bs = randn(Mi, K, seed=140 + i).to(BF), randn(N, K, seed=150 + i, scale=0.05).to(BF), randn(N, seed=160 + i).to(BF)
            ad, bd, sd = ai.to(DEV), bi.to(DEV), bs.to(DEV)
            o = torch.zeros(Mi, N, dtype=BF, device=DEV)
            g = L.GemmArgs()
            g.A1, g.B1, g.lda1, g.ldb1, g.K1 = ad.data_ptr(), bd.data_ptr(), K, K, K
            g.M, g.N, g.bias, g.C, g.ldc, g.rows_per_batch, g.epi = Mi, N, sd.data_ptr(), o.data_ptr(), N, Mi, epi
            base = rb(ai.float() @ bi.float().t() + bs.float())
            if epi == 0:        # + LoRA K extension: the base sum of BOTH K halves is rounded to bf16 before the extension is added
                a2, b2 = randn(Mi, K2, seed=170 + i).to(BF), randn(N, K2, seed=180 + i, scale=0.05).to(BF)
                a2d, b2d = a2.to(DEV), b2.to(DEV)
                g.A2, g.B2, g.lda2, g.ldb2, g.K2 = a2d.data_ptr(), b2d.data_ptr(), K2, K2, K2
                keep += [a2d, b2d]
                refs.append(rb(base + a2.float() @ b2.float().t()))
            else:               # gate * y + residual
                gate, aux = randn(1, N, seed=190).to(BF), randn(Mi, N, seed=191 + i).to(BF)
                gd, xd = gate.to(DEV), aux.to(DEV)
                g.gate, g.gate_bstride, g.aux, g.ldaux = gd.data_ptr(), N, xd.data_ptr(), N
                keep += [gd, xd]
                refs.append(rb(aux.float() + rb(gate.float() * base)))
            keep += [ad, bd, sd]; gs.append(g); outs.append(o)
        arr = (L.GemmArgs * len(gs))(*gs)
        assert lib.qfx_gemm_grouped(arr, len(gs), st) == 0
        torch.cuda.synchronize()
        first = [o.clone() for o in outs]
        assert lib.qfx_gemm_grouped(arr, len(gs), st) == 0
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(first, outs)), "launch not bit-reproducible"
        return first, refs

    try:
        got = {}
        for mode in (b"splitk=0", b"splitk=1"):
            assert lib.qfx_gemm_tune(mode, None) == 0
            got[mode] = []
            for epi in (0, 2):
                outs, refs = launch(epi)
                for k, (o, rf) in enumerate(zip(outs, refs)):
                    check(f"gemm_{mode.decode()}_epi{epi}_{k}", o, rf, 1e-2)
                got[mode] += outs
        for x, y in zip(got[b"splitk=0"], got[b"splitk=1"]):
            assert ((x.float() - y.float()).abs().max() / x.float().abs().max()).item() < 1e-2
        a, b = randn(2432, 3072, seed=7).to(BF).to(DEV), randn(3072, 3072, seed=8, scale=0.05).to(BF).to(DEV)
        assert lib.qfx_gemm_tune(b"splitk=0", None) == 0
        r0 = ops.gemm(a, b)
        assert lib.qfx_gemm_tune(b"splitk=1", None) == 0
        assert torch.equal(r0, ops.gemm(a, b))
    finally:
        assert lib.qfx_gemm_tune(b"splitk=0", None) == 0
    assert lib.qfx_gemm_tune(b"splitk=2", None) == -1 and lib.qfx_gemm_tune(b"splitk_bias=99", None) == -1


GEOMETRIES = ("256x128", "256x256", "160x192")


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_gemm_every_tile_geometry(geo):
    """Round 4: the persistent GEMM picks its tile geometry per launch (qfx_gemm_tune); here each of the three is FORCED in turn on the
    DiT's own row structure -- a grouped launch of a 2048-row (image) and a 384-row (text) problem with different weights, N = 3072,
    LoRA K segment with bf16 mid-rounding, every epilogue incl. gate + residual over a joint-buffer row map, a row mask, ragged M --
    against the fp32 product with the eager graph's rounding points, and bit-identical to the 256x128 result (the K order of an output
    element does not depend on the tile it lies in)."""
    import ctypes as C
    from qflux_amd import _lib as L
    ops = _ops()
    lib = L.lib

    def run_all():
        outs = {}
        N, K, K2 = 3072, 192, 64
        # grouped image + text problems, every epilogue
        for epi in (0, 1, 2, 3):
            gs, keep, refs = [], [], []
            for i, Mi in enumerate((2048, 384)):
                a, b = randn(Mi, K, seed=10 + i).to(BF), randn(N, K, seed=20 + i, scale=0.2).to(BF)
                a2, b2 = randn(Mi, K2, seed=30 + i).to(BF), randn(N, K2, seed=40 + i, scale=0.1).to(BF)
                bias = randn(N, seed=50 + i).to(BF)
                h = rb(rb(a.float() @ b.float().t() + bias.float()) + a2.float() @ b2.float().t())
                g = L.GemmArgs()
                t = [x.to(DEV) for x in (a, b, a2, b2, bias)]
                out = torch.zeros(Mi, N, dtype=BF, device=DEV)
                g.A1, g.B1, g.lda1, g.ldb1, g.K1 = t[0].data_ptr(), t[1].data_ptr(), K, K, K
                g.A2, g.B2, g.lda2, g.ldb2, g.K2 = t[2].data_ptr(), t[3].data_ptr(), K2, K2, K2
                g.M, g.N, g.bias, g.C, g.ldc, g.rows_per_batch, g.epi = Mi, N, t[4].data_ptr(), out.data_ptr(), N, Mi, epi
                extra = None
                if epi == 1:
                    extra = torch.zeros(Mi, N, dtype=BF, device=DEV)
                    g.C2, g.ldc2 = extra.data_ptr(), N
                    ref = (h, rb(F.gelu(h, approximate="tanh")))
                elif epi == 2:
                    gate, res = randn(1, N, seed=60 + i).to(BF), randn(Mi, N, seed=70 + i).to(BF)
                    t += [gate.to(DEV), res.to(DEV)]
                    g.gate, g.gate_bstride, g.aux, g.ldaux = t[-2].data_ptr(), N, t[-1].data_ptr(), N
                    ref = (rb(res.float() + rb(gate.float() * h)),)
                elif epi == 3:
                    hx = randn(Mi, N, seed=80 + i).to(BF)
                    hh = hx.float().requires_grad_(True)
                    F.gelu(hh, approximate="tanh").sum().backward()
                    t.append(hx.to(DEV))
                    g.aux, g.ldaux = t[-1].data_ptr(), N
                    ref = (rb(h * hh.grad),)
                else:
                    ref = (h,)
                gs.append(g); keep.append((t, out, extra)); refs.append(ref)
            arr = (L.GemmArgs * 2)(*gs)
            L.check(lib.qfx_gemm_grouped(arr, 2, ops.stream_ptr()), "qfx_gemm_grouped")
            for i in range(2):
                outs[f"grouped_epi{epi}_{i}"] = (keep[i][1].cpu(), refs[i][0])
                if epi == 1:
                    outs[f"grouped_epi1_gelu_{i}"] = (keep[i][2].cpu(), refs[i][1])
        # gate + residual with two samples, C row map into a joint buffer, row mask, ragged M (1900 = 2 x 950 rows)
        Bn, rpb, T, K = 2, 950, 24, 128
        M, S = Bn * rpb, 24 + 950
        a, b = randn(M, K, seed=1).to(BF), randn(N, K, seed=2, scale=0.2).to(BF)
        gate, res = randn(Bn, N, seed=7).to(BF), randn(M, N, seed=8).to(BF)
        y = rb(a.float() @ b.float().t())
        refg = rb(res.float() + rb(gate.float().repeat_interleave(rpb, 0) * y))
        mask = torch.ones(M)
        mask[777:1000] = 0
        refg[mask == 0] = 0
        cj = torch.zeros(Bn * S, N, dtype=BF, device=DEV)
        resj = torch.zeros(Bn, S, N, dtype=BF)
        resj[:, T:] = res.view(Bn, rpb, N)
        ops.gemm(a.to(DEV), b.to(DEV), out=cj, epi=2, aux=resj.view(Bn * S, N).to(DEV), gate=gate.to(DEV), rows_per_batch=rpb, c_map=(S, T),
                 row_mask=mask.to(DEV))
        outs["gate_res_cmap_mask"] = (cj.view(Bn, S, N)[:, T:].reshape(M, N).cpu(), refg)
        assert cj.view(Bn, S, N)[:, :T].abs().max().item() == 0.0
        return outs

    try:
        assert lib.qfx_gemm_tune(b"256x128", None) == 0
        base = run_all()
        assert lib.qfx_gemm_tune(geo.encode(), None) == 0
        got = run_all()
    finally:
        assert lib.qfx_gemm_tune(b"all", None) == 0
    assert lib.qfx_gemm_tune(b"17x3", None) == -1 and lib.qfx_gemm_tune(None, b"1,2") == -1       # unparsable: refused, policy kept
    for k, (o, ref) in got.items():
        check(f"gemm_geo_{geo}_{k}", o, ref, 1.5e-2)
        assert torch.equal(o, base[k][0]), f"{geo} {k}: differs from the 256x128 tile's result"


@pytest.mark.parametrize("geo", [g for g in GEOMETRIES if g != "256x128"])
def test_gemm_dgelu_landing_buffer(geo):
    """Round 6: on the 256x256 and 160x192 tiles the d(GELU) and gate + residual epilogues take their aux rows (pre-activation / residual)
    through a per-wave LDS landing buffer (requested one pass ahead by LDS-DMA, completion by counted waits) where every lane slot of the
    wave stores: no bias left for the epilogue, no row mask, M a multiple of 16, the wave's whole column range inside N, one sample per wave.  Shapes on both sides of each condition (full tiles, a last tile that
    ends on a 16-row group, M = 2005, a ragged last column group, a bias, a grouped image + text launch, a deep K so that requests of
    the NEXT tile are issued while the loader waves stream) -- against the fp32 reference and bit-identical to the 256x128 tile, which
    has no landing buffer."""
    from qflux_amd import _lib as L
    ops = _ops()
    lib = L.lib
    shapes = [(2432, 3072, 256, False), (2000, 3072, 192, False), (2005, 3072, 192, False), (2432, 3000, 128, False), (512, 768, 2048, False),
              (2432, 3072, 128, True), (4864, 3072, 128, False), (16, 3072, 128, False)]

    def run_all():
        outs = {}
        for M, N, K, with_bias in shapes:
            a, b = randn(M, K, seed=1).to(BF), randn(N, K, seed=2, scale=0.2).to(BF)
            hx = randn(M, N, seed=6).to(BF)
            bias = randn(N, seed=9).to(BF) if with_bias else None
            hh = hx.float().requires_grad_(True)
            F.gelu(hh, approximate="tanh").sum().backward()
            ref = rb(rb(a.float() @ b.float().t() + (bias.float() if with_bias else 0.0)) * hh.grad)
            out = ops.gemm(a.to(DEV), b.to(DEV), epi=3, aux=hx.to(DEV), bias=bias.to(DEV) if with_bias else None)
            outs[(M, N, K, with_bias)] = (out.cpu(), ref)
        gs, keep = [], []
        N, K = 3072, 192
        for i, Mi in enumerate((2048, 384)):
            a, b, hx = randn(Mi, K, seed=10 + i).to(BF), randn(N, K, seed=20 + i, scale=0.2).to(BF), randn(Mi, N, seed=80 + i).to(BF)
            hh = hx.float().requires_grad_(True)
            F.gelu(hh, approximate="tanh").sum().backward()
            t = [x.to(DEV) for x in (a, b, hx)]
            out = torch.zeros(Mi, N, dtype=BF, device=DEV)
            g = L.GemmArgs()
            g.A1, g.B1, g.lda1, g.ldb1, g.K1 = t[0].data_ptr(), t[1].data_ptr(), K, K, K
            g.M, g.N, g.C, g.ldc, g.rows_per_batch, g.epi, g.aux, g.ldaux = Mi, N, out.data_ptr(), N, Mi, 3, t[2].data_ptr(), N
            gs.append(g); keep.append((t, out, rb(rb(a.float() @ b.float().t()) * hh.grad)))
        L.check(lib.qfx_gemm_grouped((L.GemmArgs * 2)(*gs), 2, ops.stream_ptr()), "qfx_gemm_grouped")
        for i in range(2):
            outs[f"grouped_{i}"] = (keep[i][1].cpu(), keep[i][2])
        # gate + residual (it has no landing-buffer side -- measured slower, profiles/r06_gemm_aux_landing.json -- so these cases run the
        # general passes of the same kernel): two samples
        # of 1216 rows (the 256-row tile 1024..1279 crosses the boundary: its lower waves fall back) and of 1280, the C row map into a
        # joint buffer (aux indexed like C: a row delta), with and without the second output, a LoRA K segment with the bias rounded
        # in before it (landing side) and a plain bias (general side)
        for Bn, rpb, K, K2, with_c2, with_bias in ((2, 1216, 128, 0, True, False), (2, 1280, 192, 64, True, True), (1, 2432, 128, 0, False, False),
                                                   (2, 1216, 128, 0, False, True), (1, 2048, 3072, 64, True, True)):
            M, T, N = Bn * rpb, 24, 3072
            S = T + rpb
            a, b = randn(M, K, seed=1).to(BF), randn(N, K, seed=2, scale=0.2).to(BF)
            gate, res = randn(Bn, N, seed=7).to(BF), randn(M, N, seed=8).to(BF)
            bias = randn(N, seed=9).to(BF) if with_bias else None
            y = rb(a.float() @ b.float().t() + (bias.float() if with_bias else 0.0))
            kw = {}
            if K2:
                a2, b2 = randn(M, K2, seed=3).to(BF), randn(N, K2, seed=4, scale=0.1).to(BF)
                y = rb(y + a2.float() @ b2.float().t())
                kw = dict(a2=a2.to(DEV), b2=b2.to(DEV))
            refg = rb(res.float() + rb(gate.float().repeat_interleave(rpb, 0) * y))
            cj = torch.zeros(Bn * S, N, dtype=BF, device=DEV)
            resj = torch.zeros(Bn, S, N, dtype=BF)
            resj[:, T:] = res.view(Bn, rpb, N)
            c2 = torch.zeros(M, N, dtype=BF, device=DEV) if with_c2 else None
            ops.gemm(a.to(DEV), b.to(DEV), out=cj, epi=2, aux=resj.view(Bn * S, N).to(DEV), gate=gate.to(DEV), rows_per_batch=rpb, c_map=(S, T),
                     out2=c2, bias=bias.to(DEV) if with_bias else None, **kw)
            key = f"gate_res_{Bn}x{rpb}_k{K}+{K2}_c2{int(with_c2)}_b{int(with_bias)}"
            outs[key] = (cj.view(Bn, S, N)[:, T:].reshape(M, N).cpu(), refg)
            assert cj.view(Bn, S, N)[:, :T].abs().max().item() == 0.0
            if with_c2:
                outs[key + "_pre"] = (c2.cpu(), y)
        return outs

    try:
        assert lib.qfx_gemm_tune(b"256x128", None) == 0
        base = run_all()
        assert lib.qfx_gemm_tune(geo.encode(), None) == 0
        got = [run_all() for _ in range(2)]
    finally:
        assert lib.qfx_gemm_tune(b"all", None) == 0
    for k, (o, ref) in got[0].items():
        check(f"gemm_dgelu_landing_{geo}_{k}", o, ref, 1.5e-2)
        assert torch.equal(o, base[k][0]), f"{geo} {k}: differs from the 256x128 tile's result"
        assert torch.equal(o, got[1][k][0]), f"{geo} {k}: two launches differ"


@pytest.mark.parametrize("seed", range(6))
def test_gemm_dgelu_landing_buffer_shape_fuzz(seed):
    """Random shapes through the d(GELU) epilogue on every tile geometry (the counted waits of the landing-buffer side must hold for any
    mix of full / partial / dead waves, ragged last row and column tiles, one or more tiles per block): bit-identical across geometries
    (256x128 has no buffer) and within tolerance of the fp32 product."""
    import random
    from qflux_amd import _lib as L
    ops = _ops()
    lib = L.lib
    rnd = random.Random(1000 + seed)
    M = rnd.choice([16, 48, 160, 256, 272, 1040, 1216, 2000, 2432]) + rnd.choice([0, 0, 0, 5, 16, 32])
    N = rnd.choice([192, 256, 384, 768, 1536, 3072]) + rnd.choice([0, 0, 8, 64])
    K = 64 * rnd.randint(1, 12)
    a, b = randn(M, K, seed=seed).to(BF), randn(N, K, seed=100 + seed, scale=0.2).to(BF)
    hx = randn(M, N, seed=200 + seed).to(BF)
    hh = hx.float().requires_grad_(True)
    F.gelu(hh, approximate="tanh").sum().backward()
    ref = rb(rb(a.float() @ b.float().t()) * hh.grad)
    ad, bd, hd = a.to(DEV), b.to(DEV), hx.to(DEV)
    outs = {}
    try:
        for geo in GEOMETRIES:
            assert lib.qfx_gemm_tune(geo.encode(), None) == 0
            outs[geo] = ops.gemm(ad, bd, epi=3, aux=hd).cpu()
    finally:
        assert lib.qfx_gemm_tune(b"all", None) == 0
    for geo, o in outs.items():
        check(f"gemm_dgelu_fuzz_{seed}_{geo}_{M}x{N}x{K}", o, ref, 1.5e-2)
        assert torch.equal(o, outs["256x128"]), (geo, M, N, K)


# ------------------------------------------------------------------------------------------ LoRA pieces
def _split(x):
    hi = x.to(BF)
    lo = (x - hi.float()).to(BF)
    return hi, lo


@pytest.mark.parametrize("R,M,K", [(16, 100, 256), (48, 2432, 3072), (32, 77, 512)])
def test_lora_down(R, M, K):
    ops = _ops()
    x = randn(M, K, seed=1).to(BF)
    w = randn(R, K, seed=2, scale=0.1)
    hi, lo = _split(w)
    ref = x.float() @ (hi.float() + lo.float()).t()
    U = torch.empty(M, R, dtype=torch.float32, device=DEV)
    Kext = ((3 * R + 63) // 64) * 64
    ext = torch.zeros(M, Kext, dtype=BF, device=DEV)
    ops.lora_down(x.to(DEV), hi.to(DEV), lo.to(DEV), U=U, ext=ext)
    check(f"lora_down_U_{R}", U, ref, 2e-5)
    check(f"lora_down_fp32acc_{R}", U, x.float() @ w.t(), 1e-4)
    e = ext.float().cpu()
    recon = e[:, :R] + e[:, R:2 * R]
    check(f"lora_down_ext_{R}", recon, ref, 1e-4)
    assert torch.equal(e[:, :R], e[:, 2 * R:3 * R])


def test_lora_down_grouped_ext():
    ops = _ops()
    M, K, Rp, Kext = 64, 128, 16, 64
    x = randn(M, K, seed=1).to(BF)
    w = randn(3 * Rp, K, seed=2, scale=0.1)
    hi, lo = _split(w)
    ext = torch.zeros(M, 3 * Kext, dtype=BF, device=DEV)
    U = torch.empty(M, 3 * Rp, dtype=torch.float32, device=DEV)
    ops.lora_down(x.to(DEV), hi.to(DEV), lo.to(DEV), U=U, ext=ext, group_R=Rp, group_stride=Kext)
    e = ext.float().cpu().view(M, 3, Kext)
    u = U.cpu().view(M, 3, Rp)
    check("lora_down_grouped", e[:, :, :Rp] + e[:, :, Rp:2 * Rp], u, 1e-4)
    assert e[:, :, 3 * Rp:].abs().max() == 0


@pytest.mark.parametrize("dh,S,T,R,Bn", [(128, 2432, 384, 16, 1), (64, 200, 16, 32, 2), (128, 333, 48, 16, 1)])
def test_attention_forward_emits_the_out_projection_down_projection(dh, S, T, R, Bn):
    """ABI 6, qfx_head_lora slot 0 + qfx_lora_head_reduce: u = O A^T leaves the attention forward as per-head partial sums and the
    reduce launch writes qfx_lora_down's outputs -- compared with qfx_lora_down on the O the kernel wrote (image rows s >= T with
    one adapter, text rows s < T with another; ragged S, two samples, both head dims, rank 16 / 32)."""
    import ctypes as C
    from qflux_amd import _lib as L
    ops = _ops()
    H = 3
    D = H * dh
    S_pad = (S + 63) // 64 * 64
    qkv = randn(Bn, S, 3 * D, seed=4).to(BF).to(DEV)
    O = torch.zeros(Bn, S, D, dtype=BF, device=DEV)
    lse2 = torch.zeros(Bn, H, S_pad, device=DEV)
    w = {s: _split(randn(R, D, seed=10 + i, scale=0.1)) for i, s in enumerate(("img", "txt"))}
    wd = {s: (w[s][0].to(DEV), w[s][1].to(DEV)) for s in w}
    part = torch.full((H, Bn * S, R + 4), float("nan"), device=DEV)       # ld_part > R, c0 = 4: neighbours must stay untouched
    a = ops.attn_args(Bn, S, S_pad, H, dh, 1 / math.sqrt(dh), Q=qkv[:, :, :D], K=qkv[:, :, D:2 * D], V=qkv[:, :, 2 * D:], ldq=3 * D, ldk=3 * D,
                      ldv=3 * D, O=O, ldo=D, lse2=lse2)
    a.T = T
    hl = a.hl[0]
    hl.part, hl.part_hstride, hl.ld_part, hl.c0, hl.R = part.data_ptr(), Bn * S * (R + 4), R + 4, 4, R
    imgs = {s: L.head_fragment_image(wd[s][0], wd[s][1], dh) for s in wd}
    for si, s in enumerate(("img", "txt")):
        hl.w_pk[si] = imgs[s].data_ptr()
    ops.attn_call("qfx_attn_fwd", a)
    assert torch.isnan(part[:, :, :4]).all() and not torch.isnan(part[:, :, 4:]).any()
    Kext = ((3 * R + 63) // 64) * 64
    for s, (lo_, hi_) in (("txt", (0, T)), ("img", (T, S))):
        M = Bn * (hi_ - lo_)
        mp = (M + 127) // 128 * 128
        ext = torch.zeros(M, Kext, dtype=BF, device=DEV)
        Ut = (torch.zeros(R, mp, dtype=BF, device=DEV), torch.zeros(R, mp, dtype=BF, device=DEV))
        r = L.LoraHeadReduceArgs()
        pv = part[:, :, 4:]
        r.part, r.part_hstride, r.ld_part, r.H = pv.data_ptr(), Bn * S * (R + 4), R + 4, H
        r.M, r.R, r.ext, r.ld_ext = M, R, ext.data_ptr(), Kext
        r.Ut_hi, r.Ut_lo, r.ld_ut, r.group_R, r.group_stride = Ut[0].data_ptr(), Ut[1].data_ptr(), mp, R, 0
        r.rows_per_batch, r.x_batch_rows, r.x_row_off = hi_ - lo_, S, lo_
        L.check(L.lib.qfx_lora_head_reduce(C.byref(r), 1, ops.stream_ptr()), "qfx_lora_head_reduce")
        # reference: the stand-alone down projection of the same rows of O
        ext_r = torch.zeros_like(ext)
        Ut_r = (torch.zeros_like(Ut[0]), torch.zeros_like(Ut[1]))
        U_r = torch.empty(M, R, dtype=torch.float32, device=DEV)
        ops.lora_down(O.view(Bn * S, D), wd[s][0], wd[s][1], U=U_r, ext=ext_r, Ut=Ut_r, M=M, rows_per_batch=hi_ - lo_, x_map=(S, lo_))
        e, er = ext.float().cpu(), ext_r.float().cpu()
        check(f"head_lora_fwd_{dh}_{S}_{s}", e[:, :R] + e[:, R:2 * R], U_r, 2e-5)       # fp32 sums in a different order
        assert torch.equal(e[:, :R], e[:, 2 * R:3 * R]) and e[:, 3 * R:].abs().max() == 0
        check(f"head_lora_fwd_ut_{dh}_{S}_{s}", (Ut[0].float() + Ut[1].float())[:, :M].t(), U_r, 2e-5)
        assert Ut[0][:, M:].abs().sum() == 0 and (er[:, :R] - e[:, :R]).abs().max() <= 2.0 ** -7 * er[:, :R].abs().max()
    # bad arguments are refused before any launch
    hl.R = 24
    assert L.lib.qfx_attn_fwd(C.byref(a), ops.stream_ptr()) == -2
    hl.R = R
    a.T = T + 3
    assert L.lib.qfx_attn_fwd(C.byref(a), ops.stream_ptr()) == -1


def test_tr_read_lane_mapping():
    """gfx950 ds_read_b64_tr_b16: result[lane i][j] = data[lane 16*(i>>4) + 4j + ((i&15)>>2)][i&3] (documents the HW)."""
    from qflux_amd import _lib as L
    src = torch.arange(256, dtype=torch.int16, device=DEV)
    out = torch.empty_like(src)
    L.check(L.lib.qfx_debug_tr_read(src.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream), "tr")
    o = out.cpu().view(64, 4)
    exp = torch.empty(64, 4, dtype=torch.int16)
    for i in range(64):
        for j in range(4):
            lane = 16 * (i >> 4) + 4 * j + ((i & 15) >> 2)
            exp[i, j] = lane * 4 + (i & 3)
    assert torch.equal(o, exp), (o[:20], exp[:20])


@pytest.mark.parametrize("M,K,R,r", [(300, 1024, 16, 12), (2432, 3072, 16, 16), (77, 64, 32, 32)])
def test_lora_grad(M, K, R, r):
    ops = _ops()
    V = randn(M, R, seed=1)
    X = randn(M, K, seed=2).to(BF)
    Mp = (M + 127) // 128 * 128
    hi, lo = _split(V)
    Vt_hi = torch.zeros(R, Mp, dtype=BF); Vt_lo = torch.zeros(R, Mp, dtype=BF)
    Vt_hi[:, :M], Vt_lo[:, :M] = hi.t(), lo.t()
    Vt = (Vt_hi.to(DEV), Vt_lo.to(DEV))
    ref = ((hi.float() + lo.float()).t() @ X.float())[:r]
    G = torch.zeros(r, K, dtype=torch.float32, device=DEV)
    ops.lora_grad(Vt, X.to(DEV), G, K, 1, M=M, r_valid=r)
    check(f"lora_grad_A_{M}", G, ref, 1e-4)
    Gt = torch.zeros(K, r, dtype=torch.float32, device=DEV)
    ops.lora_grad(Vt, X.to(DEV), Gt, 1, r, M=M, r_valid=r, out_scale=2.0)
    check(f"lora_grad_Bt_{M}", Gt, 2.0 * ref.t(), 1e-4)


def test_lora_grad_is_bit_reproducible_and_matches_the_atomic_form():
    """ABI 7: with a scratch the token-chunk partials (5 chunks at M = 2432) are added in chunk order by the last block of each 128-column
    strip -- six launches give identical bits (the fp32-atomic form of rounds 1-5 differs in the last bit from launch to launch), both
    forms agree to fp32 rounding, and the strip counters are back at zero (ops.lora_grad asserts it)."""
    ops = _ops()
    M, K, R, r = 2432, 3072, 16, 16
    Vt = [(randn(R, 2432, seed=71 + i) * 0.3).to(BF).to(DEV) for i in range(2)]
    X = randn(M, K, seed=73).to(BF).to(DEV)
    outs = []
    for rep in range(6):
        G = torch.zeros(r, K, device=DEV)
        ops.lora_grad(Vt, X, G, K, 1, M=M, r_valid=r)
        outs.append(G)
    assert all(torch.equal(outs[0].view(torch.int32), g.view(torch.int32)) for g in outs[1:])
    Ga = torch.zeros(r, K, device=DEV)
    ops.lora_grad(Vt, X, Ga, K, 1, M=M, r_valid=r, deterministic=False)
    assert ((Ga - outs[0]).abs().max() / Ga.abs().max()).item() < 1e-6
    G2 = outs[0].clone()      # accumulation on top of an existing gradient (micro-batches)
    ops.lora_grad(Vt, X, G2, K, 1, M=M, r_valid=r)
    assert ((G2 - 2 * outs[0]).abs().max() / outs[0].abs().max()).item() < 1e-6


def test_lora_grad_fused_three_targets_and_remap():
    ops = _ops()
    Bn, rpb, T, K, Rp, r = 2, 70, 10, 256, 16, 8
    S = T + rpb
    M = Bn * rpb
    Mp = (M + 127) // 128 * 128
    V = randn(M, 3 * Rp, seed=1)
    Xj = randn(Bn * S, K, seed=2).to(BF)
    X = Xj.view(Bn, S, K)[:, T:].reshape(M, K)
    hi, lo = _split(V)
    Vt_hi = torch.zeros(3 * Rp, Mp, dtype=BF); Vt_lo = torch.zeros(3 * Rp, Mp, dtype=BF)
    Vt_hi[:, :M], Vt_lo[:, :M] = hi.t(), lo.t()
    Gs = [torch.zeros(r, K, dtype=torch.float32, device=DEV) for _ in range(3)]
    ops.lora_grad((Vt_hi.to(DEV), Vt_lo.to(DEV)), Xj.to(DEV), Gs, K, 1, M=M, r_valid=r, group_R=Rp, rows_per_batch=rpb, x_map=(S, T))
    ref = (hi.float() + lo.float()).t() @ X.float()
    for i in range(3):
        check(f"lora_grad_fused_{i}", Gs[i], ref[i * Rp:i * Rp + r], 1e-4)


def test_lora_down_transposed_output():
    ops = _ops()
    M, K, R = 100, 256, 32
    x = randn(M, K, seed=1).to(BF)
    w = randn(R, K, seed=2, scale=0.1)
    hi, lo = _split(w)
    Ut = (torch.zeros(R, 128, dtype=BF, device=DEV), torch.zeros(R, 128, dtype=BF, device=DEV))
    U = torch.empty(M, R, dtype=torch.float32, device=DEV)
    ops.lora_down(x.to(DEV), hi.to(DEV), lo.to(DEV), U=U, Ut=Ut)
    rec = (Ut[0].float() + Ut[1].float()).cpu()
    check("lora_down_Ut", rec[:, :M], U.cpu().t(), 1e-4)
    assert rec[:, M:].abs().max() == 0


def test_lora_pack():
    from qflux_amd import _lib as L
    ops = _ops()
    r, K, N, Rp, Kext, s = 4, 128, 192, 16, 64, 2.0
    A, Bm = randn(r, K, seed=1).to(DEV), randn(N, r, seed=2).to(DEV)
    A_hi = torch.empty(Rp, K, dtype=BF, device=DEV); A_lo = torch.empty_like(A_hi)
    Bt_hi = torch.empty(Rp, N, dtype=BF, device=DEV); Bt_lo = torch.empty_like(Bt_hi)
    We = torch.full((N, Kext), 7.0, dtype=BF, device=DEV); WeT = torch.full((K, Kext), 7.0, dtype=BF, device=DEV)
    d = L.LoraPackArgs()
    d.A, d.B, d.r, d.K, d.N, d.scale = A.data_ptr(), Bm.data_ptr(), r, K, N, s
    d.A_hi, d.A_lo, d.ld_a = A_hi.data_ptr(), A_lo.data_ptr(), K
    d.Bt_hi, d.Bt_lo, d.ld_bt = Bt_hi.data_ptr(), Bt_lo.data_ptr(), N
    d.We, d.ld_we, d.WeT, d.ld_wet, d.Rp, d.Kext = We.data_ptr(), Kext, WeT.data_ptr(), Kext, Rp, Kext
    # ABI 6: the head-fragment images of both operands (head dim 64: K = 2 heads, N = 3 heads)
    A_hl = torch.full((2 * Rp * K,), 7.0, dtype=BF, device=DEV); Bt_hl = torch.full((2 * Rp * N,), 7.0, dtype=BF, device=DEV)
    d.A_hl, d.Bt_hl, d.hl_dh = A_hl.data_ptr(), Bt_hl.data_ptr(), 64
    # ... and the A rows inside the fragment image of a 3-adapter row group (this adapter = rows Rp .. 2 Rp of it)
    A_fr = torch.zeros(2 * 3 * Rp * K, dtype=BF, device=DEV)
    d.A_fr, d.fr_row0, d.fr_nf = A_fr.data_ptr(), Rp, 3 * Rp // 16
    t = ops.pack_descs_tensor([d], DEV)
    ops.lora_pack(t, 1, max(K, N))
    torch.cuda.synchronize()
    assert torch.equal(A_hl, L.head_fragment_image(A_hi, A_lo, 64)) and torch.equal(Bt_hl, L.head_fragment_image(Bt_hi, Bt_lo, 64))
    g_hi = torch.zeros(3 * Rp, K, dtype=BF, device=DEV); g_lo = torch.zeros_like(g_hi)
    g_hi[Rp:2 * Rp], g_lo[Rp:2 * Rp] = A_hi, A_lo
    assert torch.equal(A_fr, L.down_fragment_image(g_hi, g_lo))
    Ap = torch.zeros(Rp, K); Ap[:r] = A.cpu()
    Bp = torch.zeros(Rp, N); Bp[:r] = s * Bm.cpu().t()
    check("pack_A", A_hi.float() + A_lo.float(), Ap, 1e-4)
    check("pack_Bt", Bt_hi.float() + Bt_lo.float(), Bp, 1e-4)
    we = We.float().cpu()
    check("pack_We", we[:, :Rp] + we[:, 2 * Rp:3 * Rp], Bp.t(), 1e-4)
    assert torch.equal(we[:, :Rp], we[:, Rp:2 * Rp]) and we[:, 3 * Rp:].abs().max() == 0
    wt = WeT.float().cpu()
    check("pack_WeT", wt[:, :Rp] + wt[:, 2 * Rp:3 * Rp], Ap.t(), 1e-4)
    assert torch.equal(wt[:, :Rp], wt[:, Rp:2 * Rp]) and wt[:, 3 * Rp:].abs().max() == 0


def test_lora_linear_composition():
    """skinny down + packed operands + GEMM K-extension == peft LoRA linear (oracle semantics)."""
    from qflux_amd import _lib as L
    ops = _ops()
    M, K, N, r, Rp, Kext, s = 200, 256, 384, 8, 16, 64, 2.0
    x = randn(M, K, seed=1).to(BF)
    W, bias = randn(N, K, seed=2, scale=0.06).to(BF), randn(N, seed=3, scale=0.1).to(BF)
    A, Bm = randn(r, K, seed=4, scale=0.2), randn(N, r, seed=5, scale=0.2)
    base = rb(x.float() @ W.float().t() + bias.float())
    ref = rb(base + (x.float() @ A.t()) @ Bm.t() * s)
    A_hi = torch.empty(Rp, K, dtype=BF, device=DEV); A_lo = torch.empty_like(A_hi)
    Bt_hi = torch.empty(Rp, N, dtype=BF, device=DEV); Bt_lo = torch.empty_like(Bt_hi)
    We = torch.empty(N, Kext, dtype=BF, device=DEV); WeT = torch.empty(K, Kext, dtype=BF, device=DEV)
    Ad, Bd = A.to(DEV), Bm.to(DEV)
    d = L.LoraPackArgs()
    d.A, d.B, d.r, d.K, d.N, d.scale = Ad.data_ptr(), Bd.data_ptr(), r, K, N, s
    d.A_hi, d.A_lo, d.ld_a = A_hi.data_ptr(), A_lo.data_ptr(), K
    d.Bt_hi, d.Bt_lo, d.ld_bt = Bt_hi.data_ptr(), Bt_lo.data_ptr(), N
    d.We, d.ld_we, d.WeT, d.ld_wet, d.Rp, d.Kext = We.data_ptr(), Kext, WeT.data_ptr(), Kext, Rp, Kext
    ops.lora_pack(ops.pack_descs_tensor([d], DEV), 1, max(K, N))
    ext = torch.zeros(M, Kext, dtype=BF, device=DEV)
    xd = x.to(DEV)
    ops.lora_down(xd, A_hi, A_lo, ext=ext)
    out = ops.gemm(xd, W.to(DEV), bias=bias.to(DEV), a2=ext, b2=We)
    check("lora_linear_fwd", out, ref, 1e-2)
    # the LoRA delta itself must be accurate (not hidden in bf16 rounding of the base)
    out0 = ops.gemm(xd, W.to(DEV), bias=bias.to(DEV))
    delta = out.float().cpu() - out0.float().cpu()
    check("lora_linear_delta", delta, ref - base, 5e-2)


# ------------------------------------------------------------------------------------------ row kernels
def _ln_mod_ref(x, shift, scale, rpb):
    ln = rb(F.layer_norm(x, (x.shape[-1],), eps=1e-6))
    t1 = rb(1 + scale.repeat_interleave(rpb, 0))
    return rb(rb(ln * t1) + shift.repeat_interleave(rpb, 0))


@pytest.mark.parametrize("D", [256, 3072])
def test_ln_modulate_fwd_bwd(D):
    ops = _ops()
    Bn, rpb = 2, 37
    rows = Bn * rpb
    x = randn(rows, D, seed=1, scale=2.0).to(BF)
    mod = randn(Bn, 6 * D, seed=2, scale=0.5).to(BF)
    shift, scale, gate = mod[:, :D], mod[:, D:2 * D], mod[:, 2 * D:3 * D]
    ref = _ln_mod_ref(x.float(), shift.float(), scale.float(), rpb)
    modd = mod.to(DEV)
    out = ops.ln_modulate_fwd(x.to(DEV), modd[:, :D], modd[:, D:2 * D], rpb)
    check(f"ln_mod_fwd_{D}", out, ref, 1e-2)
    # backward vs autograd of the fp32 graph
    dy = randn(rows, D, seed=3).to(BF)
    dres = randn(rows, D, seed=4).to(BF)
    xx = x.float().requires_grad_(True)
    y = F.layer_norm(xx, (D,), eps=1e-6) * rb(1 + scale.float().repeat_interleave(rpb, 0)) + shift.float().repeat_interleave(rpb, 0)
    y.backward(dy.float())
    dx_ref = rb(dres.float() + rb(xx.grad))
    dx, dyg = ops.ln_modulate_bwd(dy.to(DEV), x.to(DEV), modd[:, D:2 * D], rpb, dres=dres.to(DEV), gate=modd[:, 2 * D:3 * D], want_dyg=True)
    check(f"ln_mod_bwd_dx_{D}", dx, dx_ref, 1.5e-2)
    check(f"ln_mod_bwd_dyg_{D}", dyg, rb(gate.float().repeat_interleave(rpb, 0) * dx.float().cpu()), 1e-2)
    g2 = ops.gate_mul(dx, modd[:, 2 * D:3 * D], rpb)
    check(f"gate_mul_{D}", g2, rb(gate.float().repeat_interleave(rpb, 0) * dx.float().cpu()), 1e-2)


def test_rmsnorm_fwd():
    ops = _ops()
    x = randn(50, 3584, seed=1, scale=3.0).to(BF)
    w = (1 + 0.1 * randn(3584, seed=2)).to(BF)
    xf = x.float()
    ref = rb(rb(xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6)) * w.float())
    check("rmsnorm", ops.rmsnorm_fwd(x.to(DEV), w.to(DEV)), ref, 1e-2)


def test_mod_gemv_and_timestep():
    ops = _ops()
    Bn, K, N = 2, 512, 1536
    temb = randn(Bn, K, seed=1).to(BF)
    Ws = [randn(N, K, seed=10 + i, scale=0.05).to(BF) for i in range(3)]
    bs = [randn(N, seed=20 + i, scale=0.1).to(BF) for i in range(3)]
    s = rb(F.silu(temb.float()))
    out = ops.mod_gemv(temb.to(DEV), [w.to(DEV) for w in Ws], [b.to(DEV) for b in bs])
    for i in range(3):
        check(f"mod_gemv_{i}", out[i], rb(s @ Ws[i].float().t() + bs[i].float()), 1e-2)
    out = ops.mod_gemv(temb.to(DEV), [Ws[0].to(DEV)], [bs[0].to(DEV)], apply_silu=False)
    check("gemv_nosilu", out[0], rb(temb.float() @ Ws[0].float().t() + bs[0].float()), 1e-2)
    from oracle.qwen_dit import timestep_sinusoid
    t = torch.tensor([0.7109, 0.1611, 0.999])
    ref = rb(timestep_sinusoid(rb(t), 256, scale=1000.0))
    check("timestep_embed", ops.timestep_embed(t.to(DEV)), ref, 2e-2)


@pytest.mark.parametrize("Bn,K,N,nmat", [(1, 3072, 1000, 5), (2, 1024, 768, 3), (3, 512, 130, 2)])
def test_mod_gemv_transposed(Bn, K, N, nmat):
    """qfx_mod_gemv_t: sum over matrices of dy[mat] @ W_mat (fp32 accumulation) -- the backward of qfx_mod_gemv w.r.t. its input."""
    ops = _ops()
    Ws = [randn(N, K, seed=30 + i, scale=0.05).to(BF) for i in range(nmat)]
    dy = randn(nmat, Bn, N, seed=7).to(BF)
    ref = sum(dy[i].float() @ Ws[i].float() for i in range(nmat))
    out = ops.mod_gemv_t(dy.to(DEV), [w.to(DEV) for w in Ws])
    check(f"mod_gemv_t_{Bn}_{K}", out, ref, 2e-4)
    out2 = ops.mod_gemv_t(dy.to(DEV), [w.to(DEV) for w in Ws], out=out.clone())      # accumulates into `out`
    check(f"mod_gemv_t_acc_{Bn}_{K}", out2, 2 * ref, 2e-4)


@pytest.mark.parametrize("dh", [64, 128])
def test_qk_norm_rope_fwd_bwd(dh):
    from oracle.qwen_dit import OracleRMSNorm, apply_rope_complex, qwen_rope_tables
    ops = _ops()
    Bn, H, T = 2, 3, 5
    shapes = [(1, 4, 6), (1, 4, 6)]
    S_i = 48
    S = T + S_i
    D = H * dh
    axes = (16, 56, 56) if dh == 128 else (8, 28, 28)
    vid, txt = qwen_rope_tables(shapes, T, axes)
    freqs = torch.cat([txt, vid], 0)  # joint order [text, image]
    rope = torch.view_as_real(freqs).contiguous().float()  # [S, dh/2, 2]
    qkv = randn(Bn, S, 3 * D, seed=1, scale=1.5).to(BF)
    ws = [(1 + 0.2 * randn(dh, seed=10 + i)).to(BF) for i in range(4)]  # q_txt, k_txt, q_img, k_img

    def ref_fwd(qkv_f):
        outs = []
        for sec, (wt, wi) in enumerate([(ws[0], ws[2]), (ws[1], ws[3])]):
            x = qkv_f[:, :, sec * D:(sec + 1) * D].reshape(Bn, S, H, dh)
            parts = []
            for (lo, hi, wsel) in [(0, T, wt), (T, S, wi)]:
                n = OracleRMSNorm(dh)
                n.weight.data = wsel.clone()
                parts.append(apply_rope_complex(n(x[:, lo:hi].to(BF)), freqs[lo:hi]))
            outs.append(torch.cat(parts, 1).reshape(Bn, S, D))
        return outs

    q_ref, k_ref = ref_fwd(qkv)
    buf = qkv.clone().to(DEV)
    saved = torch.empty(Bn, S, 2 * D, dtype=BF, device=DEV)
    wd = [w.to(DEV) for w in ws]
    ops.qk_norm_rope(buf, saved, rope.to(DEV), wd[0], wd[1], wd[2], wd[3], Bn, S, T, H, dh)
    check(f"qk_fwd_q_{dh}", buf[:, :, :D], q_ref.float(), 1.5e-2)
    check(f"qk_fwd_k_{dh}", buf[:, :, D:2 * D], k_ref.float(), 1.5e-2)
    assert torch.equal(buf[:, :, 2 * D:].cpu(), qkv[:, :, 2 * D:])
    assert torch.equal(saved.cpu(), qkv[:, :, :2 * D])
    # out-of-place mode (flags bit1): pre-norm q,k read from `saved`, result into the q,k sections of qkv -- same bits, v untouched
    buf2 = torch.zeros_like(buf)
    buf2[:, :, 2 * D:] = buf[:, :, 2 * D:]
    ops.qk_norm_rope(buf2, saved, rope.to(DEV), wd[0], wd[1], wd[2], wd[3], Bn, S, T, H, dh, flags=2)
    assert torch.equal(buf2, buf) and torch.equal(saved.cpu(), qkv[:, :, :2 * D])
    # backward vs fp32 autograd
    dq = randn(Bn, S, 3 * D, seed=5).to(BF)
    xx = qkv.float().requires_grad_(True)
    outs = []
    for sec, (wt, wi) in enumerate([(ws[0], ws[2]), (ws[1], ws[3])]):
        x = xx[:, :, sec * D:(sec + 1) * D].reshape(Bn, S, H, dh)
        parts = []
        for (lo, hi, wsel) in [(0, T, wt), (T, S, wi)]:
            xs = x[:, lo:hi]
            n = xs * torch.rsqrt(xs.pow(2).mean(-1, keepdim=True) + 1e-6) * wsel.float()
            xc = torch.view_as_complex(n.reshape(*n.shape[:-1], -1, 2))
            parts.append(torch.view_as_real(xc * freqs[lo:hi].unsqueeze(1)).flatten(3))
        outs.append(torch.cat(parts, 1).reshape(Bn, S, D))
    (outs[0] * dq[:, :, :D].float()).sum().backward(retain_graph=True)
    (outs[1] * dq[:, :, D:2 * D].float()).sum().backward()
    dbuf = dq.clone().to(DEV)
    ops.qk_norm_rope(dbuf, saved, rope.to(DEV), wd[0], wd[1], wd[2], wd[3], Bn, S, T, H, dh, backward=True)
    check(f"qk_bwd_{dh}", dbuf[:, :, :2 * D], xx.grad[:, :, :2 * D], 2e-2)
    assert torch.equal(dbuf[:, :, 2 * D:].cpu(), dq[:, :, 2 * D:])


def test_transpose_heads():
    ops = _ops()
    Bn, S, H, dh, S_pad = 2, 100, 2, 64, 128
    x = randn(Bn, S, 3 * H * dh, seed=1).to(BF).to(DEV)
    v = x[:, :, 2 * H * dh:]
    out = ops.transpose_heads(v, 3 * H * dh, Bn, S, S_pad, H, dh)
    ref = torch.zeros(Bn, H, dh, S_pad)
    ref[..., :S] = v.float().cpu().reshape(Bn, S, H, dh).permute(0, 2, 3, 1)
    assert torch.equal(out.float().cpu(), ref)


# ------------------------------------------------------------------------------------------ attention
def _attn_case(dh, S, Bn=2, H=2, mask=False, seed=0):
    D = H * dh
    S_pad = ((S + 63) // 64) * 64
    qkv = randn(Bn, S, 3 * D, seed=seed + 1).to(BF)
    do = randn(Bn, S, D, seed=seed + 2).to(BF)
    km = None
    if mask:
        km = torch.zeros(Bn, S)
        km[1, S - 7:] = float("-inf")
    return qkv, do, km, S_pad


@pytest.mark.parametrize("dh,S,mask", [(64, 200, False), (128, 200, False), (128, 333, True), (64, 64, False), (128, 2432, False)])
def test_attention_fwd_bwd(dh, S, mask):
    ops = _ops()
    Bn, H = (2, 2) if S < 1000 else (1, 2)
    D = H * dh
    qkv, do, km, S_pad = _attn_case(dh, S, Bn, H, mask)
    scale = 1.0 / math.sqrt(dh)
    # fp32 reference with autograd
    x = qkv.float().requires_grad_(True)
    q, k, v = (x[:, :, i * D:(i + 1) * D].reshape(Bn, S, H, dh).transpose(1, 2) for i in range(3))
    am = km[:, None, None, :] if km is not None else None
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=am).transpose(1, 2).reshape(Bn, S, D)
    o.backward(do.float())
    qd = qkv.to(DEV)
    ld = 3 * D
    Q, K, V = qd[:, :, :D], qd[:, :, D:2 * D], qd[:, :, 2 * D:]
    Vt = ops.transpose_heads(V, ld, Bn, S, S_pad, H, dh)
    O = torch.empty(Bn, S, D, dtype=BF, device=DEV)
    lse2 = torch.zeros(Bn, H, S_pad, dtype=torch.float32, device=DEV)
    kmd = km.to(DEV) if km is not None else None
    a = ops.attn_args(Bn, S, S_pad, H, dh, scale, Q=Q, K=K, V=V, ldq=ld, ldk=ld, ldv=ld, Vt=Vt, O=O, ldo=D, lse2=lse2,
                      key_mask=kmd.data_ptr() if kmd is not None else None)
    ops.attn_call("qfx_attn_fwd", a)
    check(f"attn_fwd_{dh}_{S}", O, o, 1e-2)
    # lse check
    sc = (q @ k.transpose(-1, -2)) * scale
    if am is not None:
        sc = sc + am
    lse_ref = torch.logsumexp(sc, -1) / math.log(2.0)
    check(f"attn_lse_{dh}_{S}", lse2[:, :, :S], lse_ref, 1e-3)
    # backward
    dOd = do.to(DEV)
    Qt = ops.transpose_heads(Q, ld, Bn, S, S_pad, H, dh)
    Kt = ops.transpose_heads(K, ld, Bn, S, S_pad, H, dh)
    dOt = ops.transpose_heads(dOd, D, Bn, S, S_pad, H, dh)
    dsum = torch.zeros(Bn, H, S_pad, dtype=torch.float32, device=DEV)
    dqkv = torch.zeros(Bn, S, 3 * D, dtype=BF, device=DEV)
    a.Qt, a.Kt, a.dO, a.lddo, a.dOt, a.dsum = Qt.data_ptr(), Kt.data_ptr(), dOd.data_ptr(), D, dOt.data_ptr(), dsum.data_ptr()
    a.dQ, a.dK, a.dV = dqkv[:, :, :D].data_ptr(), dqkv[:, :, D:2 * D].data_ptr(), dqkv[:, :, 2 * D:].data_ptr()
    a.lddq = a.lddk = a.lddv = ld
    ops.attn_call("qfx_attn_bwd_prep", a)
    check(f"attn_dsum_{dh}_{S}", dsum[:, :, :S], (do.float() * O.float().cpu()).reshape(Bn, S, H, dh).sum(-1).transpose(1, 2), 2e-2)
    ops.attn_call("qfx_attn_bwd_dq", a)
    ops.attn_call("qfx_attn_bwd_dkv", a)
    g = x.grad
    check(f"attn_dq_{dh}_{S}", dqkv[:, :, :D], g[:, :, :D], 2e-2)
    check(f"attn_dk_{dh}_{S}", dqkv[:, :, D:2 * D], g[:, :, D:2 * D], 2e-2)
    check(f"attn_dv_{dh}_{S}", dqkv[:, :, 2 * D:], g[:, :, 2 * D:], 2e-2)


@pytest.mark.parametrize("S", [2432, 8576])
def test_attention_kernels_are_bit_reproducible(S):
    """VERDICT r4 #3 / ADVICE r4: the fused dQ epilogue once differed from run to run (profiles/r05_nondeterminism.md).  Every attention
    entry point, with the fused QK-norm backward and the fused rank-r projections on, launched 8 times on identical inputs into
    re-zeroed outputs: all outputs bit-identical, at the headline S and at the ragged-free S = 8576 of cfg #4 (3+ rounds of blocks)."""
    import ctypes as C
    import math
    from qflux_amd import _lib as L
    ops = _ops()
    H, dh, Bn, T, R = 24, 128, 1, 384, 16
    D = H * dh
    S_pad = (S + 63) // 64 * 64
    g = torch.Generator(device=DEV).manual_seed(S)
    qkv = torch.randn(Bn, S, 3 * D, device=DEV, generator=g).to(torch.bfloat16)
    dO = torch.randn(Bn, S, D, device=DEV, generator=g).to(torch.bfloat16)
    sqk = torch.randn(Bn, S, 2 * D, device=DEV, generator=g).to(torch.bfloat16)
    ang = torch.rand(S, dh // 2, device=DEV, generator=g) * 6.28
    rope = torch.stack([ang.cos(), ang.sin()], -1).contiguous()
    ws = [(1 + 0.1 * torch.randn(dh, device=DEV, generator=g)).to(torch.bfloat16) for _ in range(4)]
    O = torch.zeros(Bn, S, D, dtype=torch.bfloat16, device=DEV)
    lse2 = torch.zeros(Bn, H, S_pad, device=DEV)
    dsum = torch.zeros(Bn, H, S_pad, device=DEV)
    dqkv = torch.zeros_like(qkv)
    ld = 3 * D
    a = ops.attn_args(Bn, S, S_pad, H, dh, 1 / math.sqrt(dh), Q=qkv[:, :, :D], K=qkv[:, :, D:2 * D], V=qkv[:, :, 2 * D:], ldq=ld, ldk=ld, ldv=ld,
                      O=O, ldo=D, lse2=lse2, dsum=dsum, dO=dO, lddo=D, dQ=dqkv[:, :, :D], dK=dqkv[:, :, D:2 * D], dV=dqkv[:, :, 2 * D:],
                      lddq=ld, lddk=ld, lddv=ld)
    a.T = T
    parts, keep = [], []
    for slot in range(4):
        wts = [(torch.randn(R, D, device=DEV, generator=g) * 0.1).to(torch.bfloat16) for _ in range(2)]
        part = torch.zeros(H, Bn * S, R, device=DEV)
        hl = a.hl[slot]
        hl.part, hl.part_hstride, hl.ld_part, hl.c0, hl.R = part.data_ptr(), Bn * S * R, R, 0, R
        w = [L.head_fragment_image(wts[0], wts[1], dh), L.head_fragment_image(wts[1], wts[0], dh)]
        hl.w_pk[0], hl.w_pk[1] = (t.data_ptr() for t in w)
        parts.append(part); keep.append(w)
    st = ops.stream_ptr()

    def run(fn, outs, reps=8):
        ref = None
        for _ in range(reps):
            for t in outs:
                t.zero_()
            L.check(fn(C.byref(a), st), fn.__name__)
            torch.cuda.synchronize()
            cur = [t.clone() for t in outs]
            if ref is None:
                ref = cur
            else:
                for i, (x, y) in enumerate(zip(cur, ref)):
                    assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"{fn.__name__}: output {i} differs between two launches on identical inputs"

    for mode in ("0", "1", "1p"):       # the 32-query and both 64-query forwards
        ops.attn_tune("fwd64=" + mode)
        try:
            run(L.lib.qfx_attn_fwd, [O, lse2, parts[0]])
        finally:
            ops.attn_tune("fwd64=auto")
    a.qk_saved, a.ld_saved, a.rope, a.rope_bstride = sqk.data_ptr(), 2 * D, rope.data_ptr(), 0
    a.wq_txt, a.wk_txt, a.wq_img, a.wk_img = (t.data_ptr() for t in ws)
    a.norm_flags, a.norm_eps = 0, 1e-6
    for mode in ("0", "1"):       # the 32-query and the 64-query dQ kernel
        ops.attn_tune("dq64=" + mode)
        try:
            run(L.lib.qfx_attn_bwd_dq, [dqkv, dsum, parts[1]])
        finally:
            ops.attn_tune("dq64=auto")
    run(L.lib.qfx_attn_bwd_dkv, [dqkv, parts[2], parts[3]])
    # round 6: the one-pass backward (dQ accumulated across key blocks in a fixed order) -- every output, and the turn counters back at zero
    ws_ = ops.attn_bwd_fused_workspace(a)
    assert ws_ is not None
    run(L.lib.qfx_attn_bwd_fused, [dqkv, dsum, parts[1], parts[2], parts[3]])
    assert int(ws_[1].abs().max()) == 0


@pytest.mark.parametrize("S,H,Bn,mask,R", [(2432, 24, 1, 0, 16), (333, 2, 2, 0, 16), (333, 2, 2, 1, 0), (200, 3, 2, 2, 32), (64, 1, 1, 0, 0), (1000, 4, 1, 0, 16),
                                          (257, 2, 1, 1, 16), (4608, 24, 1, 0, 0)])
@pytest.mark.parametrize("form", ["1", "1p"], ids=["skewed", "subtile-pipeline"])
def test_attention_fwd64_matches_sdpa_and_the_32_query_kernel(S, H, Bn, mask, R, form, monkeypatch):
    """Round 5: qfx_attn_fwd on the 64-query / 32x32x16 kernel (qfx_attn64.hip; forced with QFX_ATTN_FWD64=1, the launcher's own policy
    only takes it where its 256-query blocks fill the CUs) against fp32 SDPA and against the 32-query kernels (QFX_ATTN_FWD64=0) on the
    same inputs: ragged S, additive and -inf key masks, several heads / samples, the fused rank-r projection of the epilogue."""
    import ctypes as C
    import math
    from qflux_amd import _lib as L
    ops = _ops()
    dh = 128
    D = H * dh
    S_pad = (S + 63) // 64 * 64
    T = 48 if S > 64 else 16
    g = torch.Generator(device=DEV).manual_seed(S + H)
    qkv = torch.randn(Bn, S, 3 * D, device=DEV, generator=g).to(torch.bfloat16)
    ld = 3 * D
    kmask = None
    if mask:
        kmask = torch.zeros(Bn, S, device=DEV)
        kmask[:, S - S // 5:] = -1e4 if mask == 1 else float("-inf")
    wpk = None
    if R:
        wts = [(torch.randn(R, D, device=DEV, generator=g) * 0.1).to(torch.bfloat16) for _ in range(4)]
        wpk = [L.head_fragment_image(wts[0], wts[1], dh), L.head_fragment_image(wts[2], wts[3], dh)]
    res = {}
    for mode in ("0", "1"):
        ops.attn_tune("fwd64=" + (mode if mode == "0" else form))      # reset after the test by conftest's _reset_attn_policy
        O = torch.zeros(Bn, S, D, dtype=torch.bfloat16, device=DEV)
        lse2 = torch.zeros(Bn, H, S_pad, device=DEV)
        part = torch.zeros(H, Bn * S, max(R, 1), device=DEV)
        a = ops.attn_args(Bn, S, S_pad, H, dh, 1 / math.sqrt(dh), Q=qkv[:, :, :D], K=qkv[:, :, D:2 * D], V=qkv[:, :, 2 * D:], ldq=ld, ldk=ld, ldv=ld,
                          O=O, ldo=D, lse2=lse2)
        if kmask is not None:
            a.key_mask = kmask.data_ptr()
        a.T = T
        if R:
            hl = a.hl[0]
            hl.part, hl.part_hstride, hl.ld_part, hl.c0, hl.R = part.data_ptr(), Bn * S * R, R, 0, R
            hl.w_pk[0], hl.w_pk[1] = wpk[0].data_ptr(), wpk[1].data_ptr()
        L.check(L.lib.qfx_attn_fwd(C.byref(a), ops.stream_ptr()), "qfx_attn_fwd")
        torch.cuda.synchronize()
        res[mode] = (O.float(), lse2[:, :, :S].clone(), part.clone())
    q, k, v = (qkv[:, :, i * D:(i + 1) * D].float().view(Bn, S, H, dh).transpose(1, 2) for i in range(3))
    sc = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    if kmask is not None:
        sc = sc + kmask[:, None, None, :]
    ref = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(Bn, S, D)
    lse_ref = torch.logsumexp(sc, -1) * 1.4426950408889634

    def rel(x, y):
        return ((x - y).abs().max() / (y.abs().max() + 1e-12)).item()
    new, old = res["1"], res["0"]
    assert torch.isfinite(new[0]).all()
    e_new, e_old = rel(new[0], ref), rel(old[0], ref)
    assert e_new < 6e-3 and e_new <= 1.25 * e_old + 1e-4, (e_new, e_old)          # bf16 output: ~2^-8 of the largest value
    assert rel(new[1], lse_ref) < 1e-5                                            # fp32 statistics
    assert rel(new[0], old[0]) < 6e-3
    if R:
        assert rel(new[2], old[2]) < 5e-3                                         # rank-r partial sums of bf16 O rows that differ by an ulp (3.1e-3 observed for the sub-tile form)


@pytest.mark.parametrize("S,H,Bn,mask,R", [(2432, 24, 1, 0, 16), (333, 2, 2, 0, 16), (333, 2, 2, 1, 0), (200, 3, 2, 2, 32), (64, 1, 1, 0, 0), (257, 2, 1, 1, 16)])
def test_attention_dq64_matches_autograd_and_the_32_query_kernel(S, H, Bn, mask, R, monkeypatch):
    """Round 5: qfx_attn_bwd_dq on the 64-query kernel (QFX_ATTN_DQ64=1) against the 32-query kernel (=0): plain mode against an fp32
    autograd reference of SDPA, fused mode (QK-norm + RoPE backward epilogue, fused rank-r projection) against the 32-query kernel;
    dsum is published identically."""
    import ctypes as C
    import math
    from qflux_amd import _lib as L
    ops = _ops()
    dh = 128
    D = H * dh
    S_pad = (S + 63) // 64 * 64
    T = 48 if S > 64 else 16
    g = torch.Generator(device=DEV).manual_seed(S + 3 * H)
    qkv = torch.randn(Bn, S, 3 * D, device=DEV, generator=g).to(torch.bfloat16)
    dO = torch.randn(Bn, S, D, device=DEV, generator=g).to(torch.bfloat16)
    sqk = torch.randn(Bn, S, 2 * D, device=DEV, generator=g).to(torch.bfloat16)
    ang = torch.rand(S, dh // 2, device=DEV, generator=g) * 6.28
    rope = torch.stack([ang.cos(), ang.sin()], -1).contiguous()
    ws = [(1 + 0.1 * torch.randn(dh, device=DEV, generator=g)).to(torch.bfloat16) for _ in range(4)]
    ld = 3 * D
    kmask = None
    if mask:
        kmask = torch.zeros(Bn, S, device=DEV)
        kmask[:, S - S // 5:] = -1e4 if mask == 1 else float("-inf")
    wpk = None
    if R:
        wts = [(torch.randn(R, D, device=DEV, generator=g) * 0.1).to(torch.bfloat16) for _ in range(2)]
        wpk = [L.head_fragment_image(wts[0], wts[1], dh), L.head_fragment_image(wts[1], wts[0], dh)]
    res = {}
    for fused in (0, 1):
        for mode in ("0", "1"):
            ops.attn_tune("dq64=" + mode)      # reset after the test by conftest's _reset_attn_policy
            O = torch.zeros(Bn, S, D, dtype=torch.bfloat16, device=DEV)
            lse2 = torch.zeros(Bn, H, S_pad, device=DEV)
            dsum = torch.zeros(Bn, H, S_pad, device=DEV)
            dqkv = torch.zeros_like(qkv)
            part = torch.zeros(H, Bn * S, max(R, 1), device=DEV)
            a = ops.attn_args(Bn, S, S_pad, H, dh, 1 / math.sqrt(dh), Q=qkv[:, :, :D], K=qkv[:, :, D:2 * D], V=qkv[:, :, 2 * D:], ldq=ld, ldk=ld, ldv=ld,
                              O=O, ldo=D, lse2=lse2, dsum=dsum, dO=dO, lddo=D, dQ=dqkv[:, :, :D], dK=dqkv[:, :, D:2 * D], dV=dqkv[:, :, 2 * D:],
                              lddq=ld, lddk=ld, lddv=ld)
            if kmask is not None:
                a.key_mask = kmask.data_ptr()
            a.T = T
            L.check(L.lib.qfx_attn_fwd(C.byref(a), ops.stream_ptr()), "qfx_attn_fwd")
            if fused:
                a.qk_saved, a.ld_saved, a.rope, a.rope_bstride = sqk.data_ptr(), 2 * D, rope.data_ptr(), 0
                a.wq_txt, a.wk_txt, a.wq_img, a.wk_img = (t.data_ptr() for t in ws)
                a.norm_flags, a.norm_eps = 0, 1e-6
                if R:
                    hl = a.hl[1]
                    hl.part, hl.part_hstride, hl.ld_part, hl.c0, hl.R = part.data_ptr(), Bn * S * R, R, 0, R
                    hl.w_pk[0], hl.w_pk[1] = wpk[0].data_ptr(), wpk[1].data_ptr()
            L.check(L.lib.qfx_attn_bwd_dq(C.byref(a), ops.stream_ptr()), "qfx_attn_bwd_dq")
            torch.cuda.synchronize()
            res[(fused, mode)] = (dqkv[:, :, :D].float().clone(), dsum[:, :, :S].clone(), part.clone())
    q, k, v = (qkv[:, :, i * D:(i + 1) * D].float().view(Bn, S, H, dh).transpose(1, 2).detach().requires_grad_(i == 0) for i in range(3))
    sc = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    if kmask is not None:
        sc = sc + kmask[:, None, None, :]
    o = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(Bn, S, D)
    o.backward(dO.float())
    dq_ref = q.grad.transpose(1, 2).reshape(Bn, S, D)

    def rel(x, y):
        return ((x.float() - y.float()).abs().max() / (y.float().abs().max() + 1e-12)).item()
    e_new, e_old = rel(res[(0, "1")][0], dq_ref), rel(res[(0, "0")][0], dq_ref)
    assert torch.isfinite(res[(0, "1")][0]).all() and torch.isfinite(res[(1, "1")][0]).all()
    assert e_new < 8e-3 and e_new <= 1.25 * e_old + 1e-4, (e_new, e_old)
    assert rel(res[(0, "1")][1], res[(0, "0")][1]) < 1e-5                       # dsum (fp32)
    assert rel(res[(1, "1")][0], res[(1, "0")][0]) < 6e-3                       # fused epilogue: bf16 ulp of the largest value
    if R:
        assert rel(res[(1, "1")][2], res[(1, "0")][2]) < 3e-3


@pytest.mark.parametrize("seed", range(8))
def test_attention_shape_fuzz(seed):
    """Random sequence lengths around every tile edge of the three kernels (32 queries per wave, 64-key tiles, 128 / 256-query
    blocks, ragged tails of 1..63), batch 1-3, 1-5 heads, both head dims, with / without the additive key mask."""
    import random
    rnd = random.Random(500 + seed)
    dh = rnd.choice([64, 128])
    S = rnd.choice([1, 2, 31, 33, 63, 65, 127, 129, 191, 255, 257, 383, 385, 511, 513, 700, 1025])
    Bn, H = rnd.choice([1, 2, 3]), rnd.choice([1, 2, 5])
    _attention_case(dh, S, rnd.random() < 0.4 and Bn >= 2 and S > 8, Bn, H)


def _attention_case(dh, S, mask, Bn, H):
    ops = _ops()
    D = H * dh
    qkv, do, km, S_pad = _attn_case(dh, S, Bn, H, mask)
    scale = 1.0 / math.sqrt(dh)
    x = qkv.float().requires_grad_(True)
    q, k, v = (x[:, :, i * D:(i + 1) * D].reshape(Bn, S, H, dh).transpose(1, 2) for i in range(3))
    am = km[:, None, None, :] if km is not None else None
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=am).transpose(1, 2).reshape(Bn, S, D)
    o.backward(do.float())
    qd = qkv.to(DEV)
    ld = 3 * D
    Q, K, V = qd[:, :, :D], qd[:, :, D:2 * D], qd[:, :, 2 * D:]
    Vt = ops.transpose_heads(V, ld, Bn, S, S_pad, H, dh)
    O = torch.empty(Bn, S, D, dtype=BF, device=DEV)
    lse2 = torch.zeros(Bn, H, S_pad, dtype=torch.float32, device=DEV)
    kmd = km.to(DEV) if km is not None else None
    a = ops.attn_args(Bn, S, S_pad, H, dh, scale, Q=Q, K=K, V=V, ldq=ld, ldk=ld, ldv=ld, Vt=Vt, O=O, ldo=D, lse2=lse2,
                      key_mask=kmd.data_ptr() if kmd is not None else None)
    ops.attn_call("qfx_attn_fwd", a)
    tag = f"fuzz_{dh}_{S}_{Bn}_{H}_{int(mask)}"
    check(f"attn_fwd_{tag}", O, o, 1e-2)
    dOd = do.to(DEV)
    Qt = ops.transpose_heads(Q, ld, Bn, S, S_pad, H, dh)
    Kt = ops.transpose_heads(K, ld, Bn, S, S_pad, H, dh)
    dOt = ops.transpose_heads(dOd, D, Bn, S, S_pad, H, dh)
    dsum = torch.zeros(Bn, H, S_pad, dtype=torch.float32, device=DEV)
    dqkv = torch.zeros(Bn, S, 3 * D, dtype=BF, device=DEV)
    a.Qt, a.Kt, a.dO, a.lddo, a.dOt, a.dsum = Qt.data_ptr(), Kt.data_ptr(), dOd.data_ptr(), D, dOt.data_ptr(), dsum.data_ptr()
    a.dQ, a.dK, a.dV = dqkv[:, :, :D].data_ptr(), dqkv[:, :, D:2 * D].data_ptr(), dqkv[:, :, 2 * D:].data_ptr()
    a.lddq = a.lddk = a.lddv = ld
    ops.attn_call("qfx_attn_bwd_prep", a)
    ops.attn_call("qfx_attn_bwd_dq", a)
    ops.attn_call("qfx_attn_bwd_dkv", a)
    g = x.grad
    check(f"attn_dq_{tag}", dqkv[:, :, :D], g[:, :, :D], 2e-2)
    check(f"attn_dk_{tag}", dqkv[:, :, D:2 * D], g[:, :, D:2 * D], 2e-2)
    check(f"attn_dv_{tag}", dqkv[:, :, 2 * D:], g[:, :, 2 * D:], 2e-2)
    ws = ops.attn_bwd_fused_workspace(a)      # round 6: the one-pass backward on the same shape (dh = 128, S >= 64)
    if ws is not None:
        dqkv.zero_(); dsum.zero_()
        ops.attn_call("qfx_attn_bwd_fused", a)
        check(f"attn1_dq_{tag}", dqkv[:, :, :D], g[:, :, :D], 2e-2)
        check(f"attn1_dk_{tag}", dqkv[:, :, D:2 * D], g[:, :, D:2 * D], 2e-2)
        check(f"attn1_dv_{tag}", dqkv[:, :, 2 * D:], g[:, :, 2 * D:], 2e-2)
        assert int(ws[1].abs().max()) == 0


@pytest.mark.parametrize("seed", range(12))
def test_gemm_shape_and_epilogue_fuzz(seed):
    """Random problem sizes around the tile edges of both tile shapes (M from 1 row up, N and K in steps of 8 / 64), every epilogue,
    with / without bias, LoRA K-extension (bf16 mid-rounding of the base output) and a row mask, vs the fp32 product with the
    eager graph's rounding points."""
    import random
    ops = _ops()
    rnd = random.Random(900 + seed)
    M = rnd.choice([1, 7, 16, 100, 255, 257, 384, 511, 1000, 2432])
    N = rnd.choice([64, 128, 192, 320, 1024, 3072, 6144])
    K = 64 * rnd.choice([1, 2, 3, 5, 16, 48])
    K2 = rnd.choice([0, 0, 64, 128])
    epi = rnd.choice([0, 1, 2, 3])
    use_bias = rnd.random() < 0.6
    a, b = randn(M, K, seed=seed).to(BF), randn(N, K, seed=seed + 1, scale=0.2).to(BF)
    bias = randn(N, seed=seed + 2).to(BF) if use_bias else None
    base = a.float() @ b.float().t() + (bias.float() if use_bias else 0.0)
    kw = {}
    if K2:
        a2, b2 = randn(M, K2, seed=seed + 3).to(BF), randn(N, K2, seed=seed + 4, scale=0.1).to(BF)
        h = rb(rb(base) + a2.float() @ b2.float().t())
        kw.update(a2=a2.to(DEV), b2=b2.to(DEV))
    else:
        h = rb(base)
    if epi == 0:
        ref = h
    elif epi == 1:       # GELU: C = h, C2 = gelu(h)
        ref = h
        out2 = torch.empty(M, N, dtype=BF, device=DEV)
        kw.update(out2=out2)
    elif epi == 2:       # gate * y + residual
        gate, res = randn(1, N, seed=seed + 5).to(BF), randn(M, N, seed=seed + 6).to(BF)
        ref = rb(res.float() + rb(gate.float() * h))
        kw.update(gate=gate.to(DEV), aux=res.to(DEV))
    else:                # dGELU: y * gelu'(aux)
        hx = randn(M, N, seed=seed + 7).to(BF)
        hh = hx.float().requires_grad_(True)
        F.gelu(hh, approximate="tanh").sum().backward()
        ref = rb(h * hh.grad)
        kw.update(aux=hx.to(DEV))
    out = ops.gemm(a.to(DEV), b.to(DEV), bias=bias.to(DEV) if use_bias else None, epi=epi, **kw)
    tag = f"gemm_fuzz_{M}x{N}x{K}+{K2}_epi{epi}"
    check(tag, out, ref, 1.5e-2)
    if epi == 1:
        check(tag + "_gelu", kw["out2"], rb(F.gelu(h, approximate="tanh")), 1.5e-2)


def test_mod_grad_batch_matches_column_sums_and_single_launches():
    """qfx_mod_grad(_batch): d(shift) = sum_rows dy, d(scale) = sum_rows dy * bf16(LN(x)), d(gate) = sum_rows dxo * y per sample --
    two problems of different row counts in ONE launch (one without the gate side, one with a row mask) vs fp32 torch and vs
    the same problems launched one by one."""
    import ctypes as C_
    from qflux_amd import _lib as L
    ops = _ops()
    D, Bn = 1024, 2
    g = torch.Generator().manual_seed(77)
    probs = []
    for rpb, gate, masked in ((40, True, False), (9, False, True)):
        rows = Bn * rpb
        dy = torch.randn(rows, D, generator=g).to(BF); x = (torch.randn(rows, D, generator=g) * 2 + 0.5).to(BF)
        dxo = torch.randn(rows, D, generator=g).to(BF); y = torch.randn(rows, D, generator=g).to(BF)
        mask = torch.ones(rows)
        if masked:
            mask[3] = 0; mask[rpb + 5] = 0
        probs.append(dict(rpb=rpb, rows=rows, gate=gate, dy=dy, x=x, dxo=dxo, y=y, mask=mask if masked else None))

    def run(batched):
        outs, args, keep = [], [], []
        for pr in probs:
            o = torch.zeros(Bn, 3 * D, device=DEV)
            a = L.ModGradArgs()
            t = {k: pr[k].to(DEV) for k in ("dy", "x", "dxo", "y")}
            keep.append(t)
            a.dy, a.ld_dy, a.x, a.ld_x = t["dy"].data_ptr(), D, t["x"].data_ptr(), D
            if pr["gate"]:
                a.dxo, a.ld_dxo, a.y, a.ld_y = t["dxo"].data_ptr(), D, t["y"].data_ptr(), D
                a.dgate = o.data_ptr() + 2 * D * 4
            a.dshift, a.dscale, a.out_bstride = o.data_ptr(), o.data_ptr() + D * 4, 3 * D
            if pr["mask"] is not None:
                mk = pr["mask"].to(DEV); keep.append(mk); a.row_mask = mk.data_ptr()
            a.rows, a.D, a.rows_per_batch, a.eps = pr["rows"], D, pr["rpb"], 1e-6
            outs.append(o); args.append(a)
        if batched:
            arr = (L.ModGradArgs * len(args))(*args)
            L.check(L.lib.qfx_mod_grad_batch(arr, len(args), ops.stream_ptr()), "batch")
        else:
            for a in args:
                L.check(L.lib.qfx_mod_grad(C_.byref(a), ops.stream_ptr()), "single")
        torch.cuda.synchronize()
        return [o.cpu() for o in outs]

    ob, os_ = run(True), run(False)
    for pi, pr in enumerate(probs):
        xf, dyf = pr["x"].float(), pr["dy"].float()
        xh = rb((xf - xf.mean(-1, keepdim=True)) * torch.rsqrt(xf.var(-1, unbiased=False, keepdim=True) + 1e-6))
        m = (pr["mask"] if pr["mask"] is not None else torch.ones(pr["rows"])).unsqueeze(-1)
        ref_shift = (dyf * m).view(Bn, pr["rpb"], D).sum(1)
        ref_scale = (dyf * xh * m).view(Bn, pr["rpb"], D).sum(1)
        check(f"mod_grad_shift_{pi}", ob[pi][:, :D], ref_shift, 1e-4)
        check(f"mod_grad_scale_{pi}", ob[pi][:, D:2 * D], ref_scale, 2e-3)
        if pr["gate"]:
            check(f"mod_grad_gate_{pi}", ob[pi][:, 2 * D:], (pr["dxo"].float() * pr["y"].float() * m).view(Bn, pr["rpb"], D).sum(1), 1e-4)
        else:
            assert ob[pi][:, 2 * D:].abs().max() == 0
        assert (ob[pi] - os_[pi]).abs().max().item() <= 1e-5 * ob[pi].abs().max().item()      # fp32 atomics: order only


# ------------------------------------------------------------------------------------------ criterion / optimizer
def test_flowmatch_and_mse():
    ops = _ops()
    Bn, S_t, S_c, Cc = 2, 24, 24, 64
    x0, noise, ctrl = (randn(Bn, S_t, Cc, seed=i).to(BF) for i in (1, 2, 3))
    sigma = torch.tensor([0.711, 0.161]).to(BF)
    sg = sigma.float().view(Bn, 1, 1)
    xt = rb(rb(rb(1 - sg) * x0.float()) + rb(sg * noise.float()))
    packed, target = ops.flowmatch_prepare(x0.to(DEV), noise.to(DEV), ctrl.to(DEV), sigma.to(DEV))
    assert torch.equal(packed[:, :S_t].float().cpu(), xt) and torch.equal(packed[:, S_t:].cpu(), ctrl)
    assert torch.equal(target.float().cpu(), rb(noise.float() - x0.float()))
    pred = randn(Bn, S_t + S_c, Cc, seed=5).to(BF)
    pp = pred.float().requires_grad_(True)
    el = (pp[:, :S_t] - target.float().cpu()) ** 2
    loss_ref = el.reshape(Bn, -1).mean(1).mean()
    loss_ref.backward()
    loss, dpred = ops.mse_loss_fwd_bwd(pred.to(DEV), target, S_t)
    check("mse_loss", loss.reshape(1), loss_ref.detach().reshape(1), 1e-5)
    check("mse_dpred", dpred, rb(pp.grad), 1e-2)


def test_adamw_matches_torch():
    ops = _ops()
    n = 10000
    p0, g0 = randn(n, seed=1), randn(n, seed=2) * 3
    p_ref = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([p_ref], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    p = p0.clone().to(DEV); m = torch.zeros(n, device=DEV); v = torch.zeros(n, device=DEV)
    nsq = torch.zeros((), device=DEV)
    for step in range(1, 4):
        g = g0 * step
        p_ref.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([p_ref], 1.0)
        opt.step()
        nsq.zero_()
        gd = g.to(DEV)
        ops.sumsq(gd, nsq)
        ops.adamw_step(p, gd, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, gnorm_sq=nsq, max_norm=1.0)
    check("adamw", p, p_ref.detach(), 1e-5)


def test_adam8bit_alias_is_adam_with_fp32_moments_and_deterministic_norm():
    """optimizer="adam8bit" (what most of the reference's YAMLs select: bitsandbytes.optim.Adam8bit(lr, betas)) = Adam without
    weight decay and with FP32 moments -- equal to torch.optim.Adam + clip_grad_norm_ on the same gradients; the global norm uses
    the deterministic reduction (same bits on every call, hence on every data-parallel replica)."""
    import torch.nn as nn
    from qflux_amd.modules import LoraStore, QfxLinear, QfxLoraLinear
    from qflux_amd.trainer import QwenLoraTrainStep, optimizer_kwargs_from_config
    ops = _ops()

    class Toy(nn.Module):
        def __init__(self):
            super().__init__()
            with torch.device(DEV):
                self.a = QfxLoraLinear(QfxLinear(256, 192), 16, 16, "ad")
                self.b = QfxLoraLinear(QfxLinear(192, 320), 16, 16, "ad")
            self._store = LoraStore(self)
            self._store.rebuild(DEV)
            self.device = torch.device(DEV)

        @property
        def lora_store(self):
            return self._store

    toy = Toy()
    st = toy.lora_store
    with torch.no_grad():
        st.pflat.copy_(randn(st.pflat.numel(), seed=3).to(DEV) * 0.1)
    step = QwenLoraTrainStep(toy, max_grad_norm=1.0, **optimizer_kwargs_from_config("bitsandbytes.optim.Adam8bit", {"lr": 1e-3, "betas": [0.9, 0.999]}))
    assert step.optimizer == "adamw" and step.optimizer_alias == "adam8bit" and step.weight_decay == 0.0
    ref = [p.detach().clone().cpu().requires_grad_(True) for _, p in st.params()]
    opt = torch.optim.Adam(ref, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    for k in range(1, 4):
        g = randn(st.gflat.numel(), seed=10 + k) * k
        st.gflat.copy_(g.to(DEV))
        for (_, p, off, n), r in zip(st.entries, ref):
            r.grad = g[off:off + n].view(r.shape).clone()
        torch.nn.utils.clip_grad_norm_(ref, 1.0)
        opt.step()
        step.optimizer_step()
    for (_, p, off, n), r in zip(st.entries, ref):
        check("adam8bit_alias", p.detach(), r.detach(), 1e-5)
    # the deterministic norm: identical bits on repeated evaluation, equal to the fp64 sum to fp32 accuracy
    gd = (randn(3_000_001, seed=5) * 2).to(DEV)
    o1, o2, parts = torch.zeros((), device=DEV), torch.zeros((), device=DEV), torch.zeros(1024, device=DEV)
    ops.sumsq_det(gd, o1, parts); ops.sumsq_det(gd, o2, parts)
    assert torch.equal(o1, o2) and abs(o1.item() - gd.double().pow(2).sum().item()) / o1.item() < 1e-5


@pytest.mark.parametrize("D,rows,R,rpb", [(256, 100, 16, 50), (1024, 77, 48, 77), (3072, 2048, 48, 2048), (3072, 2432, 16, 1216)])
def test_ln_down_fused_matches_the_two_separate_launches(D, rows, R, rpb):
    """qfx_ln_down_fwd == qfx_ln_modulate_fwd followed by qfx_lora_down (K-extension image, transposed split image, y)."""
    import ctypes as C
    from qflux_amd import _lib as L
    ops = _ops()
    B = rows // rpb
    x = randn(rows, D, seed=1, scale=2.0).to(BF).to(DEV)
    mod = (randn(B, 2 * D, seed=2) * 0.3).to(BF).to(DEV)
    A = randn(R, D, seed=3, scale=0.05)
    a_hi, a_lo = _split(A)
    a_hi, a_lo = a_hi.to(DEV), a_lo.to(DEV)
    gR, gS = (16, 64) if R == 48 else (R, 0)
    mp = (rows + 127) // 128 * 128
    outs = []
    w_fr = L.down_fragment_image(a_hi, a_lo)      # ABI 6: the same weights in MFMA-fragment order
    for fused in (False, True, "fragment image"):
        y = torch.empty(rows, D, dtype=BF, device=DEV)
        ext = torch.zeros(rows, 3 * 64, dtype=BF, device=DEV)
        ut = (torch.zeros(R, mp, dtype=BF, device=DEV), torch.zeros(R, mp, dtype=BF, device=DEV))
        if not fused:
            L.check(ops.lib.qfx_ln_modulate_fwd(x.data_ptr(), mod[:, :D].data_ptr(), mod[:, D:].data_ptr(), 2 * D, y.data_ptr(), rows, D, rpb, 1e-6,
                                                ops.stream_ptr()), "ln")
            ops.lora_down(y, a_hi, a_lo, ext=ext, Ut=ut, group_R=gR, group_stride=gS)
        else:
            arr = (L.LnDownArgs * 2)()
            # problem 0: adapted rows; problem 1: the same rows again as a plain LayerNorm problem (W_hi = NULL) into a scratch output
            y2 = torch.empty(rows, D, dtype=BF, device=DEV)
            for i, (yy, adapted) in enumerate(((y, True), (y2, False))):
                a = arr[i]
                a.ln.x, a.ln.shift, a.ln.scale, a.ln.mod_bstride, a.ln.y = x.data_ptr(), mod[:, :D].data_ptr(), mod[:, D:].data_ptr(), 2 * D, yy.data_ptr()
                a.ln.rows, a.ln.D, a.ln.rows_per_batch, a.ln.eps = rows, D, rpb, 1e-6
                if adapted:
                    a.W_hi, a.W_lo, a.ldw, a.R = a_hi.data_ptr(), a_lo.data_ptr(), D, R
                    if fused == "fragment image":
                        a.W_fr = w_fr.data_ptr()
                    a.ext, a.ld_ext = ext.data_ptr(), ext.stride(0)
                    a.Ut_hi, a.Ut_lo, a.ld_ut = ut[0].data_ptr(), ut[1].data_ptr(), mp
                    a.group_R, a.group_stride = gR, gS
            L.check(ops.lib.qfx_ln_down_fwd(arr, 2, ops.stream_ptr()), "ln_down")
            torch.cuda.synchronize()
            assert torch.equal(y, y2)
        torch.cuda.synchronize()
        outs.append((y.float().cpu(), ext.float().cpu(), ut[0].float().cpu() + ut[1].float().cpu()))
    (y0, e0, u0), (y1, e1, u1), (y2_, e2, u2) = outs
    assert torch.equal(y1, y2_) and torch.equal(e1, e2) and torch.equal(u1, u2)      # the fragment image changes the loads, not a bit of the result
    # y: same rounding points; the fp32 row statistics are summed in another order -> at most one bf16 ulp on rare elements
    ny = (y0 != y1).float().mean().item()
    assert ny < 2e-3 and ((y0 - y1).abs().max() / y0.abs().max()).item() < 1e-2, ny
    # u (hi + lo ~ fp32): relative to its scale
    assert ((u0 - u1).abs().max() / u0.abs().max()).item() < 2e-3
    assert ((e0 - e1).abs().max() / e0.abs().max()).item() < 8e-3
    assert mp == rows or u1[:, rows:].abs().max().item() == 0.0


def test_package_import_before_torch_still_launches():
    """`import qflux_amd` in a process that has not imported torch yet: the binding imports torch first so that libqfx.so binds to the
    HIP runtime bundled with the PyTorch wheel (two runtimes in one process = hipErrorNoDevice on every launch; round 4)."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import qflux_amd; from qflux_amd import ops; import torch; "
            "a = torch.randn(256, 128, device='cuda').bfloat16(); b = torch.randn(256, 128, device='cuda').bfloat16(); "
            "o = ops.gemm(a, b); torch.cuda.synchronize(); "
            "assert (o.float() - a.float() @ b.float().t()).abs().max().item() < 0.5; print('OK')") % os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qwen-image-finetune_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stderr[-800:]
