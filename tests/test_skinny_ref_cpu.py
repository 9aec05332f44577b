"""CPU: tests/skinny_ref.py against explicit loops on tiny sizes, the exactness guarantee of exact_case that the GPU assertions of
tests/test_skinny_gpu.py rest on, and the argument refusals of the rank-r LoRA entry points (calls that return before any launch)."""
import ctypes as C
import os

import pytest
import torch

import skinny_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def _bf(x):
    """fp32 -> bf16 round-to-nearest-even on the bit pattern, independent of torch's conversion."""
    u = torch.tensor([x], dtype=torch.float32).view(torch.int32).item() & 0xFFFFFFFF
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return torch.tensor([u << 16 if u < 0x8000 else (u << 16) - (1 << 32)], dtype=torch.int32).view(torch.float32).item()


def _split_loop(v):
    hi = _bf(v)
    return hi, _bf(torch.tensor(v, dtype=torch.float32).item() - hi)


@pytest.mark.parametrize("M,rpb,batch_rows,off", [(7, 7, 0, 0), (10, 4, 9, 3), (12, 4, 4, 0), (5, 8, 20, 2)])
def test_remap_rows_matches_the_loop(M, rpb, batch_rows, off):
    want = []
    for m in range(M):
        if batch_rows == 0:
            want.append(m)
        elif m < rpb:
            want.append(off + m)
        else:
            b = m // rpb
            want.append(b * batch_rows + off + (m - b * rpb))
    assert S.remap_rows(M, rpb, batch_rows, off).tolist() == want


def test_down_and_images_match_the_loops():
    M, K, R, gR, gs, ld_ext, ld_ut, ldx = 5, 32, 32, 16, 52, 110, 9, 40
    X, hi, lo = S.rand_case(3, (12, ldx), (R, K))
    rows = S.remap_rows(M, 3, 6, 2)
    U = S.down_ref(X, hi, lo, rows)
    for m in range(M):
        for j in range(R):
            acc = 0.0
            for k in range(K):
                acc += float(X[int(rows[m]), k]) * (float(hi[j, k]) + float(lo[j, k]))
            assert abs(U[m, j].item() - acc) <= 1e-12 * max(1.0, abs(acc))
    U32 = U.float()
    ext = S.ext_image(U32, gR, gs, ld_ext)
    uth, utl = S.ut_image(U32, ld_ut)
    written = torch.zeros(M, ld_ext, dtype=torch.bool)
    for m in range(M):
        for j in range(R):
            h, l = _split_loop(U32[m, j].item())
            c = (j // gR) * gs + j % gR
            assert ext[m, c].item() == h and ext[m, c + gR].item() == l and ext[m, c + 2 * gR].item() == h
            written[m, c] = written[m, c + gR] = written[m, c + 2 * gR] = True
            assert uth[j, m].item() == h and utl[j, m].item() == l
            assert h + l == pytest.approx(U32[m, j].item(), rel=2.0 ** -15)
    assert (S.bits(ext)[~written] == S.CANARY_BF16).all() and written.sum() == 3 * M * R
    assert (S.bits(uth)[:, M:] == S.CANARY_BF16).all() and (S.bits(utl)[:, M:] == S.CANARY_BF16).all()
    assert (S.bits(S.ut_image(U32, ld_ut, fill=0)[0])[:, M:] == 0).all()


def test_grad_ref_matches_the_loop():
    M, K, R, gR, rv = 6, 8, 32, 16, 5
    X, hi, lo = S.rand_case(4, (14, K), (R, M + 3), w_scale=1.0)
    rows = S.remap_rows(M, 3, 7, 1)
    G = S.grad_ref(hi, lo, X, rows, gR, rv)
    assert len(G) == 2 and all(g.shape == (rv, K) and g.dtype == torch.float64 for g in G)
    for grp in range(2):
        for jj in range(rv):
            for k in range(K):
                acc = 0.0
                for m in range(M):
                    j = grp * gR + jj
                    acc += (float(hi[j, m]) + float(lo[j, m])) * float(X[int(rows[m]), k])
                assert abs(G[grp][jj, k].item() - acc) <= 1e-12 * max(1.0, abs(acc))


def test_pack_ref_matches_the_loops():
    r, Rp, K, N, Kext, s = 5, 16, 6, 7, 64, 1.5
    g = torch.Generator().manual_seed(5)
    A, B = torch.randn(r, K, generator=g), torch.randn(N, r, generator=g)
    p = S.pack_ref(A, B, r, Rp, Kext, s)
    assert p["A_hi"].shape == (Rp, K) and p["Bt_lo"].shape == (Rp, N) and p["We"].shape == (N, Kext) and p["WeT"].shape == (K, Kext)
    for j in range(Rp):
        for k in range(K):
            h, l = _split_loop(A[j, k].item()) if j < r else (0.0, 0.0)
            assert p["A_hi"][j, k].item() == h and p["A_lo"][j, k].item() == l
            assert p["WeT"][k, j].item() == h and p["WeT"][k, Rp + j].item() == h and p["WeT"][k, 2 * Rp + j].item() == l
        for n in range(N):
            sb = (torch.tensor(s, dtype=torch.float32) * B[n, j]).item() if j < r else 0.0
            h, l = _split_loop(sb)
            assert p["Bt_hi"][j, n].item() == h and p["Bt_lo"][j, n].item() == l
            assert p["We"][n, j].item() == h and p["We"][n, Rp + j].item() == h and p["We"][n, 2 * Rp + j].item() == l
    assert (S.bits(p["We"])[:, 3 * Rp:] == 0).all() and (S.bits(p["WeT"])[:, 3 * Rp:] == 0).all()
    assert (S.bits(p["A_hi"])[r:] == 0).all() and (S.bits(p["Bt_lo"])[r:] == 0).all()


def test_exact_case_values_are_what_the_docstring_says():
    X, hi, lo = S.exact_case(1, (64, 96), (48, 96))
    for t, unit in ((X, 1.0), (hi, 1.0), (lo, 2.0 ** -4)):
        v = t.double() / unit
        assert (v == v.round()).all() and v.abs().max() == 2 and len(v.unique()) == 5


@pytest.mark.parametrize("what,n", [("down", S.EXACT_MAX_K), ("grad", S.EXACT_MAX_M)])
def test_exact_case_sums_are_exact_in_fp32_in_any_order(what, n):
    """The GPU tests demand bit equality with the fp64 sum on exact_case data: the fp32 sum of the products, hi and lo parts apart as
    the kernels' two MFMAs add them, under three random permutations of the contraction index (sequential, each partial sum rounded to
    fp32 -- and torch's own blocked matmul as a fourth order) equals the fp64 sum at the longest contraction the GPU tests use."""
    R, other = 16, 8
    if what == "down":
        X, hi, lo = S.exact_case(11, (other, n), (R, n))          # contraction over K = n
        xa, ha, la = X.float().t(), hi.float().t(), lo.float().t()   # [n, other], [n, R]
    else:
        X, hi, lo = S.exact_case(12, (n, other), (R, n))          # contraction over tokens
        xa, ha, la = X.float(), hi.float().t(), lo.float().t()
    ref = xa.double().t() @ (ha.double() + la.double())             # [other, R]
    assert (ref.float().double() == ref).all()
    g = torch.Generator().manual_seed(13)
    for _ in range(3):
        perm = torch.randperm(n, generator=g)
        acc = torch.zeros(other, R, dtype=torch.float32)
        for i in perm.tolist():
            acc += xa[i].view(-1, 1) * ha[i].view(1, -1)
            acc += xa[i].view(-1, 1) * la[i].view(1, -1)
        assert torch.equal(acc.double(), ref)
    assert torch.equal((xa.t() @ ha + xa.t() @ la).double(), ref)
    # the worst case of the value ranges, not just of one draw: every product at its largest magnitude
    worst = n * (2 * 2 + 2 * 2 * 2.0 ** -4)
    assert worst * 16 < 2 ** 24 and float(torch.tensor(worst, dtype=torch.float32)) == worst


# ------------------------------------------------------------------------------------------ argument refusal (no launch is reached)
def _lib():
    if not os.path.exists(os.path.join(ROOT, "qwen-image-finetune_amd", "qflux_amd", "libqfx.so")):
        import __graft_entry__ as g
        g.build()
    from qflux_amd import _lib
    return _lib


def _down(L, **kw):
    a = L.LoraDownArgs()
    a.X, a.ldx, a.M, a.K = 0x1000, 64, 40, 64
    a.W_hi, a.W_lo, a.ldw, a.R = 0x2000, 0x3000, 64, 16
    a.U, a.ldu = 0x4000, 16
    a.group_R, a.group_stride, a.rows_per_batch = 16, 0, 40
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _grad(L, **kw):
    g = L.LoraGradArgs()
    g.Vt_hi, g.Vt_lo, g.ldvt, g.R, g.r_valid, g.group_R = 0x1000, 0x2000, 64, 16, 16, 16
    g.X, g.ldx, g.M, g.K, g.G, g.g_sr, g.g_sc, g.rows_per_batch = 0x3000, 64, 40, 64, 0x4000, 64, 1, 40
    g.out_scale = 1.0
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _arr(ct, items):
    return (ct * len(items))(*items)


def test_batch_entries_refuse_bad_counts_and_mixed_or_unsupported_ranks():
    L = _lib()
    down, grad = L.lib.qfx_lora_down_batch, L.lib.qfx_lora_grad_batch
    d9, g9 = _arr(L.LoraDownArgs, [_down(L) for _ in range(9)]), _arr(L.LoraGradArgs, [_grad(L) for _ in range(9)])
    for n in (0, 9, -1):
        assert down(d9, n, None) == L.QFX_EINVAL and grad(g9, n, None) == L.QFX_EINVAL
    assert down(None, 1, None) == L.QFX_EINVAL and grad(None, 1, None) == L.QFX_EINVAL
    # one MFMA fragment count per launch: a second problem of another rank
    assert down(_arr(L.LoraDownArgs, [_down(L), _down(L, R=32, group_R=32)]), 2, None) == L.QFX_EINVAL
    assert grad(_arr(L.LoraGradArgs, [_grad(L), _grad(L, R=32, group_R=32, r_valid=32)]), 2, None) == L.QFX_EINVAL
    # a rank the dispatch has no instantiation for (R / 16 = 5), alone and batched
    assert down(_arr(L.LoraDownArgs, [_down(L, R=80, group_R=80)]), 1, None) == L.QFX_EUNSUPPORTED
    assert L.lib.qfx_lora_down(C.byref(_down(L, R=80, group_R=80)), None) == L.QFX_EUNSUPPORTED
    assert grad(_arr(L.LoraGradArgs, [_grad(L, R=80, group_R=80, r_valid=80)] * 2), 2, None) == L.QFX_EUNSUPPORTED
    assert L.lib.qfx_lora_grad(C.byref(_grad(L, R=80, group_R=80, r_valid=80)), None) == L.QFX_EUNSUPPORTED
    # a bad problem behind good ones is found before anything is launched
    assert down(_arr(L.LoraDownArgs, [_down(L), _down(L), _down(L, K=48)]), 3, None) == L.QFX_EINVAL
    assert grad(_arr(L.LoraGradArgs, [_grad(L), _grad(L), _grad(L, K=60)]), 3, None) == L.QFX_EINVAL


def test_down_refuses_shapes_it_cannot_run():
    L = _lib()
    f = lambda **kw: L.lib.qfx_lora_down(C.byref(_down(L, **kw)), None)   # noqa: E731
    assert f(K=48) == L.QFX_EINVAL and f(K=0) == L.QFX_EINVAL                      # K % 32
    assert f(Ut_hi=0x5000, Ut_lo=0x6000, ld_ut=39) == L.QFX_EINVAL                 # ld_ut < M
    assert f(Ut_hi=0x5000, Ut_lo=None, ld_ut=64) == L.QFX_EINVAL
    assert f(ext=0x5000, ld_ext=64, group_R=12) == L.QFX_EINVAL                    # R % group_R
    assert f(M=0) == L.QFX_EINVAL and f(rows_per_batch=0) == L.QFX_EINVAL and f(ldx=66) == L.QFX_EINVAL and f(R=24) == L.QFX_EINVAL
    assert f(X=None) == L.QFX_EINVAL and f(W_lo=None) == L.QFX_EINVAL
    assert L.lib.qfx_lora_down(None, None) == L.QFX_EINVAL


def test_grad_refuses_shapes_it_cannot_run():
    L = _lib()
    f = lambda **kw: L.lib.qfx_lora_grad(C.byref(_grad(L, **kw)), None)   # noqa: E731
    assert f(K=60) == L.QFX_EINVAL                                                 # K % 8
    assert f(M=40, ldvt=56) == L.QFX_EINVAL and f(M=33, ldvt=56) == L.QFX_EINVAL   # ldvt < roundup(M, 32) = 64
    assert f(ldvt=68) == L.QFX_EINVAL                                              # ldvt % 8
    assert f(R=48, G1=0x5000, G2=None) == L.QFX_EINVAL                             # a third group without G2
    assert f(R=32, G1=None) == L.QFX_EINVAL
    assert f(R=64, G1=0x5000, G2=0x6000) == L.QFX_EINVAL                           # four groups
    need = L.lib.qfx_lora_grad_ws_floats(1025, 200, 48)
    assert need == 3 * 2 * 3 * 2048
    big = dict(M=1025, rows_per_batch=1025, ldvt=1056, K=200, ldx=200, R=48, group_R=48, r_valid=48)
    assert f(**big, ws=0x7000, ws_count=0x8000, ws_floats=need - 1) == L.QFX_EINVAL   # one float short
    assert f(**big, ws=0x7000, ws_count=None, ws_floats=need) == L.QFX_EINVAL
    assert f(**big, ws=0x7004, ws_count=0x8000, ws_floats=need) == L.QFX_EINVAL       # 16-byte alignment of the scratch
    assert L.lib.qfx_lora_grad_ws_floats(512, 200, 48) == 0 and L.lib.qfx_lora_grad_ws_floats(513, 128, 96) == 2 * 1 * 6 * 2048
    assert L.lib.qfx_lora_grad(None, None) == L.QFX_EINVAL


def test_head_reduce_refuses_descriptors_that_do_not_cover_its_accesses():
    L = _lib()

    def f(n=1, **kw):
        r = L.LoraHeadReduceArgs()
        r.part, r.part_hstride, r.ld_part, r.H, r.M, r.R = 0x1000, 40 * 100, 100, 25, 40, 96
        r.ext, r.ld_ext, r.group_R, r.group_stride, r.rows_per_batch = 0x2000, 2 * 104 + 96, 32, 104, 40
        for k, v in kw.items():
            setattr(r, k, v)
        return L.lib.qfx_lora_head_reduce(_arr(L.LoraHeadReduceArgs, [r] * n), n, None)
    assert f(n=0) == L.QFX_EINVAL and f(n=3) == L.QFX_EINVAL
    assert f(ld_part=95, part_hstride=40 * 95) == L.QFX_EINVAL                     # ld_part < R
    assert f(ld_ext=2 * 104 + 95) == L.QFX_EINVAL                                  # the third group's last column is outside the row
    assert f(group_stride=-8) == L.QFX_EINVAL
    assert f(part_hstride=40 * 100 - 1) == L.QFX_EINVAL                            # a slab shorter than the last row read
    # two samples of 20 rows at joint rows 5..24 and 35..54: the last row read is 54
    remap = dict(rows_per_batch=20, x_batch_rows=30, x_row_off=5)
    assert f(**remap, part_hstride=55 * 100 - 1) == L.QFX_EINVAL
    assert f(**dict(remap, x_row_off=-1), part_hstride=55 * 100) == L.QFX_EINVAL
    assert f(ext=None, Ut_hi=0x3000, Ut_lo=0x4000, ld_ut=39) == L.QFX_EINVAL       # ld_ut < M
    assert f(ext=None) == L.QFX_EINVAL and f(Ut_hi=0x3000) == L.QFX_EINVAL         # nothing to write / half a split
    assert f(R=272, group_R=272, ld_part=272, part_hstride=40 * 272, ld_ext=3 * 272) == L.QFX_EINVAL   # more columns than a block has threads
