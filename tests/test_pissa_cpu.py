"""CPU: the numpy restatement of the PiSSA pieces (tests/pissa_ref.py) against plain fp64 algebra, the parsing of peft's option
strings, the host-side refusals of qfx_lora_fold, and the plumbing of qflux_amd.pissa with the device part replaced by the
restatement."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pissa_ref as P  # noqa: E402
from lora_dropout_ref import bf16_float, bf16_rne  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


# ------------------------------------------------------------------ the restatement

def test_bf16_rounding_is_nearest_even_including_ties():
    one = np.float32(1.0).view(np.uint32)
    for low, want in ((0x7FFF, 0), (0x8000, 0), (0x8001, 1), (0x18000, 2), (0x17FFF, 1), (0x28000, 2)):     # ties go to the even mantissa
        x = np.array([one + np.uint32(low)], dtype=np.uint32).view(np.float32)
        assert int(bf16_rne(x)[0]) == (int(one) >> 16) + want, hex(low)
    x = np.array([-1.00390625, 3.0e38, 0.0, -0.0], dtype=np.float32)                     # a negative tie, a large value, both zeros
    got = bf16_float(bf16_rne(x))
    assert got[0] == np.float32(-1.0) and np.isfinite(got[1]) and got[2] == 0 and np.signbit(got[3]) and not np.signbit(got[2])


@pytest.mark.parametrize("dtype", [P.FP32, P.BF16])
@pytest.mark.parametrize("shape", [(5, 7, 3), (33, 20, 16), (1, 1, 1), (9, 4, 64)])
def test_fold_restatement_against_plain_fp64(dtype, shape):
    """w' differs from the exact W + c B A by at most r + 2 fp64 roundings of magnitudes |c| sum |B||A| and |w'|; the stored
    value is then within half an fp32 ulp (and for bf16 within half an fp32 plus half a bf16 ulp) of w'."""
    nout, nin, r = shape
    rng = np.random.default_rng(nout * 100 + nin)
    A, B = rng.standard_normal((r, nin)).astype(np.float32), rng.standard_normal((nout, r)).astype(np.float32)
    W32 = rng.standard_normal((nout, nin)).astype(np.float32)
    W = bf16_rne(W32) if dtype == P.BF16 else W32
    Wv = (bf16_float(W) if dtype == P.BF16 else W).astype(np.float64)
    for c in (-0.5, 1.0, 0.0, -3.25):
        out = P.fold(W, A, B, c, dtype)
        assert out.dtype == (np.uint16 if dtype == P.BF16 else np.float32) and out.shape == W.shape
        got = (bf16_float(out) if dtype == P.BF16 else out).astype(np.float64)
        exact = Wv + c * (B.astype(np.float64) @ A.astype(np.float64))
        mag = np.abs(Wv) + abs(c) * (np.abs(B).astype(np.float64) @ np.abs(A).astype(np.float64))
        bound = (r + 2) * 2.0 ** -53 * mag + 2.0 ** -24 * np.abs(exact) + (2.0 ** -8 * np.abs(exact) if dtype == P.BF16 else 0.0)
        assert (np.abs(got - exact) <= bound * (1 + 1e-9) + 1e-300).all(), (c, float(np.abs(got - exact).max()))
        if c == 0.0:
            assert np.array_equal(out, W)


def test_fold_restatement_sums_in_ascending_order_from_plus_zero():
    A = np.array([[1.0], [2.0 ** -60], [-1.0]], dtype=np.float32)
    B = np.array([[1.0, 1.0, 1.0]], dtype=np.float32)
    # (1 + 2^-60) rounds to 1 in fp64, then - 1 = 0: ascending order loses the small term; any other order keeps it
    assert P.fold(np.zeros((1, 1), np.float32), A, B, 1.0)[0, 0] == 0.0
    out = P.fold(np.zeros((1, 1), np.float32), np.array([[-0.0]], np.float32), np.array([[1.0]], np.float32), 1.0)
    assert out[0, 0] == 0.0 and not np.signbit(out[0, 0])                                # +0 + (-0) = +0


def test_balanced_split_and_conversion_identities():
    rng = np.random.default_rng(1)
    W = P.planted(rng, 40, 56)
    for r, s in ((4, 2.0), (3, 0.5), (6, 1.0)):
        B0, A0, sig = P.split(W, r, s)
        U, S, Vt = np.linalg.svd(W, full_matrices=False)
        trunc = (U[:, :r] * S[:r]) @ Vt[:r]
        assert np.abs(s * B0 @ A0 - trunc).max() <= 64 * 2.0 ** -52 * S[0]
        assert np.abs(B0.T @ B0 - A0 @ A0.T).max() <= 64 * 2.0 ** -52 * S[0] / s
        assert np.abs(B0.T @ B0 - np.diag(S[:r] / s)).max() <= 64 * 2.0 ** -52 * S[0] / s
        assert abs(P.retained(sig, r) - np.sqrt((S[:r] ** 2).sum() / (S ** 2).sum())) <= 1e-15
        A, B = A0 + 0.01 * rng.standard_normal(A0.shape), B0 + 0.01 * rng.standard_normal(B0.shape)
        A2, B2, alpha2 = P.to_lora(A, B, A0, B0, s * r)
        assert A2.shape == (2 * r, 56) and B2.shape == (40, 2 * r) and alpha2 / (2 * r) == s
        want = s * (B @ A - B0 @ A0)
        assert np.abs((alpha2 / (2 * r)) * B2 @ A2 - want).max() <= 64 * 2.0 ** -52 * max(1.0, np.abs(want).max()) * r
    B0, A0, _ = P.split(np.zeros((5, 6)), 3, 2.0)                                        # sigma = 0: zero columns / rows, no division
    assert not B0.any() and not A0.any()
    B0, A0, _ = P.split(np.outer(np.arange(1.0, 4.0), np.ones(2)), 4, 1.0)               # r above min(out, in)
    assert B0.shape == (3, 4) and A0.shape == (4, 2) and not B0[:, 2:].any() and not A0[2:].any()


# ------------------------------------------------------------------ option strings

def test_option_parsing():
    from qflux_amd.pissa import parse_init
    assert parse_init("pissa") == 2
    for n in range(5):
        assert parse_init(f"pissa_niter_{n}") == n
    with pytest.raises(ValueError, match="4"):
        parse_init("pissa_niter_5")
    with pytest.raises(ValueError):
        parse_init("pissa_niter_")
    with pytest.raises(ValueError):
        parse_init("pissa_fast")
    for other in ("gaussian", True, False, "olora", "loftq", None, "kaiming"):
        assert parse_init(other) is None


def test_add_adapter_refuses_pissa_before_it_wraps_anything():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from common import TINY
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.modules import LoraConfig, QfxLoraLinear
    q = QwenImageTransformer2DModel(**TINY)
    with pytest.raises(ValueError, match="pissa_niter_4"):
        q.add_adapter(LoraConfig(r=4, lora_alpha=8, init_lora_weights="pissa_niter_5"), "a")
    with pytest.raises(RuntimeError, match="GPU"):                                      # weights on the CPU
        q.add_adapter(LoraConfig(r=4, lora_alpha=8, init_lora_weights="pissa"), "a")
    assert not any(isinstance(m, QfxLoraLinear) for m in q.modules()) and q._pissa is None
    q.add_adapter(LoraConfig(r=4, lora_alpha=8, init_lora_weights="gaussian"), "a")      # every other string as before
    assert all(not m.B.any() and m.A.any() for m in q.modules() if isinstance(m, QfxLoraLinear))
    with pytest.raises(RuntimeError, match="GPU"):
        q.pissa_init_()


# ------------------------------------------------------------------ the library's host side

def _mats(rows):
    from qflux_amd import _lib as L
    return (L.LoraFoldMat * len(rows))(*[L.LoraFoldMat(*r) for r in rows])


def _row(**kw):
    d = dict(w=0x10000, ld=16, off_a=0, off_b=64, r=4, nin=16, nout=8, dtype=0, c=-2.0)
    d.update(kw)
    return (d["w"], d["ld"], d["off_a"], d["off_b"], d["r"], d["nin"], d["nout"], d["dtype"], d["c"])


def test_fold_check_table():
    from qflux_amd import _lib as L
    chk = L.lib.qfx_lora_fold_check_table
    good = [_row(), _row(w=0x20000, off_a=100, off_b=200, r=64, nin=1, nout=1, dtype=1, ld=1)]
    assert chk(_mats(good), 2, 264) == 0 and chk(_mats(good), 2, 263) == EINVAL          # B of row 1 reaches past n_elems
    assert chk(_mats([_row(off_a=33)]), 1, 96) == EINVAL and chk(_mats([_row(off_a=32)]), 1, 96) == 0      # A reaches past n_elems
    assert chk(None, 0, 0) == 0 and chk(None, 1, 10) == EINVAL and chk(_mats(good), -1, 264) == EINVAL
    assert chk(_mats(good), 65536, 264) == EINVAL and chk(_mats(good), 2, -1) == EINVAL
    for bad in (dict(r=0), dict(r=65), dict(nin=0), dict(nin=(1 << 24) + 1, ld=1 << 25), dict(nout=0), dict(nout=(1 << 24) + 1),
                dict(ld=15), dict(dtype=2), dict(dtype=-1), dict(w=None), dict(off_a=-1), dict(off_b=-64)):
        assert chk(_mats([_row(**bad)]), 1, 1 << 40) == EINVAL, bad
    assert chk(_mats([_row(nin=1 << 24, nout=1 << 24, ld=1 << 24, r=1)]), 1, 1 << 40) == EINVAL      # more tiles than a flat grid holds
    wide = dict(nin=64 * 4096, ld=64 * 4096, r=1, off_b=1 << 20)                                     # 2^24 tiles: one above the cap
    assert chk(_mats([_row(nout=64 * 4096, **wide)]), 1, 1 << 40) == EINVAL and chk(_mats([_row(nout=64 * 4095, **wide)]), 1, 1 << 40) == 0
    assert chk(_mats([_row(), _row(off_a=0, off_b=64, w=0x10000 + (7 * 16 + 16) * 2)]), 2, 96) == 0  # A / B shared, W behind W
    assert chk(_mats([_row(), _row(w=0x10000 + (7 * 16 + 16) * 2 - 2)]), 2, 96) == EINVAL            # the W extents overlap by an element
    assert chk(_mats([_row(ld=32), _row(w=0x10000 + 32)]), 2, 96) == EINVAL                          # interleaved in the padding: refused
    assert chk(_mats([_row(c=float("nan"))]), 1, 96) == 0                                            # c is data


def test_fold_refusals_without_a_gpu():
    from qflux_amd import _lib as L
    fold = L.lib.qfx_lora_fold
    host = _mats([_row()])

    def args(**kw):
        d = dict(table=0x2000, host_table=C.cast(host, C.c_void_p), n_mats=1, reserved=0, p=0x40000, n_elems=96, tile_start=0x3000)
        d.update(kw)
        return L.LoraFoldArgs(**d)

    assert fold(None, None) == EINVAL
    for kw in (dict(n_mats=-1), dict(n_mats=65536), dict(table=None), dict(host_table=None), dict(p=None), dict(tile_start=None),
               dict(n_elems=95), dict(host_table=C.cast(_mats([_row(r=65)]), C.c_void_p)),
               dict(host_table=C.cast(_mats([_row(ld=15)]), C.c_void_p)), dict(host_table=C.cast(_mats([_row(w=None)]), C.c_void_p))):
        assert fold(C.byref(args(**kw)), None) == EINVAL, kw
    assert fold(C.byref(args(n_mats=0, table=None, host_table=None, p=None, tile_start=None)), None) == 0


def test_header_build_entry_and_abi():
    import __graft_entry__ as g
    from qflux_amd import _lib as L
    from qflux_amd import ops
    hdr = open(os.path.join(ROOT, "include", "qfx.h")).read()
    for name in ("qfx_lora_fold_check_table", "qfx_lora_fold"):
        assert name in L.SYMBOLS and f" {name}(" in hdr
    assert L.ABI_VERSION == 7 and L.lib.qfx_abi_version() == 7
    assert hdr.rindex("qfx_lowrank_sketch(") < hdr.index("qfx_lora_fold_mat")           # appended
    assert "THIS LISTING IS THE SPECIFICATION (tests/pissa_ref.py" in hdr
    assert C.sizeof(L.LoraFoldMat) == 64 and C.sizeof(L.LoraFoldArgs) == 48
    assert "qfx_lora_fold.hip" in g.PLAIN_SOURCES and g.EXTRA_FLAGS["qfx_lora_fold.hip"] == ["-ffp-contract=off"]
    assert ops.LORA_FOLD_MAX_RANK == 64


def test_ops_table_refusals():
    from qflux_amd import ops
    W = torch.zeros(8, 16)
    with pytest.raises(NotImplementedError, match="rank 65"):
        ops.lora_fold_table([(W, 0, 2048, 65, 1.0)])
    for bad in ([], [(W.double(), 0, 64, 4, 1.0)], [(W.t(), 0, 64, 4, 1.0)], [(W, 0, -64, 4, 1.0)], [(W, 0, 64, 4, 1.0), (W[:, :8], 0, 64, 4, 1.0)]):
        with pytest.raises(ValueError):
            ops.lora_fold_table(bad)
    lay = ops.lora_fold_table([(W, 0, 64, 4, -2.0), (torch.zeros(3, 9).bfloat16()[:, :5], 96, 128, 3, 0.5)])
    assert lay.rows == [(0, 64, 4, 16, 8, -2.0), (96, 128, 3, 5, 3, 0.5)] and lay.extent == 137 and lay.n_mats == 2
    assert lay.host[1].ld == 9 and lay.host[1].dtype == 0 and lay.host[0].dtype == 1 and lay.host[1].c == 0.5 and lay.tile_start.numel() == 3


# ------------------------------------------------------------------ plumbing, the device part replaced by the restatement

class _Toy(torch.nn.Module):
    """Two adapted linears and the state pissa_init_ invalidates."""

    def __init__(self, r=3, alpha=6.0, dtype=torch.bfloat16):
        super().__init__()
        from qflux_amd.modules import QfxLinear, QfxLoraLinear
        rng = np.random.default_rng(2)
        self.b = QfxLoraLinear(QfxLinear(24, 16, dtype=dtype), r, alpha, "a")
        self.a = QfxLoraLinear(QfxLinear(16, 40, dtype=dtype), r, alpha, "a")
        for m, shape in ((self.b, (16, 24)), (self.a, (40, 16))):
            m.base_layer.weight.data.copy_(torch.from_numpy(P.planted(rng, *shape, sigmas=(4.0, 2.0, 1.0))).to(dtype))
        self.invalidated, self._adapter_gen, self._pissa, self.tagged = 0, 0, None, 0
        self._lora = types.SimpleNamespace(tag=self._tag)

    def _tag(self):
        self.tagged += 1

    def _invalidate(self):
        self.invalidated += 1


@pytest.fixture()
def standins(monkeypatch):
    """_factors from numpy.linalg.svd, _fold from the restatement; the GPU check is taken out of the way."""
    from qflux_amd import pissa
    calls = dict(factors=[], fold=[])

    def factors(mats, ranks, scalings, k, niter, seed, index0):
        calls["factors"].append(([m[0] for m in mats], k, niter, seed, index0))
        chunks, where, off, sv, normsq, info, bad = [], [], 0, [], [], [], []
        for (name, W, _), r, s in zip(mats, ranks, scalings):
            Wd = W.double().numpy()
            if not np.isfinite(Wd).all():
                bad.append(name)
                continue
            B0, A0, sig = P.split(Wd, r, s)
            where.append((off, off + A0.size))
            chunks += [A0.reshape(-1), B0.reshape(-1)]
            off += A0.size + B0.size
            sv.append(np.concatenate([sig, np.zeros(64)])[:64])
            normsq.append(float((Wd ** 2).sum()))
            info.append([min(k, min(Wd.shape)), 1])
        if bad:
            return None, None, None, torch.zeros(len(mats), dtype=torch.float64), torch.zeros(len(mats), 2, dtype=torch.int32), bad
        return (torch.from_numpy(np.concatenate(chunks).astype(np.float32)), where, torch.from_numpy(np.stack(sv)),
                torch.tensor(normsq, dtype=torch.float64), torch.tensor(info, dtype=torch.int32), [])

    def fold(weights, qflat, where, ranks, coeffs):
        calls["fold"].append(len(weights))
        q = qflat.numpy()
        for W, (oa, ob), r, c in zip(weights, where, ranks, coeffs):
            nout, nin = W.shape
            A, B = q[oa:oa + r * nin].reshape(r, nin), q[ob:ob + nout * r].reshape(nout, r)
            if W.dtype == torch.bfloat16:
                bits = P.fold(W.view(torch.int16).numpy().view(np.uint16), A, B, c, P.BF16)
                W.copy_(torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16))
            else:
                W.copy_(torch.from_numpy(P.fold(W.numpy(), A, B, c, P.FP32)))

    monkeypatch.setattr(pissa, "_factors", factors)
    monkeypatch.setattr(pissa, "_fold", fold)
    monkeypatch.setattr(pissa, "_on_gpu", lambda t: True)
    return calls


def test_init_plumbing_report_state_and_groups(standins):
    from qflux_amd.pissa import pissa_init_
    toy = _Toy()
    W = {n: getattr(toy, n).base_layer.weight.detach().double().clone() for n in "ab"}
    one = 40 * 16 * 4
    report = pissa_init_(toy, niter=3, oversample=5, seed=11, group_bytes=one)
    assert standins["factors"] == [(["a"], 8, 3, 11, 0), (["b"], 8, 3, 11, 1)] and standins["fold"] == [1, 1]      # sorted; global index
    assert toy.invalidated == 1 and toy._adapter_gen == 1 and toy.tagged == 1
    st = toy._pissa
    assert (st["niter"], st["oversample"], st["seed"]) == (3, 5, 11) and sorted(st["A0"]) == sorted(st["B0"]) == ["a", "b"]
    for n in "ab":
        m, s = getattr(toy, n), 2.0
        B0, A0, sig = P.split(W[n].numpy(), 3, s)
        assert torch.equal(m.A.detach(), st["A0"][n]) and torch.equal(m.B.detach(), st["B0"][n]) and st["A0"][n].dtype == torch.float32
        assert np.abs(m.B.detach().double().numpy() @ m.A.detach().double().numpy() - B0 @ A0).max() <= 1e-6
        res = m.base_layer.weight.detach().double()
        back = res + s * (m.B.detach().double() @ m.A.detach().double())
        bound = 2.0 ** -8 * res.abs() + 2.0 ** -22 * (W[n].abs() + (back - res).abs())
        assert bool(((W[n] - back).abs() <= bound).all())
        assert float(res.norm()) < 0.01 * float(W[n].norm())                             # the trunk keeps the tail only
        rep = report[n]
        assert np.allclose(rep["sigma"], sig[:3], rtol=1e-12) and abs(rep["fro_retained"] - P.retained(sig, 3)) <= 1e-12
        assert abs(rep["weight_norm"] - float(W[n].norm())) <= 1e-12 * rep["weight_norm"] and rep["sketch_converged"]
    with pytest.raises(ValueError, match="already"):
        pissa_init_(toy)


def test_init_refusals(standins):
    from qflux_amd.pissa import MAX_RANK, pissa_init_
    toy = _Toy()
    toy.b.merged = True
    with pytest.raises(ValueError, match="merged"):
        pissa_init_(toy)
    toy = _Toy(alpha=0.0)
    with pytest.raises(ValueError, match="scaling"):
        pissa_init_(toy)
    toy = _Toy(alpha=-3.0)
    with pytest.raises(ValueError, match="scaling"):
        pissa_init_(toy)
    toy = _Toy(r=65, alpha=65.0)
    with pytest.raises(NotImplementedError, match=str(MAX_RANK)):
        pissa_init_(toy)
    for bad in (dict(niter=5), dict(niter=-1), dict(oversample=-1)):
        with pytest.raises(ValueError):
            pissa_init_(_Toy(), **bad)
    with pytest.raises(ValueError, match="no adapters"):
        pissa_init_(torch.nn.Linear(2, 2))
    toy = _Toy()                                                                         # a non-finite weight in the LAST group: nothing folded
    before = toy.a.base_layer.weight.detach().clone()
    toy.b.base_layer.weight.data[1, 2] = float("nan")
    with pytest.raises(ValueError, match="'b'"):
        pissa_init_(toy, group_bytes=1)
    assert standins["fold"] == [] and torch.equal(toy.a.base_layer.weight.detach(), before) and toy._pissa is None
    assert not toy.a.B.any() and toy.invalidated == 0


def test_weights_off_the_gpu_are_refused():
    from qflux_amd.pissa import pissa_init_
    with pytest.raises(RuntimeError, match="not on a GPU"):
        pissa_init_(_Toy())


def test_conversion_and_save(standins, tmp_path):
    from qflux_amd.lora_io import _normalise, save_lora_weights
    from qflux_amd.pissa import pissa_init_, pissa_to_lora
    from safetensors import safe_open
    from safetensors.torch import load_file
    import ast
    toy = _Toy()
    with pytest.raises(ValueError, match="no PiSSA"):
        pissa_to_lora(toy)
    pissa_init_(toy)
    with torch.no_grad():
        for n in "ab":
            getattr(toy, n).A.add_(0.01)
            getattr(toy, n).B.mul_(1.5)
    tensors, alphas = pissa_to_lora(toy)
    for n in "ab":
        m = getattr(toy, n)
        A2, B2, a2 = P.to_lora(m.A.detach().numpy(), m.B.detach().numpy(), toy._pissa["A0"][n].numpy(), toy._pissa["B0"][n].numpy(), 6.0)
        assert np.array_equal(tensors[n][0].numpy(), A2) and np.array_equal(tensors[n][1].numpy(), B2) and alphas[n] == a2 == 12.0
    path = save_lora_weights(toy, str(tmp_path / "conv"), convert_pissa=True)
    mods = _normalise(load_file(path))
    with safe_open(path, framework="pt") as f:
        assert {n: float(v) for n, v in ast.literal_eval(f.metadata()["lora_alpha"]).items()} == alphas
    assert all(torch.equal(mods[n]["A"], tensors[n][0]) and torch.equal(mods[n]["B"], tensors[n][1]) for n in "ab")
    plain = _normalise(load_file(save_lora_weights(toy, str(tmp_path / "plain"))))       # the default: residual-basis A, B
    assert all(torch.equal(plain[n]["A"], getattr(toy, n).A.detach()) and plain[n]["A"].shape[0] == 3 for n in "ab")
    with pytest.raises(ValueError, match="convert_pissa"):
        save_lora_weights(toy, str(tmp_path / "plain"), rank=2)
    big = _Toy(r=33, alpha=33.0)
    pissa_init_(big)
    with pytest.raises(NotImplementedError, match="64"):
        pissa_to_lora(big)
