"""CPU: the blockwise 8-bit Adam (bitsandbytes Adam8bit / AdamW8bit state layout) -- its restatement (tests/bnb8_ref.py), the block
table and state handling of the package, the config mapping, and the C ABI of qfx_adam8bit_step (no device needed)."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnb8_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = ["to_q", "to_k", "to_v", "to_out.0", "img_mlp.net.2", "txt_mod.1"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from qflux_amd import _lib
    return _lib


def test_code_books_identities(lib):
    from qflux_amd.trainer.adam8bit import dynamic_map
    for signed in (True, False):
        q = R.create_dynamic_map(signed)
        assert q.dtype == torch.float32 and q.numel() == 256
        assert torch.all(q[1:] > q[:-1])                               # sorted, no duplicates
        assert q[-1].item() == 1.0 and (q == 0).sum().item() == 1
        assert torch.equal(dynamic_map(signed), q)                     # the package's own code book
    s, u = R.create_dynamic_map(True), R.create_dynamic_map(False)
    pos, neg = s[(s > 0) & (s < 1)], s[s < 0]
    assert pos.numel() == neg.numel() == 127 and torch.equal(torch.sort(-neg).values, pos)
    assert s[0].item() == -pos.max().item() and s[127].item() == 0.0
    assert u[0].item() == 0.0 and (u >= 0).all() and u.numel() == 256


@pytest.mark.parametrize("signed", [True, False])
def test_quantise_is_nearest_code_with_ties_to_the_lower(signed):
    q = R.create_dynamic_map(signed)
    lo = -1.0 if signed else 0.0
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.rand(20000, generator=g) * (1 - lo) + lo,                      # uniform
                   torch.sign(torch.randn(20000, generator=g)).clamp(min=lo) * 10 ** (-7 * torch.rand(20000, generator=g)),  # log-spread
                   q, torch.tensor([lo, 1.0, 0.0])])
    c = R.quantize(x, q)
    d = (q.double()[None, :] - x.double()[:, None]).abs()
    best = d.min(1).values
    # the chosen code is a nearest one (up to the fp32 rounding of the midpoint it was compared against)
    slack = x.double().abs() * 2 ** -22 + 1e-45
    assert torch.all(d[torch.arange(x.numel()), c] <= best + slack)
    clear = d.topk(2, dim=1, largest=False).values.diff(dim=1).squeeze(1) > 1e-6 * d.min(1).values.clamp_min(1e-30) + 1e-12
    assert torch.equal(c[clear], d.argmin(1)[clear])
    # a code value maps to itself; the exact fp32 midpoint goes to the lower code, the next float above it to the upper one
    assert torch.equal(R.quantize(q, q), torch.arange(256))
    m = R.midpoints(q)
    assert torch.equal(R.quantize(m, q), torch.arange(255))
    assert torch.equal(R.quantize(torch.nextafter(m, torch.full_like(m, 2.0)), q), torch.arange(1, 256))


def test_state1_keeps_its_sign():
    q = R.create_dynamic_map(True)
    tiny = torch.tensor([-1e-9, 1e-9, -0.5e-6 * 0.1])
    c = R.keep_sign(R.quantize(tiny, q), tiny, q)
    assert q[c[0]] < 0 and q[c[1]] == 0 and q[c[2]] < 0


def test_one_step_from_zero_state_is_the_closed_form():
    """Step 1 from zero state: m = (1-b1) g, v = (1-b2) g^2, so p' = p - lr g / (|g| + eps) (1 - lr wd)."""
    torch.manual_seed(0)
    n, lr, wd, eps = 5000, 1e-3, 0.1, 1e-8
    p = torch.randn(n)
    g = torch.randn(n) * torch.logspace(-3, 1, n)
    g[:256] = 0.0                                                     # an all-zero block
    p0 = p.clone()
    opt = R.Adam8bitRef([p], lr=lr, eps=eps, weight_decay=wd)
    opt.step([g.clone()])
    want = (p0.double() - lr * g.double() / (g.double().abs() + eps)) * (1 - lr * wd)
    assert ((p.double() - want).abs() / want.abs().clamp_min(1e-3)).max() < 1e-5
    st = opt.state[0]
    assert st["state1"].dtype == torch.uint8 and st["absmax1"].numel() == (n + 255) // 256
    assert st["absmax1"][0] == 0 and st["absmax2"][0] == 0
    assert (st["state1"].view(-1)[:256] == 127).all() and (st["state2"].view(-1)[:256] == 0).all()   # the code of 0.0
    a1 = R.blocks_absmax(0.1 * g, 256)
    assert torch.allclose(st["absmax1"], a1, rtol=1e-6) and torch.allclose(st["absmax2"], R.blocks_absmax(0.001 * g * g, 256), rtol=1e-4)
    m = R.dequant(st["state1"], st["qmap1"], st["absmax1"], 256)
    assert torch.allclose(m, (0.1 * g).float(), rtol=0.1, atol=float(a1.max()) * 2e-2)


def test_non_finite_gradient_element_keeps_parameter_and_moments():
    p = torch.randn(300)
    g = torch.randn(300)
    opt = R.Adam8bitRef([p], min_8bit_size=1)
    opt.step([g])
    st = opt.state[0]
    c1, a1 = st["state1"].clone(), st["absmax1"].clone()
    p1 = p.clone()
    g2 = torch.randn(300)
    g2[7], g2[260] = float("nan"), float("inf")
    opt.step([g2])
    m_old = R.dequant(c1, st["qmap1"], a1, 256)
    assert p[7] == p1[7] and p[260] == p1[260] and torch.isfinite(p).all()
    assert st["_m"][7] == m_old[7] and torch.isfinite(st["absmax1"]).all() and torch.isfinite(st["absmax2"]).all()


def test_eight_bit_selection_and_block_table(lib):
    from qflux_amd import ops
    from qflux_amd.trainer.adam8bit import infer_blocksize
    for bs in (256, 2048):
        lay = ops.adam8bit_block_table([(0, 4095), (4096, 4096), (8192, 64), (8256, 5000)], bs, 4096)
        assert [t[2] for t in lay.tensors] == [False, True, False, True]
        nb = [-(-4096 // bs), -(-5000 // bs)]
        assert lay.n_absmax == sum(nb) and lay.n_fp32 == 4096 + 64
        rows = (lib.Adam8bitBlock * lay.n_blocks).from_buffer_copy(bytes(lay.table.numpy()))
        assert lay.n_blocks == -(-4095 // bs) + nb[0] + 1 + nb[1]
        assert sum(r.len for r in rows) == 4095 + 4096 + 64 + 5000 and max(r.len for r in rows) <= bs
        eight = [r for r in rows if r.mode == lib.ADAM8BIT_BLOCKWISE]
        assert [r.state for r in eight] == list(range(lay.n_absmax)) and all(r.off % 4 == 0 for r in rows)
        last = [r for r in eight if r.off >= 8256][-1]
        assert last.off + last.len == 8256 + 5000 and last.len == 5000 - (nb[1] - 1) * bs
        assert infer_blocksize(5000, nb[1]) == bs
        small = R.Adam8bitRef([torch.zeros(4095), torch.zeros(4096)], blocksize=bs)
        small.step([torch.ones(4095), torch.ones(4096)])
        assert small.state[0]["state1"].dtype == torch.float32 and "absmax1" not in small.state[0]
        assert small.state[1]["state1"].dtype == torch.uint8 and small.state[1]["absmax1"].numel() == -(-4096 // bs)
    with pytest.raises(ValueError):
        infer_blocksize(5000, 7)
    with pytest.raises(ValueError):
        ops.adam8bit_block_table([(0, 100)], 512, 4096)


def test_config_mapping_state_bits():
    from qflux_amd.trainer import optimizer_kwargs_from_config as f
    for cls, opt, wd in (("Adam8bit", "adam8bit_blockwise", 0.0), ("PagedAdam8bit", "adam8bit_blockwise", 0.0),
                         ("AdamW8bit", "adamw8bit_blockwise", 0.01), ("PagedAdamW8bit", "adamw8bit_blockwise", 0.01)):
        kw = f("bitsandbytes.optim." + cls, {"lr": 1e-4, "betas": [0.9, 0.99], "is_paged": True, "percentile_clipping": 100,
                                             "block_wise": True, "min_8bit_size": 2048}, state_bits=8)
        assert kw == {"lr": 1e-4, "betas": (0.9, 0.99), "optimizer": opt, "weight_decay": wd, "optimizer_args": {"min_8bit_size": 2048}}
        assert f("bitsandbytes.optim." + cls, {"lr": 1e-4, "weight_decay": 0.05}, state_bits=8)["weight_decay"] == 0.05
        for bad in ({"percentile_clipping": 5}, {"max_unorm": 1.0}, {"block_wise": False}, {"skip_zeros": True}, {"amsgrad": True}):
            with pytest.raises(NotImplementedError):
                f("bitsandbytes.optim." + cls, dict(lr=1e-4, **bad), state_bits=8)
        # state_bits=32: today's mapping, unchanged
        assert f("bitsandbytes.optim." + cls, {"lr": 1e-4, "percentile_clipping": 5})["optimizer"] in ("adam8bit", "adamw")
    assert f("bitsandbytes.optim.Adam8bit", {"lr": 1e-4, "betas": [0.9, 0.999]}) == \
        {"lr": 1e-4, "betas": (0.9, 0.999), "optimizer": "adam8bit", "weight_decay": 0.0}
    assert f("torch.optim.AdamW", {"lr": 1e-4}, state_bits=8) == f("torch.optim.AdamW", {"lr": 1e-4})
    with pytest.raises(ValueError):
        f("bitsandbytes.optim.Adam8bit", {}, state_bits=4)


def _tiny_model():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from common import TINY
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.modules import LoraConfig
    q = QwenImageTransformer2DModel(**TINY)
    q.add_adapter(LoraConfig(r=4, lora_alpha=8, target_modules=TARGETS), "lora_edit")
    return q


def _bnb_file(q, bs, steps=3, wd=0.0):
    torch.manual_seed(4)
    ps = [torch.randn(p.shape) * 0.1 for _, p in q.lora_store.params()]
    opt = R.Adam8bitRef(ps, lr=1e-3, betas=(0.9, 0.99), weight_decay=wd, blocksize=bs)
    for _ in range(steps):
        opt.step([torch.randn(p.shape) for p in ps])
    return opt.state_dict()


@pytest.mark.parametrize("bs", [256, 2048])
def test_bnb_layout_state_dict_round_trip(lib, bs):
    from qflux_amd.trainer import QwenLoraTrainStep
    q = _tiny_model()
    sd = _bnb_file(q, bs, wd=0.01)
    assert {len(e) for e in sd["state"].values()} == {3, 7}           # fp32 (small) and 8-bit tensors both present
    step = QwenLoraTrainStep(q, optimizer="adamw8bit_blockwise")
    step.load_state_dict(sd)
    assert step.optimizer_args["blocksize"] == bs and step.global_step == 3 and step.betas == (0.9, 0.99)
    out = step.state_dict()
    assert out["param_groups"][0]["weight_decay"] == 0.01 and out["param_groups"][0]["lr"] == 1e-3
    assert set(out["state"]) == set(sd["state"])
    for i, e in sd["state"].items():
        o = out["state"][i]
        assert set(o) == set(e) and o["step"] == 3
        for k, v in e.items():
            if torch.is_tensor(v):
                assert o[k].dtype == v.dtype and o[k].shape == v.shape and torch.equal(o[k], v), (i, k)


def test_alias_loads_a_bnb_layout_file_dequantised(lib):
    from qflux_amd.trainer import QwenLoraTrainStep
    q = _tiny_model()
    sd = _bnb_file(q, 256)
    step = QwenLoraTrainStep(q, optimizer="adam8bit")
    step.load_state_dict(sd)
    assert step.global_step == 3
    for i, (_, p, off, k) in enumerate(q.lora_store.entries):
        e = sd["state"][i]
        if e["state1"].dtype == torch.uint8:
            m, v = R.dequant(e["state1"], e["qmap1"], e["absmax1"], 256), R.dequant(e["state2"], e["qmap2"], e["absmax2"], 256)
        else:
            m, v = e["state1"].reshape(-1), e["state2"].reshape(-1)
        assert torch.equal(step._m[off:off + k].cpu(), m) and torch.equal(step._v[off:off + k].cpu(), v)


def test_trainer_options():
    from qflux_amd.trainer import QwenLoraTrainStep
    q = _tiny_model()
    assert QwenLoraTrainStep(q, optimizer="adam8bit_blockwise").weight_decay == 0.0
    assert QwenLoraTrainStep(q, optimizer="adamw8bit_blockwise").weight_decay == 0.01
    s = QwenLoraTrainStep(q, optimizer="adam8bit_blockwise", weight_decay=0.02, optimizer_args={"blocksize": 2048, "min_8bit_size": 100})
    assert s.weight_decay == 0.02 and s.optimizer_args == {"blocksize": 2048, "min_8bit_size": 100}
    with pytest.raises(ValueError):
        QwenLoraTrainStep(q, optimizer="adam8bit_blockwise", optimizer_args={"blocksize": 512})
    with pytest.raises(ValueError):
        QwenLoraTrainStep(q, optimizer="adam8bit_blockwise", optimizer_args={"d0": 1e-6})


def test_ctypes_layout_matches_header(tmp_path, lib):
    pairs = {"qfx_adam8bit_args": lib.Adam8bitArgs, "qfx_adam8bit_block": lib.Adam8bitBlock}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "qfx.h"', "int main(void) {"]
    for cname, ct in pairs.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'  printf(" %zu", offsetof({cname}, {fname}));')
        lines.append('  printf("\\n");')
    lines.append(f'  printf("modes %d %d\\n", QFX_ADAM8BIT_BLOCKWISE, QFX_ADAM8BIT_FP32);')
    lines += ["  return 0;", "}"]
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for line in out[:-1]:
        parts = line.split()
        ct = pairs[parts[0]]
        assert [int(v) for v in parts[1:]] == [C.sizeof(ct)] + [getattr(ct, f).offset for f, _ in ct._fields_], parts
    assert out[-1].split()[1:] == [str(lib.ADAM8BIT_BLOCKWISE), str(lib.ADAM8BIT_FP32)]


def test_bad_arguments_are_rejected_without_a_device(lib):
    f = lib.lib.qfx_adam8bit_step
    assert f(None, None) == -1
    a = lib.Adam8bitArgs()
    assert f(C.byref(a), None) == -1                                  # NULL pointers
    for name in ("p", "g", "q1", "q2", "absmax1", "absmax2", "m32", "v32", "table", "qmap1", "qmap2"):
        setattr(a, name, 0x1000)
    a.n_blocks, a.blocksize, a.step, a.lr, a.beta1, a.beta2 = 1, 512, 1, 1e-3, 0.9, 0.999
    assert f(C.byref(a), None) == -1                                  # block size outside {256, 2048}
    a.blocksize, a.n_blocks = 256, 0
    assert f(C.byref(a), None) == -1                                  # empty table
    a.n_blocks, a.step = 1, 0
    assert f(C.byref(a), None) == -1                                  # step < 1
    a.step, a.beta1 = 1, 1.0
    assert f(C.byref(a), None) == -1                                  # beta1 = 1: no bias correction
    a.beta1, a.lr = 0.9, -1.0
    assert f(C.byref(a), None) == -1
    a.lr, a.table = 1e-3, None
    assert f(C.byref(a), None) == -1
