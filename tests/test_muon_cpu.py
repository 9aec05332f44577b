"""CPU: the Muon restatement (tests/muon_ref.py) against torch.optim.Muon itself, family resolution and defaults, the config mapping
and its refusals, the state_dict layout against torch.optim.Muon's key for key, the round trip through a real torch.optim.Muon, the
ctypes layout and host-side refusals of qfx_muon_step, and the packed-VALU scan of the new translation unit.

Restatement against torch: the momentum buffer bit for bit; with ns_steps = 0 (normalisation only) O and p bit for bit; with the
iteration, torch's bf16 GEMM and the restatement's fp32 matmul may sum in different orders, so each is measured against the float64
iteration from the same normalised input and the restatement's error may be at most twice torch's (the rule the kernel is held to).

The stage tests of tests/test_muon_gpu.py, without a GPU: the sign designs normalise to {0, +-2^-j}, every product they reach is
exact in fp32 in any order (R.exact_ok), two accumulation orders give the same bits, three kernel faults (R.MUTANTS) change them;
the Gaussian cases keep their norm off the bf16 rounding boundaries; the five-iteration bar lets the chunk-dropping fault through;
and the bars of the one-iteration Gaussian test (profiles/muon_stage_parity.json; QFX_WRITE_MUON_STAGE_PARITY=1 rewrites them)."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import muon_ref as R
import test_muon_gpu as TG              # its shapes, Gaussian cases and design table; importing it needs no GPU
from test_sgd_cpu import toy_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [((s, n) if not tr else (n, s), nesterov, fn, wd)
         for s, n in ((16, 64), (48, 272), (64, 128), (96, 192)) for tr in (False, True)
         for nesterov, fn, wd in ((True, None, 0.1), (False, "match_rms_adamw", 0.0), (True, "original", 0.0))]


@pytest.mark.parametrize("shape,nesterov,fn,wd", CASES, ids=[f"{c[0][0]}x{c[0][1]}-{'nes' if c[1] else 'plain'}-{c[2]}-wd{c[3]}" for c in CASES])
def test_restatement_matches_torch_optim_muon(shape, nesterov, fn, wd):
    p0, grads = R.make_matrix(shape, 1, 0.1), [R.make_matrix(shape, 10 + t) for t in range(2)]
    for ns in (0, 5):
        kw = dict(lr=1e-2, weight_decay=wd, nesterov=nesterov, adjust_lr_fn=fn, ns_steps=ns)
        pt = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Muon([pt], **kw)
        pr, br, p64 = p0.clone(), torch.zeros(shape), p0.double()
        for g in grads:
            pt.grad = g.clone()
            opt.step()
            pr, br, o, x0 = R.step(pr, g, br, **kw)
            assert o.dtype == torch.bfloat16 and tuple(o.shape) == shape
            p64 = p64 * (1 - 1e-2 * wd) - 1e-2 * R.lr_ratio(fn, *shape) * R.untranspose(R.ns_f64(x0, ns_steps=ns), shape)
        assert torch.equal(br, opt.state[pt]["momentum_buffer"])
        if ns == 0:
            assert torch.equal(pr, pt.detach())
            continue
        d64 = p64 - p0.double()
        e_t, e_r = R.rel_err(pt.detach().double() - p0.double(), d64), R.rel_err(pr.double() - p0.double(), d64)
        assert 0 < e_r <= 2 * e_t and e_t < 0.05, (e_r, e_t)


def test_restatement_zero_gradient_non_finite_gradient_and_clip():
    p0, z = R.make_matrix((16, 64), 1, 0.1), torch.zeros(16, 64)
    pn, buf, o, _ = R.step(p0, z, z, lr=1.0, weight_decay=0.25)
    assert not o.any() and not buf.any() and torch.equal(pn, p0 * 0.75)
    g = R.make_matrix((16, 64), 2)
    g[3, 3] = float("nan")
    assert R.step(p0, g, z) is None
    assert R.clip_coef(None, 1.0, 0.5) == 0.5 and R.clip_coef(4.0, 0.0, 0.5) == 0.5
    assert abs(float(R.clip_coef(4.0, 0.5, 1.0)) - 0.25) < 1e-6 and R.clip_coef(0.01, 1.0, 1.0) == 1.0


def test_resolve_family_defaults_and_the_train_steps_accept_muon():
    from qflux_amd.trainer import FluxKontextTrainStep, QwenLoraTrainStep
    from qflux_amd.trainer.optim_state import MuonState, default_betas, resolve_family
    alias, fam, cls, wd, args = resolve_family("muon")
    assert (alias, fam, cls, wd) == (None, "muon", MuonState, 0.1)
    assert args == dict(momentum=0.95, nesterov=True, ns_coefficients=(3.4445, -4.7750, 2.0315), eps=1e-7, ns_steps=5, adjust_lr_fn=None)
    assert resolve_family("muon", 0.0, {"ns_steps": 3, "adjust_lr_fn": "match_rms_adamw"})[3:] == \
        (0.0, dict(args, ns_steps=3, adjust_lr_fn="match_rms_adamw"))
    assert MuonState.names(args) == ("buf",) and default_betas("muon") == (0.9, 0.999)
    with pytest.raises(ValueError, match="unsupported optimizer_args"):
        resolve_family("muon", None, {"dampening": 0.1})
    with pytest.raises(ValueError, match="Number of steps must be less than 100"):
        resolve_family("muon", None, {"ns_steps": 100})
    with pytest.raises(ValueError, match="Adjust learning rate function spectral is not supported"):
        resolve_family("muon", None, {"adjust_lr_fn": "spectral"})
    with pytest.raises(ValueError, match="momentum should be >= 0"):
        resolve_family("muon", None, {"momentum": -0.1})
    with pytest.raises(ValueError, match="exactly 3 values"):
        resolve_family("muon", None, {"ns_coefficients": (1.0, 2.0)})
    toy = toy_model()
    for cls_ in (QwenLoraTrainStep, FluxKontextTrainStep):
        s = cls_(toy, lr=2e-3, optimizer="muon", optimizer_args={"momentum": 0.9})
        assert s.weight_decay == 0.1 and s.optimizer_args["momentum"] == 0.9 and s.eps == 1e-8 and s.optimizer_args["eps"] == 1e-7
        sd = s.state_dict()                   # before the first step: torch's empty state, its options in the group
        g = sd["param_groups"][0]
        assert sd["state"] == {} and g["eps"] == 1e-7 and g["momentum"] == 0.9 and g["ns_steps"] == 5 and g["adjust_lr_fn"] is None
    # the lr ratio of every matrix is part of the table; adjust_lr_fn is part of the layout key
    st = toy.lora_store
    k1, k2 = MuonState.layout_key(st, args), MuonState.layout_key(st, dict(args, adjust_lr_fn="match_rms_adamw"))
    assert k1 != k2
    lay = MuonState(st, dict(args, adjust_lr_fn="match_rms_adamw")).layout
    for (off, r, c, ratio), (_, p, o, _) in zip(lay.tensors, st.entries):
        assert (off, r, c) == (o, *p.shape) and ratio == R.lr_ratio("match_rms_adamw", r, c)


def test_config_mapping_and_its_refusals():
    from qflux_amd.trainer import optimizer_kwargs_from_config as K
    for path in ("torch.optim.Muon", "qflux_amd.optim.Muon"):
        assert K(path, {"lr": 1e-3}) == {"optimizer": "muon", "optimizer_args": {}, "lr": 1e-3}
        out = K(path, dict(lr=2e-3, weight_decay=0.0, momentum=0.9, nesterov=False, ns_coefficients=[3.0, -4.0, 2.0], eps=1e-6, ns_steps=3,
                           adjust_lr_fn="match_rms_adamw"), state_bits=8)
        assert out == {"optimizer": "muon", "lr": 2e-3, "weight_decay": 0.0,
                       "optimizer_args": dict(momentum=0.9, nesterov=False, ns_coefficients=(3.0, -4.0, 2.0), eps=1e-6, ns_steps=3,
                                              adjust_lr_fn="match_rms_adamw")}
        assert "eps" not in out                       # Muon's eps is the family's own, never the train step's Adam eps
        with pytest.raises(ValueError, match="Number of steps must be less than 100"):
            K(path, {"lr": 1e-3, "ns_steps": 100})
        with pytest.raises(ValueError, match="Adjust learning rate function rms is not supported"):
            K(path, {"lr": 1e-3, "adjust_lr_fn": "rms"})
        with pytest.raises(NotImplementedError, match="betas"):
            K(path, {"lr": 1e-3, "betas": (0.9, 0.99)})
        with pytest.raises(NotImplementedError, match="dampening"):
            K(path, {"lr": 1e-3, "dampening": 0.1})


def test_torch_optim_class_has_torchs_signature_and_refusals():
    import inspect
    from qflux_amd import optim as O
    assert "Muon" in O.__all__
    ours, theirs = inspect.signature(O.Muon.__init__), inspect.signature(torch.optim.Muon.__init__)
    assert list(ours.parameters) == list(theirs.parameters)
    assert {n: p.default for n, p in ours.parameters.items()} == {n: p.default for n, p in theirs.parameters.items()}
    toy = toy_model()
    ps = [p for _, p in toy.lora_store.params()]
    opt = O.Muon(ps)
    ref = torch.optim.Muon([torch.nn.Parameter(p.detach().clone()) for p in ps])
    assert isinstance(opt, torch.optim.Optimizer) and opt.family == "muon"
    g, gt = opt.param_groups[0], ref.param_groups[0]
    assert all(g[k] == gt[k] for k in gt if k != "params"), (g, gt)
    assert opt.state_dict()["state"] == {}
    for kw, msg in ((dict(ns_steps=100), "Number of steps must be less than 100"), (dict(adjust_lr_fn="x"), "Adjust learning rate function x is not supported"),
                    (dict(lr=-1.0), "Learning rate should be >= 0"), (dict(momentum=-1.0), "momentum should be >= 0"),
                    (dict(weight_decay=-1.0), "weight decay should be >= 0")):
        with pytest.raises(ValueError, match=msg):
            O.Muon(ps, **kw)
    with pytest.raises(ValueError, match="missing"):
        O.Muon(ps[:-1])


def _filled(toy, **args):
    from qflux_amd.trainer import QwenLoraTrainStep
    step = QwenLoraTrainStep(toy, lr=3e-3, weight_decay=0.05, optimizer="muon", optimizer_args=args or None)
    step.opt_state = step._opt_cls(toy.lora_store, step.optimizer_args)
    step.opt_state.buf.copy_(torch.randn(step.opt_state.buf.shape, generator=torch.Generator().manual_seed(5)))
    step.opt_state.first = False
    step.global_step = 4
    return step


def test_state_dict_equals_torch_optim_muons_key_for_key_and_round_trips_through_it(tmp_path):
    from qflux_amd import optim as O
    from qflux_amd.trainer import QwenLoraTrainStep
    toy = toy_model()
    st = toy.lora_store
    step = _filled(toy, momentum=0.9, adjust_lr_fn="match_rms_adamw", ns_steps=4)
    assert [n for n, _ in step._state_buffers()] == ["lora", "buf"]
    torch.save(step.state_dict(), str(tmp_path / "optimizer.bin"))
    sd = torch.load(str(tmp_path / "optimizer.bin"), map_location="cpu", weights_only=False)
    # a real torch.optim.Muon over the same parameters, stepped once so that it holds state
    tp = [torch.nn.Parameter(p.detach().clone()) for _, p in st.params()]
    ref = torch.optim.Muon(tp, lr=3e-3, weight_decay=0.05, momentum=0.9, adjust_lr_fn="match_rms_adamw", ns_steps=4)
    for p in tp:
        p.grad = torch.ones_like(p)
    ref.step()
    rsd = ref.state_dict()
    assert list(sd["state"]) == list(rsd["state"]) == list(range(len(st.entries)))
    for i, (_, p, off, k) in enumerate(st.entries):
        assert set(sd["state"][i]) == set(rsd["state"][i]) == {"momentum_buffer"}
        assert sd["state"][i]["momentum_buffer"].shape == rsd["state"][i]["momentum_buffer"].shape == p.shape
        assert torch.equal(sd["state"][i]["momentum_buffer"], step.opt_state.buf[off:off + k].view(p.shape))
    g, gt = sd["param_groups"][0], rsd["param_groups"][0]
    assert set(gt) <= set(g) and all(g[k] == gt[k] for k in gt), (g, gt)          # every key of torch's group, with torch's value
    assert set(g) - set(gt) == {"betas"} and set(sd) - set(rsd) == {"global_step"}  # plus the common fields of every family's file
    # our file -> torch.optim.Muon
    ref.load_state_dict(sd)
    for i, p in enumerate(tp):
        assert torch.equal(ref.state[p]["momentum_buffer"], sd["state"][i]["momentum_buffer"])
    assert ref.param_groups[0]["momentum"] == 0.9 and ref.param_groups[0]["adjust_lr_fn"] == "match_rms_adamw"
    for p in tp:
        p.grad = torch.full_like(p, 0.5)
    ref.step()                                       # torch steps on the loaded state
    # torch's file -> a fresh train step and the torch.optim class; no step count in it
    tsd = ref.state_dict()
    fresh = QwenLoraTrainStep(toy, lr=0.5, eps=1e-6, optimizer="muon")
    fresh.load_state_dict(tsd)
    assert fresh.global_step == 0 and fresh.lr == 3e-3 and fresh.weight_decay == 0.05 and fresh.optimizer_args["ns_steps"] == 4
    assert fresh.optimizer_args["momentum"] == 0.9 and fresh.optimizer_args["adjust_lr_fn"] == "match_rms_adamw" and not fresh.opt_state.first
    for i, (_, p, off, k) in enumerate(st.entries):
        assert torch.equal(fresh.opt_state.buf[off:off + k].view(p.shape), tsd["state"][i]["momentum_buffer"])
    fresh.load_state_dict(sd)
    assert fresh.global_step == 4
    opt = O.Muon([p for _, p in st.params()])
    opt.load_state_dict(sd)
    assert opt._step_count_fused == 4 and opt.param_groups[0]["momentum"] == 0.9 and opt.param_groups[0]["ns_steps"] == 4
    back = opt.state_dict()
    for i, e in sd["state"].items():
        assert torch.equal(back["state"][i]["momentum_buffer"], e["momentum_buffer"])
    bad = {"state": {0: {"momentum_buffer": torch.zeros(3, 3)}}, "param_groups": sd["param_groups"]}
    with pytest.raises(ValueError, match="momentum_buffer has shape"):
        fresh.load_state_dict(bad)


def test_ctypes_structs_match_the_c_header_layout_and_the_abi_is_still_7(tmp_path):
    from qflux_amd import _lib as L
    pairs = {"qfx_muon_tensor": L.MuonTensor, "qfx_muon_args": L.MuonArgs}
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
        assert [int(v) for v in parts[1:]] == [C.sizeof(ct)] + [getattr(ct, f).offset for f, _ in ct._fields_], parts[0]
    assert L.ABI_VERSION == 7 and L.lib.qfx_abi_version() == 7
    assert "qfx_muon_step" in L.SYMBOLS and "qfx_muon_ws_bytes" in L.SYMBOLS
    with open(os.path.join(ROOT, "include", "qfx.h")) as f:
        hdr = f.read()
    assert "#define QFX_ABI_VERSION 7" in hdr and "int qfx_muon_step(const qfx_muon_args* a, void* stream);" in hdr


def test_table_workspace_size_and_host_side_refusals():
    from qflux_amd import _lib as L
    from qflux_amd import ops
    lay = ops.muon_table([(0, (16, 3072)), (49152, (3072, 16)), (98304, (32, 1536)), (147456, (4, 64))])
    assert lay.ws_bytes == 0 and lay.n_tensors == 4 and lay.extent == 147456 + 256         # every X fits the 96 KB of LDS
    assert lay.tensors[1] == (49152, 3072, 16, R.lr_ratio(None, 3072, 16)) and lay.tensors[0][3] == 1.0
    arr = (L.MuonTensor * 4).from_buffer_copy(lay.table.numpy().tobytes())
    assert [(d.off, d.rows, d.cols, d.reserved) for d in arr] == [(0, 16, 3072, 0), (49152, 3072, 16, 0), (98304, 32, 1536, 0), (147456, 4, 64, 0)]
    assert abs(arr[1].lr_ratio - 192 ** 0.5) < 1e-5
    # one 32-column chunk more than LDS holds: a slot per workgroup, sized by the largest such matrix (s and n padded to 16 / 32)
    assert ops.muon_table([(0, (16, 3073))]).ws_bytes == 16 * 3104 * 2
    assert ops.muon_table([(0, (16, 64)), (1024, (90, 3000)), (400000, (3000, 20))]).ws_bytes == 3 * 96 * 3008 * 2
    assert ops.muon_table([(i * 200000, (64, 3072)) for i in range(300)]).ws_bytes == 256 * 64 * 3072 * 2   # at most 256 workgroups
    for bad in ([], [(0, (2, 3, 4))], [(0, (7,))], [(-4, (2, 3))], [(0, (0, 3))], [(0, (97, 97))], [(0, (1 << 16, 1 << 15))]):
        with pytest.raises(ValueError):
            ops.muon_table(bad)
    with pytest.raises(ValueError, match="not supported"):
        ops.muon_table([(0, (4, 4))], "spectral")
    f = L.lib.qfx_muon_step

    def args(**kw):
        a = L.MuonArgs(0x1000, 0x2000, 0x3000, None, 0, 0x4000, 3, 1, 5, 1e-3, 0.1, 0.95, 0.05, 3.4445, -4.775, 2.0315, 1e-7, None, 0.0, 1.0)
        for k, v in kw.items():              # never dereferenced: every call below is rejected on the host
            setattr(a, k, v)
        return a
    assert f(None, None) == L.QFX_EINVAL
    assert f(args(n_tensors=0, table=None), None) == L.QFX_OK            # nothing to do, nothing launched
    for kw in (dict(n_tensors=-1), dict(table=None), dict(p=None), dict(g=None), dict(buf=None), dict(ws_bytes=64), dict(ws_bytes=-1),
               dict(ws=0x5008, ws_bytes=64), dict(lr=-1.0), dict(lr=float("nan")), dict(weight_decay=-0.1), dict(momentum=-0.1),
               dict(ns_steps=100), dict(ns_steps=-1), dict(eps=0.0), dict(eps=-1e-7)):
        assert f(args(**kw), None) == L.QFX_EINVAL, kw
    assert L.lib.qfx_muon_ws_bytes(None, 2) == L.QFX_EINVAL and L.lib.qfx_muon_ws_bytes(None, 0) == 0


def test_no_packed_fp32_valu_consumes_an_mfma_result_in_the_muon_kernel(tmp_path):
    """qfx_muon.hip has matrix instructions but is not in the build entry's scanned SOURCES list: the same scan, here."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as g
    import pk_mfma_scan
    assert "qfx_muon.hip" in g.PLAIN_SOURCES and "qfx_muon.hip" not in g.SOURCES
    dst = str(tmp_path / "qfx_muon.s")
    r = subprocess.run([g._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + g.CSRC,
                        *g.EXTRA_FLAGS.get("qfx_muon.hip", []), "-S", "--cuda-device-only", os.path.join(g.CSRC, "qfx_muon.hip"), "-o", dst],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    with open(dst) as f:
        asm = f.read()
    assert "v_mfma_f32_16x16x32_bf16" in asm and "scratch_" not in asm
    assert not pk_mfma_scan.scan(dst)


# ---- the stage-level GPU tests of tests/test_muon_gpu.py: their designs, their margins and their sensitivity, without a GPU -------
STAGE_PROFILE = os.path.join(ROOT, "profiles", "muon_stage_parity.json")
SEES = {"gram_chunk": ("gram", "gg"), "g_element": ("gram", "gg"), "hx_strip": ("gram", "gg")}   # H = G under "gram": H X is formed there too


def _share(a, b):
    return float((R.bf16_ulps(a, b) > 0).float().mean())


def test_sign_designs_are_exact_under_every_probe_and_every_mutant_shows():
    for i, shape in enumerate(TG.SHAPES):
        nz = TG.DESIGN_NONZEROS.get(shape)
        m = R.sign_design(shape, TG.DESIGN_SEED + i, nz)
        j = R.max_design_j(shape) - (0 if nz is None else 1)
        assert int((m != 0).sum()) == 4 ** j and set(m.unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert bool((m != 0).any(0).all()) and bool((m != 0).any(1).all())
        x0 = R.normalise(m, 1e-7)
        assert tuple(x0.shape) == (min(shape), max(shape)) and set(x0.float().abs().unique().tolist()) <= {0.0, 2.0 ** -j}
        assert torch.equal(x0.float(), R.short_image(m) * 2.0 ** -j)
        for name, coeffs in R.PROBES.items():
            x1, ok = R.probe_exact(x0, coeffs)
            assert all(ok.values()), (shape, name, ok)
            assert torch.equal(x1, R.ns_bf16(x0, coeffs, 1)), (shape, name)                     # an fp32 order against the fp64 one
            assert torch.equal(x1, R.ns_bf16(x0.flip(1).contiguous(), coeffs, 1).flip(1)), (shape, name)   # and the reversed order
            shares = {k: _share(f(x0, coeffs, 1), x1) for k, f in R.MUTANTS.items()}
            print(f"MUON_STAGE design shape={shape} nonzeros=4^{j} probe={name} exact_ok={ok} mutant_share={shares}")
            for k, probes in SEES.items():
                assert (shares[k] > 0) == (name in probes), (shape, name, k, shares[k])
            if name.startswith("ax"):
                assert torch.equal(x1.float(), x0.float() * coeffs[0])
    # why (96, 3072) takes the sparser design: with 4^9 non-zeros bf16(G G) X is past the 24 bits
    dense = R.normalise(R.sign_design((96, 3072), TG.DESIGN_SEED + TG.SHAPES.index((96, 3072))), 1e-7)
    assert not R.probe_exact(dense, R.PROBES["gg"])[1]["hx0"] and all(R.probe_exact(dense, R.PROBES["gram"])[1].values())


def test_two_step_gram_designs_keep_the_second_iteration_exact():
    """The second iteration of the "gram" probe: G G is multiplied by c = 0 and H = G, so X X^T and H X of both iterations decide."""
    for shape, nz in TG.TWO_STEP_NONZEROS.items():
        x0 = R.normalise(R.sign_design(shape, TG.TWO_STEP_SEED + TG.SHAPES.index(shape), nz), 1e-7)
        x2, ok = R.ns_staged(x0, R.PROBES["gram"], 2)
        rel = {k: v for k, v in ok.items() if not k.startswith("gg")}
        print(f"MUON_STAGE two_step shape={shape} nonzeros={nz} exact_ok={rel}")
        assert len(rel) == 4 and all(rel.values()), (shape, rel)
        assert torch.equal(x2, R.ns_bf16(x0, R.PROBES["gram"], 2)) and torch.equal(x2, R.ns_bf16(x0.flip(1).contiguous(), R.PROBES["gram"], 2).flip(1))
        assert not torch.equal(x2, R.MUTANTS["gram_chunk"](x0, R.PROBES["gram"], 2)) and bool(x2.any())
    assert {(16, 64), (64, 16)} <= set(TG.TWO_STEP_NONZEROS)


def test_gaussian_cases_keep_their_norm_off_the_bf16_rounding_boundaries():
    """The margin TG.test_normalisation_alone_is_bit_exact needs (derived there), for the seeds of TG.cases(); and the restatement's
    own fp32 sum of squares lands on the side of the float64 norm."""
    for c in TG.stage_cases():
        margin, nrm = R.norm_margin(c["u"])
        print(f"MUON_STAGE norm shape={c['shape']} norm={nrm:.8e} margin=2^{math.log2(margin):.2f} needed=2^{math.log2(TG.NORM_MARGIN):.0f}")
        assert margin >= TG.NORM_MARGIN, (c["shape"], margin)
        xf = R.short_image(c["u"].to(R.BF)).float()
        assert torch.equal(c["x0"], (xf / torch.tensor(nrm, dtype=torch.float64).to(R.BF).float()).to(R.BF)), c["shape"]


def test_five_step_bar_lets_the_chunk_dropping_mutant_through_at_the_large_shapes():
    """What the stage tests are for: e_kernel <= 2 e_torch after five iterations does not see a Gram product without its last chunk."""
    cs = {c["shape"]: c for c in TG.stage_cases()}
    for shape in ((96, 3072), (16, 3104), (32, 1568)):
        c = cs[shape]
        e_t = R.rel_err(c["o_t"], c["o64"])
        for k, f in R.MUTANTS.items():
            e_m = R.rel_err(R.untranspose(f(c["x0"], R.COEFFS, 5), shape), c["o64"])
            print(f"MUON_STAGE old_bar shape={shape} mutant={k} e_mutant/e_torch={e_m / e_t:.3f} passes_old_bar={e_m <= 2 * e_t}")
            if k == "gram_chunk":
                assert e_m <= 2 * e_t, (shape, e_m, e_t)


def _one_step_reference_noise():
    """Per Gaussian case: two accumulation orders of the reference (torch's fp32 matmul, float64 rounded to fp32) after ONE iteration
    with the default coefficients -- the share of elements that differ, the largest difference in bf16 steps, the bar the kernel is
    held to against the float64 order, and each mutant's share over that bar."""
    ref, bar, sens = {}, {}, {}
    for c in TG.stage_cases():
        key = "%dx%d" % c["shape"]
        d = R.bf16_ulps(R.ns_bf16(c["x0"], R.COEFFS, 1), c["x1"])
        n = d.numel()
        ref[key] = {"elements": n, "differing": int((d > 0).sum()), "s_ref": float((d > 0).sum()) / n, "u_ref": int(d.max())}
        bar[key] = {"share": max(8.0 * ref[key]["s_ref"], 4.0 / n), "ulps": max(ref[key]["u_ref"], 1)}
        sens[key] = {k: _share(f(c["x0"], R.COEFFS, 1), c["x1"]) / bar[key]["share"] for k, f in R.MUTANTS.items()}
    return ref, bar, sens


def test_one_step_bars_of_the_gpu_test_come_from_the_references_own_noise():
    ref, bar, sens = _one_step_reference_noise()
    if os.environ.get("QFX_WRITE_MUON_STAGE_PARITY") == "1":
        doc = {}
        if os.path.exists(STAGE_PROFILE):
            with open(STAGE_PROFILE) as f:
                doc = json.load(f)
        doc.update({"rule": "one Newton-Schulz iteration, default coefficients, Gaussian cases of tests/test_muon_gpu.py: s_ref = share of "
                            "elements on which two accumulation orders of the reference differ (torch's fp32 matmul against float64 "
                            "rounded to fp32 where the kernel holds fp32), u_ref = their largest difference in bf16 steps; the kernel "
                            "against the float64 order: differing share <= max(8 s_ref, 4 elements' worth), no element off by more "
                            "than max(u_ref, 1) bf16 steps; mutant_share_over_bar: the three faults of tests/muon_ref.py MUTANTS, "
                            "each must exceed the bar at least four times over",
                    "reference": ref, "bar": bar, "mutant_share_over_bar": sens})
        with open(STAGE_PROFILE, "w") as f:
            json.dump(doc, f, indent=1)
    with open(STAGE_PROFILE) as f:
        committed = json.load(f)
    assert set(committed["bar"]) == set(bar) == {"%dx%d" % s for s in TG.SHAPES}
    for key in bar:
        b, r = committed["bar"][key], committed["reference"][key]
        print(f"MUON_STAGE one_step shape={key} now={ref[key]} committed_bar={b} mutant_share_over_committed_bar="
              f"{ {k: round(v * bar[key]['share'] / b['share'], 1) for k, v in sens[key].items()} }")
        assert b["share"] == max(8.0 * r["s_ref"], 4.0 / r["elements"]) and b["ulps"] == max(r["u_ref"], 1) and r["elements"] == ref[key]["elements"]
        # this machine's two orders would themselves pass the committed bar, and every fault misses it four times over
        assert ref[key]["s_ref"] <= b["share"] and ref[key]["u_ref"] <= b["ulps"], (key, ref[key], b)
        for k, v in sens[key].items():
            assert v * bar[key]["share"] >= 4.0 * b["share"], (key, k, v)
