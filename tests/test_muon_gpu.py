"""GPU: the fused Muon step (qfx_muon_step) against its CPU restatement (tests/muon_ref.py) and against torch.optim.Muon's own error,
its determinism, the skipped and the all-zero matrix, the clip path, the refusals, and the trainer / torch.optim class paths.

Tolerances.  buf is plain fp32 lerp: within 1 ulp of the restatement.  The bf16 Newton-Schulz iteration is not bit-comparable between
two fp32 accumulation orders, so O is held to the reference's own error: with O64 the same iteration in float64 from the same
bf16-normalised input, e = |O - O64|_F / |O64|_F, the kernel must keep e_kernel <= 2 e_torch per matrix (both carry independent bf16
rounding noise of the same size at the same points, only the summation order differs).  The parameters use the same rule on p - p0.
A rank-1 gradient must only stay finite (the iteration amplifies rounding noise in null directions by up to a^ns_steps); its errors
are recorded.  Every measured value is printed on a MUON_PARITY line; tools/muon_bench.py --parity collects the lines of a
`pytest -s` log into profiles/muon_parity.json.

Stage tests.  The five-iteration bar is wide (e_torch is 1e-2) and the iteration repairs small errors of its own products, so each
product is also pinned alone, with no tolerance: ns_coefficients isolates G X, (G G) X and a X in ONE iteration, and on a matrix in
{0, +1, -1} with 4^j non-zeros every sum the kernel forms is exact in fp32 in any order (tests/muon_ref.py), so the kernel must
equal R.probe_exact bit for bit.  O is read back from p (p0 = 0, lr = 1, no decay) as o = bf16(-p / alr), and fl32(-alr o) must
give p back.  The normalisation alone (ns_steps = 0) is exact on the Gaussian cases too; one Gaussian iteration with the default
coefficients is held to the noise between two accumulation orders of the reference (profiles/muon_stage_parity.json, written by
tests/test_muon_cpu.py).  tests/test_muon_cpu.py shows on the CPU that the designs are exact and that three kernel faults the
five-iteration bar lets through fail every one of these comparisons."""
import ctypes as C
import json
import os
import sys

import numpy as np

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import muon_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# [16, 64] / [64, 16]: one tile, both orientations.  [48, 272]: s not a power of two, n no multiple of the 32-column chunk.
# [96, 64]: transposed, the short side is 64.  [96, 3072]: the largest Gram matrix, X in the workspace.  [20, 100]: s no multiple
# of 16.  [16, 3072] / [3072, 16] / [32, 1536]: X fills the 96 KB of LDS exactly; [16, 3104] / [32, 1568]: one chunk more, the workspace.
SHAPES = [(16, 64), (64, 16), (48, 272), (96, 64), (96, 3072), (20, 100), (16, 3072), (3072, 16), (32, 1536), (16, 3104), (32, 1568)]
_CACHE = {}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The exact designs (R.sign_design): shape i of SHAPES takes seed DESIGN_SEED + i and the most non-zeros that fit, 4^j; (96, 3072)
# takes 4^8, one step sparser, because with 4^9 the product bf16(G G) X leaves the 24 bits (tests/test_muon_cpu.py).  The two-step
# "gram" run takes 4^(j-1) non-zeros at the shapes where the second iteration is then still exact: the one-tile shapes, [48, 272]
# (three tile rows, a ragged chunk) and [96, 64]; at the n >= 1536 shapes no design with every column filled keeps X1 X1^T exact.
DESIGN_SEED, TWO_STEP_SEED, MANY_SEED = 400, 450, 500
DESIGN_NONZEROS = {(96, 3072): 4 ** 8}
TWO_STEP_NONZEROS = {(16, 64): 4 ** 4, (64, 16): 4 ** 4, (48, 272): 4 ** 5, (96, 64): 4 ** 5}
NORM_MARGIN = 2.0 ** -14          # derived in test_normalisation_alone_is_bit_exact


def cases():
    """Per Gaussian shape, computed once and never modified: p0, g, buf0, the restatement's step from them, torch's O and O64."""
    from torch.optim._muon import _zeropower_via_newtonschulz
    if "cases" not in _CACHE:
        out = []
        for i, shape in enumerate(SHAPES):
            g, p0, b0 = R.make_matrix(shape, 100 + i), R.make_matrix(shape, 200 + i, 0.1), R.make_matrix(shape, 300 + i, 5e-3)
            pn, buf, o, x0 = R.step(p0, g, b0)
            u = torch.lerp(g, torch.lerp(b0, g, 1 - 0.95), 0.95)
            o_t = _zeropower_via_newtonschulz(u, R.COEFFS, 5, 1e-7).float()
            o64 = R.untranspose(R.ns_f64(x0), shape)
            out.append(dict(shape=shape, g=g, p0=p0, b0=b0, pn=pn, buf=buf, o=o, o_t=o_t, o64=o64))
        _CACHE["cases"] = out
    return _CACHE["cases"]


def run_kernel(mats, adjust_lr_fn=None, gnorm_sq=None, max_norm=0.0, grad_scale=1.0, **kw):
    """mats: (p, g, buf) fp32 CPU matrices -> the kernel's (p, buf) per matrix, from ONE table with 64-padded offsets; the slots'
    padding must come back untouched."""
    from qflux_amd import ops
    shapes = [tuple(m[0].shape) for m in mats]
    offs, n = R.flat_offsets(shapes)
    P, G, B = (torch.full((n,), 7.0, device=DEV) for _ in range(3))
    for off, (p, g, b) in zip(offs, mats):
        k = p.numel()
        P[off:off + k] = p.reshape(-1).to(DEV); G[off:off + k] = g.reshape(-1).to(DEV); B[off:off + k] = b.reshape(-1).to(DEV)
    lay = ops.muon_table(list(zip(offs, shapes)), adjust_lr_fn, device=DEV)
    ws = torch.zeros(lay.ws_bytes // 2, dtype=torch.bfloat16, device=DEV) if lay.ws_bytes else None
    K = dict(R.DEFAULTS, **kw)
    gn = None if gnorm_sq is None else torch.tensor(gnorm_sq, dtype=torch.float32, device=DEV)
    ops.muon_step(P, G, B, ws, lay, K["lr"], K["weight_decay"], K["momentum"], K["nesterov"], K["ns_coefficients"], K["eps"],
                  K["ns_steps"], gnorm_sq=gn, max_norm=max_norm, grad_scale=grad_scale)
    torch.cuda.synchronize()
    P, B = P.cpu(), B.cpu()
    res = []
    for off, s in zip(offs, shapes):
        k = s[0] * s[1]
        pad = (k + 63) // 64 * 64
        assert (P[off + k:off + pad] == 7.0).all() and (B[off + k:off + pad] == 7.0).all(), s
        res.append((P[off:off + k].view(s).clone(), B[off:off + k].view(s).clone()))
    return res


def stage_cases():
    """cases() with what the stage tests add, computed once: the update u, the normalised X0 and one default iteration from it in
    float64 (rounded to fp32 where the kernel holds fp32)."""
    if "stage" not in _CACHE:
        out = []
        for c in cases():
            u = torch.lerp(c["g"], c["buf"], 0.95)
            x0 = R.normalise(u, 1e-7)
            out.append(dict(c, u=u, x0=x0, x1=R.ns_staged(x0, R.COEFFS, 1)[0]))
        _CACHE["stage"] = out
    return _CACHE["stage"]


def exact_refs(key, specs, coeffs, ns_steps=1):
    """specs: (shape, seed, nonzeros) -> per matrix the design g and the exact O [rows, cols]; every product that reaches O must have
    passed R.exact_ok (G G does not when c = 0: it is multiplied by zero).  Computed once per key."""
    if key not in _CACHE:
        out = []
        for shape, seed, nz in specs:
            g = R.sign_design(shape, seed, nz)
            x, ok = R.ns_staged(R.normalise(g, 1e-7), coeffs, ns_steps)
            assert all(v for k, v in ok.items() if coeffs[2] != 0 or not k.startswith("gg")), (shape, ok)
            out.append((g, R.untranspose(x, shape).contiguous()))
        _CACHE[key] = out
    return _CACHE[key]


def read_o(pk, shape):
    """O from p after a step with p0 = 0, lr = 1 and no decay: p = fl32(-alr o) with alr the fp32 lr ratio of the table, so
    o = bf16(-p / alr) (the quotient is within 2^-23 of a bf16 number), and the read-back is checked by forming p from o again."""
    alr = float(np.float32(R.lr_ratio(None, *shape)))
    o = (-pk.double() / alr).to(R.BF)
    assert torch.equal((-alr * o.double()).float(), pk), shape
    return o


def run_exact(refs, coeffs, ns_steps=1):
    """The designs through the kernel with no momentum (buf0 = 0, momentum = 0, no Nesterov, grad_scale = 1): u = g, buf = g."""
    res = run_kernel([(torch.zeros_like(g), g, torch.zeros_like(g)) for g, _ in refs], lr=1.0, weight_decay=0.0, momentum=0.0,
                     nesterov=False, ns_coefficients=coeffs, ns_steps=ns_steps)
    out = []
    for (g, _), (pk, bk) in zip(refs, res):
        assert torch.equal(bk, g), tuple(g.shape)
        out.append(read_o(pk, tuple(g.shape)))
    return out


def assert_bit_equal(pairs):
    """pairs: (name, the kernel's O, the reference's) -- elementwise, no tolerance, nothing excluded.  Every matrix is looked at before
    the verdict, and a mismatch says where: a rounding effect has no tile structure, an indexing fault has."""
    bad = []
    for what, o_k, o_ref in pairs:
        if not torch.equal(o_k, o_ref):
            at = (o_k != o_ref).nonzero()
            rows, cols = sorted(set(at[:, 0].tolist())), sorted(set(at[:, 1].tolist()))
            bad.append(f"{what}: {len(at)} of {o_ref.numel()} elements differ, largest {int(R.bf16_ulps(o_k, o_ref).max())} bf16 steps; "
                       f"rows {rows[:16]} ({len(rows)}), cols {cols[:32]} ({len(cols)})")
    assert not bad, "\n".join(bad[:16] + [f"{len(bad)} matrices differ"])


def test_normalisation_alone_is_bit_exact():
    """ns_steps = 0 on the Gaussian cases: O = X0.  Everything on the way is elementwise and correctly rounded but the sum of squares.
    Its terms are exact in fp32 (squares of bf16 numbers) and positive; a term passes through at most d = 1152 + 6 + 2 fp32 additions
    (a thread's at most ceil(96 * 3072 / 256) terms in turn, six butterfly levels, the fold of the four waves), so the computed sum is
    S (1 + t) with |t| <= (1 + 2^-24)^d - 1 < 1161 * 2^-24 < 2^-13.8, its square root is off by at most 2^-14.8 + 2^-23 < 2^-14
    relative, and a float64 norm at least NORM_MARGIN = 2^-14 relative away from every bf16 rounding boundary rounds to the same bf16
    number in the kernel's order.  (2^-16 would do for sums of depth 2^8; the kernel's depth asks for the wider margin.)
    tests/test_muon_cpu.py holds the margin for the seeds of cases() and the restatement's own sum to the float64 norm."""
    cs = stage_cases()
    res = run_kernel([(torch.zeros_like(c["p0"]), c["g"], c["b0"]) for c in cs], lr=1.0, weight_decay=0.0, ns_steps=0)
    for c, (_, bk) in zip(cs, res):
        assert R.ulp_diff(bk, c["buf"]).max().item() <= 1.0, c["shape"]
    assert_bit_equal((f"X0 {c['shape']}", read_o(pk, c["shape"]), R.untranspose(c["x0"], c["shape"]).contiguous()) for c, (pk, _) in zip(cs, res))


@pytest.mark.parametrize("probe", list(R.PROBES))
def test_each_product_alone_is_bit_exact_on_the_sign_designs(probe):
    coeffs = R.PROBES[probe]
    refs = exact_refs(("probe", probe), [(s, DESIGN_SEED + i, DESIGN_NONZEROS.get(s)) for i, s in enumerate(SHAPES)], coeffs)
    assert all(bool(o_ref.any()) for _, o_ref in refs)
    assert_bit_equal((f"{probe} {tuple(g.shape)}", o_k, o_ref) for (g, o_ref), o_k in zip(refs, run_exact(refs, coeffs)))


def test_x_handed_to_a_second_iteration_is_bit_exact():
    coeffs = R.PROBES["gram"]
    refs = exact_refs("two_step", [(s, TWO_STEP_SEED + SHAPES.index(s), nz) for s, nz in TWO_STEP_NONZEROS.items()], coeffs, 2)
    one = exact_refs("two_step_1", [(s, TWO_STEP_SEED + SHAPES.index(s), nz) for s, nz in TWO_STEP_NONZEROS.items()], coeffs, 1)
    assert not any(torch.equal(o_ref, o_one) for (_, o_ref), (_, o_one) in zip(refs, one))
    assert_bit_equal((f"gram x 2 {tuple(g.shape)}", o_k, o_ref) for (g, o_ref), o_k in zip(refs, run_exact(refs, coeffs, 2)))


def test_more_matrices_than_workgroups_are_bit_exact():
    """258 matrices on 256 workgroups: workgroups 0 and 1 take table entries 256 and 257 after a [96, 64] (X image 64 x 96) and a
    [48, 272] (48 x 288) -- the one path on which X's padded image is zero-filled over a previous matrix's."""
    shapes = [(96, 64), (48, 272)] + [(16, 64)] * 254 + [(20, 100), (16, 64)]
    coeffs = R.PROBES["gram"]
    refs = exact_refs("many", [(s, MANY_SEED + i, None) for i, s in enumerate(shapes)], coeffs)
    assert len(refs) == 258 and int((refs[0][0] != 0).sum()) == 4 ** 6
    assert_bit_equal((f"entry {i} {tuple(g.shape)}", o_k, o_ref) for i, ((g, o_ref), o_k) in enumerate(zip(refs, run_exact(refs, coeffs))))


def test_one_gaussian_iteration_within_the_noise_between_two_reference_orders():
    """The comparison that cannot be exact: one iteration, default coefficients, Gaussian cases, against the float64-accumulated
    reference.  The bars are the reference's (profiles/muon_stage_parity.json, rule there): the differing share at most
    max(8 s_ref, 4 elements' worth) -- the kernel's order is a third draw of the same rounding noise and the measured counts are
    small -- and no element off by more than max(u_ref, 1) bf16 steps.  tests/test_muon_cpu.py shows that each of the three faults
    exceeds the share bar at least four times over at every shape.  QFX_MUON_STAGE_MEASURED_OUT=<file> writes the kernel's values."""
    with open(os.path.join(ROOT, "profiles", "muon_stage_parity.json")) as f:
        bars = json.load(f)["bar"]
    cs = stage_cases()
    res = run_kernel([(torch.zeros_like(c["p0"]), c["g"], c["b0"]) for c in cs], lr=1.0, weight_decay=0.0, ns_steps=1)
    measured, fails = {}, []
    for c, (pk, _) in zip(cs, res):
        key = "%dx%d" % c["shape"]
        d = R.bf16_ulps(read_o(pk, c["shape"]), R.untranspose(c["x1"], c["shape"]).contiguous())
        measured[key] = {"differing": int((d > 0).sum()), "share": float((d > 0).sum()) / d.numel(), "ulps": int(d.max())}
        print(f"MUON_PARITY one_step shape={c['shape']} differing={measured[key]['differing']} share={measured[key]['share']:.6e} "
              f"ulps={measured[key]['ulps']} bar_share={bars[key]['share']:.6e} bar_ulps={bars[key]['ulps']}")
        if measured[key]["share"] > bars[key]["share"] or measured[key]["ulps"] > bars[key]["ulps"]:
            fails.append((key, measured[key], bars[key]))
    if os.environ.get("QFX_MUON_STAGE_MEASURED_OUT"):
        with open(os.environ["QFX_MUON_STAGE_MEASURED_OUT"], "w") as f:
            json.dump(measured, f, indent=1)
    assert not fails, fails


def test_iteration_matches_restatement_within_the_references_own_error():
    """p0 = 0, lr = 1, no decay: p = -(lr ratio) O, so the kernel's O is read back from p."""
    cs = cases()
    res = run_kernel([(torch.zeros_like(c["p0"]), c["g"], c["b0"]) for c in cs], lr=1.0, weight_decay=0.0)
    worst = 0.0
    for c, (pk, bk) in zip(cs, res):
        assert torch.isfinite(pk).all() and torch.isfinite(bk).all(), c["shape"]
        ulp = R.ulp_diff(bk, c["buf"]).max().item()
        o_k = -pk.double() / R.lr_ratio(None, *c["shape"])
        e_t, e_r, e_k = R.rel_err(c["o_t"], c["o64"]), R.rel_err(c["o"], c["o64"]), R.rel_err(o_k, c["o64"])
        print(f"MUON_PARITY kernel shape={c['shape']} buf_ulp={ulp} e_torch={e_t:.6e} e_ref={e_r:.6e} e_kernel={e_k:.6e} "
              f"ratio={e_k / e_t:.4f} bit_equal_ref={bool(torch.equal(o_k.float(), c['o'].float()))}")
        worst = max(worst, e_k / e_t)
        assert ulp <= 1.0, (c["shape"], ulp)
        assert e_k <= 2 * e_t, (c["shape"], e_k, e_t)
    print(f"MUON_PARITY kernel worst_ratio={worst:.4f}")


def test_full_update_both_lr_adjustments_and_no_nesterov():
    cs = cases()
    for fn, nesterov in ((None, True), ("match_rms_adamw", False)):
        kw = dict(lr=1e-3, weight_decay=0.1, nesterov=nesterov, adjust_lr_fn=fn)
        res = run_kernel([(c["p0"], c["g"], c["b0"]) for c in cs], **kw)
        for c, (pk, bk) in zip(cs, res):
            pn, buf, o, x0 = R.step(c["p0"], c["g"], c["b0"], **kw)
            o64 = R.untranspose(R.ns_f64(x0), c["shape"])
            p0 = c["p0"].double()
            alr = 1e-3 * R.lr_ratio(fn, *c["shape"])
            d64 = p0 * (-1e-3 * 0.1) - alr * o64
            # the restatement IS torch's arithmetic here (tests/test_muon_cpu.py): its error stands for e_torch
            e_t, e_k = R.rel_err(pn.double() - p0, d64), R.rel_err(pk.double() - p0, d64)
            print(f"MUON_PARITY update fn={fn} nesterov={nesterov} shape={c['shape']} e_torch={e_t:.6e} e_kernel={e_k:.6e} ratio={e_k / e_t:.4f}")
            assert R.ulp_diff(bk, buf).max().item() <= 1.0, c["shape"]
            assert e_k <= 2 * e_t, (c["shape"], fn, e_k, e_t)


def test_zero_gradient_gives_only_the_decay_and_rank_one_stays_finite():
    shape = (16, 64)
    p0 = R.make_matrix(shape, 1, 0.1)
    z = torch.zeros(shape)
    g1 = R.make_matrix((48, 272), 2, rank1=True)
    p1 = torch.zeros(48, 272)
    (pz, bz), (pr, br), (pn, bn) = run_kernel([(p0, z, z), (p1, g1, torch.zeros_like(g1)), (p0, R.make_matrix(shape, 3), z)],
                                               lr=1.0, weight_decay=0.25)
    assert torch.equal(pz, p0 * 0.75) and not bz.any()                        # O = 0 exactly: lora_A at step 1
    assert torch.isfinite(pr).all() and torch.isfinite(br).all() and pr.any()
    assert torch.isfinite(pn).all() and not torch.equal(pn, p0)
    _, _, o, x0 = R.step(p1, g1, torch.zeros_like(g1), lr=1.0, weight_decay=0.25)
    o64 = R.ns_f64(x0)
    from torch.optim._muon import _zeropower_via_newtonschulz
    o_t = _zeropower_via_newtonschulz(torch.lerp(g1, g1 * torch.tensor(1 - 0.95), 0.95), R.COEFFS, 5, 1e-7).float()
    print(f"MUON_PARITY rank1 shape=(48, 272) e_torch={R.rel_err(o_t, o64):.6e} e_ref={R.rel_err(o, o64):.6e} e_kernel={R.rel_err(-pr, o64):.6e}")


def test_matrix_with_an_inf_is_skipped_whole_while_its_neighbours_step():
    cs = cases()[:3]
    g_bad = cs[1]["g"].clone()
    g_bad[5, 3] = float("inf")
    res = run_kernel([(cs[0]["p0"], cs[0]["g"], cs[0]["b0"]), (cs[1]["p0"], g_bad, cs[1]["b0"]), (cs[2]["p0"], cs[2]["g"], cs[2]["b0"])])
    good = run_kernel([(c["p0"], c["g"], c["b0"]) for c in cs])
    assert torch.equal(res[1][0], cs[1]["p0"]) and torch.equal(res[1][1], cs[1]["b0"])
    for i in (0, 2):
        assert torch.equal(res[i][0], good[i][0]) and torch.equal(res[i][1], good[i][1]) and not torch.equal(res[i][0], cs[i]["p0"])


def test_clip_path_equals_an_unclipped_call_on_the_prescaled_gradient():
    """g' = g * clip is a rounding point: the clipped launch must give the bits of a launch on the gradient scaled beforehand (a
    kernel that contracts the product into the momentum's difference does not).  The coefficient is formed on the device in one
    call and on the host for the other; the scalars are chosen so that no rounding can differ between the two (sqrt(16) * 0.5 = 2
    is exact, the last factor a power of two: both round the same sum and the same quotient)."""
    cs = cases()[:4]
    gsq, max_norm, grad_scale = 16.0, 0.05, 0.5
    clip = R.clip_coef(gsq, max_norm, grad_scale)
    assert 0.0124 < clip < 0.0126
    a = run_kernel([(c["p0"], c["g"] * 20.0, c["b0"]) for c in cs], gnorm_sq=gsq, max_norm=max_norm, grad_scale=grad_scale)
    b = run_kernel([(c["p0"], (c["g"] * 20.0) * torch.tensor(float(clip)), c["b0"]) for c in cs])
    plain = run_kernel([(c["p0"], c["g"] * 20.0, c["b0"]) for c in cs])
    for (pa, ba), (pb, bb), (_, bp) in zip(a, b, plain):
        assert torch.equal(pa, pb) and torch.equal(ba, bb) and not torch.equal(ba, bp)


def test_two_runs_give_identical_bits():
    cs = cases()
    runs = [run_kernel([(c["p0"], c["g"], c["b0"]) for c in cs]) for _ in range(2)]
    for (pa, ba), (pb, bb), c in zip(runs[0], runs[1], cs):
        assert torch.equal(pa, pb) and torch.equal(ba, bb) and not torch.equal(pa, c["p0"]), c["shape"]


def test_invalid_arguments_launch_nothing():
    from qflux_amd import _lib as L, ops
    shape = (16, 64)
    p0, g = R.make_matrix(shape, 1, 0.1), R.make_matrix(shape, 2)
    P, G, B = p0.reshape(-1).to(DEV), g.reshape(-1).to(DEV), torch.zeros(1024, device=DEV)
    lay = ops.muon_table([(0, shape)], None, device=DEV)
    for bad in (dict(lr=-1.0), dict(weight_decay=-0.1), dict(momentum=-0.5), dict(ns_steps=100), dict(ns_steps=-1), dict(eps=0.0)):
        K = dict(R.DEFAULTS, **bad)
        with pytest.raises(L.QfxError):
            ops.muon_step(P, G, B, None, lay, K["lr"], K["weight_decay"], K["momentum"], K["nesterov"], K["ns_coefficients"], K["eps"],
                          K["ns_steps"])

    def raw(**kw):
        f = dict(p=P.data_ptr(), g=G.data_ptr(), buf=B.data_ptr(), table=lay.table.data_ptr(), n_tensors=1, nesterov=1, ns_steps=5,
                 lr=1e-3, weight_decay=0.1, momentum=0.95, one_minus_momentum=0.05, a=R.COEFFS[0], b=R.COEFFS[1], c=R.COEFFS[2], eps=1e-7,
                 grad_scale=1.0)
        f.update(kw)
        a = L.MuonArgs()
        for n, v in f.items():
            setattr(a, n, v)
        return L.lib.qfx_muon_step(C.byref(a), None)
    for kw in (dict(n_tensors=-1), dict(table=None), dict(p=None), dict(g=None), dict(buf=None), dict(ws=None, ws_bytes=64)):
        assert raw(**kw) == -1, kw
    assert raw(n_tensors=0, table=None) == 0                                       # does nothing
    torch.cuda.synchronize()
    assert torch.equal(P.cpu(), p0.reshape(-1)) and not B.any()
    with pytest.raises(ValueError):
        ops.muon_table([(0, (97, 128))], None)
    with pytest.raises(ValueError):
        ops.muon_step(P, G, B, None, ops.muon_table([(0, (96, 3072))], None, device=DEV), 1e-3)     # no workspace for a layout that needs one


def _three_steps_against_references(step, model, run):
    """Three train steps; the gradients, clip scalars and parameters of every optimizer step are captured, then torch.optim.Muon,
    the restatement and the float64 iteration are stepped on the same clipped gradients, per matrix, on the CPU."""
    st = model.lora_store
    ents = [(p.shape, off, k) for _, p, off, k in st.entries]
    p0 = st.pflat.detach().cpu().clone()
    rec, orig = [], step.optimizer_step

    def capture(grad_scale=1.0):
        g = st.gflat.detach().cpu().clone()
        orig(grad_scale=grad_scale)
        rec.append((g, float(step._gnorm.item()), float(grad_scale)))
    step.optimizer_step = capture
    for _ in range(3):
        assert torch.isfinite(run()).all()
    assert len(rec) == 3
    pk, bk = st.pflat.detach().cpu(), step.opt_state.buf.cpu()
    lr, wd = step.lr, step.weight_decay
    worst = 0.0
    for i, (shape, off, k) in enumerate(ents):
        start = p0[off:off + k].view(shape)
        pt = torch.nn.Parameter(start.clone())
        opt = torch.optim.Muon([pt], lr=lr, weight_decay=wd)
        pr, br, p64 = start.clone(), torch.zeros(shape), start.double()
        for g, gsq, gs in rec:
            gi = g[off:off + k].view(shape) * torch.tensor(float(R.clip_coef(gsq, step.max_grad_norm, gs)))
            pt.grad = gi.clone()
            opt.step()
            pr, br, _, x0 = R.step(pr, gi, br, lr=lr, weight_decay=wd)
            p64 = p64 * (1 - lr * wd) - lr * R.lr_ratio(None, *shape) * R.untranspose(R.ns_f64(x0), shape)
        d64 = p64 - start.double()
        e_t, e_k = R.rel_err(pt.detach().double() - start.double(), d64), R.rel_err(pk[off:off + k].view(shape).double() - start.double(), d64)
        ulp = R.ulp_diff(bk[off:off + k].view(shape), br).max().item()
        print(f"MUON_PARITY train entry={i} shape={tuple(shape)} buf_ulp={ulp} e_torch={e_t:.6e} e_kernel={e_k:.6e}")
        assert torch.equal(br, opt.state[pt]["momentum_buffer"])
        assert ulp <= 1.0, (i, ulp)
        assert e_k <= 2 * e_t, (i, tuple(shape), e_k, e_t)
        worst = max(worst, e_k / e_t if e_t > 0 else 0.0)
    print(f"MUON_PARITY train worst_ratio={worst:.4f}")
    assert not torch.equal(pk, p0)


def test_three_qwen_train_steps_against_references_on_the_same_gradients():
    from common import TINY
    from parity_util import build_pair, tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    _, m = build_pair(dict(TINY), device=DEV, targets=("to_k", "to_q", "to_v", "to_out.0", "img_mlp.net.2"), seed=2)
    step = QwenLoraTrainStep(m, lr=1e-3, optimizer="muon")
    assert step.weight_decay == 0.1 and step.optimizer_args["momentum"] == 0.95
    e, nz, u = tiny_embeddings(seed=5)
    _three_steps_against_references(step, m, lambda: step.train_step(e, noise=nz, u=u))
    sd = step.state_dict()
    assert sd["global_step"] == 3 and set(sd["state"][0]) == {"momentum_buffer"}


def test_three_flux_train_steps_against_references_on_the_same_gradients():
    from common import FLUX_TINY
    from oracle import flux_dit as FO
    from qflux_amd.models import FluxTransformer2DModel
    from qflux_amd.modules import LoraConfig
    from qflux_amd.trainer import FluxKontextTrainStep
    cfg = dict(FLUX_TINY, joint_attention_dim=64, guidance_embeds=True)
    with torch.device(DEV):
        m = FluxTransformer2DModel(**cfg)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_((torch.randn(p.shape, generator=g) * (0.5 / p.shape[-1] ** 0.5 if p.ndim == 2 else 0.05) + (1.0 if "norm_" in n and p.ndim == 1 else 0.0)).to(p.dtype))
    m.add_adapter(LoraConfig(r=4, lora_alpha=8), "a", generator=g)
    step = FluxKontextTrainStep(m, lr=1e-3, optimizer="muon")
    ctl = FO.prepare_latent_image_ids(4, 6); ctl[:, 0] = 1
    emb = dict(image_latents=torch.randn(2, 24, 64, generator=g).half(), control_latents=torch.randn(2, 24, 64, generator=g).half(),
               control_ids=ctl, text_ids=torch.zeros(7, 3), latent_hw=(4, 6),
               pooled_prompt_embeds=torch.randn(2, 16, generator=g).half(), prompt_embeds=torch.randn(2, 7, 64, generator=g).half())
    noise = torch.randn(2, 24, 64, generator=g)
    _three_steps_against_references(step, m, lambda: step.train_step(emb, noise=noise, t=torch.tensor([0.3, 0.8])))


def test_class_steps_bit_identically_to_the_train_step_and_exchanges_checkpoints():
    from common import TINY
    from parity_util import build_pair
    from qflux_amd import optim as O
    from qflux_amd.trainer import QwenLoraTrainStep
    a, b = (build_pair(dict(TINY), device=DEV, seed=2)[1] for _ in range(2))
    sa, sb = a.lora_store, b.lora_store
    start = sa.pflat.detach().clone()
    kw = dict(lr=2e-3, weight_decay=0.05, momentum=0.9, adjust_lr_fn="match_rms_adamw")
    opt = O.Muon([p for n, p in a.named_parameters() if "lora_" in n], **kw)
    args = {"momentum": 0.9, "adjust_lr_fn": "match_rms_adamw"}
    step = QwenLoraTrainStep(b, lr=2e-3, weight_decay=0.05, max_grad_norm=0, optimizer="muon", optimizer_args=args)

    def grad(it):
        g = (torch.randn(sa.gflat.shape, generator=torch.Generator().manual_seed(50 + it)) * 1e-2).to(DEV)
        for m in (a, b):
            m.lora_store.gflat.copy_(g)
    for it in range(3):
        grad(it)
        opt.step()
        step.optimizer_step()
        opt.zero_grad()
        step.zero_grad()
    assert not torch.equal(sa.pflat, start) and torch.equal(sa.pflat, sb.pflat)
    assert torch.equal(opt._opt_state.buf, step.opt_state.buf) and bool(step.opt_state.buf.any())
    sd = opt.state_dict()
    assert sd["global_step"] == 3 and list(sd["state"]) == list(step.state_dict()["state"])
    step2 = QwenLoraTrainStep(b, lr=0.5, max_grad_norm=0, optimizer="muon")
    step2.load_state_dict(sd)
    assert step2.lr == 2e-3 and step2.global_step == 3 and step2.optimizer_args["adjust_lr_fn"] == "match_rms_adamw"
    grad(3)
    opt.step()
    step2.optimizer_step()
    assert torch.equal(sa.pflat, sb.pflat)
