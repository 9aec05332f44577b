"""CPU: the exact comparison rule of the blockwise 8-bit kernels (tests/bnb8_ref.py) and the inputs tests/test_blockwise8_gpu.py runs
(tests/blockwise8_ref.py), judged from the restatement alone: the margin and tie classification at the values where it turns, the
undecided share of every GPU input against bnb8_ref.UNDECIDED_CAP, the layout claims (more table entries than two sweeps of the
launch below a million elements, both modes on consecutive trips of one workgroup in both orders, every tail length, every offset
class the builder accepts) and the branch-reach claims (sign repairs, codes 0 and 255 written, extreme block maxima, skipped
elements that still hold the block maximum, the code of 0.0 from a zero block)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util  # noqa: E402,F401  (puts the package on sys.path)
import blockwise8_ref as W  # noqa: E402
import bnb8_ref as B  # noqa: E402

FAM_BS = [(f, bs) for f in W.FAMILIES for bs in (256, 2048)]


def _ulps(x, n):
    x = np.float32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, np.float32(np.inf if n > 0 else -np.inf), dtype=np.float32)
    return float(x)


@pytest.mark.parametrize("signed", [True, False])
def test_margin_classifies_midpoints_their_neighbours_and_zero(signed):
    q = W.QMAP[signed]
    mid = B.midpoints(q)
    ks = [130, 200, 254] if signed else [1, 77, 254]
    vals, want = [1.0], [False]                                  # the block maximum itself: x = 1, far above the last midpoint
    for k in ks:
        m = float(mid[k])
        for d, und in ((0, True), (1, True), (-1, True), (64, False), (-64, False)):
            vals.append(_ulps(m, d)); want.append(und)
    vals += [0.0, -0.0]; want += [False, False]                  # 0 / mx is exact, the sign bit is nobody's rounding
    if signed:
        vals += [-float(mid[200]), 1e-30, -1e-30]; want += [True, False, False]
    m = torch.tensor(vals, dtype=torch.float32)
    und, mx = B.undecided_codes(m, m.double(), torch.zeros(m.numel(), dtype=torch.long), 1, q, signed)
    assert mx.tolist() == [1.0] and und.tolist() == want
    margin, bound = B.code_margin(m, torch.ones_like(m), q, signed)
    assert margin.dtype == torch.float64 and bool((bound[1:16] > 0).all())
    # a block whose maximum is 0 divides nothing: decided
    z = torch.zeros(5)
    assert not B.undecided_codes(z, z.double(), torch.zeros(5, dtype=torch.long), 1, q, signed)[0].any()


def test_a_tied_block_maximum_makes_its_block_undecided():
    q = W.QMAP[True]
    m = torch.tensor([1.0, _ulps(1.0, -1), 0.3, 0.5, 0.25])
    blk = torch.tensor([0, 0, 0, 1, 1])
    tied = m.double().clone()
    tied[1] = 1.0 - 1e-9                                          # within 4 fp32 ulp of the maximum in double, one ulp apart in fp32
    assert B.tied_blocks(m, tied, blk, 2).tolist() == [True, False]
    assert B.undecided_codes(m, tied, blk, 2, q, True)[0].tolist() == [True, True, True, False, False]
    assert B.tied_blocks(m, m.double(), blk, 2).tolist() == [True, False]            # one fp32 ulp IS within four
    far = m.double().clone()
    far[1] = 0.9
    assert B.tied_blocks(m, far, blk, 2).tolist() == [False, False]
    same = torch.tensor([1.0, 1.0, -1.0])                                             # equal fp32 magnitudes do not round apart
    assert not B.tied_blocks(same, same.double(), torch.zeros(3, dtype=torch.long), 1).any()


def test_sign_repair_is_the_boundary_at_zero():
    q = W.QMAP[True]
    m = torch.tensor([-1e-9, 1e-9, 1.0, -0.0, 0.0, -1.0])
    mx = torch.ones_like(m)
    assert B.sign_repaired(m, mx, q).tolist() == [True, False, False, True, False, False]
    c = B.keep_sign(B.quantize(m, q), m, q)
    assert c.tolist() == [126, 127, 255, 126, 127, 0]
    assert B.ulp_diff(torch.tensor([1.0, -0.0]), torch.tensor([_ulps(1.0, 3), 0.0])) == 3
    assert not B.same_bits(torch.tensor([0.0]), torch.tensor([-0.0])) and B.same_bits(m, m.clone())


@pytest.mark.parametrize("name", W.CASE_NAMES)
@pytest.mark.parametrize("fam,bs", FAM_BS)
def test_undecided_share_of_every_gpu_input(fam, bs, name):
    """From the restatement alone, on exactly the states and gradients the GPU tests launch (plain entry, and the grouped entry
    where the GPU test runs it): the undecided share is within the cap, and the restatement's own output is finite."""
    c = W.case(name, bs)
    for grouped in ((False, True) if name == "stride" else (False,)):
        out, info = c.reference(fam, grouped)
        total = info["codes"] + (info["elements"] if fam == "lion" else 0)
        share = info["undecided"] / max(1, total)
        print(f"{fam} bs={bs} {name} grouped={grouped}: {info['undecided']} undecided of {total} ({share:.2e}), {info['repaired']} sign repairs")
        assert share <= B.UNDECIDED_CAP, (fam, bs, name, grouped, share)
        assert torch.isfinite(out.p).all() and torch.isfinite(out.absmax).all() and torch.isfinite(out.m32).all()
        assert B.same_bits(out.g, c.state(fam).g)


@pytest.mark.parametrize("bs", [256, 2048])
def test_stride_layout_exceeds_two_sweeps_and_mixes_modes_along_every_chain(bs):
    from qflux_amd import ops
    c = W.case("stride", bs)
    per_sweep = ops.grouped_sweep_elems(bs) // bs                 # table entries one launch covers without striding
    trips, ps = c.trips()
    assert ps == per_sweep and c.lay.n_blocks > 2 * per_sweep and trips == math.ceil(c.lay.n_blocks / per_sweep) >= 3
    assert c.n < 1_000_000 and c.lay.n_blocks >= (4200 if bs == 2048 else 16500)
    modes, lens = [], []
    for off, k, e8, a0, nb, s0 in c.lay.tensors:
        n = (k + bs - 1) // bs
        modes += [bool(e8)] * n
        lens += [min(bs, k - j * bs) for j in range(n)]
    assert len(modes) == c.lay.n_blocks
    if bs == 256:                                                  # a 257-element tensor: a full entry and a 1-element entry
        i = next(i for i, (_, k, *_r) in enumerate(c.lay.tensors) if k == 257)
        first = sum((t[1] + bs - 1) // bs for t in c.lay.tensors[:i])
        assert lens[first:first + 2] == [256, 1] and modes[first:first + 2] == [True, True]
    else:
        assert all(k <= bs for _, k, *_r in c.lay.tensors)        # one short entry per tensor
    seen, third = set(), set()
    for w in range(per_sweep):                                     # the entries one workgroup (2048) or wave (256) walks
        chain = modes[w::per_sweep]
        seen |= set(zip(chain, chain[1:]))
        if len(chain) >= 3:
            third.add(chain[2])
    assert seen >= {(True, False), (False, True)}                  # 8-bit then fp32 and fp32 then 8-bit, on consecutive trips
    assert third == {True, False}                                  # third trips exist, in both modes
    per_group = {gi: {bool(t[2]) for t, a in zip(c.lay.tensors, c.assign()) if a == gi} for gi in range(3)}
    assert all(v == {True, False} for v in per_group.values())     # every group holds tensors of both modes


@pytest.mark.parametrize("bs", [256, 2048])
def test_tail_layouts_hold_every_length_and_offset_class_and_the_builder_refuses_the_rest(bs):
    from qflux_amd import ops
    for name, eight in (("tails8", True), ("tails32", False)):
        c = W.case(name, bs)
        assert {t[2] for t in c.lay.tensors} == {eight}
        want = {k * bs + j for k in (0, 1) for j in (1, 2, 3, 4, 5, 7, 8, 9)} | {bs - 1, bs - 5}
        assert set(c.sizes) == want
        assert {off % 64 for off, _ in c.entries} == set(range(0, 64, 4))
        end = W.GUARD
        for off, k in c.entries:                                   # canary words before, between and behind the tensors
            assert off >= end and off % 4 == 0
            end = off + k + 1
        assert end + W.GUARD - 1 <= c.n and c.n % 64 == 0
    for bad in (1, 2, 3, 5, 62):                                   # offsets that are no multiple of 4 elements are refused, not aligned
        with pytest.raises(ValueError):
            ops.adam8bit_block_table([(bad, 300)], bs, 256)


@pytest.mark.parametrize("fam,bs", FAM_BS)
def test_extreme_states_reach_the_sign_repair_and_both_end_codes(fam, bs):
    c = W.case("extreme", bs)
    S = c.state(fam)
    out, info = c.reference(fam)
    off0, a0 = c.entries[0][0], c.lay.tensors[0][3]
    nab = c.lay.n_absmax
    for j, sg in enumerate(W.PLANES[fam]):
        for b, code in enumerate((0, 255, W.ZERO_CODE[sg])):
            assert (S.codes[j][off0 + b * bs:off0 + (b + 1) * bs] == code).all()
        assert S.absmax[j][a0 + 3] == 0 and S.codes[j][off0 + 3 * bs:off0 + 4 * bs].ne(W.ZERO_CODE[sg]).any()
        am = S.absmax[j][:nab]
        assert float(am[am > 0].min()) == W.TINY and float(am.max()) == 1e4
        hist = torch.bincount(S.codes[j][c.X.pos].long(), minlength=256)
        assert int((hist > 0).sum()) == 256                        # every code occurs in the state the step starts from
    g = S.g[c.X.pos]
    assert bool((g > 0).any()) and bool((g < 0).any())
    print(f"{fam} bs={bs} extreme: {info['repaired']} sign repairs, {info['code0']} codes 0 and {info['code255']} codes 255 written")
    assert info["repaired"] >= 36 and info["code0"] > 0 and info["code255"] > 0
    # some first moments crossed zero: the decoded old sign and the new code's sign differ
    q = W.QMAP[True]
    e = c.X.pos[c.X.eight]
    old, new = q[S.codes[0][e].long()] * S.absmax[0][c.X.blk[c.X.eight]], q[out.codes[0][e].long()]
    assert int(((old > 0) & (new < 0)).sum()) > 36 and int(((old < 0) & (new > 0)).sum()) > 36


@pytest.mark.parametrize("fam,bs", FAM_BS)
def test_skipped_elements_keep_their_state_and_still_hold_the_block_maximum(fam, bs):
    c = W.case("skips", bs)
    S = c.state(fam)
    out, info = c.reference(fam)
    off0, a0 = c.entries[0][0], c.lay.tensors[0][3]
    assert [t[2] for t in c.lay.tensors] == [True, False, True]
    for b in range(3):
        i = off0 + b * bs + W.SKIP_AT
        assert not math.isfinite(float(S.g[i]))
        assert B.same_bits(out.p[i], S.p[i])
        blk = slice(off0 + b * bs, off0 + (b + 1) * bs)
        assert not B.same_bits(out.p[blk], S.p[blk]) and int((out.p[blk] != S.p[blk]).sum()) == bs - 1      # the neighbours stepped
        for j in range(len(W.PLANES[fam])):
            assert out.codes[j][i] == S.codes[j][i] == 255
            assert B.same_bits(out.absmax[j][a0 + b], S.absmax[j][a0 + b])      # the skipped element's old moment is the maximum
    off1, s1 = c.entries[1][0], c.lay.tensors[1][5]
    for i in (5, 50):
        assert B.same_bits(out.p[off1 + i], S.p[off1 + i]) and B.same_bits(out.m32[:, s1 + i], S.m32[:, s1 + i])
    assert int((out.m32[0, s1:s1 + 100] != S.m32[0, s1:s1 + 100]).sum()) == 98


@pytest.mark.parametrize("fam,bs", FAM_BS)
def test_first_step_from_zero_state_stores_the_code_of_zero_for_a_zero_block(fam, bs):
    c = W.case("zero", bs)
    S = c.state(fam)
    out, info = c.reference(fam)
    off0, a0 = c.entries[0][0], c.lay.tensors[0][3]
    assert not S.codes[:, c.X.pos[c.X.eight]].any() and not S.absmax[:, :c.lay.n_absmax].any() and c.t == 1
    for j, sg in enumerate(W.PLANES[fam]):
        assert out.absmax[j][a0 + 1] == 0 and (out.codes[j][off0 + bs:off0 + 2 * bs] == W.ZERO_CODE[sg]).all()
        assert out.absmax[j][a0] > 0 and out.absmax[j][a0 + 2] > 0


@pytest.mark.parametrize("bs", [256, 2048])
def test_undecided_share_of_the_adam_files_inputs(bs):
    """tests/test_adam8bit_gpu.py holds its two restatement tests to the same rule and cap, on bnb8_ref.file_reference's inputs:
    the same steps here, without a device."""
    for which in B.file_cases(bs):
        opt, steps = B.file_reference(which, bs)
        for it, (grads, gsq) in enumerate(steps):
            opt.step([g.clone() for g in grads], gnorm_sq=gsq, max_norm=B.KW["max_norm"], grad_scale=B.KW["grad_scale"])
            tot, n_und = B.census(opt, bs)
            print(f"adam8bit file inputs bs={bs} {which} step {it}: {n_und} undecided of {tot}")
            assert n_und <= B.UNDECIDED_CAP * tot, (bs, which, it, n_und, tot)


@pytest.mark.parametrize("bs", [256, 2048])
def test_every_family_is_handed_the_norm_of_its_own_gradients(bs):
    """The families draw different states before their gradients, so their norms differ; the restatement and the launch both read
    clipargs_of(fam), whatever was built before or after."""
    c = W.case("tails8", bs)
    first = {f: c.clipargs_of(f) for f in W.FAMILIES}
    refs = {f: c.reference(f) for f in reversed(W.FAMILIES)}
    assert len({v[0] for v in first.values()}) == 3
    for f in W.FAMILIES:
        g = c.state(f).g[c.X.pos].double()
        assert c.clipargs_of(f) == first[f] == (float(np.float32(float(g.pow(2).sum()))), 1.0, 0.5)
        again, _ = W.step_ref(f, c.state(f), c.X, W.HPS[f], c.t, c.clipargs_of(f))
        assert B.same_bits(again.p, refs[f][0].p)


def test_front_canaries_stand_before_the_block_maxima_and_the_fp32_moments():
    c = W.case("skips", 256)
    S = c.state("ademamix")
    out, _ = c.reference("ademamix")
    for raw, view in ((out.absmax_raw, out.absmax), (out.m32_raw, out.m32)):
        assert (raw[:W.GUARD] == W.CANARY).all() and view.shape[0] == 3 and (view[:, -W.GUARD:] == W.CANARY).all()
        assert view.data_ptr() == raw.data_ptr() + 4 * W.GUARD
    assert not B.same_bits(out.absmax_raw, S.absmax_raw) and not B.same_bits(out.m32_raw, S.m32_raw)


def test_an_undecided_lion_parameter_must_hold_one_of_the_three_signs_values():
    c = W.case("zero", 256)
    want, info = c.reference("lion")
    i = int(c.X.pos[7])
    fake = dict(info, p_und=info["p_und"].clone())
    fake["p_und"][i] = True
    lr = W.HPS["lion"][0]["lr"]
    for s, ok in ((0.0, True), (2.0, True), (1.0, True), (0.5, False), (3.0, False)):      # want took one sign; the others lie lr and 2 lr off
        got = want.clone()
        got.p[i] = fake["p_alts"][0, i] + torch.tensor(lr) * s if s != 0.0 else want.p[i]
        if s in (1.0, 2.0):
            got.p[i] = fake["p_alts"][int(s), i]
        if ok:
            W.compare("lion", got, want, fake, ("lion", s))
        else:
            with pytest.raises(AssertionError):
                W.compare("lion", got, want, fake, ("lion", s))
