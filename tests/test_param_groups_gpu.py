"""GPU: parameter groups in the fused optimizers.

Stitch tests (exact, no tolerance): every grouped kernel against its ungrouped parent run once per group on a fresh copy with that
group's scalars and the same gnorm_sq -- each tensor's slice taken from the run of its group must be torch.equal on p and on every
state buffer.  Against torch / the restatements under tests/: the bars of the existing single-group tests of the same family
(tests/test_kernels_gpu.py::test_adamw_matches_torch and tests/test_sgd_gpu.py: 1e-5 of the largest reference element;
tests/test_lion_gpu.py and tests/test_adam8bit_gpu.py: 1e-6 on p, rtol 1e-6 on moments and absmax, codes within one step, Lion's
undecided cap).  Round trips and the train step's LoRA+ shorthand are bit comparisons."""
import pytest
import torch

import bnb8_ref as R8
import lion_ref as RL
from test_optim_classes_gpu import _grad, _lora_params, _set_grad, _twins

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES, ASSIGN = [1, 63, 64, 65, 4099], [0, 1, 0, 2, 1]          # the layout of tests/test_param_groups_cpu.py
BAR = 1e-5


def _layout(extra=0):
    """LoraStore's layout of SIZES (+ one tensor of `extra` elements in group 2): (offset, numel) per tensor, assignment, flat length."""
    sizes, assign = SIZES + ([extra] if extra else []), ASSIGN + ([2] if extra else [])
    entries, off = [], 0
    for k in sizes:
        entries.append((off, k))
        off += (k + 63) // 64 * 64
    return entries, assign, off


def _rand(n, seed, scale=1.0, positive=False):
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale
    return (x.abs() if positive else x).to(DEV)


def _stitch(entries, assign, n, runs, grouped, whole_slots=True):
    """runs[k]: the buffers after the ungrouped run with group k's scalars; grouped: after the grouped run.  Every tensor's slice
    (with the padding behind it, which the flat kernels step with the tensor's group) comes from the run of its group."""
    for i, ((off, k), gi) in enumerate(zip(entries, assign)):
        end = (entries[i + 1][0] if i + 1 < len(entries) else n) if whole_slots else off + k
        for name in grouped:
            assert torch.equal(grouped[name][off:end], runs[gi][name][off:end]), (name, i, k, gi)


def _cases():
    from qflux_amd import ops
    return [0, ops.grouped_sweep_elems(0) + 12345]       # the second: the stride loop of the 16-byte form runs twice


# lr / betas / eps / wd per group; group 1 has lr = 0 and wd = 0: p keeps its bits, the moments move
ADAM_ROWS = [(3e-3, 0.9, 0.999, 1e-8, 0.01), (0.0, 0.8, 0.95, 1e-6, 0.0), (4.8e-2, 0.95, 0.99, 1e-7, 0.1)]
LION_ROWS = [(1e-3, 0.9, 0.99, 0.01), (0.0, 0.8, 0.95, 0.0), (1.6e-2, 0.95, 0.98, 0.1)]
SGD_ROWS = [(0.05, 0.9, 0.0, 1e-4, True), (0.0, 0.8, 0.1, 0.0, False), (0.2, 0.0, 0.0, 1e-3, False)]      # group 2: no momentum


def _flat_inputs(n):
    g = _rand(n, 2, 0.3)
    gsq = (g.double() ** 2).sum().float().reshape(())
    assert float(gsq) > 4.0          # max_norm 1: the clip is active
    return _rand(n, 1), g, gsq


@pytest.mark.parametrize("big", [False, True])
def test_adamw_grouped_stitches_bit_exactly(big):
    from qflux_amd import ops
    entries, assign, n = _layout(_cases()[1] if big else 0)
    p0, g, gsq = _flat_inputs(n)
    m0, v0 = _rand(n, 3, 0.1), _rand(n, 4, 0.01, positive=True)
    tg = ops.tile_group_map(entries, assign, 3, numel=n, device=DEV)
    runs = []
    for lr, b1, b2, eps, wd in ADAM_ROWS:
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        ops.adamw_step(p, g, m, v, lr, b1, b2, eps, wd, 2, gnorm_sq=gsq, max_norm=1.0, grad_scale=0.5)
        runs.append(dict(p=p, m=m, v=v))
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    ops.adamw_step_grouped(p, g, m, v, tg, ADAM_ROWS, 2, gnorm_sq=gsq, max_norm=1.0, grad_scale=0.5)
    _stitch(entries, assign, n, runs, dict(p=p, m=m, v=v))
    for (off, k), gi in zip(entries, assign):
        if gi == 1:
            assert torch.equal(p[off:off + k], p0[off:off + k]) and not torch.equal(m[off:off + k], m0[off:off + k])
            assert not torch.equal(v[off:off + k], v0[off:off + k])
        else:
            assert not torch.equal(p[off:off + k], p0[off:off + k])
    if not big:      # one group: the grouped kernel is the ungrouped kernel, bit for bit
        p1, m1, v1 = p0.clone(), m0.clone(), v0.clone()
        ops.adamw_step_grouped(p1, g, m1, v1, torch.zeros_like(tg), ADAM_ROWS[:1], 2, gnorm_sq=gsq, max_norm=1.0, grad_scale=0.5)
        assert torch.equal(p1, runs[0]["p"]) and torch.equal(m1, runs[0]["m"]) and torch.equal(v1, runs[0]["v"])
        # views off a 16-byte boundary take the scalar form: the same bits
        pu, gu, mu, vu = (torch.cat([x.new_zeros(1), x])[1:] for x in (p0, g, m0, v0))
        ops.adamw_step_grouped(pu, gu, mu, vu, tg, ADAM_ROWS, 2, gnorm_sq=gsq, max_norm=1.0, grad_scale=0.5)
        assert torch.equal(pu, p) and torch.equal(mu, m) and torch.equal(vu, v)


@pytest.mark.parametrize("big", [False, True])
def test_sgd_grouped_stitches_bit_exactly(big):
    from qflux_amd import ops
    entries, assign, n = _layout(_cases()[1] if big else 0)
    p0, g, gsq = _flat_inputs(n)
    b0 = _rand(n, 5, 0.2)
    tg = ops.tile_group_map(entries, assign, 3, numel=n, device=DEV)
    for first in (False, True):
        runs = []
        for lr, mom, damp, wd, nes in SGD_ROWS:
            p, b = p0.clone(), b0.clone()
            ops.sgd_step(p, g, b if mom else None, lr, mom, damp, wd, nes, first=first, gnorm_sq=gsq, max_norm=1.0, grad_scale=0.5)
            runs.append(dict(p=p, b=b))
        p, b = p0.clone(), b0.clone()
        ops.sgd_step_grouped(p, g, b, tg, SGD_ROWS, first=first, gnorm_sq=gsq, max_norm=1.0, grad_scale=0.5)
        _stitch(entries, assign, n, runs, dict(p=p, b=b))
        for (off, k), gi in zip(entries, assign):
            assert torch.equal(p[off:off + k], p0[off:off + k]) == (gi == 1)
            assert torch.equal(b[off:off + k], b0[off:off + k]) == (gi == 2)      # a group without momentum leaves its buffer alone
    p1, b1 = p0.clone(), b0.clone()
    ops.sgd_step_grouped(p1, g, b1, torch.zeros_like(tg), SGD_ROWS[:1], first=True, gnorm_sq=gsq, max_norm=1.0, grad_scale=0.5)
    assert torch.equal(p1, runs[0]["p"]) and torch.equal(b1, runs[0]["b"])


@pytest.mark.parametrize("big", [False, True])
def test_lion_grouped_stitches_bit_exactly(big):
    from qflux_amd import ops
    entries, assign, n = _layout(_cases()[1] if big else 0)
    p0, g, gsq = _flat_inputs(n)
    m0 = _rand(n, 3, 0.1)
    tg = ops.tile_group_map(entries, assign, 3, numel=n, device=DEV)
    runs = []
    for lr, b1, b2, wd in LION_ROWS:
        p, m = p0.clone(), m0.clone()
        ops.lion_step(p, g, m, lr, b1, b2, wd, gnorm_sq=gsq, max_norm=1.0, grad_scale=0.5)
        runs.append(dict(p=p, m=m))
    p, m = p0.clone(), m0.clone()
    ops.lion_step_grouped(p, g, m, tg, LION_ROWS, gnorm_sq=gsq, max_norm=1.0, grad_scale=0.5)
    _stitch(entries, assign, n, runs, dict(p=p, m=m))
    for (off, k), gi in zip(entries, assign):
        assert torch.equal(p[off:off + k], p0[off:off + k]) == (gi == 1) and not torch.equal(m[off:off + k], m0[off:off + k])
    p1, m1 = p0.clone(), m0.clone()
    ops.lion_step_grouped(p1, g, m1, torch.zeros_like(tg), LION_ROWS[:1], gnorm_sq=gsq, max_norm=1.0, grad_scale=0.5)
    assert torch.equal(p1, runs[0]["p"]) and torch.equal(m1, runs[0]["m"])


class _Blockwise:
    """Random blockwise 8-bit state over a layout: codes, positive absmax, fp32 moments of the small tensors."""

    def __init__(self, entries, n, bs, moments):
        from qflux_amd import ops
        self.lay = ops.adam8bit_block_table(entries, bs, 4096, device=DEV)
        gen = torch.Generator().manual_seed(11)
        self.moments = moments
        self.bufs = dict(p=_rand(n, 1))
        for j in range(1, moments + 1):
            self.bufs[f"q{j}"] = torch.randint(0, 256, (n,), generator=gen, dtype=torch.uint8).to(DEV)
            self.bufs[f"a{j}"] = (torch.rand(max(1, self.lay.n_absmax), generator=gen) * (0.1 if j == 1 else 0.01) + 1e-4).to(DEV)
            self.bufs[f"f{j}"] = _rand(max(1, self.lay.n_fp32), 20 + j, 0.1 if j == 1 else 0.01, positive=j == 2)
        self.qm = [R8.create_dynamic_map(True).to(DEV), R8.create_dynamic_map(False).to(DEV)]

    def copy(self):
        return {k: v.clone() for k, v in self.bufs.items()}

    def compare(self, grouped, runs, assign):
        for (off, k, eight, a0, nb, s0), gi in zip(self.lay.tensors, assign):
            assert torch.equal(grouped["p"][off:off + k], runs[gi]["p"][off:off + k]), ("p", k, gi)
            for j in range(1, self.moments + 1):
                if eight:
                    assert torch.equal(grouped[f"q{j}"][off:off + k], runs[gi][f"q{j}"][off:off + k]), ("codes", j, k, gi)
                    assert torch.equal(grouped[f"a{j}"][a0:a0 + nb], runs[gi][f"a{j}"][a0:a0 + nb]), ("absmax", j, k, gi)
                    assert not torch.equal(grouped[f"a{j}"][a0:a0 + nb], self.bufs[f"a{j}"][a0:a0 + nb])
                else:
                    assert torch.equal(grouped[f"f{j}"][s0:s0 + k], runs[gi][f"f{j}"][s0:s0 + k]), ("fp32 moment", j, k, gi)
                    assert not torch.equal(grouped[f"f{j}"][s0:s0 + k], self.bufs[f"f{j}"][s0:s0 + k])
            assert torch.equal(grouped["p"][off:off + k], self.bufs["p"][off:off + k]) == (gi == 1), (k, gi)


@pytest.mark.parametrize("bs,big", [(256, False), (2048, False), (256, True), (2048, True)])
def test_adam8bit_grouped_stitches_bit_exactly(bs, big):
    from qflux_amd import ops
    entries, assign, n = _layout(ops.grouped_sweep_elems(bs) + 12345 if big else 0)
    _, g, gsq = _flat_inputs(n)
    S = _Blockwise(entries, n, bs, 2)
    bg = ops.block_group_map(S.lay, assign, 3, device=DEV)

    def run(b, fn, *hyper):
        fn(b["p"], g, b["q1"], b["q2"], b["a1"], b["a2"], b["f1"], b["f2"], S.lay, S.qm[0], S.qm[1], *hyper, 2, gnorm_sq=gsq, max_norm=1.0,
           grad_scale=0.5)
        return b
    runs = [run(S.copy(), ops.adam8bit_step, lr, (b1, b2), eps, wd) for lr, b1, b2, eps, wd in ADAM_ROWS]
    grouped = run(S.copy(), ops.adam8bit_step_grouped, bg, ADAM_ROWS)
    S.compare(grouped, runs, assign)
    one = run(S.copy(), ops.adam8bit_step_grouped, torch.zeros_like(bg), ADAM_ROWS[:1])
    assert all(torch.equal(one[k], runs[0][k]) for k in one)


@pytest.mark.parametrize("bs,big", [(256, False), (2048, False), (256, True), (2048, True)])
def test_lion8bit_grouped_stitches_bit_exactly(bs, big):
    from qflux_amd import ops
    entries, assign, n = _layout(ops.grouped_sweep_elems(bs) + 12345 if big else 0)
    _, g, gsq = _flat_inputs(n)
    S = _Blockwise(entries, n, bs, 1)
    bg = ops.block_group_map(S.lay, assign, 3, device=DEV)

    def run(b, fn, *hyper):
        fn(b["p"], g, b["q1"], b["a1"], b["f1"], S.lay, S.qm[0], *hyper, gnorm_sq=gsq, max_norm=1.0, grad_scale=0.5)
        return b
    runs = [run(S.copy(), ops.lion8bit_step, lr, (b1, b2), wd) for lr, b1, b2, wd in LION_ROWS]
    grouped = run(S.copy(), ops.lion8bit_step_grouped, bg, LION_ROWS)
    S.compare(grouped, runs, assign)
    one = run(S.copy(), ops.lion8bit_step_grouped, torch.zeros_like(bg), LION_ROWS[:1])
    assert all(torch.equal(one[k], runs[0][k]) for k in one)


# ---------------------------------------------------------------- map entries past n_groups (include/qfx.h: they take the last row)
def _out_of_range(valid):
    """The map with two entries of the last group (1 of 2) replaced by 2 and by 255."""
    bad = valid.clone()
    ones = (valid == 1).nonzero().flatten()
    assert ones.numel() >= 2
    bad[ones[0]], bad[ones[-1]] = 2, 255
    return bad


def test_lion_grouped_map_entries_past_n_groups_take_the_last_row():
    from qflux_amd import ops
    entries, assign, n = _layout()
    assign = [min(a, 1) for a in assign]
    p0, g, gsq = _flat_inputs(n)
    m0 = _rand(n, 3, 0.1)
    tg = ops.tile_group_map(entries, assign, 2, numel=n, device=DEV)
    outs = []
    for tmap in (tg, _out_of_range(tg)):
        p, m = p0.clone(), m0.clone()
        ops.lion_step_grouped(p, g, m, tmap, LION_ROWS[:2], gnorm_sq=gsq, max_norm=1.0, grad_scale=0.5)
        pu, gu, mu = (torch.cat([x.new_zeros(1), x])[1:] for x in (p0, g, m0))          # the scalar form
        ops.lion_step_grouped(pu, gu, mu, tmap, LION_ROWS[:2], gnorm_sq=gsq, max_norm=1.0, grad_scale=0.5)
        assert torch.equal(pu, p) and torch.equal(mu, m)
        outs.append((p, m))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and not torch.equal(outs[0][1], m0)


@pytest.mark.parametrize("family,bs", [("adam8bit", 256), ("adam8bit", 2048), ("lion8bit", 256), ("lion8bit", 2048)])
def test_blockwise_grouped_map_entries_past_n_groups_take_the_last_row(family, bs):
    from qflux_amd import ops
    entries, assign, n = _layout()
    assign = [min(a, 1) for a in assign]
    _, g, gsq = _flat_inputs(n)
    S = _Blockwise(entries, n, bs, 2 if family == "adam8bit" else 1)
    bg = ops.block_group_map(S.lay, assign, 2, device=DEV)
    outs = []
    for bmap in (bg, _out_of_range(bg)):
        b = S.copy()
        if family == "adam8bit":
            ops.adam8bit_step_grouped(b["p"], g, b["q1"], b["q2"], b["a1"], b["a2"], b["f1"], b["f2"], S.lay, S.qm[0], S.qm[1], bmap, ADAM_ROWS[:2], 2,
                                      gnorm_sq=gsq, max_norm=1.0, grad_scale=0.5)
        else:
            ops.lion8bit_step_grouped(b["p"], g, b["q1"], b["a1"], b["f1"], S.lay, S.qm[0], bmap, LION_ROWS[:2], gnorm_sq=gsq, max_norm=1.0,
                                      grad_scale=0.5)
        outs.append(b)
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0]) and not torch.equal(outs[0]["q1"], S.bufs["q1"])


# ---------------------------------------------------------------- against torch, on the tiny Qwen model of test_optim_classes_gpu.py
def _cpu_groups(groups):
    """The same groups over fp32 CPU copies of the parameters."""
    return [dict(g, params=[torch.nn.Parameter(p.detach().cpu().clone()) for p in g["params"]]) for g in groups]


@pytest.mark.parametrize("name,kw", [("AdamW", dict(betas=(0.9, 0.999), eps=1e-8)), ("SGD", dict(momentum=0.9, nesterov=True))])
def test_loraplus_groups_with_a_scheduler_match_torch(name, kw):
    from qflux_amd import optim as O
    a, _ = _twins()
    st = a.lora_store
    groups = O.loraplus_param_groups(a, 3e-3, 16, weight_decay=0.01, b_weight_decay=0.0)
    fused = getattr(O, name)(groups, **kw)
    ref_groups = _cpu_groups(groups)
    stock = getattr(torch.optim, name)(ref_groups, **kw)
    sched = [torch.optim.lr_scheduler.LambdaLR(o, lambda s: 1.0 / (1 + s)) for o in (fused, stock)]
    where = {id(p): (off, k) for _, p, off, k in st.entries}
    for it in range(3):
        g = _grad(st, it)
        _set_grad((a,), g)
        for grp, rg in zip(groups, ref_groups):
            for p, q in zip(grp["params"], rg["params"]):
                off, k = where[id(p)]
                q.grad = g[off:off + k].view(p.shape).cpu().clone()
        fused.step(); stock.step()
        for s in sched:
            s.step()
        assert [g_["lr"] for g_ in fused.param_groups] == [g_["lr"] for g_ in stock.param_groups]
    assert fused.param_groups[1]["lr"] == pytest.approx(16 * fused.param_groups[0]["lr"]) and fused.param_groups[0]["lr"] < 3e-3
    assert fused._opt_state.group_map is not None
    worst = 0.0
    for grp, rg in zip(groups, ref_groups):
        for p, q in zip(grp["params"], rg["params"]):
            ref = q.detach()
            rel = float((p.detach().cpu() - ref).abs().max() / ref.abs().max())
            worst = max(worst, rel)
            assert rel <= BAR, (tuple(p.shape), rel)
    print(f"{name} LoRA+ vs torch: worst relative error {worst:.3e}")
    # torch's own multi-group file loads into the fused class and continues with it
    sd = stock.state_dict()
    fused2 = getattr(O, name)(groups, **kw)
    fused2.load_state_dict(sd)
    for n_, buf in fused._opt_state.buffers():
        assert torch.allclose(dict(fused2._opt_state.buffers())[n_], buf, rtol=1e-4, atol=1e-9), n_


def _ref_sizes():
    sizes, assign = [1000, 4096, 5000, 300], [0, 1, 0, 1]
    entries, off = [], 0
    for k in sizes:
        entries.append((off, k)); off += (k + 63) // 64 * 64
    return sizes, assign, entries, off


def test_lion_grouped_matches_the_restatement_run_once_per_group():
    """tests/lion_ref.py once per group, one re-synchronised step from the state its own first step left (fp32 and 8-bit moment)."""
    from qflux_amd import ops
    sizes, assign, entries, n = _ref_sizes()
    rows = [(1e-3, 0.9, 0.99, 0.01), (1.6e-2, 0.95, 0.98, 0.0)]
    gen = torch.Generator().manual_seed(5)
    params = [torch.randn(k, generator=gen) * 0.1 for k in sizes]
    grads = [[torch.randn(k, generator=gen) for k in sizes] for _ in range(2)]
    gsq = [float(sum(g.double().pow(2).sum() for g in gs)) for gs in grads]
    for min8, bs in ((None, 256), (4096, 256), (4096, 2048)):
        refs = [RL.LionRef([params[i].clone() for i in range(4) if assign[i] == k], lr=r[0], betas=r[1:3], weight_decay=r[3],
                           min_8bit_size=min8, blocksize=bs) for k, r in enumerate(rows)]
        for k, ref in enumerate(refs):
            ref.step([grads[0][i] for i in range(4) if assign[i] == k], gnorm_sq=gsq[0], max_norm=1.0, grad_scale=0.5)
        of = {i: (assign[i], [j for j in range(4) if assign[j] == assign[i]].index(i)) for i in range(4)}
        p, g = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        lay = ops.adam8bit_block_table(entries, bs, min8 or 1 << 40, device=DEV)
        q1, a1 = torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros(max(1, lay.n_absmax), device=DEV)
        m32 = torch.zeros(max(1, lay.n_fp32), device=DEV)
        for i, (off, k, eight, a0, nb, s0) in enumerate(lay.tensors):
            ref, j = refs[of[i][0]], of[i][1]
            p[off:off + k] = ref.params[j].to(DEV); g[off:off + k] = grads[1][i].to(DEV)
            stt = ref.state[j]
            if min8 is None:
                m32[s0:s0 + k] = stt["exp_avg"].to(DEV)
            elif eight:
                q1[off:off + k] = stt["state1"].to(DEV); a1[a0:a0 + nb] = stt["absmax1"].to(DEV)
            else:
                m32[s0:s0 + k] = stt["state1"].to(DEV)
        gn = torch.tensor(gsq[1], dtype=torch.float32, device=DEV)
        if min8 is None:
            m = torch.zeros(n, device=DEV)
            for i, (off, k, _, _, _, s0) in enumerate(lay.tensors):
                m[off:off + k] = m32[s0:s0 + k]
            ops.lion_step_grouped(p, g, m, ops.tile_group_map(entries, assign, 2, numel=n, device=DEV), rows, gnorm_sq=gn, max_norm=1.0,
                                  grad_scale=0.5)
        else:
            ops.lion8bit_step_grouped(p, g, q1, a1, m32, lay, RL.create_dynamic_map(True).to(DEV), ops.block_group_map(lay, assign, 2, device=DEV),
                                      rows, gnorm_sq=gn, max_norm=1.0, grad_scale=0.5)
        for k, ref in enumerate(refs):
            ref.step([grads[1][i] for i in range(4) if assign[i] == k], gnorm_sq=gsq[1], max_norm=1.0, grad_scale=0.5)
        n_und = 0
        for i, (off, k, eight, a0, nb, s0) in enumerate(lay.tensors):
            ref, j = refs[of[i][0]], of[i][1]
            und = ref.undecided[j]
            err = (p[off:off + k].cpu() - ref.params[j]).abs() / ref.params[j].abs().max()
            assert err[~und].max().item() <= 1e-6, (min8, bs, i)
            n_und += int(und.sum())
            stt = ref.state[j]
            if min8 is None:
                assert torch.allclose(m[off:off + k].cpu(), stt["exp_avg"], rtol=1e-6, atol=0)
            elif eight:
                assert torch.allclose(a1[a0:a0 + nb].cpu(), stt["absmax1"], rtol=1e-6, atol=0)
                assert (q1[off:off + k].cpu().long() - stt["state1"].long()).abs().max().item() <= 1
            else:
                assert torch.allclose(m32[s0:s0 + k].cpu(), stt["state1"], rtol=1e-6, atol=0)
        assert n_und <= RL.UNDECIDED_CAP * sum(sizes)


@pytest.mark.parametrize("bs", [256, 2048])
def test_adam8bit_grouped_matches_the_restatement_run_once_per_group(bs):
    """tests/bnb8_ref.py once per group: one re-synchronised step (t = 2) from the state its own first step left."""
    from qflux_amd import ops
    sizes, assign, entries, n = _ref_sizes()
    rows = [(1e-3, 0.9, 0.999, 1e-8, 0.01), (1.6e-2, 0.95, 0.99, 1e-6, 0.0)]
    gen = torch.Generator().manual_seed(6)
    params = [torch.randn(k, generator=gen) * 0.1 for k in sizes]
    grads = [[torch.randn(k, generator=gen) for k in sizes] for _ in range(2)]
    gsq = [float(sum(g.double().pow(2).sum() for g in gs)) for gs in grads]
    refs = [R8.Adam8bitRef([params[i].clone() for i in range(4) if assign[i] == k], lr=r[0], betas=r[1:3], eps=r[3], weight_decay=r[4],
                           blocksize=bs) for k, r in enumerate(rows)]
    for k, ref in enumerate(refs):
        ref.step([grads[0][i] for i in range(4) if assign[i] == k], gnorm_sq=gsq[0], max_norm=1.0, grad_scale=0.5)
    of = {i: (assign[i], [j for j in range(4) if assign[j] == assign[i]].index(i)) for i in range(4)}
    lay = ops.adam8bit_block_table(entries, bs, 4096, device=DEV)
    p, g = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    q = [torch.zeros(n, dtype=torch.uint8, device=DEV) for _ in range(2)]
    am = [torch.zeros(max(1, lay.n_absmax), device=DEV) for _ in range(2)]
    f32 = [torch.zeros(max(1, lay.n_fp32), device=DEV) for _ in range(2)]
    for i, (off, k, eight, a0, nb, s0) in enumerate(lay.tensors):
        ref, j = refs[of[i][0]], of[i][1]
        p[off:off + k] = ref.params[j].to(DEV); g[off:off + k] = grads[1][i].to(DEV)
        for x in (0, 1):
            if eight:
                q[x][off:off + k] = ref.state[j][f"state{x + 1}"].reshape(-1).to(DEV); am[x][a0:a0 + nb] = ref.state[j][f"absmax{x + 1}"].to(DEV)
            else:
                f32[x][s0:s0 + k] = ref.state[j][f"state{x + 1}"].reshape(-1).to(DEV)
    ops.adam8bit_step_grouped(p, g, q[0], q[1], am[0], am[1], f32[0], f32[1], lay, R8.create_dynamic_map(True).to(DEV),
                              R8.create_dynamic_map(False).to(DEV), ops.block_group_map(lay, assign, 2, device=DEV), rows, 2,
                              gnorm_sq=torch.tensor(gsq[1], dtype=torch.float32, device=DEV), max_norm=1.0, grad_scale=0.5)
    for k, ref in enumerate(refs):
        ref.step([grads[1][i] for i in range(4) if assign[i] == k], gnorm_sq=gsq[1], max_norm=1.0, grad_scale=0.5)
    for i, (off, k, eight, a0, nb, s0) in enumerate(lay.tensors):
        ref, j = refs[of[i][0]], of[i][1]
        pr = ref.params[j]
        assert ((p[off:off + k].cpu() - pr).abs() / pr.abs().max()).max().item() <= 1e-6, (bs, i)
        for x in (0, 1):
            stt = ref.state[j]
            if eight:
                assert torch.allclose(am[x][a0:a0 + nb].cpu(), stt[f"absmax{x + 1}"], rtol=1e-6, atol=0)
                assert (q[x][off:off + k].cpu().long() - stt[f"state{x + 1}"].reshape(-1).long()).abs().max().item() <= 1
            else:
                assert torch.allclose(f32[x][s0:s0 + k].cpu(), stt[f"state{x + 1}"].reshape(-1), rtol=1e-6, atol=0)


# ---------------------------------------------------------------- round trips, train step
CLASSES = [("AdamW", dict(betas=(0.9, 0.999))), ("Adam8bit", dict(min_8bit_size=1024)), ("SGD", dict(momentum=0.9)),
           ("Lion", {}), ("Lion8bit", dict(min_8bit_size=1024))]


@pytest.mark.parametrize("name,kw", CLASSES, ids=[c[0] for c in CLASSES])
def test_save_load_round_trip_is_bit_equal_to_an_uninterrupted_run(name, kw):
    from qflux_amd import optim as O
    a, b = _twins()
    groups = lambda m: O.loraplus_param_groups(m, 1e-3, 16, weight_decay=0.01, b_weight_decay=0.0)      # noqa: E731
    whole, first = getattr(O, name)(groups(a), **kw), getattr(O, name)(groups(b), **kw)
    for it in range(6):
        _set_grad((a,), _grad(a.lora_store, it))
        whole.step()
    for it in range(3):
        _set_grad((b,), _grad(b.lora_store, it))
        first.step()
    sd = first.state_dict()
    assert len(sd["param_groups"]) == 2 and sd["param_groups"][1]["lr"] == 16 * sd["param_groups"][0]["lr"]
    n0 = len(sd["param_groups"][0]["params"])
    assert sd["param_groups"][0]["params"] == list(range(n0)) and sd["param_groups"][1]["params"] == list(range(n0, 2 * n0))
    second = getattr(O, name)(groups(b), **kw)
    second.load_state_dict(sd)
    assert [g["lr"] for g in second.param_groups] == [g["lr"] for g in first.param_groups]
    for it in range(3, 6):
        _set_grad((b,), _grad(b.lora_store, it))
        second.step()
    assert torch.equal(a.lora_store.pflat, b.lora_store.pflat)
    for (n_, x), (_, y) in zip(whole._opt_state.buffers(), second._opt_state.buffers()):
        assert torch.equal(x, y), n_


def test_train_step_and_class_exchange_grouped_checkpoints():
    from qflux_amd import optim as O
    from qflux_amd.trainer import QwenLoraTrainStep
    a, b = _twins()
    rules = [{"match": r"lora_A", "lr": 1e-3, "weight_decay": 0.01}, {"match": r"lora_B", "lr": 1.6e-2, "weight_decay": 0.0}]
    step = QwenLoraTrainStep(b, lr=1e-3, weight_decay=0.01, max_grad_norm=0, optimizer="adamw", param_groups=rules)
    opt = O.AdamW(O.loraplus_param_groups(a, 1e-3, 16, weight_decay=0.01, b_weight_decay=0.0))
    for it in range(2):
        g = _grad(a.lora_store, it)
        _set_grad((a, b), g)
        opt.step(); step.optimizer_step()
    assert torch.equal(a.lora_store.pflat, b.lora_store.pflat)
    sd_cls, sd_step = opt.state_dict(), step.state_dict()
    assert [g_["params"] for g_ in sd_cls["param_groups"]] == [g_["params"] for g_ in sd_step["param_groups"]]
    opt2 = O.AdamW(O.loraplus_param_groups(a, 0.5, 2))
    opt2.load_state_dict(sd_step)
    step2 = QwenLoraTrainStep(b, lr=0.5, max_grad_norm=0, optimizer="adamw", param_groups=[dict(r, lr=0.5) for r in rules])
    step2.load_state_dict(sd_cls)
    g = _grad(a.lora_store, 2)
    _set_grad((a, b), g)
    opt2.step(); step2.optimizer_step()
    assert torch.equal(a.lora_store.pflat, b.lora_store.pflat)
    for (n_, x), (_, y) in zip(opt2._opt_state.buffers(), step2.opt_state.buffers()):
        assert torch.equal(x, y), n_
    with pytest.raises(ValueError, match="different number of parameter groups"):
        O.AdamW(_lora_params(a)).load_state_dict(sd_step)


def test_train_step_loraplus_ratio_is_the_two_groups_spelled_out():
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    a, b = _twins()
    start = a.lora_store.pflat.clone()
    emb = tiny_embeddings(seed=300)[0]
    gen = torch.Generator().manual_seed(3)
    noise, u = torch.randn(emb["image_latents"].shape, generator=gen), torch.rand(emb["image_latents"].shape[0], generator=gen)
    s1 = QwenLoraTrainStep(a, lr=1e-3, weight_decay=0.01, loraplus_lr_ratio=16)
    s2 = QwenLoraTrainStep(b, lr=1e-3, weight_decay=0.01, param_groups=[{"match": "lora_A", "lr": 1e-3}, {"match": "lora_B", "lr": 1.6e-2}])
    for s in (s1, s2):
        s.train_step(emb, noise=noise, u=u)
    assert s1.opt_state.group_map is not None and s2.opt_state.key == s1.opt_state.key
    assert torch.equal(a.lora_store.pflat, b.lora_store.pflat)
    moved = (a.lora_store.pflat - start).abs()
    for n_, _, off, k in a.lora_store.entries:      # AdamW's first step moves every element with a gradient by about its group's lr
        top = float(moved[off:off + k].max())
        assert (top > 8e-3) == ("lora_B" in n_) or top == 0.0, (n_, top)
