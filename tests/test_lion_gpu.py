"""GPU: the fused Lion steps (qfx_lion_step, qfx_lion8bit_step) against their CPU restatement (tests/lion_ref.py), their determinism,
the trainer / checkpoint path with optimizer="lion" / "lion8bit_blockwise", and the torch.optim classes in the stock loop.

The parameter comparison: the restatement's bits on every element but those where the restatement itself calls the sign of
c = m b1 + (1 - b1) g' undecided (lion_ref.update: the clip coefficient is formed on the host there and on the device here, and a
last-bit difference in g' can turn a near-cancelled sign, which moves p by 2 lr).  That set is computed from the restatement alone
and may hold at most lion_ref.UNDECIDED_CAP of the compared elements per step; tests/test_lion_cpu.py checks that the shared inputs
keep within it."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnb8_ref as B  # noqa: E402
import lion_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# attention adapters (1024 elements: fp32 moment) and the feed-forward down projection's LoRA-A (4096: 8-bit); see test_adam8bit_gpu.py
TARGETS = ("to_k", "to_q", "to_v", "to_out.0", "img_mlp.net.2")
SIZES = R.SIZES


def _check_params(pk, p_ref, und, where):
    """One tensor's parameters against the restatement's outside the undecided set; returns the set's size."""
    assert torch.isfinite(pk).all(), where
    assert B.same_bits(pk[~und], p_ref.reshape(-1)[~und]), (where, "parameters", B.ulp_diff(pk[~und], p_ref.reshape(-1)[~und]))
    return int(und.sum())


def _check_state8(got_m32, got_a1, got_codes, st, m64, bs, where):
    """One tensor's state under the exact rule of bnb8_ref: the fp32 moment or the block maxima bit for bit, every decided code
    identical, an undecided one within one step.  Returns (codes compared, undecided codes)."""
    if st["state1"].dtype != torch.uint8:
        assert B.same_bits(got_m32, st["state1"].reshape(-1)), (where, "fp32 moment")
        return 0, 0
    assert B.same_bits(got_a1, st["absmax1"]), (where, "block maxima")
    k = st["_m"].numel()
    und, _ = B.undecided_codes(st["_m"], m64, torch.arange(k) // bs, st["absmax1"].numel(), st["qmap1"], True)
    B.check_codes(got_codes, st["state1"], und, where)
    return k, int(und.sum())


def test_fp32_kernel_matches_restatement():
    from qflux_amd import ops
    offs, n = R.flat_offsets(SIZES)
    p, g, m = (torch.zeros(n, device=DEV) for _ in range(3))
    for it, rec in enumerate(R.run_reference(None, 0.0)):
        p0, s0 = rec["before"]
        p.zero_(); g.zero_(); m.zero_()
        for off, pt, st, gr in zip(offs, p0, s0, rec["grads"]):                 # re-synchronised: one step at a time is compared
            k = pt.numel()
            p[off:off + k] = pt.to(DEV); g[off:off + k] = gr.to(DEV)
            if st:
                m[off:off + k] = st["exp_avg"].to(DEV)
        gn = torch.tensor(rec["gsq"], dtype=torch.float32, device=DEV)
        ops.lion_step(p, g, m, R.KW["lr"], *R.KW["betas"], 0.0, gnorm_sq=gn, max_norm=R.KW["max_norm"], grad_scale=R.KW["grad_scale"])
        torch.cuda.synchronize()
        p1, s1 = rec["after"]
        n_und = 0
        for i, (off, pt, st) in enumerate(zip(offs, p1, s1)):
            k = pt.numel()
            n_und += _check_params(p[off:off + k].cpu(), pt, rec["undecided"][i], (it, k))
            assert torch.allclose(m[off:off + k].cpu(), st["exp_avg"], rtol=1e-6, atol=0), (it, k)
            pad = (k + 63) // 64 * 64
            assert not p[off + k:off + pad].any() and not m[off + k:off + pad].any()    # zero slots stay zero: sgn(0) = 0
        print(f"lion fp32 step {it}: {n_und} undecided of {sum(SIZES)}")
        assert n_und <= R.UNDECIDED_CAP * sum(SIZES)


def test_fp32_kernel_unaligned_and_odd_lengths():
    """The 16-byte path needs aligned buffers and handles n % 4 itself; views that start off a 16-byte boundary take the scalar path.
    Both must give the bits of the aligned run on the same values."""
    from qflux_amd import ops
    g0 = torch.Generator().manual_seed(7)
    n = 1027
    vals = [torch.randn(n, generator=g0) * s for s in (0.1, 1.0, 0.01)]
    outs = []
    for shift in (0, 1):
        bufs = [torch.zeros(n + 8, device=DEV) for _ in range(3)]
        p, g, m = (b[shift:shift + n] for b in bufs)
        for t, v in zip((p, g, m), vals):
            t.copy_(v.to(DEV))
        ops.lion_step(p, g, m, 1e-3, 0.9, 0.99, 0.01)
        torch.cuda.synchronize()
        outs.append((p.cpu(), m.cpu()))
        assert not bufs[0][shift + n:].any() and not bufs[2][shift + n:].any() and not bufs[0][:shift].any()      # nothing past the end
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    K = R.step_scalars(1e-3, 0.9, 0.99, 0.01)
    pr, mr, und = R.update(vals[0], vals[1], vals[2], K)
    assert torch.equal(outs[0][1], mr) and torch.equal(outs[0][0][~und], pr[~und])      # no clip: the same fp32 operations, the same bits


def test_fp32_kernel_clip_active_aligned_and_offset_view():
    """The clip at work (coefficient ~ 1/16) at the smallest length with a 16-byte body and a scalar tail, on an aligned buffer and on
    a view one element in (the scalar instantiation): both runs give the same bits, and those are the restatement's, as in the clip-free case
    above (the coefficient is formed on the host there, on the device here, by the same fp32 operations)."""
    from qflux_amd import ops
    g0 = torch.Generator().manual_seed(7)
    n = 4 * 256 + 3
    vals = [torch.randn(n, generator=g0) * s for s in (0.1, 1.0, 0.01)]
    gsq = float(vals[1].double().pow(2).sum())
    clip = R.clip_coef(gsq, R.KW["max_norm"], R.KW["grad_scale"])
    assert clip < 0.1 * R.KW["grad_scale"]                                 # the clip is active
    outs = []
    for shift in (0, 1):
        bufs = [torch.zeros(n + 8, device=DEV) for _ in range(3)]
        p, g, m = (b[shift:shift + n] for b in bufs)
        for t, v in zip((p, g, m), vals):
            t.copy_(v.to(DEV))
        ops.lion_step(p, g, m, 1e-3, 0.9, 0.99, 0.01, gnorm_sq=torch.tensor(gsq, dtype=torch.float32, device=DEV),
                      max_norm=R.KW["max_norm"], grad_scale=R.KW["grad_scale"])
        torch.cuda.synchronize()
        outs.append((p.cpu(), m.cpu()))
        assert not bufs[0][shift + n:].any() and not bufs[2][shift + n:].any() and not bufs[0][:shift].any()      # nothing past the end
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    pr, mr, und = R.update(vals[0], vals[1] * torch.tensor(clip), vals[2], R.step_scalars(1e-3, 0.9, 0.99, 0.01))
    n_und = _check_params(outs[0][0], pr, und, n)
    print(f"lion fp32 clipped n={n}: {n_und} undecided")
    # bnb8_ref.clip_coef restates the prologue's fp32 operations one by one (correctly rounded sqrt and division on both sides): the
    # same coefficient, so the same bits as the clip-free case above asks for
    assert torch.equal(outs[0][1], mr) and torch.equal(outs[0][0][~und], pr[~und])
    assert n_und <= R.UNDECIDED_CAP * sum(SIZES)


@pytest.mark.parametrize("n", [64 * 4 + 3, 4096 * 1024 + 64 + 3])
def test_fp32_kernels_quad_body_tail_and_second_trip(n):
    """qfx_lion_step and qfx_lion_step_grouped (two rows, alternating 64-element tiles) at a length with a 16-byte body and an n % 4
    tail, and at one where 4096 workgroups of 256 quads leave a second trip of the stride loop with such a tail behind it; the short
    length also through views one float in (the scalar instantiation).  No clip: the restatement's bits, as in
    test_fp32_kernel_unaligned_and_odd_lengths."""
    from qflux_amd import ops
    g0 = torch.Generator().manual_seed(9)
    vals = [torch.randn(n, generator=g0) * s for s in (0.1, 1.0, 0.01)]
    rows = [(1e-3, 0.9, 0.99, 0.01), (1.6e-2, 0.95, 0.98, 0.0)]
    refs = [R.update(vals[0], vals[1], vals[2], R.step_scalars(*r)) for r in rows]
    tg = (torch.arange((n + 63) // 64) % 2).to(torch.uint8)
    sel = tg.repeat_interleave(64)[:n].bool()
    pr, mr, und = (torch.where(sel, refs[1][i], refs[0][i]) for i in range(3))
    assert int(und.sum()) + int(refs[0][2].sum()) <= R.UNDECIDED_CAP * 2 * n
    for shift in (0, 1) if n < 1024 else (0,):
        for grouped in (False, True):
            bufs = [torch.zeros(n + 8, device=DEV) for _ in range(3)]
            p, g, m = (b[shift:shift + n] for b in bufs)
            for t, v in zip((p, g, m), vals):
                t.copy_(v.to(DEV))
            if grouped:
                ops.lion_step_grouped(p, g, m, tg.to(DEV), rows)
            else:
                ops.lion_step(p, g, m, *rows[0])
            torch.cuda.synchronize()
            wp, wm, wu = (pr, mr, und) if grouped else refs[0]
            pk, mk = p.cpu(), m.cpu()
            assert torch.equal(mk, wm) and torch.equal(pk[~wu], wp[~wu]), (n, shift, grouped)
            assert torch.equal(g.cpu(), vals[1])
            assert not bufs[0][shift + n:].any() and not bufs[2][shift + n:].any() and not bufs[0][:shift].any()      # nothing past the end


class _Dev8:
    """The device buffers of the 8-bit step, loaded from / compared with the restatement's state."""

    def __init__(self, sizes, bs, min8=4096):
        from qflux_amd import ops
        self.offs, n = R.flat_offsets(sizes)
        self.lay = ops.adam8bit_block_table(list(zip(self.offs, sizes)), bs, min8, device=DEV)
        self.p = torch.zeros(n, device=DEV)
        self.g = torch.zeros(n, device=DEV)
        self.q1 = torch.zeros(n, dtype=torch.uint8, device=DEV)
        self.a1 = torch.zeros(max(1, self.lay.n_absmax), device=DEV)
        self.m32 = torch.zeros(max(1, self.lay.n_fp32), device=DEV)
        self.qm1 = R.create_dynamic_map(True).to(DEV)

    def load(self, params, state):
        for (off, k, eight, a0, nb, s0), p, st in zip(self.lay.tensors, params, state):
            self.p[off:off + k] = p.to(DEV)
            if not st:
                continue
            if eight:
                self.q1[off:off + k] = st["state1"].reshape(-1).to(DEV)
                self.a1[a0:a0 + nb] = st["absmax1"].to(DEV)
            else:
                self.m32[s0:s0 + k] = st["state1"].reshape(-1).to(DEV)

    def step(self, grads, gnorm_sq, weight_decay, **kw):
        from qflux_amd import ops
        for off, g in zip(self.offs, grads):
            self.g[off:off + g.numel()] = g.to(DEV)
        gn = torch.tensor(gnorm_sq, dtype=torch.float32, device=DEV)
        ops.lion8bit_step(self.p, self.g, self.q1, self.a1, self.m32, self.lay, self.qm1, kw["lr"], kw["betas"], weight_decay,
                          gnorm_sq=gn, max_norm=kw["max_norm"], grad_scale=kw["grad_scale"])


@pytest.mark.parametrize("bs", [256, 2048])
def test_8bit_kernel_matches_restatement(bs):
    d = _Dev8(SIZES, bs)
    stats = []
    for it, rec in enumerate(R.run_reference(bs, 0.01)):
        d.load(*rec["before"])                                           # re-synchronised: one step at a time is compared
        d.step(rec["grads"], rec["gsq"], 0.01, **R.KW)
        torch.cuda.synchronize()
        p1, s1 = rec["after"]
        tot = n_und = 0
        for i, ((off, k, eight, a0, nb, s0), pt, st) in enumerate(zip(d.lay.tensors, p1, s1)):
            n_und += _check_params(d.p[off:off + k].cpu(), pt, rec["undecided"][i], (it, k))
            n, u = _check_state8(d.m32[s0:s0 + k].cpu() if not eight else None, d.a1[a0:a0 + nb].cpu() if eight else None,
                                 d.q1[off:off + k].cpu(), st, rec["m64"][i], bs, (it, k))
            tot += n; n_und += u
            if not eight:
                continue
            ck = d.q1[off:off + k].cpu().long()
            z = (st["absmax1"] == 0).repeat_interleave(bs)[:k]
            assert (ck[z] == 127).all()                                  # a zero block stores the code of 0.0
            if i == 4:
                assert z[:bs].all() and torch.equal(d.p[off:off + bs].cpu(), pt[:bs])       # sgn(0) = 0: only the decay moved them
        stats.append((tot, n_und))
        assert n_und <= R.UNDECIDED_CAP * sum(SIZES), (it, n_und)
    print(f"lion8bit bs={bs}: per step (codes compared, undecided parameters and codes) {stats}")


@pytest.mark.parametrize("bs", [256, 2048])
def test_8bit_kernel_clip_active_on_short_block_one_block_and_fp32_tensors(bs):
    """min_8bit_size 256 and three tensors: 259 elements (8-bit, the last block short), exactly one block, and 5 elements (fp32
    moment); the clip is active at every step.  Compared as test_8bit_kernel_matches_restatement compares."""
    sizes, min8, wd = [256 + 3, bs, 5], 256, 0.01
    opt = R.LionRef(R.make_params(sizes, seed=3), lr=R.KW["lr"], betas=R.KW["betas"], weight_decay=wd, min_8bit_size=min8, blocksize=bs)
    d = _Dev8(sizes, bs, min8)
    assert [t[2] for t in d.lay.tensors] == [True, True, False] and d.lay.tensors[1][4] == 1
    for it in range(3):
        grads = R.make_grads(sizes, it, bs)
        gsq = R.gnorm_sq(grads)
        assert gsq * R.KW["grad_scale"] ** 2 > 4.0                        # the clip is active
        d.load([p.clone() for p in opt.params], opt.state)                # re-synchronised: one step at a time is compared
        d.step(grads, gsq, wd, **R.KW)
        opt.step([g.clone() for g in grads], gnorm_sq=gsq, max_norm=R.KW["max_norm"], grad_scale=R.KW["grad_scale"])
        torch.cuda.synchronize()
        tot = n_und = 0
        for i, ((off, k, eight, a0, nb, s0), pt, st) in enumerate(zip(d.lay.tensors, opt.params, opt.state)):
            n_und += _check_params(d.p[off:off + k].cpu(), pt, opt.undecided[i], (it, k))
            n, u = _check_state8(d.m32[s0:s0 + k].cpu() if not eight else None, d.a1[a0:a0 + nb].cpu() if eight else None,
                                 d.q1[off:off + k].cpu(), st, opt.m64[i], bs, (it, k))
            tot += n; n_und += u
        print(f"lion8bit clipped bs={bs} step {it}: {tot} codes compared, {n_und} undecided")
        assert n_und <= R.UNDECIDED_CAP * sum(SIZES), (it, n_und)


def test_kernels_are_deterministic():
    from qflux_amd import ops
    sizes = [70000, 3000, 130000]
    params = R.make_params(sizes, seed=2)
    offs, n = R.flat_offsets(sizes)
    kw = dict(lr=1e-3, betas=(0.9, 0.99), max_norm=1.0, grad_scale=1.0)
    runs = []
    for _ in range(2):
        out = []
        p, g, m = (torch.zeros(n, device=DEV) for _ in range(3))
        for off, t in zip(offs, params):
            p[off:off + t.numel()] = t.to(DEV)
        for it in range(3):
            for off, t in zip(offs, R.make_grads(sizes, it + 5, 256)):
                g[off:off + t.numel()] = t.to(DEV)
            ops.lion_step(p, g, m, kw["lr"], *kw["betas"], 0.01, gnorm_sq=torch.tensor(1e4, device=DEV), max_norm=1.0, grad_scale=1.0)
        out += [p.clone(), m.clone()]
        for bs in (256, 2048):
            d = _Dev8(sizes, bs)
            d.load(params, [{} for _ in params])
            for it in range(3):
                d.step(R.make_grads(sizes, it + 5, bs), 1e4, 0.0, **kw)
            out += [t.clone() for t in (d.p, d.q1, d.a1, d.m32)]
        torch.cuda.synchronize()
        runs.append(out)
    assert len(runs[0]) == 10
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert bool(runs[0][3].ne(0).any()) and bool(runs[0][4].ne(0).any())           # the 8-bit state did move


def _pair(seed=2):
    from common import TINY
    from parity_util import build_pair
    _, m = build_pair(dict(TINY), device=DEV, targets=TARGETS, seed=seed)
    return m


@pytest.mark.parametrize("family", ["lion", "lion8bit_blockwise"])
def test_trainer_learns_saves_the_documented_layout_and_resumes_bit_identically(tmp_path, family):
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    a = _pair()
    sa = QwenLoraTrainStep(a, lr=1e-3, optimizer=family)
    assert sa.weight_decay == 0.0 and sa.betas == (0.9, 0.99)
    e, nz, u = tiny_embeddings(seed=5)
    losses = [sa.train_step(e, noise=nz, u=u).item() for _ in range(12)]
    print(f"{family}: losses {losses}")
    assert losses[-1] < losses[0], losses
    sa.save_checkpoint(str(tmp_path / "ck"))
    sd = torch.load(str(tmp_path / "ck" / "optimizer.bin"), map_location="cpu", weights_only=False)
    kinds = set()
    for i, (_, p, off, k) in enumerate(a.lora_store.entries):
        s = sd["state"][i]
        if family == "lion":
            assert set(s) == {"exp_avg"} and s["exp_avg"].dtype == torch.float32 and s["exp_avg"].shape == p.shape
            continue
        if k >= 4096:
            assert set(s) == {"step", "state1", "qmap1", "absmax1"}
            assert s["state1"].dtype == torch.uint8 and s["state1"].shape == p.shape
            assert s["absmax1"].dtype == torch.float32 and s["absmax1"].numel() == (k + 255) // 256
            assert torch.equal(s["qmap1"], R.create_dynamic_map(True))
        else:
            assert set(s) == {"step", "state1"} and s["state1"].dtype == torch.float32 and s["state1"].shape == p.shape
        kinds.add(k >= 4096)
        assert s["step"] == 12
    assert family == "lion" or kinds == {True, False}
    g0 = sd["param_groups"][0]
    assert set(g0) >= {"lr", "betas", "weight_decay", "params"} and tuple(g0["betas"]) == (0.9, 0.99) and sd["global_step"] == 12
    for _ in range(3):
        sa.train_step(e, noise=nz, u=u)
    want = a.lora_store.pflat.detach().cpu().clone()
    b = _pair()
    sb = QwenLoraTrainStep(b, lr=0.5, betas=(0.5, 0.5), optimizer=family)
    sb.load_checkpoint(str(tmp_path / "ck"), adapter_name="lora_edit")
    assert sb.global_step == 12 and sb.lr == 1e-3 and sb.betas == (0.9, 0.99)
    for _ in range(3):
        sb.train_step(e, noise=nz, u=u)
    assert torch.equal(b.lora_store.pflat.detach().cpu(), want)


def test_flux_step_runs_with_blockwise_lion_state():
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
    step = FluxKontextTrainStep(m, lr=1e-3, optimizer="lion8bit_blockwise", optimizer_args={"min_8bit_size": 256})
    ctl = FO.prepare_latent_image_ids(4, 6); ctl[:, 0] = 1
    emb = dict(image_latents=torch.randn(2, 24, 64, generator=g).half(), control_latents=torch.randn(2, 24, 64, generator=g).half(),
               control_ids=ctl, text_ids=torch.zeros(7, 3), latent_hw=(4, 6),
               pooled_prompt_embeds=torch.randn(2, 16, generator=g).half(), prompt_embeds=torch.randn(2, 7, 64, generator=g).half())
    for it in range(2):
        before = m.lora_store.pflat.detach().clone()
        loss = step.train_step(emb, noise=torch.randn(2, 24, 64, generator=g), t=torch.tensor([0.3, 0.8]))
        assert torch.isfinite(loss).all() and not torch.equal(before, m.lora_store.pflat) and torch.isfinite(m.lora_store.pflat).all()
    assert step.state_dict()["state"][0]["step"] == 2 and step.opt_state.layout.n_absmax > 0 and step.betas == (0.9, 0.99)


_TWINS = {}


def _twins():
    """Two tiny models with equal weights, built once; every case starts from the same adapter values and a zero gradient."""
    from common import TINY
    from parity_util import build_pair
    if not _TWINS:
        _TWINS["models"] = [build_pair(dict(TINY), device=DEV, targets=TARGETS, seed=2)[1] for _ in range(2)]
        _TWINS["start"] = _TWINS["models"][0].lora_store.pflat.detach().clone()
    for m in _TWINS["models"]:
        with torch.no_grad():
            m.lora_store.pflat.copy_(_TWINS["start"])
            m.lora_store.gflat.zero_()
    return _TWINS["models"]


CLASSES = [("Lion", "lion", dict(lr=1e-3, weight_decay=0.01), None),
           ("Lion8bit", "lion8bit_blockwise", dict(lr=1e-3, weight_decay=0.01, blocksize=2048), {"blocksize": 2048}),
           ("PagedLion8bit", "lion8bit_blockwise", dict(lr=1e-3, is_paged=True), None)]


@pytest.mark.parametrize("name,family,kw,args", CLASSES, ids=[c[0] for c in CLASSES])
def test_class_steps_bit_identically_to_the_train_step_and_exchanges_checkpoints(name, family, kw, args):
    from qflux_amd import optim as O
    from qflux_amd.trainer import QwenLoraTrainStep
    a, b = _twins()
    sa, sb = a.lora_store, b.lora_store
    params = [p for n, p in a.named_parameters() if "lora_" in n]
    opt = getattr(O, name)(params, **kw)
    step = QwenLoraTrainStep(b, lr=kw["lr"], weight_decay=kw.get("weight_decay"), max_grad_norm=0, optimizer=family, optimizer_args=args)

    def grad(it):
        g = (torch.randn(sa.gflat.shape, generator=torch.Generator().manual_seed(50 + it)) * 1e-2).to(DEV)
        for m in (a, b):
            m.lora_store.gflat.copy_(g)
    for it in range(3):
        grad(it)
        opt.step()
        step.optimizer_step()
        opt.zero_grad()                       # set_to_none: the next step() re-attaches the flat views
        step.zero_grad()
    assert not torch.equal(sa.pflat, _TWINS["start"]) and torch.equal(sa.pflat, sb.pflat)
    x, y = opt._opt_state.buffers(), step.opt_state.buffers()
    assert [n for n, _ in x] == [n for n, _ in y] and x and all(torch.equal(s, t) for (_, s), (_, t) in zip(x, y))
    # the class's file resumes a fresh train step, which then steps like the class that never stopped
    sd = opt.state_dict()
    assert sd["global_step"] == 3 and list(sd["state"]) == list(step.state_dict()["state"])
    step2 = QwenLoraTrainStep(b, lr=0.5, max_grad_norm=0, optimizer=family, optimizer_args=args)
    step2.load_state_dict(sd)
    assert step2.lr == kw["lr"] and step2.global_step == 3 and step2.betas == (0.9, 0.99)
    grad(3)
    opt.step()
    step2.optimizer_step()
    assert torch.equal(sa.pflat, sb.pflat)
