"""GPU: the fused blockwise 8-bit Adam step (qfx_adam8bit_step) against its CPU restatement (tests/bnb8_ref.py), its determinism, and
the trainer / checkpoint path with optimizer="adam8bit_blockwise" / "adamw8bit_blockwise" (bitsandbytes' state layout)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnb8_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# attention adapters (1024 elements: fp32 moments) and the feed-forward down projection's LoRA-A (4096: 8-bit).  Not txt_mod.1: the
# LoRA-A gradient of the modulation head is not bit-reproducible run to run (under the fp32 AdamW step as well), which a
# bit-identical resume cannot absorb
TARGETS = ("to_k", "to_q", "to_v", "to_out.0", "img_mlp.net.2")
SIZES, _flat, _grads = R.SIZES, R.flat_offsets, R.make_grads      # shared with the CPU census (tests/test_blockwise8_cpu.py)


class _Dev:
    """The device buffers of one step, loaded from / compared with the restatement's state."""

    def __init__(self, sizes, bs, params, min8=4096):
        from qflux_amd import ops
        self.offs, n = _flat(sizes)
        self.lay = ops.adam8bit_block_table(list(zip(self.offs, sizes)), bs, min8, device=DEV)
        self.p = torch.zeros(n, device=DEV)
        self.g = torch.zeros(n, device=DEV)
        self.q1 = torch.zeros(n, dtype=torch.uint8, device=DEV)
        self.q2 = torch.zeros(n, dtype=torch.uint8, device=DEV)
        self.a1 = torch.zeros(max(1, self.lay.n_absmax), device=DEV)
        self.a2 = torch.zeros_like(self.a1)
        self.m32 = torch.zeros(max(1, self.lay.n_fp32), device=DEV)
        self.v32 = torch.zeros_like(self.m32)
        self.qm1 = R.create_dynamic_map(True).to(DEV)
        self.qm2 = R.create_dynamic_map(False).to(DEV)
        for (off, k, _, _, _, _), p in zip(self.lay.tensors, params):
            self.p[off:off + k] = p.to(DEV)

    def load(self, opt):
        for (off, k, eight, a0, nb, s0), p, st in zip(self.lay.tensors, opt.params, opt.state):
            self.p[off:off + k] = p.to(DEV)
            if not st:
                continue
            if eight:
                self.q1[off:off + k] = st["state1"].reshape(-1).to(DEV); self.q2[off:off + k] = st["state2"].reshape(-1).to(DEV)
                self.a1[a0:a0 + nb] = st["absmax1"].to(DEV); self.a2[a0:a0 + nb] = st["absmax2"].to(DEV)
            else:
                self.m32[s0:s0 + k] = st["state1"].reshape(-1).to(DEV); self.v32[s0:s0 + k] = st["state2"].reshape(-1).to(DEV)

    def views(self):
        out = []
        for off, k, eight, a0, nb, s0 in self.lay.tensors:
            if eight:
                out.append((True, self.p[off:off + k].cpu(), self.q1[off:off + k].cpu(), self.q2[off:off + k].cpu(), self.a1[a0:a0 + nb].cpu(),
                            self.a2[a0:a0 + nb].cpu()))
            else:
                out.append((False, self.p[off:off + k].cpu(), self.m32[s0:s0 + k].cpu(), self.v32[s0:s0 + k].cpu(), None, None))
        return out

    def step(self, grads, t, gnorm_sq, **kw):
        from qflux_amd import ops
        for off, g in zip(self.offs, grads):
            self.g[off:off + g.numel()] = g.to(DEV)
        gn = torch.tensor(gnorm_sq, dtype=torch.float32, device=DEV)
        ops.adam8bit_step(self.p, self.g, self.q1, self.q2, self.a1, self.a2, self.m32, self.v32, self.lay, self.qm1, self.qm2,
                          kw["lr"], kw["betas"], kw["eps"], kw["weight_decay"], t, gnorm_sq=gn, max_norm=kw["max_norm"],
                          grad_scale=kw["grad_scale"])



def check_step(where, bs, views, opt, zero_blocks=False):
    """One step under the exact rule of bnb8_ref: parameters, fp32 moments and block maxima bit for bit, every decided code identical,
    an undecided one within one step.  views: per tensor (eight, p, state1, state2, absmax1, absmax2) as CPU tensors, the kernel's;
    opt: the restatement after the same step.  Returns (codes compared, undecided ones, those that differ)."""
    tot = n_und = n_diff = 0
    for i, ((eight, pk, s1, s2, a1k, a2k), p, st) in enumerate(zip(views, opt.params, opt.state)):
        k = p.numel()
        assert torch.isfinite(pk).all()
        assert R.same_bits(pk, p.reshape(-1)), (where, i, "parameters", R.ulp_diff(pk, p.reshape(-1)))
        if not eight:
            assert R.same_bits(s1, st["state1"].reshape(-1)) and R.same_bits(s2, st["state2"].reshape(-1)), (where, i, "fp32 moments")
            continue
        assert R.same_bits(a1k, st["absmax1"]) and R.same_bits(a2k, st["absmax2"]), (where, i, "block maxima")
        blk = torch.arange(k) // bs
        for ck, key, mk, qk, sg in ((s1, "state1", "_m", "qmap1", True), (s2, "state2", "_v", "qmap2", False)):
            und, _ = R.undecided_codes(st[mk], st[mk + "64"], blk, a1k.numel(), st[qk], sg)
            n_diff += R.check_codes(ck, st[key], und, (where, i, key))[1]
            n_und += int(und.sum()); tot += k
        if zero_blocks:
            z = (st["absmax1"] == 0).repeat_interleave(bs)[:k]
            assert (s1[z] == 127).all()                                        # a zero block stores the code of 0.0
    assert n_und <= R.UNDECIDED_CAP * tot, (where, n_und, tot)
    return tot, n_und, n_diff


@pytest.mark.parametrize("bs", [256, 2048])
def test_kernel_matches_restatement(bs):
    kw = R.KW
    opt, steps = R.file_reference("sizes", bs)
    d = _Dev(SIZES, bs, [p.clone() for p in opt.params])
    stats = []
    for it, (grads, gsq) in enumerate(steps):
        assert gsq * kw["grad_scale"] ** 2 > 1.0                        # the clip is active
        d.load(opt)                                                      # re-synchronised: one step at a time is compared
        d.step(grads, it + 1, gsq, **kw)
        opt.step([g.clone() for g in grads], gnorm_sq=gsq, max_norm=kw["max_norm"], grad_scale=kw["grad_scale"])
        torch.cuda.synchronize()
        stats.append(check_step((bs, it), bs, d.views(), opt, zero_blocks=True))
    print(f"adam8bit bs={bs}: per step (codes, undecided, undecided that differ) {stats}")


@pytest.mark.parametrize("bs", [256, 2048])
def test_kernel_clip_active_on_short_block_one_block_and_fp32_tensors(bs):
    """min_8bit_size 256 and three tensors: 259 elements (8-bit, the last block short), exactly one block, and 5 elements (fp32
    moments); the clip is active at every step.  Compared as test_kernel_matches_restatement compares (check_step)."""
    kw = R.KW
    sizes, min8, _, _ = R.file_cases(bs)["clipped"]
    opt, steps = R.file_reference("clipped", bs)
    d = _Dev(sizes, bs, [p.clone() for p in opt.params], min8)
    assert [t[2] for t in d.lay.tensors] == [True, True, False] and d.lay.tensors[1][4] == 1
    for it, (grads, gsq) in enumerate(steps):
        assert gsq * kw["grad_scale"] ** 2 > 4.0                        # the clip is active
        d.load(opt)                                                      # re-synchronised: one step at a time is compared
        d.step(grads, it + 1, gsq, **kw)
        opt.step([g.clone() for g in grads], gnorm_sq=gsq, max_norm=kw["max_norm"], grad_scale=kw["grad_scale"])
        torch.cuda.synchronize()
        print(f"adam8bit clipped bs={bs} step {it}: (codes, undecided, undecided that differ) {check_step((bs, it), bs, d.views(), opt)}")


def test_kernel_is_deterministic():
    torch.manual_seed(2)
    sizes = [70000, 3000, 130001 // 4 * 4]
    params = [torch.randn(k) for k in sizes]
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=1.0, grad_scale=1.0)
    for bs in (256, 2048):
        outs = []
        for _ in range(2):
            d = _Dev(sizes, bs, params)
            for it in range(3):
                d.step(_grads(sizes, it + 5, bs), it + 1, 1e4, **kw)
            torch.cuda.synchronize()
            outs.append([t.clone() for t in (d.p, d.q1, d.q2, d.a1, d.a2, d.m32, d.v32)])
        for a, b in zip(*outs):
            assert torch.equal(a, b)


def _pair(seed=2):
    from common import TINY
    from parity_util import build_pair
    _, m = build_pair(dict(TINY), device=DEV, targets=TARGETS, seed=seed)
    return m


def test_trainer_blockwise_learns_saves_bnb_layout_and_resumes_bit_identically(tmp_path):
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    a = _pair()
    sa = QwenLoraTrainStep(a, lr=3e-3, optimizer="adamw8bit_blockwise")
    assert sa.weight_decay == 0.01
    e, nz, u = tiny_embeddings(seed=5)
    losses = [sa.train_step(e, noise=nz, u=u).item() for _ in range(12)]
    assert losses[-1] < losses[0], losses
    sa.save_checkpoint(str(tmp_path / "ck"))
    sd = torch.load(str(tmp_path / "ck" / "optimizer.bin"), map_location="cpu", weights_only=False)
    kinds = set()
    for i, (_, p, off, k) in enumerate(a.lora_store.entries):
        s = sd["state"][i]
        if k >= 4096:
            assert set(s) == {"step", "state1", "state2", "qmap1", "qmap2", "absmax1", "absmax2"}
            assert s["state1"].dtype == s["state2"].dtype == torch.uint8 and s["state1"].shape == p.shape
            assert s["absmax1"].dtype == torch.float32 and s["absmax1"].numel() == (k + 255) // 256
            assert torch.equal(s["qmap1"], R.create_dynamic_map(True)) and torch.equal(s["qmap2"], R.create_dynamic_map(False))
        else:
            assert set(s) == {"step", "state1", "state2"} and s["state1"].dtype == torch.float32 and s["state1"].shape == p.shape
        kinds.add(k >= 4096)
        assert s["step"] == 12
    assert kinds == {True, False}
    assert set(sd["param_groups"][0]) >= {"lr", "betas", "eps", "weight_decay", "params"}
    for _ in range(3):
        sa.train_step(e, noise=nz, u=u)
    want = a.lora_store.pflat.detach().cpu().clone()
    b = _pair()
    sb = QwenLoraTrainStep(b, lr=0.5, optimizer="adamw8bit_blockwise")
    sb.load_checkpoint(str(tmp_path / "ck"), adapter_name="lora_edit")
    assert sb.global_step == 12 and sb.lr == 3e-3
    for _ in range(3):
        sb.train_step(e, noise=nz, u=u)
    assert torch.equal(b.lora_store.pflat.detach().cpu(), want)


def test_flux_step_runs_with_blockwise_optimizer_state():
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
    step = FluxKontextTrainStep(m, lr=3e-3, optimizer="adam8bit_blockwise", optimizer_args={"min_8bit_size": 256})
    ctl = FO.prepare_latent_image_ids(4, 6); ctl[:, 0] = 1
    emb = dict(image_latents=torch.randn(2, 24, 64, generator=g).half(), control_latents=torch.randn(2, 24, 64, generator=g).half(),
               control_ids=ctl, text_ids=torch.zeros(7, 3), latent_hw=(4, 6),
               pooled_prompt_embeds=torch.randn(2, 16, generator=g).half(), prompt_embeds=torch.randn(2, 7, 64, generator=g).half())
    before = m.lora_store.pflat.detach().clone()
    loss = step.train_step(emb, noise=torch.randn(2, 24, 64, generator=g), t=torch.tensor([0.3, 0.8]))
    assert torch.isfinite(loss).all() and not torch.equal(before, m.lora_store.pflat)
    assert step.state_dict()["state"][0]["step"] == 1 and step.opt_state.layout.n_absmax > 0


@pytest.mark.parametrize("bs", [256, 2048])
def test_bnb_layout_file_resumes_in_both_modes(tmp_path, bs):
    """An optimizer.bin in bitsandbytes' layout (built by the restatement after 3 steps) resumes (a) in blockwise mode: one more step
    equals the restatement's next step; (b) with the fp32 alias "adam8bit": the moments are the dequantised ones."""
    from qflux_amd.trainer import QwenLoraTrainStep
    m = _pair()
    st = m.lora_store
    torch.manual_seed(4)
    ps = [torch.randn(p.shape) * 0.1 for _, p, _, _ in st.entries]
    opt = R.Adam8bitRef(ps, lr=1e-3, betas=(0.9, 0.99), weight_decay=0.0, blocksize=bs)
    for _ in range(3):
        opt.step([torch.randn(p.shape) for p in ps])
    torch.save(opt.state_dict(), str(tmp_path / "optimizer.bin"))
    sd = torch.load(str(tmp_path / "optimizer.bin"), map_location="cpu", weights_only=False)
    with torch.no_grad():
        for (_, p, _, _), r in zip(st.entries, ps):
            p.copy_(r.to(DEV))
    s8 = QwenLoraTrainStep(m, optimizer="adam8bit_blockwise", max_grad_norm=1.0)
    s8.load_state_dict(sd)
    assert s8.optimizer_args["blocksize"] == bs and s8.global_step == 3
    grads = [torch.randn(p.shape) for p in ps]
    for (_, _, off, k), g in zip(st.entries, grads):
        st.gflat[off:off + k] = g.reshape(-1).to(DEV)
    s8.optimizer_step()
    gsq = float(s8._gnorm.item())
    opt.step(grads, gnorm_sq=gsq, max_norm=1.0)
    for (_, p, _, _), r in zip(st.entries, ps):
        assert ((p.detach().cpu() - r).abs().max() / r.abs().max()).item() <= 1e-6
    out = s8.state_dict()["state"]
    for i, e in opt.state_dict()["state"].items():
        for key in ("state1", "state2"):
            if e[key].dtype == torch.uint8:
                assert (out[i][key].long() - e[key].long()).abs().max() <= 1
    # (b) the fp32 alias
    sa = QwenLoraTrainStep(m, optimizer="adam8bit")
    sa.load_state_dict(sd)
    for i, (_, p, off, k) in enumerate(st.entries):
        e = sd["state"][i]
        want = R.dequant(e["state1"], e["qmap1"], e["absmax1"], bs) if e["state1"].dtype == torch.uint8 else e["state1"].reshape(-1)
        assert torch.equal(sa._m[off:off + k].cpu(), want)
    st.gflat.normal_()
    sa.optimizer_step()
    assert torch.isfinite(st.pflat).all() and sa.global_step == 4
