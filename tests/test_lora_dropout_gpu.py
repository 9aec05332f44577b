"""GPU: network_dropout / rank_dropout of the adapters (csrc/qfx_lora_dropout.hip, plan/emit.py, the train steps).  The kernel
is held to tests/lora_dropout_ref.py word for word (same fp32 multiply, same two roundings: equality is derived, not measured);
the model tests hand the oracle the reference's factors through forward hooks on its lora_A modules and reuse the parity drivers
and bars of tests/parity_util.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lora_dropout_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
P_E, P_R, SEED = 0.25, 0.25, 20261019


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _state(dev=DEV, **kw):
    w = R.make_state(**kw)
    return torch.from_numpy(w.view(np.int32).copy()).to(dev), w


class _Problem:
    """One qfx_lora_down call on random X, A and what it wrote; r_valid < R leaves the padded ranks' weights zero."""

    def __init__(self, seed, M, K, R_, group_R, group_stride, rows_per_batch, sites, r_valid=None):
        from qflux_amd import _lib as L
        g = torch.Generator().manual_seed(seed)
        self.M, self.R, self.group_R, self.group_stride, self.rpb, self.sites = M, R_, group_R, group_stride, rows_per_batch, sites
        x = torch.randn(M, K, generator=g).to(BF)
        w = torch.randn(R_, K, generator=g) / K ** 0.5
        if r_valid is not None:
            for g0 in range(0, R_, group_R):
                w[g0 + r_valid:g0 + group_R] = 0
        w_hi = w.to(BF)
        w_lo = (w - w_hi.float()).to(BF)
        self.ld_ext = (R_ // group_R - 1) * group_stride + 3 * group_R + 8          # 8 columns the kernels never write
        ld_ut = (M + 127) // 128 * 128
        self.x, self.w_hi, self.w_lo = x.to(DEV), w_hi.to(DEV), w_lo.to(DEV)
        self.ext = torch.zeros(M, self.ld_ext, dtype=BF, device=DEV)
        self.ut = (torch.zeros(R_, ld_ut, dtype=BF, device=DEV), torch.zeros(R_, ld_ut, dtype=BF, device=DEV))
        a = L.LoraDownArgs()
        a.X, a.ldx, a.M, a.K = self.x.data_ptr(), K, M, K
        a.W_hi, a.W_lo, a.ldw, a.R = self.w_hi.data_ptr(), self.w_lo.data_ptr(), K, R_
        a.ext, a.ld_ext = self.ext.data_ptr(), self.ld_ext
        a.Ut_hi, a.Ut_lo, a.ld_ut = self.ut[0].data_ptr(), self.ut[1].data_ptr(), ld_ut
        a.group_R, a.group_stride, a.rows_per_batch = group_R, group_stride, M
        L.check(L.lib.qfx_lora_down(C.byref(a), torch.cuda.current_stream().cuda_stream), "qfx_lora_down")
        torch.cuda.synchronize()
        self.base = (_bits(self.ut[0]), _bits(self.ut[1]), _bits(self.ext))
        assert self.base[0][:, :M].any() and not self.base[0][:, M:].any()

    def fresh(self):
        """(args, buffers): a copy of the producer's outputs and the dropout problem over it."""
        from qflux_amd import ops
        ut = (self.ut[0].clone(), self.ut[1].clone())
        ext = self.ext.clone()
        a = ops.lora_dropout_args(Ut=ut, M=self.M, R=self.R, rows_per_batch=self.rpb, sites=self.sites, ext=ext, group_R=self.group_R,
                                  group_stride=self.group_stride)
        return a, (ut[0], ut[1], ext)

    def expected(self, words):
        f = R.problem_factors(words, self.sites, self.M, self.rpb, self.group_R)
        hi, lo = self.base[0].copy(), self.base[1].copy()
        hi[:, :self.M], lo[:, :self.M] = R.apply_ref(hi[:, :self.M], lo[:, :self.M], f)
        return hi, lo, R.ext_ref(hi, lo, self.M, self.group_R, self.group_stride, self.ld_ext, base=self.base[2]), f


@pytest.fixture(scope="module")
def problems():
    # M = 70 = 2 samples of 35 tokens: no multiple of 32 or 64, two blocks of 64 rows
    return {"R16": _Problem(1, 70, 64, 16, 16, 0, 35, (R.site_key("a.to_q"),)),
            "R48x3": _Problem(2, 70, 96, 48, 16, 64, 35, tuple(R.site_key(n) for n in ("a.to_q", "a.to_k", "a.to_v"))),
            "R32r24": _Problem(3, 70, 64, 32, 32, 0, 35, (R.site_key("b.to_out.0"),), r_valid=24)}


def _check(prob, bufs, words):
    hi, lo, ext, f = prob.expected(words)
    got = tuple(_bits(t) for t in bufs)
    assert 0.2 < float((f == 0).mean()) < 0.7, "the case must drop some elements and keep some"
    for name, g, w in zip(("Ut_hi", "Ut_lo", "ext"), got, (hi, lo, ext)):
        assert np.array_equal(g, w), (name, int((g != w).sum()))
    assert not got[0][:, prob.M:].any() and not got[1][:, prob.M:].any()      # Ut columns >= M stay zero
    return got


@pytest.mark.parametrize("name", ["R16", "R48x3", "R32r24"])
def test_kernel_is_element_exact(problems, name):
    from qflux_amd import ops
    prob = problems[name]
    st, words = _state(seed=SEED, step=5, active=1, network_dropout=P_E, rank_dropout=P_R, sample0=3)
    a, bufs = prob.fresh()
    ops.lora_dropout_apply([a], st)
    torch.cuda.synchronize()
    got = _check(prob, bufs, words)
    if name == "R32r24":      # padded ranks stay zero, dropped elements are exact zeros
        assert not got[0][24:, :].any() and not got[1][24:, :].any()
    f = prob.expected(words)[3]
    assert not got[0][:, :prob.M][f.T == 0].any() and not got[1][:, :prob.M][f.T == 0].any()
    # the same state again on a fresh copy: the same bits
    a2, bufs2 = prob.fresh()
    ops.lora_dropout_apply([a2], st)
    torch.cuda.synchronize()
    assert all(np.array_equal(_bits(x), y) for x, y in zip(bufs2, got))
    # each option alone
    for kw in (dict(network_dropout=P_E), dict(rank_dropout=P_R)):
        st1, words1 = _state(seed=SEED, step=6, active=1, sample0=0, **kw)
        a3, bufs3 = prob.fresh()
        ops.lora_dropout_apply([a3], st1)
        torch.cuda.synchronize()
        hi, lo, ext, _ = prob.expected(words1)
        assert all(np.array_equal(_bits(x), y) for x, y in zip(bufs3, (hi, lo, ext))), kw


def test_kernel_batch_of_three_problems_in_one_launch(problems):
    from qflux_amd import ops
    st, words = _state(seed=SEED + 1, step=2, active=1, network_dropout=P_E, rank_dropout=P_R, sample0=0)
    fresh = [(p, *p.fresh()) for p in problems.values()]
    ops.lora_dropout_apply([a for _, a, _ in fresh], st)
    torch.cuda.synchronize()
    for p, _, bufs in fresh:
        _check(p, bufs, words)


@pytest.mark.parametrize("kw", [dict(active=0, network_dropout=P_E, rank_dropout=P_R), dict(active=1)], ids=["inactive", "p=0"])
def test_kernel_leaves_every_byte_alone_when_off(problems, kw):
    from qflux_amd import ops
    st, _ = _state(seed=SEED, step=5, **kw)
    for p in problems.values():
        a, bufs = p.fresh()
        ops.lora_dropout_apply([a], st)
        torch.cuda.synchronize()
        assert all(np.array_equal(_bits(x), y) for x, y in zip(bufs, p.base))


def test_advance_counts_training_forwards_only():
    from qflux_amd import ops
    st, _ = _state(seed=1, step=41, active=1, network_dropout=P_E)
    ops.lora_dropout_advance(st)
    assert st.cpu().tolist()[2] == 42
    st[3] = 0
    ops.lora_dropout_advance(st)
    assert st.cpu().tolist()[2] == 42


# ---------------------------------------------------------------------------------------------- model level
def _hook_oracle(oracle, words_of_step, seen=None):
    """The reference's factors on every lora_A output of the oracle (fp32 [B, tokens, r]): site = crc32 of the wrapped module's
    name, local samples 0..B-1, tokens in stream order."""
    for name, mod in oracle.named_modules():
        if hasattr(mod, "lora_A") and hasattr(mod, "base_layer"):
            for lin in mod.lora_A.values():
                def hook(_m, _inp, out, name=name):
                    f = R.factors(words_of_step(), R.site_key(name), np.arange(out.shape[0]), np.arange(out.shape[1]), out.shape[2])
                    if seen is not None:
                        seen.add(name)
                    return out * torch.from_numpy(f).to(out.device)
                lin.register_forward_hook(hook)


def _with_dropout(monkeypatch, pe=P_E, pr=P_R, seed=SEED, step=1):
    """The parity drivers build their own pair: their oracle gets the hooks (step: the first training forward draws step 1), their
    HIP model the option, both right where the adapters are injected."""
    from oracle import qwen_dit as O
    from qflux_amd.models import QwenImageTransformer2DModel as Model
    words = R.make_state(seed=seed, step=step, active=1, network_dropout=pe, rank_dropout=pr)
    seen = set()
    add_lora, add_adapter = O.add_lora, Model.add_adapter

    def oracle_add(model, *a, **k):
        r = add_lora(model, *a, **k)
        _hook_oracle(model, lambda: words, seen)
        return r

    def hip_add(self, *a, **k):
        r = add_adapter(self, *a, **k)
        self.set_lora_dropout(pe, pr, seed)
        return r
    monkeypatch.setattr(O, "add_lora", oracle_add)
    monkeypatch.setattr(Model, "add_adapter", hip_add)
    return seen


FF = ("to_k", "to_q", "to_v", "to_out.0", "img_mlp.net.0.proj", "img_mlp.net.2", "txt_mlp.net.0.proj", "txt_mlp.net.2")
_P0 = {}


def _p0_loss(kind, targets=None):
    """The p = 0 loss of the same fixture, computed once."""
    import parity_util as PU
    key = (kind, targets)
    if key not in _P0:
        res = PU.run_tiny_step_parity(device=DEV, targets=targets) if kind == "qwen" else PU.run_flux_step_parity(device=DEV)
        assert res["ok"], res
        _P0[key] = res["loss_hip"]
    return _P0[key]


@pytest.mark.parametrize("targets", [("to_k", "to_q", "to_v", "to_out.0"), FF], ids=["attn", "attn+mlp"])
def test_qwen_step_parity_with_the_mask(monkeypatch, targets):
    import parity_util as PU
    base = _p0_loss("qwen", targets)
    seen = _with_dropout(monkeypatch)
    res = PU.run_tiny_step_parity(device=DEV, targets=targets, verbose=True)      # loss, prediction and every gradient at QWEN_BARS
    assert res["ok"], res
    assert len(seen) >= 8 and res["loss_hip"] != base and res["loss_oracle"] != base


def test_flux_step_parity_with_the_mask(monkeypatch):
    import parity_util as PU
    base = _p0_loss("flux")
    seen = _with_dropout(monkeypatch)
    res = PU.run_flux_step_parity(device=DEV, verbose=True)                        # ... at FLUX_BARS
    assert res["ok"], res
    assert len(seen) >= 8 and res["loss_hip"] != base


def _qwen_step(targets=("to_k", "to_q", "to_v", "to_out.0"), **kw):
    from common import TINY
    from parity_util import build_pair
    from qflux_amd.trainer import QwenLoraTrainStep
    _, hip = build_pair(dict(TINY), device=DEV, targets=targets)
    return hip, QwenLoraTrainStep(hip, lr=1e-2, **kw)


def _flux_step(**kw):
    from common import FLUX_TINY, fill_weights
    from qflux_amd.models import FluxTransformer2DModel
    from qflux_amd.modules import LoraConfig
    from qflux_amd.trainer import FluxKontextTrainStep
    cfg = dict(FLUX_TINY, joint_attention_dim=64, guidance_embeds=True)
    with torch.device(DEV):
        hip = FluxTransformer2DModel(**cfg)
    hip.add_adapter(LoraConfig(r=4, lora_alpha=8, target_modules=["to_k", "to_q", "to_v", "to_out.0"]), "lora_edit")
    fill_weights(hip, seed=5)
    hip._invalidate()
    return hip, FluxKontextTrainStep(hip, lr=1e-2, **kw)


def _flux_batch(cfg_pooled=16, Jd=64, B=2, hw=(4, 6), T=7, seed=31):
    from oracle import flux_dit as FO
    g = torch.Generator().manual_seed(seed)
    h, w = hw
    ctl = FO.prepare_latent_image_ids(h, w)
    ctl[:, 0] = 1
    emb = dict(image_latents=torch.randn(B, h * w, 64, generator=g).half(), control_latents=torch.randn(B, h * w, 64, generator=g).half(),
               control_ids=ctl, text_ids=torch.zeros(T, 3), latent_hw=(h, w),
               pooled_prompt_embeds=torch.randn(B, cfg_pooled, generator=g).half(), prompt_embeds=torch.randn(B, T, Jd, generator=g).half())
    return emb, torch.randn(B, h * w, 64, generator=g).to(BF), torch.tensor([0.7109, 0.1611]).to(BF)


def _one_step(hip, step, batch, kind):
    emb, noise, u = batch
    loss = step.forward_backward(emb, noise=noise, **({"u": u} if kind == "qwen" else {"t": u}))
    g = hip.lora_store.gflat.clone()
    step.optimizer_step()
    step.zero_grad()
    torch.cuda.synchronize()
    return loss.clone(), g, hip.lora_store.pflat.clone()


def _loss_same(a, b):
    """The scalar loss is a sum of fp32 atomics (one per block of the criterion kernel) and moves in its last bit from run to run,
    with or without this feature: held to 1e-6 as in parity_util.assert_step_bit_reproducible.  Everything else is compared bitwise."""
    a, b = float(a), float(b)
    return abs(a - b) <= 1e-6 * abs(a)


def _same(a, b):
    """(loss, flat gradient, weights) of two steps: the tensors bit for bit."""
    return _loss_same(a[0], b[0]) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[1:], b[1:]))


@pytest.mark.parametrize("kind", ["qwen", "flux"])
def test_off_means_off(kind):
    """Keywords absent, both probabilities 0, and p > 0 under eval(): loss, flat gradient and the weights after one optimizer step
    are the bits of the path without the option, and no dropout launch is emitted with the feature off."""
    from parity_util import tiny_embeddings
    make = _qwen_step if kind == "qwen" else _flux_step
    batch = tiny_embeddings(seed=11) if kind == "qwen" else _flux_batch()
    hip0, s0 = make()
    want = _one_step(hip0, s0, batch, kind)
    hip1, s1 = make(network_dropout=0.0, rank_dropout=0.0)
    assert hip1.lora_dropout is None
    assert _same(_one_step(hip1, s1, batch, kind), want)
    for plan in hip1._plans.values():
        assert not [e for prog in (plan.fwd, plan.bwd) for e in prog.calls if e[0] is not None and "dropout" in e[0].__name__]
    hip2, s2 = make(network_dropout=P_E, rank_dropout=P_R, dropout_seed=SEED)
    s2.eval()
    assert _same(_one_step(hip2, s2, batch, kind), want)
    assert hip2.lora_dropout.step() == 0          # an evaluation forward consumes no masks
    s2.train()
    got = _one_step(hip2, s2, batch, kind)
    assert not _loss_same(got[0], want[0]) and not torch.equal(got[1], want[1]) and hip2.lora_dropout.step() == 1


def test_same_mask_in_forward_and_backward():
    """rank_dropout alone, seed chosen on the CPU so that one rank of one adapter is dropped for every sample of the batch at step
    1: that row of dA and that column of dB are exactly zero -- the backward regenerated the forward's mask."""
    from parity_util import tiny_embeddings
    hip, _ = _qwen_step()
    names = [n for n, m in hip.named_modules() if hasattr(m, "lora_A") and ".attn." in n]
    pick = None
    for seed in range(200):
        words = R.make_state(seed=seed, step=1, active=1, rank_dropout=0.5)
        for n in names:
            f = R.factors(words, R.site_key(n), [0, 1], [0], 4)[:, 0, :]          # [B, r], constant over tokens
            dead = np.nonzero((f == 0).all(axis=0))[0]
            alive = np.nonzero((f != 0).any(axis=0))[0]
            if len(dead) and len(alive):
                pick = (seed, n, int(dead[0]), int(alive[0]))
                break
        if pick:
            break
    assert pick is not None
    seed, name, j, k = pick
    hip, step = _qwen_step(rank_dropout=0.5, dropout_seed=seed)
    emb, noise, u = tiny_embeddings(seed=11)
    step.forward_backward(emb, noise=noise, u=u)
    torch.cuda.synchronize()
    m = hip.get_submodule(name)
    assert float(m.A.grad[j].abs().max()) == 0.0 and float(m.B.grad[:, j].abs().max()) == 0.0
    assert float(m.A.grad[k].abs().max()) > 0.0 and float(m.B.grad[:, k].abs().max()) > 0.0


def test_stepping_graph_and_resume(tmp_path):
    """Two consecutive steps draw different masks and leave step = 2; the captured-graph step advances the same way and matches the
    eager one bit for bit; a checkpoint after step 2 resumes into a step 3 with the bits of the uninterrupted run (the weights, hence
    every gradient, bitwise; the scalar losses as _loss_same says)."""
    from parity_util import tiny_embeddings
    kw = dict(network_dropout=P_E, rank_dropout=P_R, dropout_seed=SEED)
    b1 = tiny_embeddings(seed=11)
    hip_a, sa = _qwen_step(**kw)
    assert "lora_dropout" not in _qwen_step()[1].state_dict()
    l1 = sa.train_step(b1[0], noise=b1[1], u=b1[2]).clone()
    p1 = hip_a.lora_store.pflat.clone()
    l2 = sa.train_step(b1[0], noise=b1[1], u=b1[2]).clone()        # the same batch: only the mask (and the weights) moved on
    assert hip_a.lora_dropout.step() == 2
    # the second mask differs from the first: a twin restarted at the weights after step 1 with step = 0 draws mask 1 again
    hip_t, st_ = _qwen_step(**kw)
    st_.train_step(b1[0], noise=b1[1], u=b1[2])
    assert torch.equal(hip_t.lora_store.pflat, p1)                 # (same seed, same step: the same run so far)
    hip_t.lora_dropout.set_step(0)
    l2_mask1 = st_.train_step(b1[0], noise=b1[1], u=b1[2])
    assert not _loss_same(l2_mask1, l2)
    # captured graph
    hip_g, sg = _qwen_step(**kw)
    gstep = sg.capture_graph(b1[0])
    assert hip_g.lora_dropout.step() == 0                          # capturing is not a step
    g1 = gstep(b1[0], noise=b1[1], u=b1[2]).clone()
    g2 = gstep(b1[0], noise=b1[1], u=b1[2]).clone()
    assert hip_g.lora_dropout.step() == 2
    assert _loss_same(g1, l1) and _loss_same(g2, l2)
    assert torch.equal(hip_g.lora_store.pflat.view(torch.int32), hip_a.lora_store.pflat.view(torch.int32))
    # resume
    sa.save_checkpoint(str(tmp_path / "ck"))
    sd = torch.load(os.path.join(tmp_path, "ck", "optimizer.bin"), map_location="cpu", weights_only=False)
    assert sd["lora_dropout"] == {"seed": SEED, "step": 2, "network_dropout": P_E, "rank_dropout": P_R}
    b3 = tiny_embeddings(seed=13)
    l3 = sa.train_step(b3[0], noise=b3[1], u=b3[2]).clone()
    hip_b, sb = _qwen_step()                                        # a fresh step object, the option comes from the file
    sb.load_checkpoint(str(tmp_path / "ck"), adapter_name="lora_edit")
    assert hip_b.lora_dropout is not None and hip_b.lora_dropout.step() == 2
    r3 = sb.train_step(b3[0], noise=b3[1], u=b3[2])
    assert _loss_same(r3, l3)
    assert torch.equal(hip_b.lora_store.pflat.view(torch.int32), hip_a.lora_store.pflat.view(torch.int32))
    assert hip_b.lora_dropout.step() == 3


def test_mxfp8_trunk_is_refused_and_samplers_ignore_the_option():
    from qflux_amd.sampling import FluxSampler, QwenSampler
    hip, step = _qwen_step(network_dropout=P_E)
    with pytest.raises(NotImplementedError):
        hip.quantize_trunk("mxfp8")
    hip_q, _ = _qwen_step()
    hip_q.quantize_trunk("mxfp8")
    with pytest.raises(NotImplementedError):
        hip_q.set_lora_dropout(P_E, 0.0)
    # samplers: p > 0 gives the bits of p = 0, with and without the train step, in training mode
    g = torch.Generator().manual_seed(3)
    B, T, Jd = 2, 5, 512
    emb = dict(control_latents=torch.randn(B, 24, 64, generator=g), prompt_embeds=torch.randn(B, T, Jd, generator=g) * 4,
               prompt_embeds_mask=torch.ones(B, T, dtype=torch.int64), img_shapes=[[(1, 4, 6), (1, 4, 6)]] * B,
               num_inference_steps=2, true_cfg_scale=1.0, latents=torch.randn(B, 24, 64, generator=g))
    hip0, _ = _qwen_step()
    want = QwenSampler(hip0).sample(emb)
    assert torch.equal(QwenSampler(hip).sample(emb), want) and torch.equal(QwenSampler(hip).sample(emb, train_step=step), want)
    assert hip.lora_dropout.enabled and hip.lora_dropout.step() == 0
    from oracle import flux_dit as FO
    femb, _, _ = _flux_batch()
    lat_ids = FO.prepare_latent_image_ids(4, 6)
    femb = dict(femb, latents=torch.randn(2, 24, 64, generator=g), latent_ids=lat_ids, guidance=1.0, num_inference_steps=2, true_cfg_scale=1.0)
    f0, _ = _flux_step()
    f1, _ = _flux_step(network_dropout=P_E, rank_dropout=P_R)
    assert torch.equal(FluxSampler(f1).sample(femb), FluxSampler(f0).sample(femb))
