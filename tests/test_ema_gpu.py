"""GPU: the fused EMA update and the bit-exact swap (qfx_ema_update, qfx_ema_swap) against tests/ema_ref.py, EMA inside the train
steps (eager and through the captured graph), the eval form, the sampler, checkpoints and the stock-loop class.  Every numeric
comparison is bit for bit, on int32 views: the package's three fp32 roundings are the specification, and a swap moves words."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TARGETS = ("to_k", "to_q", "to_v", "to_out.0", "img_mlp.net.2")
# 1, 3: tail only; 63..65, 255..257, 1023: around the 64-lane wave, the 256-lane workgroup and the 16-byte body; the last: more
# quads than 4096 workgroups of 256 lanes take in one pass (the stride loop runs) and a 1-element tail behind them
SIZES = [1, 3, 63, 64, 65, 255, 256, 257, 1023, 4 * 256 * 4096 + 5]
OMDS = (0.0, 1.0, 1e-4, 0.5)
CANARY = 12345.0
# (offset of p, offset of the last buffer) in floats from a fresh allocation: all 16-byte aligned, then p and then one shadow one
# float off (the scalar instantiation)
ALIGNMENTS = ((0, 0), (1, 0), (0, 1))


def _slot(n, shift):
    """n floats `shift` into a fresh canary-filled allocation with 8 canary floats (and more) behind them."""
    buf = torch.full((n + 8 + 4,), CANARY, device=DEV)
    return buf, buf[shift:shift + n]


def _canaries_ok(buf, n, shift):
    return bool((buf[:shift] == CANARY).all()) and bool((buf[shift + n:] == CANARY).all()) and buf.numel() - shift - n >= 8


def _same(a, b):
    """Bit equality of two device tensors (the long case stays on the device)."""
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


_DATA = {}


def _data(n):
    """p and four shadows for one length, generated once and never modified; some elements are zero or equal to p."""
    if n not in _DATA:
        g = torch.Generator().manual_seed(1000 + n % 997)
        p = torch.randn(n, generator=g) * 0.1
        shadows = [p + torch.randn(n, generator=g) * 0.01 for _ in range(4)]
        for k, s in enumerate(shadows):
            s[k::7] = p[k::7]
            s[(k + 3)::11] = 0.0
        p[5::13] = 0.0
        _DATA[n] = (p, shadows)
    return _DATA[n]


@pytest.mark.parametrize("n", SIZES)
def test_update_matches_the_restatement_bit_for_bit(n):
    from qflux_amd import ops
    p, shadows = _data(n)
    want = {}
    for ns in (1, 2, 4):
        omds = OMDS[4 - ns:] if ns < 4 else OMDS           # a different rate per shadow: (0.5), (1e-4, 0.5), (0, 1, 1e-4, 0.5)
        ref = [s.clone() for s in shadows[:ns]]
        snaps = []
        for _ in range(2):                                  # two launches: the second starts from the first one's bits
            for s, omd in zip(ref, omds):
                R.update([s], [p], omd)
            snaps.append([s.to(DEV) for s in ref])
        want[ns] = (omds, snaps)
    assert n < 4 or not _same(want[4][1][1][2], shadows[2].to(DEV))
    p_dev = p.to(DEV)
    for ns in (1, 2, 4):
        omds, snaps = want[ns]
        for p_shift, s_shift in ALIGNMENTS:
            pbuf, pd = _slot(n, p_shift)
            pd.copy_(p)
            slots = [_slot(n, s_shift if k == ns - 1 else 0) for k in range(ns)]
            for (_, sd), s in zip(slots, shadows):
                sd.copy_(s)
            for it in range(2):
                ops.ema_update(pd, [sd for _, sd in slots], list(omds))
                for k, (_, sd) in enumerate(slots):
                    assert _same(sd, snaps[it][k]), (n, ns, p_shift, s_shift, it, k, omds[k])
            assert _same(pd, p_dev) and _canaries_ok(pbuf, n, p_shift), (n, ns, p_shift, s_shift)
            for k, (buf, _) in enumerate(slots):
                assert _canaries_ok(buf, n, s_shift if k == ns - 1 else 0), (n, ns, p_shift, s_shift, k)


def _words(n, seed, flip=False):
    """n random 32-bit patterns (NaN payloads, infinities and denormals among them) with the named special values up front (flip:
    in reverse order, so that two buffers differ from the first word on)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    special = torch.tensor([0x00000000, -0x80000000, 0x7FC00001, -0x00345678, 0x7F800001, 0x00000001, -0x7FFFFFFF, 0x007FFFFF,
                            0x7F800000, -0x00800000], dtype=torch.int64).to(torch.int32)   # +0 -0 qNaN+payload -NaN sNaN denormals inf
    k = min(n, special.numel())
    w[:k] = (special.flip(0) if flip else special)[:k]
    return w


@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_every_word_and_twice_is_the_identity(n):
    from qflux_amd import ops
    a, b = _words(n, 7 + n % 89), _words(n, 11 + n % 97, flip=True)
    assert not bool((a == b).all())
    f = a.view(torch.float32)
    assert n < 16 or (bool(torch.isnan(f).any()) and bool((f == 0).any()) and bool(((f != 0) & (f.abs() < 1.1754944e-38)).any()))
    for p_shift, s_shift in ALIGNMENTS:
        pbuf, pd = _slot(n, p_shift)
        sbuf, sd = _slot(n, s_shift)
        pd.view(torch.int32).copy_(a)
        sd.view(torch.int32).copy_(b)
        ops.ema_swap(pd, sd)
        assert torch.equal(pd.view(torch.int32).cpu(), b) and torch.equal(sd.view(torch.int32).cpu(), a), (n, p_shift, s_shift)
        ops.ema_swap(pd, sd)
        assert torch.equal(pd.view(torch.int32).cpu(), a) and torch.equal(sd.view(torch.int32).cpu(), b), (n, p_shift, s_shift)
        assert _canaries_ok(pbuf, n, p_shift) and _canaries_ok(sbuf, n, s_shift), (n, p_shift, s_shift)


def _pair(seed=2):
    from common import TINY
    from parity_util import build_pair
    _, m = build_pair(dict(TINY), device=DEV, targets=TARGETS, seed=seed)
    return m


EMA_KW = dict(ema_decay=(0.5, 0.9), ema_args={"update_after_step": 1})


def _refs(pflat, decays=(0.5, 0.9), **kw):
    return [R.Ema([pflat], d, **kw) for d in decays]


def _check_shadows(step, refs, pflat, what):
    got = []
    for k, ref in enumerate(refs):
        got.append(ref.step([pflat]))
        assert R.same_bits(step.ema.shadows[k], ref.shadow[0]), (what, k)
    return got


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_in_the_step_shadows_follow_the_restatement_and_training_is_untouched(captured):
    """Batch 1: the criterion kernel then adds ONE non-zero partial sum to the loss (one workgroup holds every target token), so
    the loss itself is the same bits run after run and can be compared bit for bit as the weights are."""
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    a, b = _pair(), _pair()
    sa, sb = QwenLoraTrainStep(a, lr=1e-2, **EMA_KW), QwenLoraTrainStep(b, lr=1e-2)
    e, nz, u = tiny_embeddings(B=1, seed=5)
    start = a.lora_store.pflat.detach().clone()
    refs = _refs(start, update_after_step=1)
    run_a, run_b = (s.capture_graph(e) for s in (sa, sb)) if captured else (sa.train_step, sb.train_step)
    assert sa.ema is None and R.same_bits(a.lora_store.pflat, start)               # capturing is not a step
    la, lb, decays = [], [], []
    for it in range(3 if captured else 6):
        la.append(run_a(e, noise=nz, u=u).detach().cpu().clone())
        lb.append(run_b(e, noise=nz, u=u).detach().cpu().clone())
        decays.append(_check_shadows(sa, refs, a.lora_store.pflat, f"step {it}"))
        assert sa.ema.optimization_step == sa.global_step == it + 1
    assert decays[:3] == [[0.0, 0.0], [0.0, 0.0], [2 / 11, 2 / 11]]
    if not captured:      # (1 + s) / (10 + s) stays below both decays over these steps: the two shadows carry the same values
        assert decays[3:] == [[3 / 12, 3 / 12], [4 / 13, 4 / 13], [5 / 14, 5 / 14]]
    assert all(R.same_bits(x, y) for x, y in zip(la, lb)), (la, lb)
    assert R.same_bits(a.lora_store.pflat, b.lora_store.pflat) and not R.same_bits(a.lora_store.pflat, start)
    assert not R.same_bits(sa.ema.shadows[0], a.lora_store.pflat) and sa.ema.shadows[0].data_ptr() != sa.ema.shadows[1].data_ptr()
    assert sb.ema is None and sb.train_mode and sa.train_mode


def _trained(steps=4, ema_args=None):
    """A model trained for a few steps with two shadows whose decays part at the first averaged step (0.1 clamps 2 / 11)."""
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    m = _pair()
    step = QwenLoraTrainStep(m, lr=1e-2, ema_decay=(0.1, 0.9), ema_args=ema_args)
    e, nz, u = tiny_embeddings(seed=5)
    for _ in range(steps):
        step.train_step(e, noise=nz, u=u)
    return m, step, (e, nz, u)


def _forward(m, e, nz):
    """One DiT forward as the sampling loop calls it."""
    x = torch.cat([nz.to(DEV, torch.bfloat16), e["control_latents"].to(DEV, torch.bfloat16)], dim=1)
    pe, mask = e["prompt_embeds"].to(DEV, torch.bfloat16), e["prompt_embeds_mask"]
    ts = torch.full((x.shape[0],), 0.5, dtype=torch.bfloat16, device=DEV)
    with torch.inference_mode():
        return m(hidden_states=x, timestep=ts, guidance=None, encoder_hidden_states_mask=mask, encoder_hidden_states=pe,
                 img_shapes=e["img_shapes"], txt_seq_lens=mask.sum(dim=1).tolist(), attention_kwargs={}, return_dict=False)[0]


def test_eval_form_is_the_shadow_and_the_way_back_is_exact(tmp_path):
    from qflux_amd.sampling import QwenSampler
    from qflux_amd.trainer import QwenLoraTrainStep
    m, step, (e, nz, u) = _trained()
    ck = str(tmp_path / "ck")
    step.save_checkpoint(ck)
    st = m.lora_store
    trained = st.pflat.detach().clone()
    shadows = [s.detach().clone() for s in step.ema.shadows]
    assert not R.same_bits(shadows[1], trained) and not R.same_bits(shadows[0], shadows[1])
    other1, other0 = _pair(), _pair()
    for o in (other1, other0):
        QwenLoraTrainStep(o, lr=1e-2)              # set up like m: a train step prepares the model's modulation table
    other1.load_lora_adapter(os.path.join(ck, "pytorch_lora_weights_ema1.safetensors"), adapter_name="lora_edit")
    other0.load_lora_adapter(os.path.join(ck, "pytorch_lora_weights_ema.safetensors"), adapter_name="lora_edit")
    assert R.same_bits(other1.lora_store.pflat, shadows[1]) and R.same_bits(other0.lora_store.pflat, shadows[0])
    from_trained = _forward(m, e, nz)
    with step.eval_mode(ema=1):
        assert step.train_mode is False and step.ema.active == 1
        assert R.same_bits(st.pflat, shadows[1]) and R.same_bits(step.ema.shadows[1], trained)
        inside = _forward(m, e, nz)
        with pytest.raises(RuntimeError, match=r"EMA shadow 1.*train\(\) first"):
            step.optimizer_step()
        with pytest.raises(RuntimeError, match=r"EMA shadow 1.*train\(\) first"):
            step.forward_backward(e, noise=nz, u=u)
        with pytest.raises(RuntimeError, match=r"train\(\) first"):
            step.train_step(e, noise=nz, u=u)
        with pytest.raises(ValueError, match="shadows 0..1"):
            step.eval(ema=2)
        step.eval(ema=1)                                                           # the same shadow again: nothing moves
        assert R.same_bits(st.pflat, shadows[1])
        step.eval(ema=0)                                                           # another shadow: 1 goes out first
        assert R.same_bits(st.pflat, shadows[0]) and R.same_bits(step.ema.shadows[1], shadows[1]) and step.ema.active == 0
    assert step.train_mode is True and step.ema.active is None and step.global_step == 4
    assert R.same_bits(st.pflat, trained) and all(R.same_bits(s, t) for s, t in zip(step.ema.shadows, shadows))
    assert float(st.gflat.abs().max()) == 0.0                                      # the refused passes left no gradient behind
    assert torch.equal(inside, _forward(other1, e, nz)) and not torch.equal(inside, from_trained)
    # the sampler under train_step= samples from shadow 0 and leaves the trained weights in place
    emb = dict(e, latents=nz.clone(), num_inference_steps=2, true_cfg_scale=1.0)
    from_ema = QwenSampler(m).sample(emb, train_step=step)
    assert torch.equal(from_ema, QwenSampler(other0).sample(emb)) and not torch.equal(from_ema, QwenSampler(m).sample(emb))
    assert R.same_bits(st.pflat, trained) and step.train_mode is True
    step.train_step(e, noise=nz, u=u)                                              # training goes on
    assert step.global_step == step.ema.optimization_step == 5 and not R.same_bits(st.pflat, trained)


def test_checkpoint_files_and_bit_exact_resume(tmp_path):
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    a, sa, (e, nz, u) = _trained(steps=3, ema_args={"update_after_step": 1})
    ck = str(tmp_path / "ck")
    with sa.eval_mode(ema=1):                                                      # saved from the eval form: same files, same form after
        sa.save_checkpoint(ck)
        assert sa.ema.active == 1
    for f in ("pytorch_lora_weights.safetensors", "pytorch_lora_weights_ema.safetensors", "pytorch_lora_weights_ema1.safetensors",
              "ema.bin", "optimizer.bin", "state.json"):
        assert os.path.exists(os.path.join(ck, f)), f
    at_save = a.lora_store.pflat.detach().clone()
    plain = _pair()
    plain.load_lora_adapter(ck, adapter_name="lora_edit")
    assert R.same_bits(plain.lora_store.pflat, at_save)                            # the plain file holds the trained weights
    sd = torch.load(os.path.join(ck, "ema.bin"), map_location="cpu", weights_only=False)
    assert len(sd) == 2 and all(set(s) == R.KEYS and s["optimization_step"] == 3 and s["update_after_step"] == 1 for s in sd)
    assert [s["decay"] for s in sd] == [0.1, 0.9] and not R.same_bits(sa.ema.shadows[0], sa.ema.shadows[1])
    for k, s in enumerate(sd):
        assert [t.shape for t in s["shadow_params"]] == [p.shape for _, p, _, _ in a.lora_store.entries]
        assert all(R.same_bits(t.reshape(-1), sa.ema.shadows[k][off:off + n]) for t, (_, _, off, n) in zip(s["shadow_params"], a.lora_store.entries))
    for _ in range(2):
        sa.train_step(e, noise=nz, u=u)
    b = _pair()
    sb = QwenLoraTrainStep(b, lr=0.5, ema_decay=(0.3, 0.2))
    sb.load_checkpoint(ck, adapter_name="lora_edit")
    assert sb.ema.optimization_step == 3 and sb.ema.decays == sb.ema_decays == (0.1, 0.9) and sb.ema.args["update_after_step"] == 1 and sb.global_step == 3
    for _ in range(2):
        sb.train_step(e, noise=nz, u=u)
    assert R.same_bits(b.lora_store.pflat, a.lora_store.pflat)
    assert all(R.same_bits(x, y) for x, y in zip(sb.ema.shadows, sa.ema.shadows)) and sb.ema.optimization_step == 5
    # without ema.bin: a warning, shadows from the loaded weights, no update counted; without ema_decay the file is not read
    c = _pair()
    QwenLoraTrainStep(c, lr=0.5).load_checkpoint(ck, adapter_name="lora_edit")
    os.remove(os.path.join(ck, "ema.bin"))
    sc = QwenLoraTrainStep(c, lr=0.5, ema_decay=(0.5, 0.9))
    with pytest.warns(UserWarning, match="no ema.bin"):
        sc.load_checkpoint(ck)
    assert sc.ema.optimization_step == 0 and all(R.same_bits(s, at_save) for s in sc.ema.shadows) and R.same_bits(c.lora_store.pflat, at_save)


def _nudge(params, g):
    """Move every parameter a little (through the parameters: the padding between them in the flat buffer stays zero)."""
    with torch.no_grad():
        for p in params:
            p.add_((torch.randn(p.shape, generator=g) * 0.01).to(p.device))


def test_stock_loop_class_on_store_backed_parameters():
    from qflux_amd.ema import EMAModel
    m = _pair()
    st = m.lora_store
    params = [p for n, p in m.named_parameters() if "lora_" in n]
    kw = dict(decay=0.9, use_ema_warmup=True, power=0.75)
    ema = EMAModel(params, **kw)
    assert ema._state is not None and [tuple(s.shape) for s in ema.shadow_params] == [tuple(p.shape) for p in params]
    ref = R.Ema([st.pflat], 0.9, use_ema_warmup=True, power=0.75)
    g = torch.Generator().manual_seed(4)
    for it in range(4):
        _nudge(params, g)
        ema.step(params)
        assert ema.cur_decay_value == ref.step([st.pflat]) and ema.optimization_step == it + 1
        assert R.same_bits(ema._state.shadows[0], ref.shadow[0]), it
    assert not R.same_bits(ref.shadow[0], st.pflat)
    sd = ema.state_dict()
    assert set(sd) == R.KEYS and sd["optimization_step"] == 4 and [t.shape for t in sd["shadow_params"]] == [p.shape for p in params]
    other = EMAModel(params, decay=0.5)
    assert R.same_bits(other._state.shadows[0], st.pflat)
    other.load_state_dict(sd)
    assert other.decay == 0.9 and other.power == 0.75 and other.optimization_step == 4 and R.same_bits(other._state.shadows[0], ref.shadow[0])
    trained = st.pflat.detach().clone()
    ema.store(params)
    ema.copy_to(params)
    assert R.same_bits(st.pflat, ref.shadow[0]) and all(R.same_bits(p, s) for p, s in zip(params, ema.shadow_params))
    ema.restore(params)
    assert R.same_bits(st.pflat, trained) and ema.temp_stored_params is None
    _nudge(params, g)
    ema.step(params); other.step(params); ref.step([st.pflat])
    assert R.same_bits(ema._state.shadows[0], ref.shadow[0]) and R.same_bits(other._state.shadows[0], ref.shadow[0])


def test_flux_step_keeps_its_shadow():
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
    step = FluxKontextTrainStep(m, lr=1e-3, ema_decay=0.9)
    ctl = FO.prepare_latent_image_ids(4, 6); ctl[:, 0] = 1
    emb = dict(image_latents=torch.randn(2, 24, 64, generator=g).half(), control_latents=torch.randn(2, 24, 64, generator=g).half(),
               control_ids=ctl, text_ids=torch.zeros(7, 3), latent_hw=(4, 6),
               pooled_prompt_embeds=torch.randn(2, 16, generator=g).half(), prompt_embeds=torch.randn(2, 7, 64, generator=g).half())
    refs = _refs(m.lora_store.pflat, decays=(0.9,))
    for it in range(2):
        before = m.lora_store.pflat.detach().clone()
        loss = step.train_step(emb, noise=torch.randn(2, 24, 64, generator=g), t=torch.tensor([0.3, 0.8]))
        assert torch.isfinite(loss).all() and not torch.equal(before, m.lora_store.pflat)
        assert _check_shadows(step, refs, m.lora_store.pflat, f"flux step {it}") == [[0.0], [2 / 11]][it]
    assert not R.same_bits(step.ema.shadows[0], m.lora_store.pflat)
    trained = m.lora_store.pflat.detach().clone()
    with step.eval_mode():
        assert R.same_bits(m.lora_store.pflat, refs[0].shadow[0]) and step.train_mode is False
    assert R.same_bits(m.lora_store.pflat, trained)


def test_buffer_names_and_replica_check():
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    m = _pair()
    step = QwenLoraTrainStep(m, lr=1e-3, **EMA_KW)
    assert [n for n, _ in step._state_buffers()] == ["lora", "m", "v", "ema0", "ema1"] and step._state_buffers()[-1][1] is None
    e, nz, u = tiny_embeddings(seed=5)
    step.train_step(e, noise=nz, u=u)
    bufs = step._state_buffers()
    assert [n for n, _ in bufs] == ["lora", "m", "v", "ema0", "ema1"] and bufs[3][1] is step.ema.shadows[0] and bufs[4][1] is step.ema.shadows[1]
    assert step.check_replicas() is True
    plain = QwenLoraTrainStep(m, lr=1e-3)
    plain.train_step(e, noise=nz, u=u)
    assert plain.ema is None and [n for n, _ in plain._state_buffers()] == ["lora", "m", "v"]
