"""GPU: the max-norm launch (qfx_maxnorm_apply) against tests/maxnorm_ref.py on mixed tables, then inside the train steps (eager,
captured, with EMA, under other optimizer families) and in the stock loop.  The norm is compared to 1 fp32 ulp (two fp64 sums in
different orders, rounded once); everything behind it -- the ratio from the kernel's own norm, the scaled weights from the kernel's
own ratio, what must stay untouched -- bit for bit on int32 views."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_ref as E  # noqa: E402
import maxnorm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TARGETS = ("to_k", "to_q", "to_v", "to_out.0", "img_mlp.net.2")
CANARY = 12345.0
M = 2.0
# a single row; below and across the 64-lane and 256-lane boundaries; a rank that is no multiple of 16 (nor of the 4 x 4 blocks);
# 8 x 8 blocks with a ragged edge; the largest rank; one real pair
SHAPES = [(1, 5, 3), (4, 64, 48), (16, 256, 192), (17, 100, 7), (96, 257, 33), (128, 64, 64), (16, 3072, 3072)]
FACTORS = (0.25, 0.75, 1.5, 4.0)          # norm_raw / M
INF, NAN = float("inf"), float("nan")
_FIX = {}


def _make_pairs(specs, seed):
    """specs: (r, in, out, scale, kind) with kind a factor of FACTORS, "zero" (B = 0) or "nan".  CPU fp32 (A, B, scale)."""
    g = torch.Generator().manual_seed(seed)
    pairs = []
    for r, nin, nout, scale, kind in specs:
        A, B = torch.randn(r, nin, generator=g) * 0.1, torch.randn(nout, r, generator=g) * 0.1
        if kind == "zero":
            B.zero_()
        elif kind == "nan":
            A[r // 2, nin // 3] = NAN
        else:           # rescaled in fp64 so that norm_raw lands on kind * M
            nr = abs(float(R.f32(scale))) * float((B.double() @ A.double()).pow(2).sum().sqrt())
            B = (B.double() * (kind * M / nr)).float()
        pairs.append((A, B, scale))
    return pairs


def _lay_out(pairs, odd):
    """Offsets of every matrix in one flat buffer with at least 4 canary floats before, between and behind them: all multiples of 4
    floats, or (odd) 1 or 3 floats off a 16-byte boundary.  Returns (rows for ops.maxnorm_table, CPU buffer, matrix mask)."""
    rows, spans, cur, k = [], [], 0, 0
    for A, B, scale in pairs:
        offs = []
        for t in (A, B):
            cur = (cur + 3) // 4 * 4 + 4 + ((1, 3)[k % 2] if odd else 0)
            k += 1
            offs.append(cur)
            spans.append((cur, t))
            cur += t.numel()
        rows.append((offs[0], offs[1], A.shape[0], A.shape[1], B.shape[0], scale))
    buf = torch.full(((cur + 3) // 4 * 4 + 8,), CANARY)
    mask = torch.zeros(buf.numel(), dtype=torch.bool)
    for off, t in spans:
        buf[off:off + t.numel()] = t.reshape(-1)
        mask[off:off + t.numel()] = True
    return rows, buf, mask


def _fixture(name):
    """One table, its reference result on the CPU and (computed once, never modified) the reference with the threshold at inf."""
    if name not in _FIX:
        if name == "many":       # more pairs than CUs
            specs = [(4, 64, 48, (0.5, 2.0, -1.0)[i % 3], FACTORS[i % 4]) for i in range(300)]
            odd = False
        else:                    # every shape once below and once above the threshold, plus B = 0 and a NaN
            specs = [(r, i, o, (0.5, 2.0, -1.0, 1.0)[(k + j) % 4], FACTORS[(k + 2 * j) % 4]) for k, (r, i, o) in enumerate(SHAPES) for j in range(2)]
            specs += [(4, 64, 48, 1.0, "zero"), (16, 256, 192, 1.0, "nan")]
            odd = name == "odd"
        pairs = _make_pairs(specs, seed=len(name))
        rows, buf, mask = _lay_out(pairs, odd)
        after = [(a.clone(), b.clone(), s) for a, b, s in pairs]
        keys, mean, mx, norms, ratios, raw = R.apply(after, M)
        _FIX[name] = dict(pairs=pairs, rows=rows, buf=buf, mask=mask, keys=keys, mean=mean, max=mx, norms=norms, ratios=ratios, raw=raw)
    return _FIX[name]


def _launch(fx, max_norm):
    from qflux_amd import ops
    buf = fx["buf"].to(DEV)
    lay = ops.maxnorm_table(fx["rows"], device=DEV, n_elems=buf.numel())
    n = lay.n_pairs
    norms, ratios, summary = (torch.full((k,), -7.0, device=DEV) for k in (n, n, 4))
    ops.maxnorm_apply(buf, lay, max_norm, norms, ratios, summary)
    return buf.cpu(), norms.cpu(), ratios.cpu(), summary.cpu()


def _mat(buf, off, like):
    return buf[off:off + like.numel()].view(like.shape)


def _check(fx, buf, norms, ratios, summary, what):
    raw = fx["raw"]
    finite = torch.isfinite(raw)
    # the condition on the fixture: no finite pair within 1e-3 of the threshold, so the last bit of a norm flips no decision
    assert bool(((raw[finite] / M - 1).abs() > 1e-3).all())
    assert bool((buf[~fx["mask"]] == CANARY).all()), what
    want_scaled = fx["ratios"] != 1
    assert torch.equal(ratios != 1, want_scaled), what
    for i, ((A, B, _), row) in enumerate(zip(fx["pairs"], fx["rows"])):
        got_a, got_b = _mat(buf, row[0], A), _mat(buf, row[1], B)
        if not bool(want_scaled[i]):
            # unscaled, zero and NaN pairs: the reported value is norm_raw, the weights are the bits they were
            assert R.ulps(norms[i], raw[i]) <= 1, (what, i, float(norms[i]), float(raw[i]))
            assert float(ratios[i]) == 1.0 and R.same_bits(got_a, A) and R.same_bits(got_b, B), (what, i)
            continue
        # scaled: ratio = M / norm_raw for a norm_raw within 1 ulp of the reference's
        cands = torch.stack([torch.nextafter(raw[i], R.f32(0.0)), raw[i], torch.nextafter(raw[i], R.f32(INF))])
        hit = (R.f32(M) / cands) == ratios[i]
        assert bool(hit.any()), (what, i, float(ratios[i]), float(raw[i]))
        nr = cands[hit][0]
        assert R.same_bits(norms[i], nr * ratios[i]), (what, i)
        q = torch.sqrt(ratios[i])
        assert R.same_bits(got_a, A * q) and R.same_bits(got_b, B * q), (what, i)
    assert summary[0].item() == fx["keys"] and summary[3].item() == 0.0, what
    assert R.ulps(summary[1], fx["mean"]) <= 1 and R.ulps(summary[2], fx["max"]) <= 1, (what, summary, fx["mean"], fx["max"])


@pytest.mark.parametrize("name", ["aligned", "odd", "many"])
def test_launch_matches_the_restatement(name):
    fx = _fixture(name)
    n = len(fx["pairs"])
    assert 0 < fx["keys"] < n and (name == "many" or (int(torch.isnan(fx["raw"]).sum()) == 1 and int((fx["raw"] == 0).sum()) == 1))
    if name != "many":
        assert all(((off % 4) in (1, 3)) == (name == "odd") for row in fx["rows"] for off in row[:2])
    first = _launch(fx, M)
    _check(fx, *first, what=name)
    again = _launch(fx, M)                 # the same inputs: the same bits
    assert all(R.same_bits(x, y) for x, y in zip(first, again))
    # measure only: nothing is written, every raw norm is reported
    buf, norms, ratios, summary = _launch(fx, INF)
    assert R.same_bits(buf, fx["buf"]) and bool((ratios == 1).all()) and summary[0].item() == 0.0
    assert R.ulps(norms, fx["raw"]) <= 1
    keys, mean, mx = R.summarize(fx["raw"], torch.ones(n))
    assert R.ulps(summary[1], mean) <= 1 and R.ulps(summary[2], mx) <= 1


# ------------------------------------------------------------------ inside the train steps

def _qwen(seed=2):
    from common import TINY
    from parity_util import build_pair
    return build_pair(dict(TINY), device=DEV, targets=TARGETS, seed=seed)[1]


def _batch():
    from parity_util import tiny_embeddings
    return tiny_embeddings(B=1, seed=5)


def _between(norms):
    """A threshold between the two middle norms: about half of the pairs lie above it, none on it."""
    s = norms.detach().cpu().sort().values
    lo, hi = float(s[len(s) // 2 - 1]), float(s[len(s) // 2])
    assert 0 < lo < hi
    return (lo + hi) / 2


def _qwen_threshold():
    """Between the adapters' norms after the first step of the run the tests repeat (measured once, with the threshold at inf)."""
    if "qwen_m" not in _FIX:
        from qflux_amd.trainer import QwenLoraTrainStep
        step = QwenLoraTrainStep(_qwen(), lr=1e-2, max_weight_norm=INF)
        e, nz, u = _batch()
        step.train_step(e, noise=nz, u=u)
        assert step.weight_norm_stats()[0] == 0
        _FIX["qwen_m"] = _between(step.last_weight_norms.norms)
    return _FIX["qwen_m"]


def _run_pair(sa, sb, reg, run_a, run_b, a, b, steps=3):
    """sa carries max_weight_norm, sb is the plain step with MaxNorm.step() by hand behind it: bit-equal adapter weights after every
    step; after the first one some pairs are scaled and some are not."""
    m = sa.max_weight_norm
    for it in range(steps):
        run_a(it)
        run_b(it)
        reg.step()
        assert R.same_bits(a.lora_store.pflat, b.lora_store.pflat), it
        assert R.same_bits(sa.last_weight_norms.norms, reg.norms) and R.same_bits(sa.last_weight_norms.ratios, reg.ratios), it
        keys, mean, mx = sa.weight_norm_stats()
        assert (keys, mean, mx) == reg.stats() and 0 < keys and (it > 0 or keys < len(reg.names)), (it, keys)      # first step: some scale, some do not
        assert mx <= m * (1 + 1e-6) and int((sa.last_weight_norms.ratios != 1).sum()) == keys
    assert sb.last_weight_norms is None and sb.weight_norm_stats() is None


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_in_the_qwen_step_equals_the_launch_applied_by_hand(captured):
    from qflux_amd.regularize import MaxNorm
    from qflux_amd.trainer import QwenLoraTrainStep
    m = _qwen_threshold()
    a, b = _qwen(), _qwen()
    sa, sb = QwenLoraTrainStep(a, lr=1e-2, max_weight_norm=m), QwenLoraTrainStep(b, lr=1e-2)
    reg = MaxNorm(b, m)
    e, nz, u = _batch()
    fa, fb = (s.capture_graph(e) for s in (sa, sb)) if captured else (sa.train_step, sb.train_step)
    assert sa.last_weight_norms is None
    _run_pair(sa, sb, reg, lambda it: fa(e, noise=nz, u=u), lambda it: fb(e, noise=nz, u=u), a, b)
    assert reg.names == sa.last_weight_norms.names and len(reg.names) == len([n for n, _ in a.named_parameters() if "lora_A" in n])


def test_ema_averages_the_clamped_weights():
    from qflux_amd.trainer import QwenLoraTrainStep
    m = _qwen_threshold()
    a = _qwen()
    step = QwenLoraTrainStep(a, lr=1e-2, max_weight_norm=m, ema_decay=0.9)
    ref = E.Ema([a.lora_store.pflat.detach().clone()], 0.9)
    e, nz, u = _batch()
    for it in range(3):
        step.train_step(e, noise=nz, u=u)
        assert step.weight_norm_stats()[0] > 0
        ref.step([a.lora_store.pflat])             # the restatement sees the weights as the clamp left them
        assert E.same_bits(step.ema.shadows[0], ref.shadow[0]), it


@pytest.mark.parametrize("family,lr", [("adam8bit", 1e-2), ("prodigy", 1.0)])
def test_the_clamp_holds_under_other_families(family, lr):
    from qflux_amd.trainer import QwenLoraTrainStep
    step = QwenLoraTrainStep(_qwen(), lr=lr, optimizer=family, max_weight_norm=INF)
    e, nz, u = _batch()
    step.train_step(e, noise=nz, u=u)
    m = _between(step.last_weight_norms.norms)     # this family's own norms after its first step
    step.max_weight_norm = m
    for _ in range(2):
        step.train_step(e, noise=nz, u=u)
        norms = step.last_weight_norms.norms.cpu()
        assert bool(torch.isfinite(norms).all()) and float(norms.max()) <= m * (1 + 1e-6) and float(norms.max()) > 0


def test_without_the_option_nothing_is_allocated():
    from qflux_amd.trainer import QwenLoraTrainStep
    step = QwenLoraTrainStep(_qwen(), lr=1e-2)
    e, nz, u = _batch()
    step.train_step(e, noise=nz, u=u)
    assert step.max_weight_norm is None and step.last_weight_norms is None and step.weight_norm_stats() is None


def _flux():
    from common import FLUX_TINY
    from qflux_amd.models import FluxTransformer2DModel
    from qflux_amd.modules import LoraConfig
    cfg = dict(FLUX_TINY, joint_attention_dim=64, guidance_embeds=True)
    with torch.device(DEV):
        m = FluxTransformer2DModel(**cfg)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_((torch.randn(p.shape, generator=g) * (0.5 / p.shape[-1] ** 0.5 if p.ndim == 2 else 0.05) + (1.0 if "norm_" in n and p.ndim == 1 else 0.0)).to(p.dtype))
    m.add_adapter(LoraConfig(r=4, lora_alpha=8), "a", generator=g)
    return m


def test_in_the_flux_step_equals_the_launch_applied_by_hand():
    from oracle import flux_dit as FO
    from qflux_amd.regularize import MaxNorm
    from qflux_amd.trainer import FluxKontextTrainStep
    g = torch.Generator().manual_seed(4)
    ctl = FO.prepare_latent_image_ids(4, 6); ctl[:, 0] = 1
    emb = dict(image_latents=torch.randn(1, 24, 64, generator=g).half(), control_latents=torch.randn(1, 24, 64, generator=g).half(),
               control_ids=ctl, text_ids=torch.zeros(7, 3), latent_hw=(4, 6),
               pooled_prompt_embeds=torch.randn(1, 16, generator=g).half(), prompt_embeds=torch.randn(1, 7, 64, generator=g).half())
    noise = [torch.randn(1, 24, 64, generator=g) for _ in range(3)]
    t = torch.tensor([0.3])
    probe = FluxKontextTrainStep(_flux(), lr=1e-2, max_weight_norm=INF)
    probe.train_step(emb, noise=noise[0], t=t)
    m = _between(probe.last_weight_norms.norms)
    a, b = _flux(), _flux()
    sa, sb = FluxKontextTrainStep(a, lr=1e-2, max_weight_norm=m), FluxKontextTrainStep(b, lr=1e-2)
    reg = MaxNorm(b, m)
    _run_pair(sa, sb, reg, lambda it: sa.train_step(emb, noise=noise[it], t=t), lambda it: sb.train_step(emb, noise=noise[it], t=t), a, b)


def test_stock_loop_equals_the_fused_step():
    """The reference's loop body on the drop-in autograd path -- compute_loss, backward, qflux_amd.optim.AdamW.step(),
    MaxNorm.step() -- against the fused step's optimizer_step with max_weight_norm on a twin model.  The twin is handed the
    gradient the autograd pass left in the flat buffer (the pattern of test_optim_classes_gpu.py): the fused forward/backward
    rounds its gradient elsewhere than autograd does, which is not what this test is about."""
    from qflux_amd import optim as O
    from qflux_amd.regularize import MaxNorm
    from qflux_amd.trainer import QwenLoraTrainStep
    m = _qwen_threshold()
    a, b = _qwen(), _qwen()
    opt = O.AdamW([p for n, p in a.named_parameters() if "lora_" in n], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    reg = MaxNorm(a, m)
    helper = QwenLoraTrainStep(a)
    step = QwenLoraTrainStep(b, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=0, max_weight_norm=m)
    e, nz, u = _batch()
    start = a.lora_store.pflat.detach().clone()
    for it in range(2):
        loss = helper.compute_loss(e, noise=nz, u=u)
        loss.backward()
        b.lora_store.gflat.copy_(a.lora_store.gflat)
        assert float(a.lora_store.gflat.abs().max()) > 0
        opt.step()
        reg.step()
        step.optimizer_step()
        opt.zero_grad()
        step.zero_grad()
        assert R.same_bits(a.lora_store.pflat, b.lora_store.pflat), it
        assert R.same_bits(reg.norms, step.last_weight_norms.norms) and reg.stats() == step.weight_norm_stats()
        assert 0 < reg.stats()[0] and (it > 0 or reg.stats()[0] < len(reg.names)), (it, reg.stats())
    assert not R.same_bits(a.lora_store.pflat, start)
