"""GPU: qfx_adapter_stats against its restatement (tests/adapter_stats_ref.py) and the train steps' adapter_stats_every.

Bounds (derived, adapter_stats_ref.bound): every term of a sum is non-negative and passes through at most ceil(numel / 256) + 11
fp32 additions and one rounded square, so |sum - sum64| <= (ceil(numel / 256) + 12) 2^-24 sum64; + 2 in the factor for update_sq,
whose difference is rounded before it is squared.  grad_absmax, the counts and the snapshot are exact.  The kernel's sums are also
compared bit for bit with the restatement's fp32 sums in the kernel's order: that order is the specification (include/qfx.h)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapter_stats_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TARGETS = ("to_k", "to_q", "to_v", "to_out.0", "img_mlp.net.2")
NUMELS = (1, 63, 64, 65, 255, 256, 257, 1024, 4097, 16 * 3072)
GUARD = 12345.0
# six tensors of the list above at 64-aligned offsets, in non-monotonic offset order, with padding between them
MIXED = [(53312, 4097), (0, 1), (4160, 16 * 3072), (64, 65), (3072, 255), (1024, 1024)]
MIXED_TOTAL = 53312 + 4097

_DATA = {}


def _data(total, seed):
    """(p before, g, p after) as fp32 numpy vectors, made once per (length, seed) and never modified."""
    if (total, seed) not in _DATA:
        p0 = R.make_tensor(total, seed)
        g = R.make_tensor(total, seed + 1, scale=0.1)
        p1 = (p0 - np.float32(1e-3) * R.make_tensor(total, seed + 2)).astype(np.float32)
        for a in (p0, g, p1):
            a.setflags(write=False)
        _DATA[total, seed] = (p0, g, p1)
    return _DATA[total, seed]


def _run(entries, p0, g, p1, shift=0, gnorm_sq=None, max_norm=0.0, grad_scale=1.0, out_fill=0xA5):
    """Phase 0 on (p0, g), then p <- p1, then phase 1, on views that start `shift` elements into larger allocations.
    -> (rows after phase 0, rows after phase 1, prev after phase 0 with its guard elements, the layout)."""
    from qflux_amd import ops
    total = p0.size
    lay = ops.stats_table_entries(entries, device=DEV)
    assert lay.extent <= total
    bufs = [torch.full((total + 8,), GUARD, device=DEV) for _ in range(3)]
    p, gt, prev = (b[shift:shift + total] for b in bufs)
    p.copy_(torch.tensor(p0))
    gt.copy_(torch.tensor(g))
    out = torch.full((32 * lay.n_entries,), out_fill, dtype=torch.uint8, device=DEV)
    gn = None if gnorm_sq is None else torch.tensor(gnorm_sq, dtype=torch.float32, device=DEV)
    ops.adapter_stats(p, gt, prev, lay, out, 0, gn, max_norm, grad_scale)
    torch.cuda.synchronize()
    rows0, prev0 = ops.stats_rows(out, lay.n_entries).copy(), bufs[2].cpu().numpy().copy()
    p.copy_(torch.tensor(p1))
    ops.adapter_stats(p, None, prev, lay, out, 1)
    torch.cuda.synchronize()
    rows1 = ops.stats_rows(out, lay.n_entries).copy()
    assert np.array_equal(bufs[2].cpu().numpy(), prev0)                       # phase 1 does not write prev
    for b, src in ((bufs[0], p1), (bufs[1], g)):                              # p and g are only read
        h = b.cpu().numpy()
        assert np.array_equal(h[shift:shift + total].view(np.uint32), src.view(np.uint32))
        assert (h[:shift] == GUARD).all() and (h[shift + total:] == GUARD).all()
    return rows0, rows1, prev0, lay


def _check(entries, rows0, rows1, prev0, p0, g, p1, shift, clip=np.float32(1.0)):
    covered = np.zeros(prev0.size, bool)
    for i, (off, k) in enumerate(entries):
        r0, r1 = rows0[i], rows1[i]
        e0, e1 = R.phase0(g, off, k, clip), R.phase1(p1, p0, off, k)
        o0, o1 = R.phase0(g, off, k, clip, ordered=True), R.phase1(p1, p0, off, k, ordered=True)
        for name, got, want, bound in (("grad_sq", r0["grad_sq"], e0["grad_sq"], R.bound(k, e0["grad_sq"])),
                                       ("weight_sq", r1["weight_sq"], e1["weight_sq"], R.bound(k, e1["weight_sq"])),
                                       ("update_sq", r1["update_sq"], e1["update_sq"], R.bound(k, e1["update_sq"], update=True))):
            print(f"entry {i} (off {off}, numel {k}, shift {shift}) {name}: kernel {float(got):.9e} fp64 {want:.9e} "
                  f"|diff| {abs(float(got) - want):.3e} bound {bound:.3e}")
            assert abs(float(got) - want) <= bound, (i, name)
        # the order of the sums is the specification: the restatement's fp32 sums in that order, bit for bit
        assert float(r0["grad_sq"]) == o0["grad_sq"] and float(r1["weight_sq"]) == o1["weight_sq"] and \
            float(r1["update_sq"]) == o1["update_sq"], (i, r0, r1, o0, o1)
        assert float(r0["grad_absmax"]) == e0["grad_absmax"] and int(r0["grad_nonfinite"]) == e0["grad_nonfinite"]
        assert int(r1["weight_nonfinite"]) == e1["weight_nonfinite"]
        # phase 0 wrote the whole row, phase 1 left its fields alone
        assert (r0["weight_sq"], r0["update_sq"], r0["weight_nonfinite"], r0["r0"], r0["r1"]) == (0, 0, 0, 0, 0)
        for f in ("grad_sq", "grad_absmax", "grad_nonfinite", "r0", "r1"):
            assert r0[f].tobytes() == r1[f].tobytes(), (i, f)
        if k > 0 and off >= 0:
            covered[shift + off:shift + off + k] = True
            # the snapshot equals p bit for bit
            assert np.array_equal(prev0[shift + off:shift + off + k].view(np.uint32), p0[off:off + k].view(np.uint32)), i
    # the padding behind each tensor (and everything else of the allocation) is as it was
    assert (prev0[~covered] == GUARD).all()


@pytest.mark.parametrize("shift", (0, 1, 3))
@pytest.mark.parametrize("numel", NUMELS)
def test_one_tensor_against_the_restatement(numel, shift):
    p0, g, p1 = _data(numel, seed=numel)
    rows0, rows1, prev0, _ = _run([(0, numel)], p0, g, p1, shift)
    _check([(0, numel)], rows0, rows1, prev0, p0, g, p1, shift)


@pytest.mark.parametrize("shift", (0, 1, 3))
def test_six_tensors_in_non_monotonic_offset_order(shift):
    p0, g, p1 = _data(MIXED_TOTAL, seed=11)
    rows0, rows1, prev0, _ = _run(MIXED, p0, g, p1, shift)
    _check(MIXED, rows0, rows1, prev0, p0, g, p1, shift)


def test_same_inputs_and_any_alignment_give_the_same_bits():
    p0, g, p1 = _data(MIXED_TOTAL, seed=11)
    runs = [_run(MIXED, p0, g, p1, s) for s in (0, 0, 1, 3)]
    for r in runs[1:]:
        assert r[0].tobytes() == runs[0][0].tobytes() and r[1].tobytes() == runs[0][1].tobytes()


def test_non_finite_elements_are_counted_and_left_out():
    entries = [(0, 4097), (4160, 1024), (5184, 257)]
    total = 5184 + 257
    p0, g, p1 = (a.copy() for a in _data(total, seed=21))
    clean = _run(entries, p0, g, p1)
    g[100], g[4000] = np.nan, np.inf                  # entry 0: the gradient
    p1[4160 + 513] = np.nan                           # entry 1: the weights after the step
    rows0, rows1, prev0, _ = _run(entries, p0, g, p1)
    assert [int(r["grad_nonfinite"]) for r in rows0] == [2, 0, 0] and [int(r["weight_nonfinite"]) for r in rows1] == [0, 1, 0]
    _check(entries, rows0, rows1, prev0, p0, g, p1, 0)      # the restatement leaves the same elements out
    for rows in (rows0, rows1):
        for f in ("grad_sq", "weight_sq", "update_sq", "grad_absmax"):
            assert np.isfinite(rows[f]).all()
    # removed, not zeroed by accident: entry 0's sum is the clean one minus the two squares, within both bounds
    keep = np.delete(_data(total, seed=21)[1][:4097], [100, 4000])
    assert abs(float(rows0[0]["grad_sq"]) - R.sumsq64(keep)) <= R.bound(4097, R.sumsq64(keep))
    assert float(rows0[0]["grad_absmax"]) == float(np.abs(keep).max())
    # the other entries are unaffected, bit for bit
    assert rows0[1:].tobytes() == clean[0][1:].tobytes() and rows1[2:].tobytes() == clean[1][2:].tobytes()
    assert rows1[0].tobytes()[4:12] == clean[1][0].tobytes()[4:12]      # entry 0's weight_sq / update_sq


def test_clip_is_the_optimizers():
    p0, g, p1 = _data(MIXED_TOTAL, seed=11)
    gsq, max_norm, scale = 16.0, 1.0, 0.5
    clip = R.clip_factor(gsq, max_norm, scale)
    assert clip != np.float32(1.0) and clip != np.float32(scale)
    rows0, rows1, prev0, _ = _run(MIXED, p0, g, p1, 0, gnorm_sq=gsq, max_norm=max_norm, grad_scale=scale)
    _check(MIXED, rows0, rows1, prev0, p0, g, p1, 0, clip)
    # no norm and grad_scale 1: clip is exactly 1 whatever max_norm says
    rows0b, _, _, _ = _run(MIXED, p0, g, p1, 0, gnorm_sq=None, max_norm=1.0, grad_scale=1.0)
    plain, _, _, _ = _run(MIXED, p0, g, p1, 0)
    assert rows0b.tobytes() == plain.tobytes()
    assert float(plain[2]["grad_absmax"]) == float(np.abs(g[4160:4160 + 16 * 3072]).max())
    # grad_scale alone scales the gradient
    rows0c, _, _, _ = _run(MIXED, p0, g, p1, 0, grad_scale=0.25)
    assert float(rows0c[2]["grad_absmax"]) == 0.25 * float(plain[2]["grad_absmax"])


def test_skipped_entries_give_zero_rows_and_touch_nothing():
    entries = [(64, 255), (0, 0), (-64, 17), (512, -3), (1024, 65)]
    total = 1024 + 65
    p0, g, p1 = _data(total, seed=31)
    for fill in (0xA5, 0xFF):
        rows0, rows1, prev0, _ = _run(entries, p0, g, p1, out_fill=fill)
        for i in (1, 2, 3):
            assert rows0[i].tobytes() == bytes(32) and rows1[i].tobytes() == bytes(32), i
        _check(entries, rows0, rows1, prev0, p0, g, p1, 0)


def test_more_entries_than_workgroups_are_walked_by_stride():
    n = 4096 + 37                                     # the grid cap of the launch is 4096 workgroups
    entries = [(64 * i, 1 + i % 64) for i in range(n)]
    total = 64 * n
    p0, g, p1 = _data(total, seed=41)
    rows0, rows1, _, _ = _run(entries, p0, g, p1)
    for i in (0, 1, 4095, 4096, n - 1):
        off, k = entries[i]
        assert float(rows0[i]["grad_sq"]) == R.phase0(g, off, k, np.float32(1.0), ordered=True)["grad_sq"]
        assert float(rows1[i]["update_sq"]) == R.phase1(p1, p0, off, k, ordered=True)["update_sq"]
    want = np.array([float(R.ordered_sumsq(p1[off:off + k])) for off, k in entries], np.float32)
    assert np.array_equal(rows1["weight_sq"], want)


# ---------------------------------------------------------------- the train steps
def _qwen_model(seed=2):
    from common import TINY
    from parity_util import build_pair
    return build_pair(dict(TINY), device=DEV, targets=TARGETS, seed=seed)[1]


def _flux_model():
    from common import FLUX_TINY
    from qflux_amd.models import FluxTransformer2DModel
    from qflux_amd.modules import LoraConfig
    cfg = dict(FLUX_TINY, joint_attention_dim=64, guidance_embeds=True)
    with torch.device(DEV):
        m = FluxTransformer2DModel(**cfg)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_((torch.randn(p.shape, generator=g) * (0.5 / p.shape[-1] ** 0.5 if p.ndim == 2 else 0.05) +
                     (1.0 if "norm_" in n and p.ndim == 1 else 0.0)).to(p.dtype))
    m.add_adapter(LoraConfig(r=4, lora_alpha=8), "a", generator=g)
    return m


def _flux_batch():
    from oracle import flux_dit as FO
    g = torch.Generator().manual_seed(4)
    ctl = FO.prepare_latent_image_ids(4, 6)
    ctl[:, 0] = 1
    emb = dict(image_latents=torch.randn(2, 24, 64, generator=g).half(), control_latents=torch.randn(2, 24, 64, generator=g).half(),
               control_ids=ctl, text_ids=torch.zeros(7, 3), latent_hw=(4, 6),
               pooled_prompt_embeds=torch.randn(2, 16, generator=g).half(), prompt_embeds=torch.randn(2, 7, 64, generator=g).half())
    return emb, torch.randn(2, 24, 64, generator=g), torch.tensor([0.3, 0.8])


def _three_steps(step, batch, check):
    """Three optimisation steps, written out as train_step writes them so that the buffers can be copied in between."""
    from qflux_amd import ops
    from qflux_amd.lora_io import get_lora_state_dict
    st = step.dit.lora_store
    for it in range(3):
        step.forward_backward(*batch)
        g, p0 = st.gflat.detach().cpu().numpy().copy(), st.pflat.detach().cpu().numpy().copy()
        scale = step.allreduce_grads()
        step.optimizer_step(grad_scale=scale)
        p1 = st.pflat.detach().cpu().numpy().copy()
        if check:
            stats, tel = step.last_adapter_stats, step._adapter_stats
            lay = tel.layout
            assert tel.collected == it + 1 and list(stats) == lay.names and set(stats) == set(get_lora_state_dict(step.dit))
            rows = ops.stats_rows(tel.out, lay.n_entries)
            clip = R.clip_factor(float(step._gnorm.item()), step.max_grad_norm, scale)
            assert np.array_equal(tel.prev.cpu().numpy().view(np.uint32), p0.view(np.uint32))      # (the padding is zero in both)
            for (off, k), name, r in zip(lay.entries, lay.names, rows):
                e0, e1 = R.phase0(g, off, k, clip), R.phase1(p1, p0, off, k)
                assert abs(float(r["grad_sq"]) - e0["grad_sq"]) <= R.bound(k, e0["grad_sq"]), name
                assert abs(float(r["weight_sq"]) - e1["weight_sq"]) <= R.bound(k, e1["weight_sq"]), name
                assert abs(float(r["update_sq"]) - e1["update_sq"]) <= R.bound(k, e1["update_sq"], update=True), name
                assert float(r["grad_absmax"]) == e0["grad_absmax"] and int(r["grad_nonfinite"]) == 0 == int(r["weight_nonfinite"])
                s = stats[name]
                assert s["grad_norm"] == float(r["grad_sq"]) ** 0.5 and s["weight_norm"] == float(r["weight_sq"]) ** 0.5
                assert s["update_norm"] == float(r["update_sq"]) ** 0.5
                assert s["update_ratio"] == (s["update_norm"] / s["weight_norm"] if s["weight_norm"] > 0 else 0.0)
            # something was measured: gradients flow and the step moved the weights
            assert sum(float(r["grad_sq"]) for r in rows) > 0 and sum(float(r["update_sq"]) for r in rows) > 0
            summ = step.adapter_stats_summary()
            assert summ["first_nonfinite_grad"] is None and summ["update_ratio_max_A"] >= summ["update_ratio_median_A"] >= 0
            total = float(np.sum(R._finite_or_zero(R.clipped(g, clip).astype(np.float64)) ** 2)) ** 0.5
            assert abs(summ["grad_norm"] - total) <= 1e-5 * total      # the padding's gradient is zero: the sum over tensors is the whole
        step.zero_grad()
    return st.pflat.detach().cpu().clone()


@pytest.mark.parametrize("optimizer", ("adamw", "prodigy"))
def test_qwen_train_step_reports_the_restatement_and_trains_the_same_bits(optimizer):
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    batch = tiny_embeddings(seed=5)
    kw = dict(lr=1.0 if optimizer == "prodigy" else 1e-3, optimizer=optimizer)
    on = QwenLoraTrainStep(_qwen_model(), adapter_stats_every=1, **kw)
    assert on.last_adapter_stats is None and on.adapter_stats_summary() is None
    trained_on = _three_steps(on, batch, check=True)
    off = QwenLoraTrainStep(_qwen_model(), **kw)
    trained_off = _three_steps(off, batch, check=False)
    assert off.last_adapter_stats is None and off._adapter_stats is None
    assert torch.equal(trained_on, trained_off)


def test_flux_train_step_reports_the_restatement_and_trains_the_same_bits():
    from qflux_amd.trainer import FluxKontextTrainStep
    batch = _flux_batch()
    trained_on = _three_steps(FluxKontextTrainStep(_flux_model(), lr=1e-3, optimizer="adamw", adapter_stats_every=1), batch, check=True)
    trained_off = _three_steps(FluxKontextTrainStep(_flux_model(), lr=1e-3, optimizer="adamw"), batch, check=False)
    assert torch.equal(trained_on, trained_off)


def test_every_n_collects_on_multiples_of_n_only():
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    e, nz, u = tiny_embeddings(seed=5)
    step = QwenLoraTrainStep(_qwen_model(), lr=1e-3, adapter_stats_every=2)
    step.train_step(e, noise=nz, u=u)
    assert step.last_adapter_stats is None
    step.train_step(e, noise=nz, u=u)
    first = step.last_adapter_stats
    assert first is not None and step._adapter_stats.collected == 1
    step.train_step(e, noise=nz, u=u)
    assert step.last_adapter_stats is first and step._adapter_stats.collected == 1      # step 3: not collected, nothing re-read
    with pytest.raises(NotImplementedError, match="adapter_stats_every"):
        step.capture_graph(e)


def test_stock_loop_object_goes_around_the_optimizer_class():
    from qflux_amd import optim as O
    from qflux_amd.telemetry import AdapterStats
    m = _qwen_model()
    st = m.lora_store
    opt = O.AdamW([p for _, p in st.params()], lr=1e-2)
    stats = AdapterStats.from_optimizer(opt)
    assert stats.read() is None
    gen = torch.Generator().manual_seed(9)
    st.gflat.copy_(torch.randn(st.gflat.shape, generator=gen).to(DEV) * 0.01)
    g, p0 = st.gflat.cpu().numpy().copy(), st.pflat.detach().cpu().numpy().copy()
    stats.before_step()
    opt.step()
    stats.after_step()
    p1 = st.pflat.detach().cpu().numpy().copy()
    got = stats.read()
    for (off, k), name in zip(stats.layout.entries, stats.names):
        e0, e1 = R.phase0(g, off, k, np.float32(1.0)), R.phase1(p1, p0, off, k)
        assert abs(got[name]["grad_norm"] ** 2 - e0["grad_sq"]) <= R.bound(k, e0["grad_sq"]) + 1e-15 * e0["grad_sq"]
        assert abs(got[name]["update_norm"] ** 2 - e1["update_sq"]) <= R.bound(k, e1["update_sq"], update=True) + 1e-15 * e1["update_sq"]
        assert got[name]["update_norm"] > 0
    assert stats.summary()["update_ratio_max_A"] > 0
