"""The per-timestep modulation table of the frozen conditioning head: qfx_mod_table_fetch, qfx_mod_gemv_unless, and the table
path of the tiny Qwen model against the computed path (QFX_MOD_TABLE=0) -- bit for bit everywhere, a table row IS what the step
computes for that timestep.

Shapes of the whole-step cases: image grids of 4 x 4 tokens, so that the criterion's loss is the sum of at most two per-block fp32
atomics (order-independent) and "bit-identical" can be asked of the loss too."""
import pytest
import torch

from parity_util import ROOT  # noqa: F401  (puts the repository root and the package on sys.path)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SENT = -7.0          # sentinel fill of destinations that must stay untouched
SHAPES = ((1, 4, 4), (1, 4, 4))
OFF_T = 123.45       # timesteps / 1000 = 0.12345: between two keys of the training list


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == BF else torch.int32)


# ---------------------------------------------------------------------------------------------- fetch kernel
def _fetch_case(n, B, N, nmat=4, N_out=None, seed=0):
    g = torch.Generator().manual_seed(seed + 13 * n + B + N)
    N_out = N // 2 + 1 if N_out is None else N_out          # 49 / 51: a second odd length
    keys = (torch.arange(n, dtype=torch.float32) + 1.0) / 1000.0
    tbl_mods = torch.randn(n, nmat, N, generator=g).to(BF).to(DEV)
    tbl_out = torch.randn(n, N_out, generator=g).to(BF).to(DEV)
    return keys, tbl_mods, tbl_out


def _run_fetch(t, keys, tbl_mods, tbl_out):
    from qflux_amd import ops
    B = t.numel()
    n, nmat, N = tbl_mods.shape
    mods = torch.full((nmat, B, N), SENT, dtype=BF, device=DEV)
    mod_out = torch.full((B, tbl_out.shape[1]), SENT, dtype=BF, device=DEV)
    hit = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    ops.mod_table_fetch(t.to(DEV), keys.to(DEV), tbl_mods, tbl_out, mods, mod_out, hit)
    torch.cuda.synchronize()
    return mods, mod_out, int(hit.item())


@pytest.mark.parametrize("N", [96, 100])
@pytest.mark.parametrize("B", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [5, 1000])
def test_fetch_hits_copy_rows_bit_exactly_and_misses_touch_nothing(n, B, N):
    keys, tbl_mods, tbl_out = _fetch_case(n, B, N)
    # hits: the first key, the last key, an interior key, in every position of the batch (repeats allowed)
    pool = [0, n - 1, n // 2]
    idx = torch.tensor([pool[(b + B) % 3] for b in range(B)])
    mods, mod_out, hit = _run_fetch(keys[idx], keys, tbl_mods, tbl_out)
    assert hit == 1
    assert torch.equal(_bits(mods), _bits(tbl_mods[idx.to(DEV)].transpose(0, 1)))
    assert torch.equal(_bits(mod_out), _bits(tbl_out[idx.to(DEV)]))
    for b in range(B):      # each single position alone
        one = keys[idx].clone()
        one[b] = keys[pool[b % 3]]
        assert _run_fetch(one, keys, tbl_mods, tbl_out)[2] == 1
    # one sample of the batch off the table (last position, and first): flag 0, both destinations keep their fill
    for pos in {0, B - 1}:
        t = keys[idx].clone()
        t[pos] = 0.12345
        mods, mod_out, hit = _run_fetch(t, keys, tbl_mods, tbl_out)
        assert hit == 0
        assert bool((mods == SENT).all()) and bool((mod_out == SENT).all())


@pytest.mark.parametrize("B", [1, 3])
def test_fetch_matches_words_not_values(B):
    """NaN never hits (not even a NaN key with the same bits); -0.0 is not the key +0.0."""
    n, N = 5, 100
    keys, tbl_mods, tbl_out = _fetch_case(n, B, N)
    keys = keys.clone()
    keys[1] = 0.0
    keys[3] = float("nan")
    base = keys[torch.tensor([0, 2, 4][:B])]
    for bad, want in ((float("nan"), 0), (-0.0, 0), (0.0, 1)):
        t = base.clone()
        t[B - 1] = bad
        mods, mod_out, hit = _run_fetch(t, keys, tbl_mods, tbl_out)
        assert hit == want, (bad, hit)
        if not want:
            assert bool((mods == SENT).all()) and bool((mod_out == SENT).all())
    t = base.clone()
    t[0] = keys[3]                      # the very word of the NaN key
    assert _run_fetch(t, keys, tbl_mods, tbl_out)[2] == 0


# ---------------------------------------------------------------------------------------------- guarded GEMV
@pytest.mark.parametrize("B", [1, 3])
def test_guarded_gemv_is_the_plain_one_or_nothing(B):
    from qflux_amd import ops
    K, N, nmat = 64, 100, 3
    g = torch.Generator().manual_seed(5 + B)
    temb = torch.randn(B, K, generator=g).to(BF).to(DEV)
    Ws = [(torch.randn(N, K, generator=g) * 0.1).to(BF).to(DEV) for _ in range(nmat)]
    bs = [torch.randn(N, generator=g).to(BF).to(DEV) for _ in range(nmat)]
    for silu in (True, False):
        want = ops.mod_gemv(temb, Ws, bs, apply_silu=silu)
        for flag in (None, 0, 1):
            out = torch.full((nmat, B, N), SENT, dtype=BF, device=DEV)
            skip = None if flag is None else torch.tensor([flag], dtype=torch.int32, device=DEV)
            ops.mod_gemv_unless(temb, Ws, bs, out, skip, apply_silu=silu)
            torch.cuda.synchronize()
            if flag == 1:
                assert bool((out == SENT).all())
            else:
                assert torch.equal(_bits(out), _bits(want)), (silu, flag)


# ---------------------------------------------------------------------------------------------- the tiny model
def _tiny(targets=("to_k", "to_q", "to_v", "to_out.0")):
    from common import TINY
    from parity_util import build_pair
    return build_pair(dict(TINY), device=DEV, targets=targets)[1]


def _emb(B, seed):
    from parity_util import tiny_embeddings
    e, noise, _ = tiny_embeddings(B=B, shapes=SHAPES, seed=seed)
    return e, noise


def _pin_timesteps(step, ts):
    """The step's sampling hook: these timesteps (scheduler units, 1..1000) instead of a draw from the training list."""
    ts = torch.tensor(ts, dtype=torch.float32)
    step.sample_timesteps = lambda batch_size, u=None: (ts, ts / 1000)


def test_table_rows_equal_what_the_step_computes_for_every_default_key(monkeypatch):
    """All 1000 default keys, in batches of 8, against the head of the lever-off plan (its first five launches)."""
    from qflux_amd import _lib as L
    from qflux_amd.trainer import QwenLoraTrainStep
    from qflux_amd.trainer.qwen_step import flowmatch_tables
    m = _tiny()
    step = QwenLoraTrainStep(m)
    tb = m.modulation_table
    keys = flowmatch_tables()[0] / 1000
    assert tb is not None and torch.equal(tb["keys"].cpu().view(torch.int32), keys.view(torch.int32)) and keys.numel() == 1000
    cfg = m.config
    assert tb["mods"].numel() * 2 + tb["out"].numel() * 2 == m.modulation_table_bytes(1000, cfg.num_layers, m.inner_dim)
    mods_t, out_t = tb["mods"].clone(), tb["out"].clone()
    monkeypatch.setenv("QFX_MOD_TABLE", "0")
    m.drop_modulation_table()
    e, _ = _emb(8, 3)
    plan = m.get_plan(8, 2 * 16, 5, e["img_shapes"], None)
    assert m.modulation_table is None and [c[0] for c in plan.fwd.calls[:5]] == [L.lib.qfx_timestep_embed] + [L.lib.qfx_mod_gemv] * 4
    for i0 in range(0, 1000, 8):
        plan.A["t"].copy_(keys[i0:i0 + 8])
        plan.fwd.run(0, 5)
        assert torch.equal(_bits(plan.A["mods"].transpose(0, 1)), _bits(mods_t[i0:i0 + 8])), i0
        assert torch.equal(_bits(plan.A["mod_out"][0]), _bits(out_t[i0:i0 + 8])), i0
    del step


def _whole_steps(table_on, monkeypatch):
    """prediction, loss, flat gradient, post-AdamW parameters (and the hit cell) of: an on-table step, an off-table step, B = 2 with
    one of each, and an on-table step after load_state_dict changed an img_mod weight."""
    from qflux_amd.trainer import QwenLoraTrainStep
    monkeypatch.setenv("QFX_MOD_TABLE", "1" if table_on else "0")
    m = _tiny()
    step = QwenLoraTrainStep(m, lr=1e-2)
    assert (m.modulation_table is not None) == table_on
    res = []

    def one(B, ts, seed):
        e, noise = _emb(B, seed)
        _pin_timesteps(step, ts)
        loss = step.forward_backward(e, noise=noise)
        plan = [p for p in m._plans.values() if p.B == B][0]
        hit = int(plan.A["mod_hit"].item()) if table_on else None
        assert ("mod_hit" in plan.A) == table_on
        r = [plan.A["out"].clone(), loss.clone(), m.lora_store.gflat.clone()]
        step.optimizer_step()
        step.zero_grad()
        res.append((hit, r + [m.lora_store.pflat.clone()]))

    one(1, [712.0], 11)
    one(1, [OFF_T], 12)
    one(2, [162.0, OFF_T], 13)
    one(2, [1000.0, 1.0], 14)
    sd = m.state_dict()
    k = next(n for n in sd if n.endswith("transformer_blocks.1.img_mod.1.weight"))
    sd[k] = (sd[k].float() * 1.5 + 0.01).to(sd[k].dtype)
    m.load_state_dict(sd)
    assert m.modulation_table is None          # dropped with the prepared weights ...
    one(1, [712.0], 11)
    assert (m.modulation_table is not None) == table_on      # ... and rebuilt by the next training step
    return res


def test_whole_step_is_bit_identical_with_and_without_the_table(monkeypatch):
    on = _whole_steps(True, monkeypatch)
    off = _whole_steps(False, monkeypatch)
    assert [h for h, _ in on] == [1, 0, 0, 1, 1]
    for i, ((_, a), (_, b)) in enumerate(zip(on, off)):
        for name, x, y in zip(("prediction", "loss", "gradient", "parameters"), a, b):
            assert torch.equal(_bits(x), _bits(y)), (i, name)
    # the changed img_mod weight reached the table: same inputs as case 0, another prediction
    assert not torch.equal(on[0][1][0], on[4][1][0])


def test_adapters_on_the_conditioning_head_keep_the_table_out():
    from qflux_amd import _lib as L
    from qflux_amd.trainer import QwenLoraTrainStep
    m = _tiny(targets="all-linear")
    step = QwenLoraTrainStep(m)
    assert m.cond_lora and m.modulation_table is None
    e, noise = _emb(1, 11)
    step.forward_backward(e, noise=noise)
    plan = list(m._plans.values())[0]
    assert not any(c[0] is L.lib.qfx_mod_table_fetch or c[0] is L.lib.qfx_mod_gemv_unless for c in plan.fwd.calls)
    assert "mod_hit" not in plan.A


def test_inference_uses_a_table_but_never_builds_one():
    m = _tiny()
    e, _ = _emb(1, 11)
    x = torch.randn(1, 32, 64, device=DEV).to(BF)
    pe = e["prompt_embeds"].to(BF).to(DEV)
    t = torch.tensor([0.712], device=DEV)
    with torch.no_grad():
        m(hidden_states=x, encoder_hidden_states=pe, timestep=t, img_shapes=e["img_shapes"], txt_seq_lens=[5])
    assert m.modulation_table is None
    m.eval()
    m(hidden_states=x, encoder_hidden_states=pe, timestep=t, img_shapes=e["img_shapes"], txt_seq_lens=[5])
    assert m.modulation_table is None
    m.train()
    a = m(hidden_states=x, encoder_hidden_states=pe, timestep=t, img_shapes=e["img_shapes"], txt_seq_lens=[5]).sample
    assert m.modulation_table is not None      # the drop-in module's first training-mode forward
    plan = list(m._plans.values())[0]
    assert int(plan.A["mod_hit"].item()) == 1
    with torch.no_grad():                      # an off-table sampling timestep simply misses
        m(hidden_states=x, encoder_hidden_states=pe, timestep=torch.tensor([0.7125], device=DEV), img_shapes=e["img_shapes"], txt_seq_lens=[5])
        assert int(plan.A["mod_hit"].item()) == 0
        b = m(hidden_states=x, encoder_hidden_states=pe, timestep=t, img_shapes=e["img_shapes"], txt_seq_lens=[5]).sample
    assert int(plan.A["mod_hit"].item()) == 1 and torch.equal(a, b)


def test_graph_replay_hits_misses_and_hits_like_the_eager_replay():
    """One captured graph, replayed with an on-table, an off-table and again an on-table timestep: the hit / miss decision is taken
    on the device inside the graph, each replay equals the eager step."""
    from qflux_amd.trainer import QwenLoraTrainStep
    a, b = _tiny(), _tiny()
    sa, sb = QwenLoraTrainStep(a, lr=1e-2), QwenLoraTrainStep(b, lr=1e-2)
    e0, _ = _emb(1, 11)
    gstep = sb.capture_graph(e0)
    plan_b = list(b._plans.values())[0]
    for seed, ts, hit in ((11, [712.0], 1), (12, [OFF_T], 0), (13, [33.0], 1)):
        e, noise = _emb(1, seed)
        _pin_timesteps(sa, ts)
        _pin_timesteps(sb, ts)
        la = sa.train_step(e, noise=noise)
        lb = gstep(e, noise=noise)
        assert int(plan_b.A["mod_hit"].item()) == hit
        assert torch.equal(_bits(la), _bits(lb)), (seed, la.item(), lb.item())
        assert torch.equal(_bits(a.lora_store.pflat), _bits(b.lora_store.pflat)), seed
