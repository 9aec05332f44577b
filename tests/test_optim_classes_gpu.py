"""GPU: the torch.optim classes of qflux_amd.optim -- bit identity with QwenLoraTrainStep's optimizer_step per family (same state
object, same kernel, same arguments), checkpoint exchange between the two, and the reference's loop body under a real
accelerate.Accelerator (the pattern of test_accelerate_gpu.py) with qflux_amd.optim.AdamW in torch.optim.AdamW's place."""
import pytest
import torch
import torch.nn as nn

from parity_util import QWEN_BARS, build_pair, tiny_embeddings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# attention adapters (1024 elements: fp32 moments under the 8-bit family) and the feed-forward down projection's LoRA-A (4096: 8-bit)
TARGETS = ("to_k", "to_q", "to_v", "to_out.0", "img_mlp.net.2")
_TWINS = {}


def _twins():
    """Two tiny models with equal weights, built once; every test starts from the same adapter values and a zero gradient."""
    from common import TINY
    if not _TWINS:
        _TWINS["models"] = [build_pair(dict(TINY), device=DEV, targets=TARGETS, seed=2)[1] for _ in range(2)]
        _TWINS["start"] = _TWINS["models"][0].lora_store.pflat.detach().clone()
    for m in _TWINS["models"]:
        st = m.lora_store
        with torch.no_grad():
            st.pflat.copy_(_TWINS["start"])
            st.gflat.zero_()
    a, b = _TWINS["models"]
    assert torch.equal(a.lora_store.pflat, b.lora_store.pflat) and bool(a.lora_store.pflat.ne(0).any())
    return a, b


def _get_lora_layers(model):
    """qflux.utils.lora_utils.get_lora_layers (:25-38) restated: every submodule whose dotted name contains 'lora'."""
    out = {}

    def rec(name, module):
        if "lora" in name:
            out[name] = module
        for sub, child in module.named_children():
            rec(f"{name}.{sub}", child)
    for name, module in model.named_children():
        rec(name, module)
    return out


class _AttnProcsLayers(nn.Module):
    """Stand-in for diffusers.loaders.AttnProcsLayers (third party): a ModuleList over the dict's values."""

    def __init__(self, state_dict):
        super().__init__()
        self.layers = nn.ModuleList(state_dict.values())


def _set_grad(models, g):
    """The same flat gradient into every model, through the `lora_store` property (it re-attaches the views a set-to-none
    zero_grad dropped BEFORE the gradient is written, as the forward does in the real loop)."""
    for m in models:
        m.lora_store.gflat.copy_(g)


def _lora_params(m):
    return [p for n, p in m.named_parameters() if "lora_" in n]


def _grad(st, it):
    g = torch.Generator().manual_seed(50 + it)
    return (torch.randn(st.gflat.shape, generator=g) * 1e-2).to(DEV)


def _same_state(opt, step):
    a, b = opt._opt_state.buffers(), step.opt_state.buffers()
    assert [n for n, _ in a] == [n for n, _ in b] and a
    for (n, x), (_, y) in zip(a, b):
        assert torch.equal(x, y), n


FAMILIES = [("AdamW", "adamw", dict(lr=3e-3, weight_decay=0.01), None),
            ("Prodigy", "prodigy", dict(lr=1.0, weight_decay=0.01, use_bias_correction=True), {"use_bias_correction": True}),
            ("Adam8bit", "adam8bit_blockwise", dict(lr=3e-3, blocksize=256), {"blocksize": 256}),
            ("SGD", "sgd", dict(lr=0.1, momentum=0.9, weight_decay=1e-4), {"momentum": 0.9})]


@pytest.mark.parametrize("name,family,kw,args", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_class_steps_bit_identically_to_the_train_step_and_exchanges_checkpoints(name, family, kw, args):
    from qflux_amd import optim as O
    from qflux_amd.trainer import QwenLoraTrainStep
    a, b = _twins()
    sa, sb = a.lora_store, b.lora_store
    opt = getattr(O, name)(_lora_params(a), **kw)
    step = QwenLoraTrainStep(b, lr=kw["lr"], weight_decay=kw.get("weight_decay"), max_grad_norm=0, optimizer=family, optimizer_args=args)
    for it in range(3):
        g = _grad(sa, it)
        _set_grad((a, b), g)
        opt.step()
        step.optimizer_step()
        opt.zero_grad()                       # set_to_none: the next step() re-attaches the flat views
        step.zero_grad()
    assert not torch.equal(sa.pflat, _TWINS["start"])
    assert torch.equal(sa.pflat, sb.pflat)
    _same_state(opt, step)
    # one writes the file, the other resumes it: the class's into a fresh train step, the train step's into a fresh class
    a2 = sa.pflat.detach().clone()
    sd_cls, sd_step = opt.state_dict(), step.state_dict()
    assert sd_cls["global_step"] == sd_step["global_step"] == 3 and list(sd_cls["state"]) == list(sd_step["state"])
    opt2 = getattr(O, name)(_lora_params(a), **dict(kw, lr=0.5))
    opt2.load_state_dict(sd_step)
    step2 = QwenLoraTrainStep(b, lr=0.5, max_grad_norm=0, optimizer=family, optimizer_args=args)
    step2.load_state_dict(sd_cls)
    assert opt2.param_groups[0]["lr"] == kw["lr"] and step2.lr == kw["lr"] and step2.global_step == 3
    g = _grad(sa, 3)
    _set_grad((a, b), g)
    opt2.step()
    step2.optimizer_step()
    assert not torch.equal(sa.pflat, a2) and torch.equal(sa.pflat, sb.pflat)
    _same_state(opt2, step2)
    # and the resumed pair equals a run that never stopped
    sa.pflat.copy_(a2)
    _set_grad((a,), g)
    opt.step()
    assert torch.equal(sa.pflat, sb.pflat)


def _loop(accelerator, model, optimizer, scheduler, helper, pool, k, max_norm, micro_steps, seed=17):
    """The reference's loop body (base_trainer.py:518-533), as in test_accelerate_gpu.py."""
    g = torch.Generator().manual_seed(seed)
    losses = []
    for it in range(micro_steps):
        emb = pool[it % len(pool)]
        noise = torch.randn(emb["image_latents"].shape, generator=g)
        u = torch.rand(emb["image_latents"].shape[0], generator=g)
        with accelerator.accumulate(model):
            loss = helper.compute_loss(emb, noise=noise, u=u)
            accelerator.backward(loss)
            if accelerator.sync_gradients:
                accelerator.clip_grad_norm_(model.parameters(), max_norm)
            optimizer.step()
            scheduler.step()
            optimizer.zero_grad()
        losses.append(loss.item())
    return losses


def _prepared(accelerator, model, optimizer, steps):
    from qflux_amd.trainer import QwenLoraTrainStep, get_scheduler
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, get_scheduler("cosine", 0, steps))
    layers = _AttnProcsLayers(_get_lora_layers(model))
    layers, optimizer, scheduler = accelerator.prepare(layers, optimizer, scheduler)          # base_trainer.py:385-387
    model = model.to(accelerator.device)
    assert model.lora_store.is_consistent(DEV)
    return optimizer, scheduler, QwenLoraTrainStep(model)


def test_reference_loop_under_accelerate_with_the_fused_adamw_class():
    accelerate = pytest.importorskip("accelerate")
    from qflux_amd import optim as O
    k, steps, lr, wd, max_norm = 2, 3, 3e-3, 0.01, 1.0
    a, b = _twins()
    start = _TWINS["start"]
    accelerator = accelerate.Accelerator(gradient_accumulation_steps=k, mixed_precision="no")
    pool = [tiny_embeddings(seed=300 + i)[0] for i in range(k * steps)]
    fused = O.AdamW(_lora_params(a), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    stock = torch.optim.AdamW(_lora_params(b), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    runs = []
    for model, optimizer in ((a, fused), (b, stock)):
        optimizer, scheduler, helper = _prepared(accelerator, model, optimizer, steps)
        losses = _loop(accelerator, model, optimizer, scheduler, helper, pool, k, max_norm, k * steps)
        runs.append((optimizer, scheduler, helper, losses))
        assert model.lora_store.is_consistent(DEV)
    assert fused._step_count_fused == steps                 # one fused step per k micro-steps
    la, lb = runs[0][3], runs[1][3]
    rel = [abs(x - y) / abs(y) for x, y in zip(la, lb)]
    du_a, du_b = (a.lora_store.pflat - start).flatten(), (b.lora_store.pflat - start).flatten()
    cos = float(torch.dot(du_a, du_b) / (du_a.norm() * du_b.norm() + 1e-30))
    print("fused vs stock AdamW under accelerate: loss rel", rel, "update cosine", cos)
    # the bars of test_accelerate_gpu.py between the HIP model and its torch-trained oracle
    assert max(rel) < QWEN_BARS[0] * 4, rel
    assert cos > 0.9 and float(du_a.abs().max()) > 0, cos
    # the scheduler's lr reaches the kernel: the cosine schedule has arrived at 0, and a step taken there changes nothing
    optimizer, scheduler, helper, _ = runs[0]
    assert fused.param_groups[0]["lr"] == 0.0
    before = a.lora_store.pflat.detach().clone()
    _loop(accelerator, a, optimizer, scheduler, helper, pool, k, max_norm, k, seed=18)
    assert fused._step_count_fused == steps + 1 and torch.equal(a.lora_store.pflat, before)


@pytest.mark.parametrize("name,kw", [("Adam8bit", dict(lr=3e-3)), ("SGD", dict(lr=0.1, momentum=0.9, weight_decay=1e-4))])
def test_reference_loop_smoke_with_the_8bit_and_sgd_classes(name, kw):
    accelerate = pytest.importorskip("accelerate")
    from qflux_amd import optim as O
    k, steps = 2, 2
    a, _ = _twins()
    accelerator = accelerate.Accelerator(gradient_accumulation_steps=k, mixed_precision="no")
    pool = [tiny_embeddings(seed=300 + i)[0] for i in range(k * steps)]
    raw = getattr(O, name)(_lora_params(a), **kw)
    optimizer, scheduler, helper = _prepared(accelerator, a, raw, steps + 1)
    losses = _loop(accelerator, a, optimizer, scheduler, helper, pool, k, 1.0, k * steps)
    st = a.lora_store
    assert all(torch.isfinite(torch.tensor(losses))) and torch.isfinite(st.pflat).all() and not torch.equal(st.pflat, _TWINS["start"])
    # what accelerator.save_state writes (optimizer.state_dict()) resumes into a fresh optimizer with the same buffers
    sd = optimizer.state_dict()
    assert sd["global_step"] == steps and len(sd["state"]) == len(st.entries)
    fresh = getattr(O, name)(_lora_params(a), **kw)
    fresh.load_state_dict(sd)
    assert fresh._step_count_fused == steps
    for (n, x), (_, y) in zip(raw._opt_state.buffers(), fresh._opt_state.buffers()):
        assert torch.equal(x, y), n
    back = fresh.state_dict()
    for i, e in sd["state"].items():
        for key, v in e.items():
            assert torch.equal(back["state"][i][key], v) if torch.is_tensor(v) else back["state"][i][key] == v
