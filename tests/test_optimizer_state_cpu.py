"""CPU: the fused trainer step's optimizer state in and out of optimizer.bin (no device, no kernel) -- the prodigyopt and
torch.optim.AdamW layouts round trip key by key, and state_dict() before the first step, for every optimizer family."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = ["to_q", "to_k", "to_v", "to_out.0", "img_mlp.net.2", "txt_mod.1"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from qflux_amd import _lib
    return _lib


def _tiny_model():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from common import TINY
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.modules import LoraConfig
    q = QwenImageTransformer2DModel(**TINY)
    q.add_adapter(LoraConfig(r=4, lora_alpha=8, target_modules=TARGETS), "lora_edit")
    return q


def _assert_same_state(out, ref):
    assert list(out) == list(ref)
    for i, e in ref.items():
        o = out[i]
        assert list(o) == list(e), i
        for k, v in e.items():
            if torch.is_tensor(v):
                assert o[k].dtype == v.dtype and o[k].shape == v.shape and torch.equal(o[k], v), (i, k)
            else:
                assert type(o[k]) is type(v) and o[k] == v, (i, k)


def test_prodigy_state_dict_round_trip(lib):
    """A prodigyopt-layout file (the oracle after 3 steps, no top-level global_step as the package writes it) loads and saves back
    unchanged; a p0 stored as a 0-dim zero (prodigyopt's form for an all-zero parameter) comes back as zeros of the parameter's size."""
    from oracle.prodigy import Prodigy
    from qflux_amd.trainer import QwenLoraTrainStep
    q = _tiny_model()
    torch.manual_seed(6)
    ps = [torch.randn(p.shape) * 0.1 for _, p in q.lora_store.params()]
    opt = Prodigy(ps, lr=1.0, weight_decay=0.01, use_bias_correction=True, d0=1e-5)
    for _ in range(3):
        opt.step([torch.randn(p.shape) for p in ps])
    sd = {"state": {i: dict(s) for i, s in enumerate(opt.state)}, "param_groups": [dict(opt.group, params=list(range(len(ps))))]}
    step = QwenLoraTrainStep(q, optimizer="prodigy")
    step.load_state_dict(sd)
    assert step.global_step == 3 and step.optimizer_args["d0"] == 1e-5 and step.optimizer_args["use_bias_correction"] is True
    out = step.state_dict()
    assert out["global_step"] == 3
    _assert_same_state(out["state"], sd["state"])
    g, gin = out["param_groups"][0], sd["param_groups"][0]
    assert set(g) == set(gin) and all(g[k] == gin[k] for k in gin) and type(g["k"]) is int and g["k"] == 3

    sd["state"][1]["p0"] = torch.tensor(0.0)
    step = QwenLoraTrainStep(q, optimizer="prodigy")
    step.load_state_dict(sd)
    p0 = step.state_dict()["state"][1]["p0"]
    assert p0.shape == (ps[1].numel(),) and p0.dtype == torch.float32 and not p0.any()


def test_adamw_state_dict_round_trip(lib):
    """torch.optim.AdamW's own state_dict after 2 steps loads and saves back unchanged (step as a float tensor)."""
    from qflux_amd.trainer import QwenLoraTrainStep
    q = _tiny_model()
    torch.manual_seed(7)
    ps = [torch.nn.Parameter(torch.randn(p.shape) * 0.1) for _, p in q.lora_store.params()]
    opt = torch.optim.AdamW(ps, lr=1e-3, betas=(0.9, 0.99), weight_decay=0.02)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn(p.shape)
        opt.step()
    sd = opt.state_dict()
    step = QwenLoraTrainStep(q)
    step.load_state_dict(sd)
    assert step.global_step == 2 and step.betas == (0.9, 0.99) and step.weight_decay == 0.02
    out = step.state_dict()
    _assert_same_state(out["state"], sd["state"])
    assert out["param_groups"][0] == {"lr": 1e-3, "betas": (0.9, 0.99), "eps": 1e-8, "weight_decay": 0.02, "amsgrad": False,
                                      "params": list(range(len(ps)))}


_D0 = dict(d=1e-6, d_max=1e-6, d_numerator=0.0, d_denom=0.0, d_hat=1e-6, k=0)
_PRODIGY_ARGS = dict(beta3=None, decouple=True, use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0,
                     growth_rate=float("inf"))


@pytest.mark.parametrize("optimizer,extra", [("adamw", {"weight_decay": 0.01, "amsgrad": False}),
                                             ("adam8bit", {"weight_decay": 0.0, "amsgrad": False}),
                                             ("prodigy", dict(weight_decay=0.0, **_PRODIGY_ARGS, **_D0)),
                                             ("adam8bit_blockwise", {"weight_decay": 0.0}),
                                             ("adamw8bit_blockwise", {"weight_decay": 0.01})])
def test_state_dict_before_the_first_step(lib, optimizer, extra):
    """No per-parameter state yet; the group holds the hyperparameters (Prodigy: its init_args and the d0 defaults), keys in order."""
    from qflux_amd.trainer import QwenLoraTrainStep
    q = _tiny_model()
    n = len(q.lora_store.entries)
    sd = QwenLoraTrainStep(q, optimizer=optimizer).state_dict()
    group = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, **extra, params=list(range(n)))
    assert sd == {"state": {}, "param_groups": [group], "global_step": 0}
    assert list(sd) == ["state", "param_groups", "global_step"] and list(sd["param_groups"][0]) == list(group)


_SGD_ARGS = dict(momentum=0.0, dampening=0.0, nesterov=False)
_ADAFACTOR_ARGS = dict(eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, scale_parameter=True, relative_step=True,
                       warmup_init=False)
_MUON_ARGS = dict(momentum=0.95, nesterov=True, ns_coefficients=(3.4445, -4.7750, 2.0315), eps=1e-7, ns_steps=5, adjust_lr_fn=None)
_SF_ARGS = dict(warmup_steps=0, r=0.0, weight_lr_power=2.0)
_BLOCK_ARGS = dict(min_8bit_size=4096, blocksize=256)
# optimizer= name -> (alias, family, state class, weight decay, optimizer_args) as resolve_family returned them before the families
# shared one table ("adamw" and its aliases have always carried Prodigy's defaults, which nothing reads)
_FAMILIES = {
    "adamw": (None, "adamw", "AdamWState", 0.01, _PRODIGY_ARGS),
    "adam": ("adam", "adamw", "AdamWState", 0.0, _PRODIGY_ARGS),
    "adam8bit": ("adam8bit", "adamw", "AdamWState", 0.0, _PRODIGY_ARGS),
    "prodigy": (None, "prodigy", "ProdigyState", 0.0, _PRODIGY_ARGS),
    "sgd": (None, "sgd", "SgdState", 0.0, _SGD_ARGS),
    "adafactor": (None, "adafactor", "AdafactorState", 0.0, _ADAFACTOR_ARGS),
    "muon": (None, "muon", "MuonState", 0.1, _MUON_ARGS),
    "adamw_schedulefree": (None, "adamw_schedulefree", "ScheduleFreeAdamWState", 0.0, _SF_ARGS),
    "adam8bit_blockwise": (None, "adam8bit_blockwise", "BlockwiseState", 0.0, _BLOCK_ARGS),
    "adamw8bit_blockwise": (None, "adamw8bit_blockwise", "BlockwiseState", 0.01, _BLOCK_ARGS),
    "lion": (None, "lion", "LionState", 0.0, {}),
    "lion8bit_blockwise": (None, "lion8bit_blockwise", "LionBlockwiseState", 0.0, _BLOCK_ARGS),
}


@pytest.mark.parametrize("optimizer", sorted(_FAMILIES))
def test_resolve_family_table(lib, optimizer):
    """Every accepted name resolves to what it always has; an unknown optimizer_args key, and any key for a family that takes none,
    is refused with the same exception."""
    from qflux_amd.trainer import optim_state as OS
    alias, family, cls, wd, args = OS.resolve_family(optimizer)
    want = _FAMILIES[optimizer]
    assert (alias, family, cls.__name__, wd, args) == want and list(args) == list(want[4])
    assert type(wd) is float and cls is getattr(OS, want[2])
    with pytest.raises(ValueError) as ei:
        OS.resolve_family(optimizer, None, {"bogus": 1})
    assert str(ei.value) == f"unsupported optimizer_args for {family}: ['bogus']"
    if family in ("adamw", "lion"):      # no optimizer_args at all, not even a name another family knows
        with pytest.raises(ValueError) as ei:
            OS.resolve_family(optimizer, None, {"d0": 1e-6})
        assert str(ei.value) == f"unsupported optimizer_args for {family}: ['d0']"


def test_resolve_family_unknown_name(lib):
    from qflux_amd.trainer import optim_state as OS
    with pytest.raises(ValueError) as ei:
        OS.resolve_family("adagrad")
    assert str(ei.value) == "unknown optimizer 'adagrad'"
    with pytest.raises(NotImplementedError, match="adam8bit with L2 weight decay 0.01"):
        OS.resolve_family("adam8bit", 0.01)


@pytest.mark.parametrize("name", ["BlockwiseState", "LionBlockwiseState"])
@pytest.mark.parametrize("blocksize", [256, 2048])
def test_blockwise_state_save_load_round_trip(lib, name, blocksize):
    """One 8-bit tensor (a short last block) and one fp32-moment tensor: every buffer comes back from save -> load bit for bit, the
    block size from the file."""
    import types
    from qflux_amd.trainer import optim_state as OS
    cls = getattr(OS, name)
    ps = [torch.zeros(3, blocksize + 1), torch.zeros(5)]
    entries, off = [], 0
    for i, p in enumerate(ps):
        entries.append((f"p{i}", p, off, p.numel()))
        off += (p.numel() + 3) // 4 * 4                                     # the flat buffer's 16-byte alignment
    store = types.SimpleNamespace(entries=entries, pflat=torch.zeros(off))
    args = dict(min_8bit_size=64, blocksize=blocksize)
    state = cls(store, args)
    assert [e[2] for e in state.layout.tensors] == [True, False]
    g = torch.Generator().manual_seed(11)
    (o8, k8, _, a0, nb, _), (_, k32, _, _, _, s0) = state.layout.tensors
    for n, t in state.buffers():          # random values in the elements a parameter owns (the rest is never saved)
        lo, k = (o8, k8) if n[0] == "q" else (a0, nb) if n.startswith("absmax") else (s0, k32)
        if not n.startswith("qmap"):
            t[lo:lo + k] = torch.randint(0, 256, (k,), generator=g).to(t.dtype) if t.dtype == torch.uint8 else torch.randn(k, generator=g)
    state.qmap1[3] += 1e-3                                                  # the file's code book, not the default one, comes back
    extra, per = cls.save(state, entries, 7, args)
    assert extra == {} and sorted(per) == [0, 1]
    moments = 2 if name == "BlockwiseState" else 1
    assert sorted(per[1]) == ["state1", "state2"][:moments] + ["step"]
    args2 = dict(min_8bit_size=64, blocksize=256)
    loaded, step = cls.load(store, {"state": per, "param_groups": [{}]}, args2)
    assert step == 7 and args2["blocksize"] == blocksize
    assert [n for n, _ in loaded.buffers()] == list(cls.NAMES) and len(cls.NAMES) == 4 * moments
    for (n, a), (_, b) in zip(state.buffers(), loaded.buffers()):
        assert a.dtype == b.dtype and torch.equal(a, b), n
