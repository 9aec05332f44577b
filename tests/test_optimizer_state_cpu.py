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
