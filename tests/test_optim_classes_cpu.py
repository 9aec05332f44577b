"""CPU: qflux_amd.optim -- the fused optimizers as torch.optim.Optimizer classes: config mapping, constructor validation on a
CPU-resident store, and state_dict() / load_state_dict() sharing QwenLoraTrainStep's layouts (no launch anywhere)."""
import pickle

import pytest
import torch
import torch.nn as nn

from test_sgd_cpu import _torch_sgd_file, toy_model

# (class name, optimizer= keyword of the train step, constructor keywords, the train step's optimizer_args)
FAMILIES = [("AdamW", "adamw", {}, None), ("Adam", "adam", {}, None), ("Adam8bit", "adam8bit_blockwise", {}, None),
            ("AdamW8bit", "adamw8bit_blockwise", {"min_8bit_size": 64, "blocksize": 2048}, {"min_8bit_size": 64, "blocksize": 2048}),
            ("Prodigy", "prodigy", {"use_bias_correction": True, "d0": 1e-5}, {"use_bias_correction": True, "d0": 1e-5}),
            ("SGD", "sgd", {"momentum": 0.9, "weight_decay": 1e-4}, {"momentum": 0.9})]


def _params(toy):
    return [p for n, p in toy.named_parameters() if "lora_" in n]


def test_config_mapping_of_the_six_class_paths():
    from qflux_amd.trainer import optimizer_kwargs_from_config as f
    assert f("qflux_amd.optim.AdamW", {"lr": 1e-4, "weight_decay": 0.01, "betas": [0.9, 0.999], "eps": 1e-8}) == \
        {"lr": 1e-4, "weight_decay": 0.01, "betas": (0.9, 0.999), "eps": 1e-8, "optimizer": "adamw"}
    assert f("qflux_amd.optim.Adam", {"lr": 1e-4}) == {"lr": 1e-4, "optimizer": "adam", "weight_decay": 0.0}
    # the class is named for its 8-bit state: blockwise whatever state_bits says, with the refusals of state_bits=8
    for bits in (8, 32):
        assert f("qflux_amd.optim.Adam8bit", {"lr": 1e-4, "betas": [0.9, 0.999]}, state_bits=bits) == \
            {"lr": 1e-4, "betas": (0.9, 0.999), "optimizer": "adam8bit_blockwise", "weight_decay": 0.0}
    assert f("qflux_amd.optim.AdamW8bit", {"lr": 1e-4, "min_8bit_size": 1024, "is_paged": True}) == \
        {"lr": 1e-4, "optimizer": "adamw8bit_blockwise", "weight_decay": 0.01, "optimizer_args": {"min_8bit_size": 1024}}
    for bad in ({"percentile_clipping": 5}, {"block_wise": False}, {"amsgrad": True}, {"max_unorm": 1.0}):
        with pytest.raises(NotImplementedError):
            f("qflux_amd.optim.Adam8bit", dict(lr=1e-4, **bad))
    kw = f("qflux_amd.optim.Prodigy", {"lr": 1.0, "use_bias_correction": True, "safeguard_warmup": True, "weight_decay": 0.01})
    assert kw == {"lr": 1.0, "weight_decay": 0.01, "optimizer": "prodigy", "optimizer_args": {"use_bias_correction": True, "safeguard_warmup": True}}
    # docs/guide/training.md:768-826: SGD with momentum 0.9, weight_decay 1e-4
    kw = f("qflux_amd.optim.SGD", {"lr": 1e-3, "momentum": 0.9, "weight_decay": 1e-4})
    assert kw == {"lr": 1e-3, "weight_decay": 1e-4, "optimizer": "sgd", "optimizer_args": {"momentum": 0.9}}
    kw = f("qflux_amd.optim.SGD", {"lr": 1e-3, "momentum": 0.9, "nesterov": True, "dampening": 0, "foreach": None})
    assert kw["optimizer_args"] == {"momentum": 0.9, "nesterov": True, "dampening": 0}
    with pytest.raises(NotImplementedError):
        f("qflux_amd.optim.SGD", {"lr": 0.1, "maximize": True})
    with pytest.raises(NotImplementedError):
        f("qflux_amd.optim.SGD", {"lr": 0.1, "betas": [0.9, 0.99], "bogus": 1})
    with pytest.raises(NotImplementedError):          # torch's own SGD is not mapped by this change (tests/test_abi_cpu.py pins it)
        f("torch.optim.SGD", {"lr": 0.1})
    with pytest.raises(NotImplementedError):
        f("qflux_amd.optim.Lion", {"lr": 0.1})


def test_constructor_refuses_anything_but_one_models_whole_adapter_set():
    from qflux_amd import optim as O
    toy, other = toy_model(), toy_model()
    ps = _params(toy)
    assert isinstance(O.SGD(ps, lr=0.1), torch.optim.Optimizer)
    with pytest.raises(ValueError, match=r"parameter 12 \(shape \(3, 5\)\) is not an adapter parameter"):
        O.AdamW(ps + [nn.Parameter(torch.zeros(3, 5))])
    with pytest.raises(ValueError, match=r"'transformer_blocks.2.to_k.lora_B.ad.weight' of the model is missing"):
        O.Adam8bit(ps[:-1])
    with pytest.raises(ValueError, match="2 parameter groups"):
        O.Prodigy([{"params": ps[:4]}, {"params": ps[4:], "lr": 0.5}])
    with pytest.raises(ValueError, match="parameter 12 .* belongs to another model"):
        O.SGD(ps + _params(other))
    with pytest.raises(ValueError, match="Nesterov momentum requires a momentum and zero dampening"):
        O.SGD(ps, lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)
    with pytest.raises(ValueError, match="Nesterov"):
        O.SGD(ps, lr=0.1, nesterov=True)
    with pytest.raises(NotImplementedError):
        O.SGD(ps, lr=0.1, maximize=True)
    with pytest.raises(NotImplementedError):
        O.Adam(ps, weight_decay=0.01)
    with pytest.raises(NotImplementedError):
        O.AdamW8bit(ps, percentile_clipping=5)
    with pytest.raises(ValueError, match="blocksize"):
        O.Adam8bit(ps, blocksize=512)
    # the back-reference does not keep a parameter from being pickled or the model from being copied
    assert pickle.loads(pickle.dumps(ps[0]))._lora_store() is None


@pytest.mark.parametrize("name,family,kw,args", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_state_dict_before_the_first_step_equals_the_train_steps(name, family, kw, args):
    from qflux_amd import optim as O
    from qflux_amd.trainer import QwenLoraTrainStep
    toy = toy_model()
    opt = getattr(O, name)(_params(toy), lr=2e-3, **kw)
    step = QwenLoraTrainStep(toy, lr=2e-3, weight_decay=kw.get("weight_decay"), optimizer=family, optimizer_args=args)
    sd = opt.state_dict()
    assert sd == step.state_dict() and sd["state"] == {} and sd["global_step"] == 0
    # torch's schedulers drive it: they write param_groups[0]["lr"], which state_dict() (and step()) read
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 0.25)
    assert opt.state_dict()["param_groups"][0]["lr"] == 5e-4 and sched.get_last_lr() == [5e-4]
    # and the file loads back (what accelerate's prepare() does with every optimizer it is given)
    opt.load_state_dict(sd)
    back = opt.state_dict()
    assert opt.param_groups[0]["lr"] == 2e-3 and back["param_groups"] == sd["param_groups"] and back["global_step"] == 0


def test_sgd_class_exchanges_files_with_torch_sgd_and_the_train_step():
    from qflux_amd import optim as O
    from qflux_amd.trainer import QwenLoraTrainStep
    toy = toy_model()
    st = toy.lora_store
    sd, ps = _torch_sgd_file(st, lr=0.05, momentum=0.9, weight_decay=1e-4)
    opt = O.SGD(_params(toy), lr=1.0)
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g["nesterov"]) == (0.05, 0.9, 1e-4, False)
    ours = opt.state_dict()
    for i, e in sd["state"].items():
        assert torch.equal(ours["state"][i]["momentum_buffer"], e["momentum_buffer"])
    step = QwenLoraTrainStep(toy, optimizer="sgd")
    step.load_state_dict(ours)
    mine, theirs = step.state_dict(), ours
    assert mine["param_groups"] == theirs["param_groups"] and list(mine["state"]) == list(theirs["state"])
    for i in mine["state"]:
        assert torch.equal(mine["state"][i]["momentum_buffer"], theirs["state"][i]["momentum_buffer"])
    torch.optim.SGD(ps, lr=1.0).load_state_dict(ours)
