"""CPU: optimizer="sgd" (trainer/optim_state.SgdState) -- argument validation of qfx_sgd_step without a launch, torch.optim.SGD's
checkpoint layout in both directions against the installed torch.optim.SGD, and the rank-0 broadcast / replica check over gloo."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def toy_model(n_blocks=3):
    """A CPU-resident LoraStore over a few adapters (the pattern of test_dp_gloo_cpu.py)."""
    from qflux_amd.modules import LoraStore, QfxLinear, QfxLoraLinear

    class Blk(nn.Module):
        def __init__(self):
            super().__init__()
            self.to_q = QfxLoraLinear(QfxLinear(8, 8), 4, 8, "ad")
            self.to_k = QfxLoraLinear(QfxLinear(8, 12), 4, 8, "ad")

    class Toy(nn.Module):
        def __init__(self):
            super().__init__()
            self.transformer_blocks = nn.ModuleList([Blk() for _ in range(n_blocks)])
            self._store = LoraStore(self)
            self._store.rebuild("cpu")

        @property
        def lora_store(self):
            return self._store

        device = torch.device("cpu")

    return Toy()


def test_sgd_step_rejects_bad_arguments_before_any_launch():
    from qflux_amd import _lib
    f = _lib.lib.qfx_sgd_step
    P, G, B = 0x1000, 0x2000, 0x3000        # never dereferenced: every call below is rejected on the host
    #        p  g  buf n  lr   mom  damp wd   nest first gnorm max  scale stream
    assert f(None, G, B, 8, 0.1, 0.9, 0.0, 0.0, 0, 0, None, 0.0, 1.0, None) == _lib.QFX_EINVAL
    assert f(P, None, B, 8, 0.1, 0.9, 0.0, 0.0, 0, 0, None, 0.0, 1.0, None) == _lib.QFX_EINVAL
    assert f(P, G, B, 0, 0.1, 0.9, 0.0, 0.0, 0, 0, None, 0.0, 1.0, None) == _lib.QFX_EINVAL
    assert f(P, G, B, -3, 0.1, 0.9, 0.0, 0.0, 0, 0, None, 0.0, 1.0, None) == _lib.QFX_EINVAL
    assert f(P, G, None, 8, 0.1, 0.9, 0.0, 0.0, 0, 0, None, 0.0, 1.0, None) == _lib.QFX_EINVAL      # momentum without a buffer
    assert f(P, G, B, 8, 0.1, 0.0, 0.0, 0.0, 1, 0, None, 0.0, 1.0, None) == _lib.QFX_EINVAL         # Nesterov without momentum
    assert f(P, G, B, 8, 0.1, -0.5, 0.0, 0.0, 1, 0, None, 0.0, 1.0, None) == _lib.QFX_EINVAL
    assert f(P, G, B, 8, 0.1, 0.9, 0.1, 0.0, 1, 0, None, 0.0, 1.0, None) == _lib.QFX_EINVAL         # Nesterov with dampening


def test_trainer_accepts_sgd_and_raises_torchs_errors():
    from qflux_amd.trainer import FluxKontextTrainStep, QwenLoraTrainStep
    toy = toy_model()
    s = QwenLoraTrainStep(toy, optimizer="sgd")
    assert s.weight_decay == 0.0 and s.optimizer_args == {"momentum": 0.0, "dampening": 0.0, "nesterov": False}
    s = FluxKontextTrainStep(toy, optimizer="sgd", weight_decay=1e-4, optimizer_args={"momentum": 0.9})
    assert s.weight_decay == 1e-4 and s.optimizer_args["momentum"] == 0.9
    with pytest.raises(ValueError, match="Nesterov"):
        QwenLoraTrainStep(toy, optimizer="sgd", optimizer_args={"nesterov": True})
    with pytest.raises(ValueError, match="Nesterov"):
        QwenLoraTrainStep(toy, optimizer="sgd", optimizer_args={"nesterov": True, "momentum": 0.9, "dampening": 0.1})
    with pytest.raises(ValueError):
        QwenLoraTrainStep(toy, optimizer="sgd", optimizer_args={"maximize": True})
    with pytest.raises(ValueError):
        QwenLoraTrainStep(toy, optimizer="sgd", optimizer_args={"momentum": -0.1})
    # before the first step: torch.optim.SGD's empty state and its group fields
    sd = QwenLoraTrainStep(toy, lr=0.1, optimizer="sgd", optimizer_args={"momentum": 0.9}).state_dict()
    g = sd["param_groups"][0]
    assert sd["state"] == {} and (g["momentum"], g["dampening"], g["nesterov"], g["maximize"]) == (0.9, 0.0, False, False)


def _torch_sgd_file(st, steps=3, **kw):
    """`steps` steps of the installed torch.optim.SGD on CPU copies of the store's parameters -> (its state_dict, the copies)."""
    g = torch.Generator().manual_seed(9)
    ps = [nn.Parameter(torch.randn(p.shape, generator=g) * 0.1) for _, p in st.params()]
    opt = torch.optim.SGD(ps, **kw)
    for _ in range(steps):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt.state_dict(), ps


def test_file_of_torch_sgd_loads_with_exact_momentum_buffers(tmp_path):
    from qflux_amd.trainer import QwenLoraTrainStep
    toy = toy_model()
    st = toy.lora_store
    sd, _ = _torch_sgd_file(st, lr=0.05, momentum=0.9, weight_decay=1e-4)
    torch.save(sd, str(tmp_path / "optimizer.bin"))
    sd = torch.load(str(tmp_path / "optimizer.bin"), map_location="cpu", weights_only=False)
    assert "betas" not in sd["param_groups"][0] and "eps" not in sd["param_groups"][0]
    step = QwenLoraTrainStep(toy, lr=1.0, betas=(0.8, 0.9), eps=1e-6, optimizer="sgd")
    step.load_state_dict(sd)
    assert (step.lr, step.weight_decay, step.betas, step.eps) == (0.05, 1e-4, (0.8, 0.9), 1e-6)
    assert step.optimizer_args == {"momentum": 0.9, "dampening": 0, "nesterov": False}
    assert step.opt_state is not None and step.opt_state.first is False          # a loaded state has stepped: no buf = g restart
    for i, (_, p, off, k) in enumerate(st.entries):
        assert torch.equal(step.opt_state.buf[off:off + k].view(p.shape), sd["state"][i]["momentum_buffer"])
    out = step.state_dict()
    assert list(out["state"]) == list(sd["state"])
    for i, e in sd["state"].items():
        assert list(out["state"][i]) == ["momentum_buffer"] and torch.equal(out["state"][i]["momentum_buffer"], e["momentum_buffer"])
    # a momentum-free file: no state at all, as torch writes it
    sd0, _ = _torch_sgd_file(st, lr=0.05)
    step0 = QwenLoraTrainStep(toy, optimizer="sgd", optimizer_args={"momentum": 0.9})
    step0.load_state_dict(sd0)
    assert step0.opt_state is None and step0.optimizer_args["momentum"] == 0 and step0.state_dict()["state"] == {}


def test_torch_sgd_accepts_our_file(tmp_path):
    from qflux_amd.trainer import QwenLoraTrainStep
    toy = toy_model()
    st = toy.lora_store
    sd, ps = _torch_sgd_file(st, lr=0.05, momentum=0.9, weight_decay=1e-4)
    step = QwenLoraTrainStep(toy, optimizer="sgd")
    step.load_state_dict(sd)
    torch.save(step.state_dict(), str(tmp_path / "optimizer.bin"))
    ours = torch.load(str(tmp_path / "optimizer.bin"), map_location="cpu", weights_only=False)
    opt = torch.optim.SGD(ps, lr=1.0)
    opt.load_state_dict(ours)
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"], g["maximize"]) == (0.05, 0.9, 0, 1e-4, False, False)
    for i, p in enumerate(ps):
        assert torch.equal(opt.state[p]["momentum_buffer"], sd["state"][i]["momentum_buffer"])
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()                     # and it steps from there
    # the file written before any step loads too (empty state)
    torch.optim.SGD(ps, lr=1.0).load_state_dict(QwenLoraTrainStep(toy, optimizer="sgd", optimizer_args={"momentum": 0.9}).state_dict())


def _worker_sgd_broadcast(rank, world, port, q, momentum):
    """Rank 0 alone resumed a torch.optim.SGD file: check_replicas() flags it, broadcast_state() repairs it -- with momentum 0 the
    buffer list is empty on EVERY rank (a rank without state must not list a buffer the others lack) -- and a stray state of rank 1
    is dropped when rank 0 has none."""
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "qwen-image-finetune_amd")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from qflux_amd.trainer import QwenLoraTrainStep
    from qflux_amd.trainer.optim_state import SgdState
    toy = toy_model()
    st = toy.lora_store
    with torch.no_grad():
        st.pflat.copy_(torch.randn(st.pflat.shape, generator=torch.Generator().manual_seed(100 + rank)))
    sd, _ = _torch_sgd_file(st, lr=0.05, momentum=momentum)
    sd["global_step"] = 3
    args = {"momentum": momentum}
    step = QwenLoraTrainStep(toy, optimizer="sgd", optimizer_args=args)
    if rank == 0:
        step.load_state_dict(sd)
        if momentum == 0:          # a momentum-free run that has stepped: a state object without buffers
            step.opt_state = SgdState(st, step.optimizer_args)
            step.opt_state.first = False
    ok = len(step._state_buffers()) == (2 if momentum else 1)          # the same list with and without a state object
    flagged = False
    try:
        step.check_replicas()
    except RuntimeError:
        flagged = True
    step.broadcast_state()
    ok = ok and flagged and step.check_replicas() and step.global_step == 3
    ok = ok and torch.equal(st.pflat, torch.randn(st.pflat.shape, generator=torch.Generator().manual_seed(100)))
    ok = ok and step.opt_state is not None and step.opt_state.first is False
    out = step.state_dict()
    ok = ok and list(out["state"]) == list(sd["state"])
    for i, e in sd["state"].items():
        ok = ok and torch.equal(out["state"][i]["momentum_buffer"], e["momentum_buffer"])
    # rank 1 carries state, rank 0 has none: the same collectives everywhere, the stray state is dropped
    step = QwenLoraTrainStep(toy, optimizer="sgd", optimizer_args=args)
    if rank == 1:
        step.opt_state = SgdState(st, step.optimizer_args)
        if momentum:
            step.opt_state.buf.fill_(3.0)
    step.broadcast_state()
    ok = ok and step.opt_state is None and step.state_dict()["state"] == {} and step.check_replicas()
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_rank0_broadcast_of_sgd_state_world2(momentum):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 41500 + (os.getpid() % 2000) + (7 if momentum else 0)
    procs = [ctx.Process(target=_worker_sgd_broadcast, args=(r, 2, port, q, momentum)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(60)
    assert sorted(res) == [(0, True), (1, True)], res
