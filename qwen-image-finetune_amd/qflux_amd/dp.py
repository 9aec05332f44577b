"""Data-parallel plumbing over the flat LoRA buffers: the bucketed gradient exchange (LoraGradSync), the process-group set-up
(init_distributed_from_env) and the replica checksum (check_replicas).

The DROP-IN path (the reference's own trainer loop around `dit(...)` / `loss.backward()`):

The reference wraps its container of LoRA layers in DDP (accelerator.prepare, src/qflux/trainer/base_trainer.py:384-393) and DDP
reduces a gradient when autograd ACCUMULATES it into the parameter.  Here the whole DiT is one autograd node whose kernels write
dA / dB straight into the flat gradient buffer -- autograd never touches the LoRA parameters, DDP's hooks never fire.  The model
therefore exchanges its gradients itself:

    dit.enable_data_parallel(process_group=None, bucket_mb=24)      # once, after add_adapter (no-op without torch.distributed)
    ...
    loss.backward()          # bucketed all-reduce (SUM) of the flat LoRA gradient behind the backward program, drained and
                             # averaged (DDP semantics) before backward() returns
    with dit.no_sync(): ...  # gradient-accumulation micro-steps (accelerate's `accumulate(self.dit)` finds this method by name)

The fused step (QwenLoraTrainStep.train_step) holds a LoraGradSync of its own (step.sync: its group and bucket size may differ),
drains it with finish(average=False) and folds the 1/world factor into the optimizer kernel.
"""
from __future__ import annotations

import contextlib
import os

import torch
import torch.distributed as dist


def contiguous_runs(idx, ents):
    """Entry indices -> [lo, hi) element ranges of the flat buffer, merged where adjacent (64-element padded slots)."""
    runs = []
    for i in idx:
        lo = ents[i][2]
        hi = lo + (ents[i][3] + 63) // 64 * 64
        if runs and runs[-1][1] == lo:
            runs[-1][1] = hi
        else:
            runs.append([lo, hi])
    return [(a, b) for a, b in runs]


class LoraGradSync:
    def __init__(self, dit, process_group=None, bucket_mb: float = 24.0, force: bool = False):
        """force: exchange on a ONE-rank group too (the fused step's QFX_DP_FORCE=1; read by the owner, who decides when to hook)."""
        self.dit, self.group, self.force = dit, process_group, force
        self.world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        self.bucket_bytes = int(bucket_mb * (1 << 20))
        self.enabled = True
        self.exchanged = False     # set by finish(): the flat gradient currently holds the exchanged + averaged sum (cleared by the
                                   # trainer step's zero_grad / by the next local-only backward)
        self._pending, self._finish = [], None

    def hook(self):
        """on_segment callback of plan.run_backward: starts an async all-reduce on the contiguous slice of the blocks whose
        gradients are final once >= bucket_bytes have accumulated.  Conditioning-head adapters (their gradients are written by the
        LAST entries of the backward program) and anything outside the marked blocks go out with finish()."""
        st = self.dit.lora_store
        ents = st.entries
        todo = set(range(len(ents)))
        acc = []
        self._pending = []
        cond_sfx = tuple(getattr(self.dit, "_COND_SUFFIXES", ()))
        late = {i for i in todo if cond_sfx and ents[i][0].split(".lora_")[0].endswith(cond_sfx)}

        def flush(force=False):
            nbytes = sum(((ents[i][3] + 63) // 64 * 64) * 4 for i in acc)
            if not acc or (not force and nbytes < self.bucket_bytes):
                return
            for lo, hi in contiguous_runs(sorted(acc), ents):
                self._pending.append(dist.all_reduce(st.gflat[lo:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
            acc.clear()

        def on_segment(prefix):
            done = [i for i in todo if i not in late and ents[i][0].startswith(prefix)]
            todo.difference_update(done)
            acc.extend(done)
            flush()

        def finish():
            acc.extend(sorted(todo))
            todo.clear()
            flush(force=True)

        self._finish = finish
        return on_segment

    def finish(self, average: bool = True):
        """Drain the buckets; average=True divides by the world size (what DDP hands to the optimizer)."""
        if self._finish is not None:
            self._finish()
            self._finish = None
        for w in self._pending:
            w.wait()
        self._pending = []
        if average and self.world > 1:
            self.dit.lora_store.gflat.mul_(1.0 / self.world)
        self.exchanged = True

    @property
    def armed(self):
        """A hook() of this object was handed to a backward program and finish() has not drained it yet."""
        return self._finish is not None

    def disarm(self):
        """Drop an armed hook without running it (nothing was started through it: a captured graph replays no callback)."""
        self._finish = None


class DataParallelMixin:
    """enable_data_parallel / no_sync for the drop-in DiT modules (see module docstring)."""

    _dp = None

    def enable_data_parallel(self, process_group=None, bucket_mb: float = 24.0):
        self._dp = LoraGradSync(self, process_group, bucket_mb) if (dist.is_available() and dist.is_initialized()
                                                                    and dist.get_world_size(process_group) > 1) else None
        return self

    @contextlib.contextmanager
    def no_sync(self):
        """DDP.no_sync look-alike: backward passes inside the context only accumulate locally."""
        dp = self._dp
        old = dp.enabled if dp is not None else None
        if dp is not None:
            dp.enabled = False
        try:
            yield
        finally:
            if dp is not None:
                dp.enabled = old

    def _dp_backward(self, plan, grad_out):
        """The autograd node's backward: launch program + (when enabled) the overlapped exchange."""
        dp = self._dp
        if dp is None or not dp.enabled:
            if dp is not None:
                dp.exchanged = False       # local-only gradients were just added on top of whatever the buffer held
            plan.run_backward(grad_out)
            return
        plan.run_backward(grad_out, on_segment=dp.hook())
        dp.finish(average=True)


def init_distributed_from_env():
    """One process per GPU; backend "nccl" is RCCL on ROCm.  Returns (rank, local_rank, world).
    Test hooks: QFX_DIST_BACKEND=gloo and QFX_SHARE_GPU=1 let several ranks share device 0 (RCCL refuses duplicate devices), so
    the multi-rank code path can be exercised on a one-GPU box."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("QFX_SHARE_GPU") == "1":
        local = 0
    if torch.cuda.is_available():
        torch.cuda.set_device(local)   # before the process group: RCCL binds to the current device
    if (world > 1 or os.environ.get("QFX_BENCH_INIT_PG") == "1") and not dist.is_initialized():     # (one-rank group: tools/rccl_one_rank.py)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("QFX_DIST_BACKEND", "nccl" if torch.cuda.is_available() else "gloo")
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, local, world


def check_replicas(buffers, world, group=None, what: str = "adapter weights"):
    """Raises if the named buffers [(name, tensor or None)] differ between ranks: two order-sensitive fp64 checksums per buffer (and
    whether the rank has it at all), gathered and compared on every rank of the group (`world` of them, more than one).  Cheap: one
    small all-gather."""
    dev = buffers[0][1].device
    sums = []
    for _, t in buffers:      # fixed layout: a buffer a rank lacks is part of the verdict
        if t is None:
            sums += [torch.zeros((), dtype=torch.float64, device=dev)] * 3
            continue
        d = t.detach().double().flatten()
        w = torch.arange(1, d.numel() + 1, device=d.device, dtype=torch.float64) % 8191
        sums += [torch.ones((), dtype=torch.float64, device=dev), d.sum(), (d * w).sum()]
    mine = torch.stack(sums)
    out = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(out, mine, group=group)
    for r, o in enumerate(out):
        if not torch.equal(o, out[0]):
            raise RuntimeError(f"data-parallel replicas diverged ({what}): rank {r} differs from rank 0 "
                               f"(checksums {o.tolist()} vs {out[0].tolist()}); call broadcast_state() after loading state")
    return True
