"""Blockwise 8-bit Adam / AdamW state with bitsandbytes' layout (bitsandbytes.optim.Adam8bit / AdamW8bit / PagedAdam8bit /
PagedAdamW8bit, what most of the reference's optimizer blocks select, e.g. configs/face_seg_config.yaml:55-59) over the flat LoRA
buffers, stepped by ONE qfx_adam8bit_step launch (include/qfx.h).  optimizer.bin then holds bnb's per-parameter state: step,
state1 / state2 (uint8 codes shaped like the parameter, fp32 moments below min_8bit_size), qmap1 / qmap2, absmax1 / absmax2."""
from __future__ import annotations

import torch

from .. import ops

BLOCKWISE = ("adam8bit_blockwise", "adamw8bit_blockwise")
BLOCKSIZES = (256, 2048)


def dynamic_map(signed: bool = True, max_exponent_bits: int = 7, total_bits: int = 8) -> torch.Tensor:
    """bnb's create_dynamic_map: 256 sorted fp32 code values in [-1, 1] (signed) or [0, 1] (unsigned), 0 and 1.0 included."""
    data = []
    non_sign_bits = total_bits - 1
    for i in range(max_exponent_bits):
        items = 2 ** (i + non_sign_bits - max_exponent_bits) + 1 if signed else 2 ** (i + non_sign_bits - max_exponent_bits + 1) + 1
        bounds = torch.linspace(0.1, 1, items, dtype=torch.float32)
        means = (bounds[:-1] + bounds[1:]) / 2.0
        data += ((10 ** (-(max_exponent_bits - 1) + i)) * means).tolist()
        if signed:
            data += (-(10 ** (-(max_exponent_bits - 1) + i)) * means).tolist()
    data += [0.0, 1.0]
    data += [0.0] * (2 ** total_bits - len(data))
    data.sort()
    return torch.tensor(data, dtype=torch.float32)


def dequantize(codes: torch.Tensor, qmap: torch.Tensor, absmax: torch.Tensor, blocksize: int) -> torch.Tensor:
    """fp32 moments of one parameter's 8-bit state: qmap[code] * absmax[block] (the kernel's decode, same rounding)."""
    flat = codes.reshape(-1).long()
    blk = torch.arange(flat.numel(), device=flat.device) // blocksize
    return (qmap.to(flat.device)[flat] * absmax.to(flat.device)[blk]).view(codes.shape)


def infer_blocksize(numel: int, n_absmax: int) -> int:
    for bs in BLOCKSIZES:
        if n_absmax == (numel + bs - 1) // bs:
            return bs
    raise ValueError(f"8-bit state of a {numel}-element tensor with {n_absmax} absmax blocks: no block size in {BLOCKSIZES} fits")


def bnb_moments(e: dict):
    """(exp_avg, exp_avg_sq) in fp32 of one bnb-layout parameter state (8-bit codes dequantised, fp32 moments as they are)."""
    if e["state1"].dtype != torch.uint8:
        return e["state1"].float(), e["state2"].float()
    k = e["state1"].numel()
    bs = infer_blocksize(k, e["absmax1"].numel())
    return (dequantize(e["state1"], e["qmap1"].float(), e["absmax1"].float(), bs),
            dequantize(e["state2"], e["qmap2"].float(), e["absmax2"].float(), bs))


class BlockwiseState:
    """Device buffers of the blockwise 8-bit optimizer for one LoraStore layout: codes indexed like pflat, absmax per 8-bit block,
    fp32 moments of the small tensors, the two code books, and the cached block table."""

    def __init__(self, store, blocksize: int, min_8bit_size: int, qmap1=None, qmap2=None):
        dev = store.pflat.device
        self.key = self.layout_key(store, blocksize, min_8bit_size)
        self.layout = ops.adam8bit_block_table([(off, k) for _, _, off, k in store.entries], blocksize, min_8bit_size, device=dev)
        n = store.pflat.numel()
        self.q1 = torch.zeros(n, dtype=torch.uint8, device=dev)     # bnb's initial state: codes 0, absmax 0 (decodes to 0)
        self.q2 = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.absmax1 = torch.zeros(max(1, self.layout.n_absmax), dtype=torch.float32, device=dev)
        self.absmax2 = torch.zeros_like(self.absmax1)
        self.m32 = torch.zeros(max(1, self.layout.n_fp32), dtype=torch.float32, device=dev)
        self.v32 = torch.zeros_like(self.m32)
        self.qmap1 = (dynamic_map(True) if qmap1 is None else qmap1).to(device=dev, dtype=torch.float32).contiguous()
        self.qmap2 = (dynamic_map(False) if qmap2 is None else qmap2).to(device=dev, dtype=torch.float32).contiguous()

    @staticmethod
    def layout_key(store, blocksize, min_8bit_size):
        return (tuple((off, k) for _, _, off, k in store.entries), str(store.pflat.device), int(blocksize), int(min_8bit_size))

    def buffers(self):
        return [("_a8_q1", self.q1), ("_a8_q2", self.q2), ("_a8_absmax1", self.absmax1), ("_a8_absmax2", self.absmax2),
                ("_a8_m32", self.m32), ("_a8_v32", self.v32), ("_a8_qmap1", self.qmap1), ("_a8_qmap2", self.qmap2)]

    def step(self, store, lr, betas, eps, weight_decay, step, gnorm_sq, max_norm, grad_scale):
        ops.adam8bit_step(store.pflat, store.gflat, self.q1, self.q2, self.absmax1, self.absmax2, self.m32, self.v32, self.layout,
                          self.qmap1, self.qmap2, lr, betas, eps, weight_decay, step, gnorm_sq=gnorm_sq, max_norm=max_norm,
                          grad_scale=grad_scale)

    def param_state(self, i, shape, step):
        """bnb's per-parameter state of entry i (CPU tensors)."""
        off, k, eight, a0, nb, s0 = self.layout.tensors[i]
        if not eight:
            return {"step": step, "state1": self.m32[s0:s0 + k].view(shape).cpu().clone(),
                    "state2": self.v32[s0:s0 + k].view(shape).cpu().clone()}
        return {"step": step, "state1": self.q1[off:off + k].view(shape).cpu().clone(), "state2": self.q2[off:off + k].view(shape).cpu().clone(),
                "qmap1": self.qmap1.cpu().clone(), "qmap2": self.qmap2.cpu().clone(),
                "absmax1": self.absmax1[a0:a0 + nb].cpu().clone(), "absmax2": self.absmax2[a0:a0 + nb].cpu().clone()}

    def load_param_state(self, i, e):
        off, k, eight, a0, nb, s0 = self.layout.tensors[i]
        if (e["state1"].dtype == torch.uint8) != eight:
            raise ValueError(f"optimizer state of parameter {i} ({k} elements) is {'8-bit' if not eight else 'fp32'} in the file: it was "
                             f"saved with another min_8bit_size than {self.layout.min_8bit_size}")
        if not eight:
            self.m32[s0:s0 + k].copy_(e["state1"].reshape(-1)); self.v32[s0:s0 + k].copy_(e["state2"].reshape(-1))
            return
        if e["absmax1"].numel() != nb or e["absmax2"].numel() != nb:
            raise ValueError(f"optimizer state of parameter {i}: {e['absmax1'].numel()} absmax blocks, {nb} expected")
        self.q1[off:off + k].copy_(e["state1"].reshape(-1)); self.q2[off:off + k].copy_(e["state2"].reshape(-1))
        self.absmax1[a0:a0 + nb].copy_(e["absmax1"].reshape(-1)); self.absmax2[a0:a0 + nb].copy_(e["absmax2"].reshape(-1))


def file_layout(states: dict, entries):
    """(blocksize, qmap1, qmap2) of a bnb-layout state dict: the block size inferred from the absmax sizes (one for all tensors), the
    code books of the first 8-bit tensor (None when every tensor is below the 8-bit size)."""
    bs, q1, q2 = None, None, None
    for i, (_, _, _, k) in enumerate(entries):
        e = states.get(i)
        if e is None or e["state1"].dtype != torch.uint8:
            continue
        b = infer_blocksize(k, e["absmax1"].numel())
        if bs is not None and b != bs:
            raise ValueError(f"optimizer state mixes block sizes {bs} and {b}")
        bs = b
        if q1 is None:
            q1, q2 = e["qmap1"].float(), e["qmap2"].float()
    return bs, q1, q2
