"""Blockwise 8-bit Adam / AdamW state with bitsandbytes' layout (bitsandbytes.optim.Adam8bit / AdamW8bit / PagedAdam8bit /
PagedAdamW8bit, what most of the reference's optimizer blocks select, e.g. configs/face_seg_config.yaml:55-59): the code books and
the file format.  optimizer.bin holds bnb's per-parameter state: step, state1 / state2 (uint8 codes shaped like the parameter, fp32
moments below min_8bit_size), qmap1 / qmap2, absmax1 / absmax2.  The device buffers over the flat LoRA buffers, stepped by ONE
qfx_adam8bit_step launch (include/qfx.h), are optim_state.BlockwiseState."""
from __future__ import annotations

import torch

BLOCKWISE = ("adam8bit_blockwise", "adamw8bit_blockwise")
LION_BLOCKWISE = ("lion8bit_blockwise",)      # bitsandbytes.optim.Lion8bit: ONE moment in the same layout (optim_state.LionBlockwiseState)
ADEMAMIX_BLOCKWISE = ("ademamix8bit_blockwise",)      # bitsandbytes.optim.AdEMAMix8bit: state1 holds two planes (optim_state.AdEMAMixBlockwiseState)
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


def bnb_moment1(e: dict):
    """state1 in fp32 of one bnb-layout parameter state with ONE moment (Lion: there is no state2)."""
    if e["state1"].dtype != torch.uint8:
        return e["state1"].float()
    bs = infer_blocksize(e["state1"].numel(), e["absmax1"].numel())
    return dequantize(e["state1"], e["qmap1"].float(), e["absmax1"].float(), bs)


def file_layout(states: dict, entries):
    """(blocksize, qmap1, qmap2) of a bnb-layout state dict: the block size inferred from the absmax sizes (one for all tensors), the
    code books of the first 8-bit tensor (None when every tensor is below the 8-bit size; qmap2 also for a one-moment file)."""
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
            q1, q2 = e["qmap1"].float(), (e["qmap2"].float() if "qmap2" in e else None)
    return bs, q1, q2
