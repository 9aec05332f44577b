"""Fingerprint of a plan's launch programs: every call of plan.fwd and plan.bwd with its arguments, pointers canonicalised.

For each entry of `calls`, in order: the C function's name ("py" for a Python entry), the side-stream flag and every argument --
scalars verbatim, ctypes structs and arrays walked field by field through `_fields_` (nested structs too).  Pointers (c_void_p
fields; positional arguments whose `argtypes` entry is a pointer) become 0 for null, else the index of the address's first
appearance counted over the forward and then the backward program; so two builds of the same plan, or the same plan built by
two revisions of the plan builder, give the same fingerprint exactly when they launch the same kernels on the same operands.
The `marks` lists follow.  Reads plan.fwd / plan.bwd only.

    python tools/plan_fingerprint.py --list
    python tools/plan_fingerprint.py --config qwen_attn [--full]
    python tools/plan_fingerprint.py --all [--out hashes.json]

Another checkout is fingerprinted by pointing PYTHONPATH (its qwen-image-finetune_amd directory) and QFX_LIB_PATH at it.
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "qwen-image-finetune_amd")):
    if _p not in sys.path:
        sys.path.append(_p)      # appended: a PYTHONPATH that names another checkout wins

LEVERS = ("QFX_SIDE_GRADS", "QFX_SIDE_GRADS_FF", "QFX_FUSE_QKNORM_BWD", "QFX_FUSE_HEAD_LORA", "QFX_FUSE_LN_DOWN", "QFX_LN_DOWN_FRAG",
          "QFX_FP8_FUSED_QUANT", "QFX_GRAD_DET")
_PTR_BASES = (C._Pointer, C.c_void_p, C.c_char_p)


class _Canon:
    def __init__(self):
        self.seen = {}

    def ptr(self, v):
        if not v:
            return 0
        return self.seen.setdefault(int(v), len(self.seen) + 1)

    def value(self, v, ctype=None):
        if isinstance(v, C.Structure):
            return {name: self.value(getattr(v, name), ftype) for name, ftype, *_ in v._fields_}
        if isinstance(v, C.Array):
            return [self.value(x, v._type_) for x in v]
        if hasattr(v, "_obj"):                      # ctypes.byref(struct)
            return self.value(v._obj)
        if ctype is not None and isinstance(ctype, type) and issubclass(ctype, _PTR_BASES):
            return {"p": self.ptr(v.value if isinstance(v, C.c_void_p) else v)}
        if isinstance(v, C._SimpleCData):
            return self.value(v.value, type(v))
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        raise TypeError(f"plan_fingerprint: argument of type {type(v).__name__}")

    def program(self, prog):
        out = []
        for ent in prog.calls:
            fn, args = ent[0], ent[1]
            if fn is None:
                out.append({"fn": "py", "side": False, "args": []})
                continue
            types = list(fn.argtypes or [])
            out.append({"fn": fn.__name__, "side": len(ent) > 2,
                        "args": [self.value(a, types[i] if i < len(types) else None) for i, a in enumerate(args)]})
        return out


def fingerprint(plan):
    """-> dict(calls=[...forward entries, then backward entries...], marks=dict(fwd, bwd))."""
    c = _Canon()
    calls = c.program(plan.fwd) + c.program(plan.bwd)
    return {"calls": calls, "marks": {"fwd": [list(m) for m in plan.fwd.marks], "bwd": [list(m) for m in plan.bwd.marks]}}


def digest(fp) -> str:
    return hashlib.sha256(json.dumps(fp, sort_keys=True).encode()).hexdigest()


# ---------------------------------------------------------------------------------------------- configurations
ATTN = ("to_k", "to_q", "to_v", "to_out.0")
FF = ATTN + ("img_mlp.net.0.proj", "img_mlp.net.2", "txt_mlp.net.0.proj", "txt_mlp.net.2")
COND = ATTN + ("timestep_embedder.linear_1", "timestep_embedder.linear_2", "img_mod.1", "txt_mod.1", "norm_out.linear")
# the narrowest width whose block linears are eligible for the MX-FP8 trunk (K % 128 == 0, K >= 1024): tests/test_mxfp8_gpu.py
W1024 = dict(patch_size=2, in_channels=64, out_channels=16, num_layers=2, attention_head_dim=128, num_attention_heads=8,
             joint_attention_dim=1024, axes_dims_rope=(16, 56, 56))
FLUX_W1024 = dict(patch_size=1, in_channels=64, out_channels=64, num_layers=1, num_single_layers=1, attention_head_dim=128,
                  num_attention_heads=8, joint_attention_dim=64, pooled_projection_dim=32, guidance_embeds=False, axes_dims_rope=(16, 56, 56))


def _qwen(cfg=None, targets=ATTN, r=4, quant=None, device="cuda:0"):
    import torch
    from common import TINY
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.modules import LoraConfig
    with torch.device(device):
        m = QwenImageTransformer2DModel(**dict(TINY if cfg is None else cfg))
    if targets:
        m.add_adapter(LoraConfig(r=r, lora_alpha=2 * r, target_modules=list(targets)), "lora_edit")
    if quant:
        m.quantize_trunk(quant)
    return m


def _qwen_plan(m, B=2, shapes=((1, 4, 6), (1, 4, 6)), T=5):
    S_i = sum(f * h * w for f, h, w in shapes)
    return m.get_plan(B, S_i, T, [[tuple(s) for s in shapes]] * B, [T] * B)


def _qwen_multires(m, T=5):
    import torch
    per = [[(1, 4, 6), (1, 4, 6)], [(1, 2, 4), (1, 4, 4)]]      # two samples of different size, right-padded to the first
    lens = [sum(f * h * w for f, h, w in sh) for sh in per]
    S_i = max(lens)
    mask = torch.zeros(2, T + S_i, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, : T + n] = True
    return m.get_plan_multires(2, S_i, T, per, [T, T], mask)


def _flux(cfg=None, quant=None, device="cuda:0"):
    import torch
    from common import FLUX_TINY
    from qflux_amd.models import FluxTransformer2DModel
    from qflux_amd.modules import LoraConfig
    with torch.device(device):
        m = FluxTransformer2DModel(**(dict(FLUX_TINY, joint_attention_dim=64, guidance_embeds=True) if cfg is None else dict(cfg)))
    m.add_adapter(LoraConfig(r=4, lora_alpha=8), "a")
    if quant:
        m.quantize_trunk(quant)
    return m


def _flux_ids(h, w, frame):
    import torch
    ids = torch.zeros(h, w, 3)
    ids[..., 0] = frame
    ids[..., 1] = torch.arange(h)[:, None]
    ids[..., 2] = torch.arange(w)[None, :]
    return ids.reshape(h * w, 3)


def _flux_plan(m, B=2, hw=(4, 6), T=7):
    import torch
    img_ids = torch.cat([_flux_ids(*hw, 0), _flux_ids(*hw, 1)], dim=0)
    return m.get_plan(B, img_ids.shape[0], T, img_ids, torch.zeros(T, 3))


def _flux_multires(m, T=7):
    import torch
    img_ids = torch.cat([_flux_ids(4, 6, 0), _flux_ids(4, 6, 1)], dim=0)
    return m.get_plan_multires(2, img_ids.shape[0], T, img_ids, [img_ids.shape[0], 31])


CONFIGS = {
    "qwen_plain": lambda: _qwen_plan(_qwen(targets=None)),
    "qwen_attn": lambda: _qwen_plan(_qwen()),
    "qwen_ff": lambda: _qwen_plan(_qwen(targets=FF)),
    "qwen_cond": lambda: _qwen_plan(_qwen(targets=COND)),
    "qwen_head_lora": lambda: _qwen_plan(_qwen(), T=16),        # T % 16 == 0: rank-r projections in the attention epilogues
    "qwen_multires": lambda: _qwen_multires(_qwen()),
    "qwen_mxfp8": lambda: _qwen_plan(_qwen(W1024, r=8, quant="mxfp8"), shapes=((1, 12, 12), (1, 12, 12)), T=40),
    "qwen_mxfp8_fb": lambda: _qwen_plan(_qwen(W1024, r=8, quant="mxfp8-fb"), shapes=((1, 12, 12), (1, 12, 12)), T=40),
    "flux_attn": lambda: _flux_plan(_flux()),
    "flux_multires": lambda: _flux_multires(_flux()),
    "flux_mxfp8_fb": lambda: _flux_plan(_flux(FLUX_W1024, quant="mxfp8-fb"), hw=(8, 8), T=16),
}
for _name in LEVERS:      # the attention-adapter Qwen plan once more with each lever switched off
    CONFIGS["qwen_attn," + _name + "=0"] = CONFIGS["qwen_attn"]
CONFIGS["qwen_head_lora,QFX_FUSE_HEAD_LORA=0"] = CONFIGS["qwen_head_lora"]


def build(config: str):
    """Model + plan of a named configuration (levers of `NAME,VAR=0` set around the build only)."""
    name, _, lever = config.partition(",")
    saved = {k: os.environ.pop(k, None) for k in LEVERS}
    try:
        if lever:
            var, _, val = lever.partition("=")
            os.environ[var] = val
        return CONFIGS[config]()
    finally:
        for k in LEVERS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--full", action="store_true", help="print the fingerprint itself, not only its sha256")
    ap.add_argument("--out", help="also write {config: sha256} to this JSON file")
    a = ap.parse_args()
    if a.list:
        print("\n".join(CONFIGS))
        return
    hashes = {}
    for name in (list(CONFIGS) if a.all else [a.config]):
        fp = fingerprint(build(name))
        hashes[name] = digest(fp)
        print(json.dumps({"config": name, "entries": len(fp["calls"]), "sha256": hashes[name], **({"fingerprint": fp} if a.full else {})}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(hashes, f, indent=1)


if __name__ == "__main__":
    main()
