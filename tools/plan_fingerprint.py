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
    python tools/plan_fingerprint.py --dry-run --all [--out hashes.json]      (no GPU: see dry_run)

A configuration the plan builder refuses (NotImplementedError) is recorded as "refused: <message>" in place of its digest.
Another checkout is fingerprinted by pointing PYTHONPATH (its qwen-image-finetune_amd directory) and QFX_LIB_PATH at it.
"""
from __future__ import annotations

import argparse
import contextlib
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
          "QFX_FP8_FUSED_QUANT", "QFX_GRAD_DET", "QFX_ATTN_BWD")      # cleared around every build: a fingerprint is of the defaults
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
EMBED = ATTN + ("img_in", "txt_in", "proj_out")
# FLUX: every adaptable linear of the double and the single blocks ("proj_out" also names the final projection) + the two embedders
FLUX_ALL = ATTN + ("add_q_proj", "add_k_proj", "add_v_proj", "to_add_out", "ff.net.0.proj", "ff.net.2", "ff_context.net.0.proj",
                   "ff_context.net.2", "proj_mlp", "proj_out", "x_embedder", "context_embedder")
FLUX_COND = ATTN + ("timestep_embedder.linear_1", "timestep_embedder.linear_2", "guidance_embedder.linear_1", "guidance_embedder.linear_2",
                    "text_embedder.linear_1", "text_embedder.linear_2", "norm1.linear", "norm1_context.linear", "norm.linear",
                    "norm_out.linear")
# the narrowest width whose block linears are eligible for the MX-FP8 trunk (K % 128 == 0, K >= 1024): tests/test_mxfp8_gpu.py
W1024 = dict(patch_size=2, in_channels=64, out_channels=16, num_layers=2, attention_head_dim=128, num_attention_heads=8,
             joint_attention_dim=1024, axes_dims_rope=(16, 56, 56))
FLUX_W1024 = dict(patch_size=1, in_channels=64, out_channels=64, num_layers=1, num_single_layers=1, attention_head_dim=128,
                  num_attention_heads=8, joint_attention_dim=64, pooled_projection_dim=32, guidance_embeds=False, axes_dims_rope=(16, 56, 56))


DEVICE = "cuda:0"      # where the configurations build their models (dry_run: "cpu")


def _qwen(cfg=None, targets=ATTN, r=4, quant=None):
    import torch
    from common import TINY
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.modules import LoraConfig
    with torch.device(DEVICE):
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


def _flux(cfg=None, quant=None, targets=ATTN, **over):
    """cfg None: the tiny FLUX model with guidance, `over` on top (num_layers=0, ...); targets None: no adapter."""
    import torch
    from common import FLUX_TINY
    from qflux_amd.models import FluxTransformer2DModel
    from qflux_amd.modules import LoraConfig
    with torch.device(DEVICE):
        m = FluxTransformer2DModel(**(dict(FLUX_TINY, joint_attention_dim=64, guidance_embeds=True, **over) if cfg is None else dict(cfg)))
    if targets:
        m.add_adapter(LoraConfig(r=4, lora_alpha=8, target_modules=list(targets)), "a")
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
    "qwen_q_only": lambda: _qwen_plan(_qwen(targets=("to_q",))),      # per-section dA, no fused q/k/v head projection
    "qwen_ff": lambda: _qwen_plan(_qwen(targets=FF)),
    "qwen_cond": lambda: _qwen_plan(_qwen(targets=COND)),
    "qwen_embed": lambda: _qwen_plan(_qwen(targets=EMBED)),           # stand-alone sites, in_grad, the full backward of block 0
    "qwen_head_lora": lambda: _qwen_plan(_qwen(), T=16),        # T % 16 == 0: rank-r projections in the attention epilogues
    "qwen_multires": lambda: _qwen_multires(_qwen()),
    "qwen_mxfp8": lambda: _qwen_plan(_qwen(W1024, r=8, quant="mxfp8"), shapes=((1, 12, 12), (1, 12, 12)), T=40),
    "qwen_mxfp8_fb": lambda: _qwen_plan(_qwen(W1024, r=8, quant="mxfp8-fb"), shapes=((1, 12, 12), (1, 12, 12)), T=40),
    "flux_plain": lambda: _flux_plan(_flux(targets=None)),            # the two-segment proj_out of the single block
    "flux_attn": lambda: _flux_plan(_flux()),
    "flux_q_only": lambda: _flux_plan(_flux(targets=("to_q",))),      # per-section dA in both block kinds
    "flux_all": lambda: _flux_plan(_flux(targets=FLUX_ALL)),
    "flux_cond": lambda: _flux_plan(_flux(targets=FLUX_COND)),
    "flux_single_only": lambda: _flux_plan(_flux(num_layers=0)),
    "flux_double_only": lambda: _flux_plan(_flux(num_single_layers=0)),
    "flux_multires": lambda: _flux_multires(_flux()),
    "flux_mxfp8_fb": lambda: _flux_plan(_flux(FLUX_W1024, quant="mxfp8-fb"), hw=(8, 8), T=16),
}
# a plan once more with one lever switched off, on the configuration where that lever changes the programs
for _base, _name in (("qwen_attn", "QFX_SIDE_GRADS"), ("qwen_attn", "QFX_FUSE_QKNORM_BWD"), ("qwen_attn", "QFX_FUSE_LN_DOWN"),
                     ("qwen_attn", "QFX_LN_DOWN_FRAG"), ("qwen_attn", "QFX_GRAD_DET"), ("qwen_ff", "QFX_SIDE_GRADS"),
                     ("qwen_ff", "QFX_SIDE_GRADS_FF"), ("qwen_mxfp8", "QFX_FP8_FUSED_QUANT"), ("qwen_head_lora", "QFX_FUSE_HEAD_LORA"),
                     ("qwen_head_lora", "QFX_FUSE_QKNORM_BWD")):
    CONFIGS[f"{_base},{_name}=0"] = CONFIGS[_base]


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


class _HostDevice(str):
    """Device of a dry-run model: names host memory to every tensor factory, answers "cuda" where a builder checks `.type`."""
    type = "cuda"


@contextlib.contextmanager
def dry_run():
    """Build models and plans in host memory, with no GPU: CPU tensors; the models' `device` property (the GPU-only assertion of
    `_prepare` reads it) answers with a host device of type "cuda"; `ops.side_stream` is stubbed; `ops.quant_mxfp8`, the
    device-side weight quantiser the MX-FP8 builder calls, returns buffers of the right shape.  Plans are only built, nothing is
    launched, so the emitted calls and argument bytes are what a GPU build emits."""
    global DEVICE
    import torch
    from qflux_amd import ops
    from qflux_amd.models import QwenImageTransformer2DModel as Model      # (the FLUX model inherits `device`)

    def quant_shapes(x, M=None, **_):
        M, K = (x.shape[0] if M is None else M), x.shape[1]
        return torch.empty(M, K, dtype=torch.uint8), torch.empty(K // 128, M, 4, dtype=torch.uint8)

    saved = DEVICE, Model.device, ops.side_stream, ops.quant_mxfp8
    DEVICE, Model.device = "cpu", property(lambda self: _HostDevice("cpu"))
    ops.side_stream, ops.quant_mxfp8 = (lambda device: None), quant_shapes
    try:
        yield
    finally:
        DEVICE, Model.device, ops.side_stream, ops.quant_mxfp8 = saved


def digest_or_refusal(config: str):
    """-> (sha256 | "refused: <message>", number of entries) of a named configuration."""
    try:
        fp = fingerprint(build(config))
    except NotImplementedError as e:
        return f"refused: {e}", 0
    return digest(fp), len(fp["calls"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dry-run", action="store_true", help="build in host memory, without a GPU (see dry_run)")
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
    with dry_run() if a.dry_run else contextlib.nullcontext():
        for name in (list(CONFIGS) if a.all else [a.config]):
            hashes[name], n = digest_or_refusal(name)
            print(json.dumps({"config": name, "entries": n, "sha256": hashes[name],
                              **({"fingerprint": fingerprint(build(name))} if a.full and n else {})}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(hashes, f, indent=1)


if __name__ == "__main__":
    main()
