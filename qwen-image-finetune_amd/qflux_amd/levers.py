"""The environment levers the Python side reads while it prepares a model or builds a plan -- one table, one reader.

Every switch is ON unless its variable is set to exactly "0" (unset, "", "1", anything else: on); every default is the measured-best
path.  QFX_ATTN_BWD, the one lever that is a choice and not a switch, is taken verbatim.  `read()` takes an
immutable snapshot of the current environment: a plan takes one when it is set up, a model one per `_prepare_lora` call, and neither
looks at the environment again.  Levers that libqfx.so reads itself, QFX_AUTO_DP (the model's add_adapter) and the plan-cache
variables are not part of this table.
"""
from __future__ import annotations

import os
from collections import namedtuple

# (environment variable, default, meaning when on -- of a string-valued lever: its values)
TABLE = (
    ("QFX_SIDE_GRADS", True, "the batched lora_grad launch of a block runs on a low-priority side stream"),
    ("QFX_SIDE_GRADS_FF", True, "... also in plans with feed-forward adapters"),
    ("QFX_FUSE_QKNORM_BWD", True, "QK-norm + RoPE backward in the epilogues of the attention backward kernels"),
    ("QFX_FUSE_HEAD_LORA", True, "rank-r projections of the attention adapters in the attention epilogues (needs the weight images too)"),
    ("QFX_FUSE_LN_DOWN", True, "LayerNorm + modulate and the q/k/v down projection in one launch"),
    ("QFX_LN_DOWN_FRAG", True, "MFMA-fragment-order image of the q/k/v A rows for that launch"),
    ("QFX_FP8_FUSED_QUANT", True, "MX-FP8 trunk: producers quantise their output for the GEMM that follows"),
    ("QFX_GRAD_DET", True, "lora_grad adds its token chunks in a fixed order (off: fp32 atomics)"),
    ("QFX_ATTN_BWD", "auto", "attention backward: 2pass | 1pass | auto = the measured-faster one (plan/emit.py: emit_attn_backward)"),
)


def field(env_name: str) -> str:
    """Snapshot field of a variable: QFX_SIDE_GRADS -> side_grads."""
    return env_name[len("QFX_"):].lower()


Levers = namedtuple("Levers", [field(name) for name, _, _ in TABLE])


def read(environ=None) -> Levers:
    env = os.environ if environ is None else environ
    return Levers(*(env.get(name, default) if isinstance(default, str) else env.get(name, "1" if default else "0") != "0"
                    for name, default, _ in TABLE))
