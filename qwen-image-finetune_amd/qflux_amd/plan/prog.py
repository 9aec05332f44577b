"""The launch-program container and the two helpers every plan module uses."""
from __future__ import annotations

import torch

from .. import _lib as L


def _ceil(a, b):
    return (a + b - 1) // b * b


class _Prog:
    """A flat launch program: list of (callable, args); C calls get the stream appended."""

    def __init__(self):
        self.calls = []
        self.keep = []
        self.marks = []   # (call index, parameter-name prefix): every LoRA gradient under `prefix` is final after calls[:index]

    def c(self, fn, *args):
        self.calls.append((fn, args))

    def c_side(self, fn, *args):
        """C call issued on the program's side stream (leaf work that overlaps the main stream; joined by explicit events)."""
        self.calls.append((fn, args, True))

    def py(self, fn):
        self.calls.append((None, fn))

    def mark(self, prefix: str):
        self.marks.append((len(self.calls), prefix))

    side = None   # torch.cuda.Stream for c_side calls (set by the plan that uses them)

    def run(self, start: int = 0, end: int | None = None):
        st = torch.cuda.current_stream().cuda_stream
        for ent in self.calls[start:end]:
            fn, args = ent[0], ent[1]
            if fn is None:
                args()
            else:
                rc = fn(*args, st if len(ent) < 3 else self.side.cuda_stream)
                if rc != 0:
                    raise L.QfxError(f"{fn.__name__} failed with code {rc}")


def _ptr(t):
    if t is None:
        return None
    return t.data_ptr() if isinstance(t, torch.Tensor) else t
