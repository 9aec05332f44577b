"""GPU: the three blockwise 8-bit optimizer kernels (qfx_adam8bit_step, qfx_lion8bit_step, qfx_ademamix8bit_step and their _grouped
entries) against the restatement of one step from a given state (tests/blockwise8_ref.py), at both block sizes, under the exact
rule of tests/bnb8_ref.py: parameters, block maxima and the fp32 moments of small tensors bit for bit, every decided code identical,
an undecided one within one step, the undecided share within bnb8_ref.UNDECIDED_CAP.  The whole buffers are compared, so every
canary word around every tensor (p, the code planes, the fp32 moments, the block maxima) is compared with them, and g must come
back as it went in.

  stride   more table entries than two sweeps of the launch: second and third trips of the stride loop, 8-bit and fp32-mode entries
           on consecutive trips of one workgroup in both orders; plain entry, and the grouped entry with three rows against the
           restatement run once per row
  extreme  uniform codes, all-0 / all-255 / all-zero-code blocks, block maxima from the smallest normal fp32 to 1e4, a zero maximum
           over non-zero codes, moments that cross zero, the sign repair
  tails    lengths k bs + j, bs - 1, bs - 5 at every offset class the builder accepts, as 8-bit and as fp32-mode tensors
  skips    NaN / +-inf gradient elements on the lane that holds the block maximum, and in an fp32-mode tensor
  zero     step 1 from bnb's initial state; a zero block stores the code of 0.0
tests/test_blockwise8_cpu.py shows from the restatement alone that these inputs reach what they claim and keep within the cap.
Every figure is printed before it is judged and dumped as blockwise8_parity_gpu.json (kept as profiles/blockwise8_parity.json)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from parity_util import _observe  # noqa: E402
import blockwise8_ref as W  # noqa: E402
import bnb8_ref as B  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAM_BS = [(f, bs) for f in W.FAMILIES for bs in (256, 2048)]
_STATS = {"what": "tests/test_blockwise8_gpu.py: per family and block size, per case and entry: elements stepped, codes compared, the "
                  "undecided share by the restatement's rule, decided codes that differ (must be 0), the worst difference of the "
                  "parameters, block maxima and fp32 moments in ulp (must be 0), sign repairs taken, trips of the stride loop",
          "tables": {}}


def _record(fam, bs, name, entry, rec):
    _STATS["tables"].setdefault(f"{fam} bs={bs}", {})[f"{name} {entry}"] = rec
    _observe(None, None, dump=("blockwise8_parity_gpu.json", _STATS))


class Dev:
    """The device buffers of one launch, uploaded from / downloaded into a blockwise8_ref.Flat."""

    def __init__(self, fam, S, lay):
        from qflux_amd import ops
        self.fam = fam
        self.lay = ops.Adam8bitLayout(lay.table.to(DEV), lay.tensors, lay.blocksize, lay.min_8bit_size, lay.n_absmax, lay.n_fp32, lay.extent)
        self.dev = W.Flat(*(t.to(DEV) for t in S.buffers()))       # the views behind the front canaries are what the launch gets
        self.p, self.g, self.codes, self.absmax, self.m32 = self.dev.p, self.dev.g, self.dev.codes, self.dev.absmax, self.dev.m32
        self.qm = [W.QMAP[True].to(DEV), W.QMAP[False].to(DEV)]

    def launch(self, hps, t, clipargs, assign=None):
        from qflux_amd import ops
        gsq, max_norm, grad_scale = clipargs
        kw = dict(gnorm_sq=None if gsq is None else torch.tensor(gsq, dtype=torch.float32, device=DEV), max_norm=max_norm, grad_scale=grad_scale)
        bmap = None if assign is None else ops.block_group_map(self.lay, assign, len(hps), device=DEV)
        c, a, m = self.codes, self.absmax, self.m32
        if self.fam == "adam":
            rows = [(h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"]) for h in hps]
            if bmap is None:
                h = hps[0]
                ops.adam8bit_step(self.p, self.g, c[0], c[1], a[0], a[1], m[0], m[1], self.lay, *self.qm, h["lr"], h["betas"], h["eps"],
                                  h["weight_decay"], t, **kw)
            else:
                ops.adam8bit_step_grouped(self.p, self.g, c[0], c[1], a[0], a[1], m[0], m[1], self.lay, *self.qm, bmap, rows, t, **kw)
        elif self.fam == "lion":
            rows = [(h["lr"], h["betas"][0], h["betas"][1], h["weight_decay"]) for h in hps]
            if bmap is None:
                h = hps[0]
                ops.lion8bit_step(self.p, self.g, c[0], a[0], m[0], self.lay, self.qm[0], h["lr"], h["betas"], h["weight_decay"], **kw)
            else:
                ops.lion8bit_step_grouped(self.p, self.g, c[0], a[0], m[0], self.lay, self.qm[0], bmap, rows, **kw)
        else:
            ops.ademamix8bit_step(self.p, self.g, c[0:2], c[2], a[0:2], a[2], m[0:2], m[2], self.lay, *self.qm,
                                  hps if bmap is not None else hps[:1], t, block_group=bmap, **kw)
        torch.cuda.synchronize()

    def get(self):
        return W.Flat(*(t.cpu() for t in self.dev.buffers()))


def _run(fam, bs, name, grouped=False):
    """One launch of the case from its state, compared with the restatement's step under the exact rule; returns (case, state, output)."""
    c = W.case(name, bs)
    S = c.state(fam)
    want, info = c.reference(fam, grouped)
    d = Dev(fam, S, c.lay)
    d.launch(W.HPS[fam], c.t, c.clipargs_of(fam), c.assign() if grouped else None)
    got = d.get()
    entry = "grouped" if grouped else "plain"
    rec = W.compare(fam, got, want, info, (fam, bs, name, entry))
    rec["stride_trips"] = c.trips()[0]
    _record(fam, bs, name, entry, rec)
    return c, S, got


@pytest.mark.parametrize("fam,bs", FAM_BS)
def test_second_and_third_stride_trips_match_the_restatement(fam, bs):
    c, S, got = _run(fam, bs, "stride")
    assert c.trips()[0] >= 3
    last = c.entries[-1]                                           # the last tensor belongs to the last trip: it was stepped
    assert not B.same_bits(got.p[last[0]:last[0] + last[1]], S.p[last[0]:last[0] + last[1]])


@pytest.mark.parametrize("fam,bs", FAM_BS)
def test_grouped_entry_over_three_trips_matches_the_restatement_run_per_group(fam, bs):
    c, S, got = _run(fam, bs, "stride", grouped=True)
    plain = c.reference(fam, False)[0]
    assert not B.same_bits(got.p, plain.p)                         # the rows do differ


@pytest.mark.parametrize("fam,bs", FAM_BS)
def test_arbitrary_and_extreme_states(fam, bs):
    c, S, got = _run(fam, bs, "extreme")
    for j in range(len(W.PLANES[fam])):                            # both end codes were written by the kernel
        new = got.codes[j][c.X.pos]
        assert bool((new == 0).any()) and bool((new == 255).any())


@pytest.mark.parametrize("fam,bs", FAM_BS)
def test_tail_arms_at_every_offset_class(fam, bs):
    _run(fam, bs, "tails8")
    _run(fam, bs, "tails32")


@pytest.mark.parametrize("fam,bs", FAM_BS)
def test_non_finite_gradient_elements_are_skipped_and_still_hold_the_block_maximum(fam, bs):
    c, S, got = _run(fam, bs, "skips")
    off0, a0 = c.entries[0][0], c.lay.tensors[0][3]
    for b in range(3):
        i = off0 + b * bs + W.SKIP_AT
        assert B.same_bits(got.p[i], S.p[i])
        for j in range(len(W.PLANES[fam])):
            assert got.codes[j][i] == 255 and B.same_bits(got.absmax[j][a0 + b], S.absmax[j][a0 + b])
    off1, s1 = c.entries[1][0], c.lay.tensors[1][5]
    for i in (5, 50):
        assert B.same_bits(got.p[off1 + i], S.p[off1 + i]) and B.same_bits(got.m32[:, s1 + i], S.m32[:, s1 + i])


@pytest.mark.parametrize("fam,bs", FAM_BS)
def test_first_step_from_zero_state(fam, bs):
    c, S, got = _run(fam, bs, "zero")
    off0, a0 = c.entries[0][0], c.lay.tensors[0][3]
    for j, sg in enumerate(W.PLANES[fam]):                         # a zero block stores the code of 0.0, in every family and state
        assert got.absmax[j][a0 + 1] == 0 and (got.codes[j][off0 + bs:off0 + 2 * bs] == W.ZERO_CODE[sg]).all()
