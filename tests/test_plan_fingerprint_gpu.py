"""tools/plan_fingerprint.py on the tiny Qwen configuration with r = 4 attention adapters: building a plan is deterministic, the
fingerprint covers every call, and QFX_SIDE_GRADS decides whether any call sits on the side stream.  Plans are built, not run."""
import pytest

from parity_util import ROOT  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pf():
    from tools import plan_fingerprint
    return plan_fingerprint


@pytest.fixture(scope="module")
def default_plan(pf):
    plan = pf.build("qwen_attn")
    return plan, pf.fingerprint(plan)


def test_same_plan_twice_gives_the_same_fingerprint(pf, default_plan):
    _, fp = default_plan
    again = pf.fingerprint(pf.build("qwen_attn"))
    assert again == fp and pf.digest(again) == pf.digest(fp)


def test_one_entry_per_call(default_plan):
    plan, fp = default_plan
    assert len(fp["calls"]) == len(plan.fwd.calls) + len(plan.bwd.calls)
    assert fp["marks"]["bwd"] == [list(m) for m in plan.bwd.marks]


def test_side_stream_calls_follow_the_lever(pf, default_plan):
    plan, fp = default_plan
    assert plan.side_grads is True and any(c["side"] for c in fp["calls"])
    off = pf.build("qwen_attn,QFX_SIDE_GRADS=0")
    assert off.side_grads is False and not any(c["side"] for c in pf.fingerprint(off)["calls"])
