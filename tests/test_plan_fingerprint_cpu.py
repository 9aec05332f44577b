"""Every configuration of tools/plan_fingerprint.py, built in host memory (its dry run: nothing is launched), emits the launch
programs recorded in tests/golden/plan_fingerprints.json: a change of the plan builders that alters one call, one argument or the
order of two operands of any adapter placement fails here, without a GPU."""
import json
import os

import pytest

from parity_util import ROOT

# configurations without a recorded digest, each with its reason (only MX-FP8 ones may stand here: the dry run replaces the
# device-side weight quantiser, and that is the one stub a test run might not be able to place)
NOT_RECORDED = {}


@pytest.fixture(scope="module")
def pf():
    from tools import plan_fingerprint
    return plan_fingerprint


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "plan_fingerprints.json")) as f:
        return json.load(f)["sha256"]


def test_every_configuration_is_recorded_or_listed(pf, recorded):
    assert set(NOT_RECORDED) <= {n for n in pf.CONFIGS if "mxfp8" in n}
    assert not set(NOT_RECORDED) & set(recorded)
    assert set(pf.CONFIGS) == set(recorded) | set(NOT_RECORDED)


def test_dry_run_programs_match_the_recorded_digests(pf, recorded):
    with pf.dry_run():
        got = {name: pf.digest_or_refusal(name)[0] for name in pf.CONFIGS if name not in NOT_RECORDED}
    assert {n: (got[n], recorded[n]) for n in got if got[n] != recorded[n]} == {}
