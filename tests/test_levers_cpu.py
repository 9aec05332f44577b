"""qflux_amd/levers.py: the one table of plan levers and its immutable snapshot."""
import pytest

from parity_util import ROOT  # noqa: F401  (puts the package on sys.path)

# name -> default, as DESIGN.md section 3 states them (every fusion / side-stream / deterministic path is on by default)
EXPECTED = {"QFX_SIDE_GRADS": True, "QFX_SIDE_GRADS_FF": True, "QFX_FUSE_QKNORM_BWD": True, "QFX_FUSE_HEAD_LORA": True,
            "QFX_FUSE_LN_DOWN": True, "QFX_LN_DOWN_FRAG": True, "QFX_FP8_FUSED_QUANT": True, "QFX_GRAD_DET": True}
CHOICES = {"QFX_ATTN_BWD": "auto"}      # the levers that are not switches: taken verbatim, the last fields of the snapshot


def _clear(monkeypatch):
    for name in (*EXPECTED, *CHOICES):
        monkeypatch.delenv(name, raising=False)


def test_defaults_match_the_table(monkeypatch):
    from qflux_amd import levers
    _clear(monkeypatch)
    both = {**EXPECTED, **CHOICES}
    assert {name: default for name, default, _ in levers.TABLE} == both
    assert all(isinstance(meaning, str) and meaning for _, _, meaning in levers.TABLE)
    snap = levers.read()
    assert snap._fields == tuple(levers.field(name) for name in both)
    assert {name: getattr(snap, levers.field(name)) for name in both} == both


@pytest.mark.parametrize("value", [None, "auto", "2pass", "1pass", "0"])
def test_the_attention_backward_choice_is_taken_verbatim(monkeypatch, value):
    from qflux_amd import levers
    _clear(monkeypatch)
    if value is not None:
        monkeypatch.setenv("QFX_ATTN_BWD", value)
    snap = levers.read()
    assert snap.attn_bwd == ("auto" if value is None else value)
    assert all(getattr(snap, levers.field(name)) is True for name in EXPECTED)


@pytest.mark.parametrize("name", sorted(EXPECTED))
@pytest.mark.parametrize("value", [None, "0", "1"])
def test_each_lever_follows_the_expression_the_plan_builder_used(monkeypatch, name, value):
    """Before the table every read was `os.environ.get(NAME, "1") != "0"` (or its negation `== "0"` guarding the off branch):
    on when unset, off for "0" only.  One lever changes, the others keep their defaults."""
    import os
    from qflux_amd import levers
    _clear(monkeypatch)
    if value is not None:
        monkeypatch.setenv(name, value)
    snap = levers.read()
    for other in EXPECTED:
        assert getattr(snap, levers.field(other)) == (os.environ.get(other, "1") != "0"), other
    assert getattr(snap, levers.field(name)) == (value != "0")


def test_snapshot_is_immutable(monkeypatch):
    from qflux_amd import levers
    _clear(monkeypatch)
    snap = levers.read()
    with pytest.raises(AttributeError):
        snap.side_grads = False
    with pytest.raises(AttributeError):
        snap.new_lever = True
    with pytest.raises(TypeError):
        snap[0] = False
    assert snap.side_grads is True and hash(snap) == hash(levers.read())


def test_snapshot_does_not_see_a_later_environment_change(monkeypatch):
    from qflux_amd import levers
    _clear(monkeypatch)
    before = levers.read()
    monkeypatch.setenv("QFX_SIDE_GRADS", "0")
    monkeypatch.setenv("QFX_GRAD_DET", "0")
    after = levers.read()
    assert before.side_grads is True and before.grad_det is True
    assert after.side_grads is False and after.grad_det is False and after.fuse_ln_down is True
