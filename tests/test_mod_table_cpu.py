"""CPU: argument validation of the modulation-table entry points (no launch), the levers and the size formula."""
import pytest

from parity_util import ROOT  # noqa: F401  (puts the repository root and the package on sys.path)

P = 0x10000          # an aligned, never dereferenced "device pointer"


def _fetch(**kw):
    from qflux_amd import _lib
    a = dict(t=P, B=2, keys=P, n=5, tbl_mods=P, ld_mods=400, nmat=4, N=100, tbl_out=P, ld_out=50, N_out=50, mods=P, mod_out=P, hit=P)
    a.update(kw)
    return _lib.lib.qfx_mod_table_fetch(a["t"], a["B"], a["keys"], a["n"], a["tbl_mods"], a["ld_mods"], a["nmat"], a["N"], a["tbl_out"],
                                        a["ld_out"], a["N_out"], a["mods"], a["mod_out"], a["hit"], None)


@pytest.mark.parametrize("bad", [dict(B=9), dict(B=0), dict(n=0), dict(n=-3), dict(t=None), dict(keys=None), dict(tbl_mods=None),
                                 dict(tbl_out=None), dict(mods=None), dict(mod_out=None), dict(hit=None), dict(nmat=0), dict(N=0),
                                 dict(N_out=0), dict(ld_mods=399), dict(ld_out=49), dict(mods=P + 2), dict(tbl_out=P + 8), dict(hit=P + 1)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_fetch_rejects_bad_arguments_before_any_launch(bad):
    from qflux_amd import _lib
    assert _fetch(**bad) == _lib.QFX_EINVAL


def test_guarded_gemv_rejects_what_the_plain_one_rejects():
    from qflux_amd import _lib
    f, g = _lib.lib.qfx_mod_gemv_unless, _lib.lib.qfx_mod_gemv
    for B, K, W, nmat, N, temb, out in ((9, 64, P, 1, 100, P, P), (0, 64, P, 1, 100, P, P), (2, 60, P, 1, 100, P, P), (2, 64, None, 1, 100, P, P),
                                        (2, 64, P, 0, 100, P, P), (2, 64, P, 1, 0, P, P), (2, 64, P, 1, 100, None, P), (2, 64, P, 1, 100, P, None)):
        assert f(temb, B, K, W, None, nmat, N, 1, out, P, None) == _lib.QFX_EINVAL
        assert f(temb, B, K, W, None, nmat, N, 1, out, None, None) == _lib.QFX_EINVAL
        assert g(temb, B, K, W, None, nmat, N, 1, out, None) == _lib.QFX_EINVAL
    assert f(P, 8, 8192, P, None, 1, 100, 1, P, P, None) == _lib.QFX_EUNSUPPORTED      # 8 rows of 8192 do not fit the LDS


def test_levers_and_size_formula():
    from qflux_amd import levers
    from qflux_amd.models import QwenImageTransformer2DModel as M
    lv = M.modulation_table_levers
    assert lv({}) == (True, 8.0)
    assert lv({"QFX_MOD_TABLE": "0"}) == (False, 8.0) and lv({"QFX_MOD_TABLE": "1"})[0] and lv({"QFX_MOD_TABLE": ""})[0]
    assert lv({"QFX_MOD_TABLE_GB": "2.5"}) == (True, 2.5) and lv({"QFX_MOD_TABLE_GB": "0"}) == (True, 0.0)
    for bad in ("-1", "nan", "lots"):
        with pytest.raises(ValueError):
            lv({"QFX_MOD_TABLE_GB": bad})
    assert not any("MOD_TABLE" in name for name in levers.TABLE)      # read by the model, not a plan lever
    # the headline model: 60 blocks, D = 3072, the 1000 training timesteps -> 4.44 GB under the default cap; one key: 4.44 MB
    assert M.modulation_table_bytes(1, 60, 3072) == (120 * 18432 + 6144) * 2 == 4435968
    assert M.modulation_table_bytes(1000, 60, 3072) == 4435968000 < 8e9
    assert M.modulation_table_bytes(1000, 2, 256) == 1000 * (4 * 1536 + 512) * 2


def test_keys_default_to_the_training_timesteps_and_can_be_set():
    import torch
    from common import TINY
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.trainer.qwen_step import flowmatch_tables
    m = QwenImageTransformer2DModel(**TINY)
    assert torch.equal(m._modulation_keys(), flowmatch_tables()[0] / 1000) and m._modulation_keys().numel() == 1000
    m.set_modulation_keys([0.25, 0.5])
    assert m._modulation_keys().tolist() == [0.25, 0.5] and m._modulation_keys().dtype == torch.float32
    with pytest.raises(ValueError):
        m.set_modulation_keys([])
    assert m.ensure_modulation_table() is False and m.modulation_table is None      # no table off the GPU
