"""CPU: parameter groups in the fused optimizers -- constructors, refusals, the tile / block group maps, the train steps' regex
rules, the LoRA+ helper, torch's checkpoint numbering and the argument validation of the grouped C entry points (no launch)."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

from test_sgd_cpu import toy_model

ACCEPTING = [("AdamW", {}), ("Adam", {}), ("Adam8bit", {}), ("AdamW8bit", {"blocksize": 2048}), ("SGD", {"momentum": 0.9}), ("Lion", {}),
             ("Lion8bit", {}), ("PagedLion8bit", {})]
REFUSING = [("Prodigy", {}), ("Adafactor", {}), ("Muon", {}), ("AdamWScheduleFree", {})]
SIZES, ASSIGN = [1, 63, 64, 65, 4099], [0, 1, 0, 2, 1]


def _params(toy):
    return [p for n, p in toy.named_parameters() if "lora_" in n]


def _two(toy):
    ps = _params(toy)
    return [{"params": ps[0::2], "lr": 1e-4}, {"params": ps[1::2], "lr": 1.6e-3, "weight_decay": 0.0}]


@pytest.mark.parametrize("name,kw", ACCEPTING, ids=[c[0] for c in ACCEPTING])
def test_accepting_classes_take_two_groups(name, kw):
    from qflux_amd import optim as O
    toy = toy_model()
    opt = getattr(O, name)(_two(toy), **kw)
    assert isinstance(opt, torch.optim.Optimizer) and [g["lr"] for g in opt.param_groups] == [1e-4, 1.6e-3]
    assert opt.param_groups[1]["weight_decay"] == 0.0
    st = toy.lora_store
    members = opt._members(st)
    assert members == (tuple(range(0, len(st.entries), 2)), tuple(range(1, len(st.entries), 2)))
    # the grouping is part of the layout key; re-grouping rebuilds the map and keeps the moments
    state = opt._ensure_state(st)
    assert state.key == opt._cls.layout_key(st, opt._args, members) != opt._cls.layout_key(st, opt._args)
    assert state.group_map is not None and state.group_map.dtype == torch.uint8
    first = [b for _, b in state.buffers()][0]
    from qflux_amd.trainer import optim_state as OS
    swapped = OS.ensure_state(opt._cls, state, st, opt._args, members[::-1])
    assert swapped is state and [b for _, b in state.buffers()][0] is first and state.members == members[::-1]
    assert OS.ensure_state(opt._cls, state, st, opt._args, None).group_map is None


@pytest.mark.parametrize("name,kw", REFUSING, ids=[c[0] for c in REFUSING])
def test_refusing_families_name_themselves(name, kw):
    from qflux_amd import optim as O
    from qflux_amd.trainer import QwenLoraTrainStep
    toy = toy_model()
    with pytest.raises(NotImplementedError, match=name):
        getattr(O, name)(_two(toy), **kw)
    family = {"Prodigy": "prodigy", "Adafactor": "adafactor", "Muon": "muon", "AdamWScheduleFree": "adamw_schedulefree"}[name]
    with pytest.raises(NotImplementedError, match=name):
        QwenLoraTrainStep(toy, lr=None if family == "adafactor" else 1e-3, optimizer=family,
                          param_groups=[{"match": "lora_A"}, {"match": "lora_B"}])


def test_group_errors_name_the_group():
    from qflux_amd import optim as O
    toy, other = toy_model(), toy_model()
    ps = _params(toy)
    with pytest.raises(ValueError, match=r"parameter 0 \(shape .*\) of parameter group 1 is in parameter group 0 already"):
        O.AdamW([{"params": ps[:7]}, {"params": ps[6:]}])
    with pytest.raises(ValueError, match=r"of the model is missing from all 2 parameter groups"):
        O.AdamW([{"params": ps[:6]}, {"params": ps[7:]}])
    with pytest.raises(ValueError, match=r"parameter 6 \(shape \(3, 5\)\) of parameter group 1 is not an adapter parameter"):
        O.SGD([{"params": ps[:6]}, {"params": ps[6:] + [nn.Parameter(torch.zeros(3, 5))]}])
    with pytest.raises(ValueError, match=r"parameter 0 .* of parameter group 1 belongs to another model"):
        O.Lion([{"params": ps}, {"params": _params(other)}])
    with pytest.raises(ValueError, match="at most 16"):
        O.AdamW([{"params": [p]} for p in _params(toy_model(n_blocks=5))])          # 20 groups
    opt = O.AdamW(_two(toy))
    opt._step_count_fused = 1
    with pytest.raises(RuntimeError, match="add_param_group after the first step"):
        opt.add_param_group({"params": [nn.Parameter(torch.zeros(2))]})


def _hand_layout():
    entries, off = [], 0
    for k in SIZES:
        entries.append((off, k))
        off += (k + 63) // 64 * 64
    return entries, off


def test_tile_and_block_group_maps_on_a_hand_made_layout():
    from qflux_amd import _lib as L
    from qflux_amd import ops
    entries, n = _hand_layout()
    assert [off for off, _ in entries] == [0, 64, 128, 192, 320] and n == 4480
    tg = ops.tile_group_map(entries, ASSIGN, 3, numel=n)
    assert tg.dtype == torch.uint8 and tg.numel() == n // 64
    for i, ((off, k), gi) in enumerate(zip(entries, ASSIGN)):
        end = entries[i + 1][0] if i + 1 < len(entries) else n
        assert (tg[off // 64:end // 64] == gi).all()        # every tile of the tensor, the pad tail and pad tiles behind it included
    assert tg.tolist()[:5] == [0, 1, 0, 2, 2]                # the 65-element tensor owns its second tile and that tile's tail
    # a gap of whole tiles belongs to the tensor before it
    assert ops.tile_group_map([(0, 10), (256, 10)], [1, 0], 2, numel=320).tolist() == [1, 1, 1, 1, 0]
    for bad, msg in (((entries, [0, 1, 0, 3, 1], 3), "outside 0..2"), ((entries, ASSIGN[:4], 3), "4 group indices for 5"),
                     ((entries, ASSIGN, 17), "1 to 16"), (([(0, 10), (32, 10)], [0, 1], 2), "multiples of 64")):
        with pytest.raises(ValueError, match=msg):
            ops.tile_group_map(*bad)
    for bs in (256, 2048):
        lay = ops.adam8bit_block_table(entries, bs, 4096)
        bg = ops.block_group_map(lay, ASSIGN, 3)
        rows = (L.Adam8bitBlock * lay.n_blocks).from_buffer_copy(lay.table.numpy().tobytes())
        assert bg.numel() == lay.n_blocks == 4 + (4099 + bs - 1) // bs
        for r, gi in zip(rows, bg.tolist()):               # an entry lies inside ONE tensor, and carries that tensor's group
            owner = [i for i, (off, k) in enumerate(entries) if off <= r.off and r.off + r.len <= off + k]
            assert len(owner) == 1 and ASSIGN[owner[0]] == gi
        with pytest.raises(ValueError, match="outside 0..2"):
            ops.block_group_map(lay, [0, 1, 0, 3, 1], 3)


def test_regex_rules_first_match_wins_and_default_group():
    from qflux_amd.trainer import FluxKontextTrainStep, QwenLoraTrainStep
    toy = toy_model()
    st = toy.lora_store
    rules = [{"match": r"blocks\.0\.", "lr": 5e-4}, {"match": r"lora_B", "lr": 1.6e-3, "weight_decay": 0.0, "betas": [0.8, 0.9]},
             {"match": r"to_q\.lora_B", "lr": 9.0}]
    with pytest.raises(ValueError, match=r"param_groups\[2\].*matches no adapter parameter"):
        QwenLoraTrainStep(toy, lr=1e-4, weight_decay=0.01, param_groups=rules).param_groups_of(st)      # shadowed by rule 1
    for cls in (QwenLoraTrainStep, FluxKontextTrainStep):
        step = cls(toy, lr=1e-4, weight_decay=0.01, eps=1e-7, param_groups=rules[:2])
        rows, members = step.param_groups_of(st)
        names = [n for n, _, _, _ in st.entries]
        want = [[i for i, n in enumerate(names) if "blocks.0." in n],
                [i for i, n in enumerate(names) if "blocks.0." not in n and "lora_B" in n],
                [i for i, n in enumerate(names) if "blocks.0." not in n and "lora_B" not in n]]
        assert [list(m) for m in members] == want and all(want)
        assert [r["lr"] for r in rows] == [5e-4, 1.6e-3, 1e-4] and [r["weight_decay"] for r in rows] == [0.01, 0.0, 0.01]
        assert rows[1]["betas"] == (0.8, 0.9) and rows[0]["betas"] == rows[2]["betas"] == (0.9, 0.999) and rows[1]["eps"] == 1e-7
        step.lr = 0.5e-4                # a schedule through the train step scales every group alike
        assert [r["lr"] for r in step._scheduled_rows(rows)] == pytest.approx([2.5e-4, 0.8e-3, 0.5e-4])
    with pytest.raises(ValueError, match="'match'"):
        QwenLoraTrainStep(toy, param_groups=[{"lr": 1e-3}])
    with pytest.raises(ValueError, match="momentum"):
        QwenLoraTrainStep(toy, param_groups=[{"match": "x", "momentum": 0.9}])
    assert QwenLoraTrainStep(toy, lr=1e-4).param_groups_of(st) == (None, None)
    assert QwenLoraTrainStep(toy, lr=1e-4, param_groups=[{"match": "lora_", "lr": 1.0}]).param_groups_of(st) == (None, None)      # one group


def test_loraplus_groups():
    from qflux_amd import optim as O
    from qflux_amd.trainer import QwenLoraTrainStep
    toy = toy_model()
    a, b = O.loraplus_param_groups(toy, 1e-4, 16, weight_decay=0.01, b_weight_decay=0.0)
    named = dict(toy.named_parameters())
    name_of = {id(p): n for n, p in named.items()}
    assert a["params"] and all("lora_A" in name_of[id(p)] for p in a["params"]) and all("lora_B" in name_of[id(p)] for p in b["params"])
    assert len(a["params"]) + len(b["params"]) == len(_params(toy))
    assert (a["lr"], b["lr"], a["weight_decay"], b["weight_decay"]) == (1e-4, 1e-4 * 16, 0.01, 0.0)
    assert O.loraplus_param_groups(toy, 1e-4, 4, weight_decay=0.1)[1]["weight_decay"] == 0.1
    with pytest.raises(ValueError, match="positive"):
        O.loraplus_param_groups(toy, 1e-4, 0)
    step = QwenLoraTrainStep(toy, lr=1e-4, loraplus_lr_ratio=16)
    rows, members = step.param_groups_of(toy.lora_store)
    at = {id(p): i for i, (_, p, _, _) in enumerate(toy.lora_store.entries)}
    assert [r["lr"] for r in rows] == [1e-4, 1e-4 * 16]
    assert [list(m) for m in members] == [[at[id(p)] for p in a["params"]], [at[id(p)] for p in b["params"]]]
    with pytest.raises(ValueError, match="either"):
        QwenLoraTrainStep(toy, loraplus_lr_ratio=2, param_groups=[{"match": "x"}])


def _torch_run(groups, cls, steps=3, **kw):
    g = torch.Generator().manual_seed(9)
    copies = [dict(gr, params=[nn.Parameter(torch.randn(p.shape, generator=g) * 0.1) for p in gr["params"]]) for gr in groups]
    opt = cls(copies, **kw)
    for _ in range(steps):
        for gr in copies:
            for p in gr["params"]:
                p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt, copies


def test_state_dict_has_torchs_numbering_and_torchs_files_load():
    from qflux_amd import optim as O
    toy = toy_model()
    st = toy.lora_store
    groups = O.loraplus_param_groups(toy, 1e-4, 16, weight_decay=0.01, b_weight_decay=0.0)
    n0, n1 = len(groups[0]["params"]), len(groups[1]["params"])
    stock, copies = _torch_run(groups, torch.optim.AdamW, betas=(0.8, 0.9))
    sd = stock.state_dict()
    opt = O.AdamW(groups, lr=0.5)
    fresh = opt.state_dict()
    assert [g["params"] for g in fresh["param_groups"]] == [list(range(n0)), list(range(n0, n0 + n1))] == [g["params"] for g in sd["param_groups"]]
    assert [g["lr"] for g in fresh["param_groups"]] == [1e-4, 1e-4 * 16] and fresh["state"] == {}
    sd["param_groups"][1]["lr"] = 7e-3
    opt.load_state_dict(sd)
    assert [g["lr"] for g in opt.param_groups] == [1e-4, 7e-3] and opt.param_groups[0]["betas"] == (0.8, 0.9) and opt._step_count_fused == 3
    at = {id(p): (off, k) for _, p, off, k in st.entries}
    flat = [p for g in groups for p in g["params"]]
    for number, p in enumerate(flat):                      # moments and steps per parameter, through the groups' lists
        off, k = at[id(p)]
        assert torch.equal(opt._opt_state.m[off:off + k], sd["state"][number]["exp_avg"].reshape(-1))
        assert torch.equal(opt._opt_state.v[off:off + k], sd["state"][number]["exp_avg_sq"].reshape(-1))
    back = opt.state_dict()
    assert list(back["state"]) == list(range(n0 + n1)) and float(back["state"][n0]["step"]) == 3.0
    for number in range(n0 + n1):
        assert torch.equal(back["state"][number]["exp_avg"], sd["state"][number]["exp_avg"])
    torch.optim.AdamW([dict(g, params=c["params"]) for g, c in zip(groups, copies)]).load_state_dict(back)      # torch reads it back
    # SGD: torch's multi-group file, per-group momentum
    sgroups = [dict(groups[0], momentum=0.9), dict(groups[1], momentum=0.5)]
    ssd = _torch_run(sgroups, torch.optim.SGD, lr=0.1)[0].state_dict()
    sopt = O.SGD(sgroups, lr=0.1)
    sopt.load_state_dict(ssd)
    assert [g["momentum"] for g in sopt.param_groups] == [0.9, 0.5]
    off, k = at[id(flat[n0])]
    assert torch.equal(sopt._opt_state.buf[off:off + k], ssd["state"][n0]["momentum_buffer"].reshape(-1))
    # mismatches raise what torch raises
    with pytest.raises(ValueError, match="different number of parameter groups"):
        O.AdamW(_params(toy)).load_state_dict(sd)
    with pytest.raises(ValueError, match="different number of parameter groups"):
        opt.load_state_dict(O.AdamW(_params(toy)).state_dict())
    moved = [{"params": groups[0]["params"] + groups[1]["params"][:1]}, {"params": groups[1]["params"][1:]}]
    with pytest.raises(ValueError, match="doesn't match the size of optimizer's group"):
        O.AdamW(moved).load_state_dict(sd)


def test_one_group_file_is_what_it_was():
    """One group: the dict a single-group optimizer writes has exactly the keys and values it had before groups existed."""
    from qflux_amd import optim as O
    toy = toy_model()
    sd = O.AdamW(_params(toy), lr=1e-3).state_dict()
    assert list(sd) == ["state", "param_groups", "global_step"] and len(sd["param_groups"]) == 1
    assert list(sd["param_groups"][0]) == ["lr", "betas", "eps", "weight_decay", "amsgrad", "params"]
    assert sd["param_groups"][0]["params"] == list(range(len(_params(toy))))


def test_grouped_entry_points_validate_their_arguments():
    """Rejected with QFX_EINVAL before any launch (no device here): NULL pointers, 0 and 17 groups, a negative lr, a beta of 1.0."""
    from qflux_amd import _lib as L
    lib, P = L.lib, 0x1000
    assert lib.qfx_grouped_sweep_elems(0) == 4096 * 256 * 4 and lib.qfx_grouped_sweep_elems(256) == 2048 * 4 * 256
    assert lib.qfx_grouped_sweep_elems(2048) == 2048 * 2048 and lib.qfx_grouped_sweep_elems(7) == -1

    def rows(ct, *vals):
        return (ct * max(1, len(vals)))(*[ct(*v) for v in vals])
    ok_a = (1e-3, 0.9, 0.999, 1e-8, 0.01, 0.1, 0.001)
    aw = lambda p, g, m, v, tg, r, n: lib.qfx_adamw_step_grouped(p, g, m, v, 64, tg, r, n, None, 0.0, 1.0, None)      # noqa: E731
    good = rows(L.AdamwGroup, ok_a)
    for args in ((0, P, P, P, P, good, 1), (P, 0, P, P, P, good, 1), (P, P, 0, P, P, good, 1), (P, P, P, 0, P, good, 1), (P, P, P, P, 0, good, 1),
                 (P, P, P, P, P, None, 1), (P, P, P, P, P, good, 0), (P, P, P, P, P, rows(L.AdamwGroup, *[ok_a] * 17), 17),
                 (P, P, P, P, P, rows(L.AdamwGroup, (-1e-3,) + ok_a[1:]), 1), (P, P, P, P, P, rows(L.AdamwGroup, (1e-3, 1.0) + ok_a[2:]), 1),
                 (P, P, P, P, P, rows(L.AdamwGroup, ok_a[:2] + (1.0,) + ok_a[3:]), 1), (P, P, P, P, P, rows(L.AdamwGroup, ok_a[:3] + (-1e-8,) + ok_a[4:]), 1),
                 (P, P, P, P, P, rows(L.AdamwGroup, ok_a[:4] + (-0.1,) + ok_a[5:]), 1), (P, P, P, P, P, rows(L.AdamwGroup, ok_a, (float("nan"),) + ok_a[1:]), 2)):
        assert aw(*args) == -1, args
    ok_s = (0.1, 0.9, 0.0, 1e-4, 0)
    sg = lambda p, g, b, tg, r, n: lib.qfx_sgd_step_grouped(p, g, b, 64, tg, r, n, 0, None, 0.0, 1.0, None)      # noqa: E731
    for args in ((0, P, P, P, rows(L.SgdGroup, ok_s), 1), (P, P, P, 0, rows(L.SgdGroup, ok_s), 1), (P, P, P, P, rows(L.SgdGroup, ok_s), 0),
                 (P, P, P, P, rows(L.SgdGroup, *[ok_s] * 17), 17), (P, P, P, P, rows(L.SgdGroup, (-0.1,) + ok_s[1:]), 1),
                 (P, P, 0, P, rows(L.SgdGroup, (0.1, 0.0, 0.0, 0.0, 0), ok_s), 2),                  # no buffer, a group with momentum
                 (P, P, P, P, rows(L.SgdGroup, (0.1, 0.9, 0.1, 0.0, 1)), 1), (P, P, P, P, rows(L.SgdGroup, (0.1, 0.9, 0.0, -1e-4, 0)), 1)):
        assert sg(*args) == -1, args
    ok_l = (1e-4, 0.9, 0.99, 0.0)
    lg = lambda p, g, m, tg, r, n: lib.qfx_lion_step_grouped(p, g, m, 64, tg, r, n, None, 0.0, 1.0, None)      # noqa: E731
    for args in ((0, P, P, P, rows(L.LionGroup, ok_l), 1), (P, P, P, 0, rows(L.LionGroup, ok_l), 1), (P, P, P, P, None, 1),
                 (P, P, P, P, rows(L.LionGroup, ok_l), 0), (P, P, P, P, rows(L.LionGroup, *[ok_l] * 17), 17),
                 (P, P, P, P, rows(L.LionGroup, (-1e-4,) + ok_l[1:]), 1), (P, P, P, P, rows(L.LionGroup, (1e-4, 1.0, 0.99, 0.0)), 1),
                 (P, P, P, P, rows(L.LionGroup, ok_l, (1e-4, 0.9, 0.99, -0.1)), 2)):
        assert lg(*args) == -1, args
    a8 = L.Adam8bitArgs(*([P] * 9), 4, 256, P, P, 0.0, 0.0, 0.0, 0.0, 0.0, 1, None, 0.0, 1.0)
    ok_8 = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    f8 = lib.qfx_adam8bit_step_grouped
    assert f8(None, P, rows(L.Adam8bitGroup, ok_8), 1, None) == -1 and f8(C.byref(a8), None, rows(L.Adam8bitGroup, ok_8), 1, None) == -1
    assert f8(C.byref(a8), P, None, 1, None) == -1 and f8(C.byref(a8), P, rows(L.Adam8bitGroup, ok_8), 0, None) == -1
    assert f8(C.byref(a8), P, rows(L.Adam8bitGroup, *[ok_8] * 17), 17, None) == -1
    assert f8(C.byref(a8), P, rows(L.Adam8bitGroup, (-1e-3,) + ok_8[1:]), 1, None) == -1
    assert f8(C.byref(a8), P, rows(L.Adam8bitGroup, ok_8, (1e-3, 0.9, 1.0, 1e-8, 0.0)), 2, None) == -1
    a8.step = 0
    assert f8(C.byref(a8), P, rows(L.Adam8bitGroup, ok_8), 1, None) == -1
    a8.step, a8.q2 = 1, None
    assert f8(C.byref(a8), P, rows(L.Adam8bitGroup, ok_8), 1, None) == -1
    l8 = L.Lion8bitArgs(P, P, P, P, P, P, 4, 256, P, 0.0, 0.0, 0.0, 0.0, None, 0.0, 1.0)
    fl = lib.qfx_lion8bit_step_grouped
    assert fl(None, P, rows(L.LionGroup, ok_l), 1, None) == -1 and fl(C.byref(l8), None, rows(L.LionGroup, ok_l), 1, None) == -1
    assert fl(C.byref(l8), P, rows(L.LionGroup, ok_l), 0, None) == -1 and fl(C.byref(l8), P, rows(L.LionGroup, *[ok_l] * 17), 17, None) == -1
    assert fl(C.byref(l8), P, rows(L.LionGroup, (-1e-4,) + ok_l[1:]), 1, None) == -1
    assert fl(C.byref(l8), P, rows(L.LionGroup, (1e-4, 0.9, 1.0, 0.0)), 1, None) == -1
    l8.blocksize = 512
    assert fl(C.byref(l8), P, rows(L.LionGroup, ok_l), 1, None) == -1


def test_ctypes_group_rows_match_the_header(tmp_path):
    """sizeof / field offsets of the group rows against include/qfx.h compiled with gcc, as tests/test_abi_cpu.py does for the argument structs."""
    import os
    import subprocess
    from qflux_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pairs = {"qfx_adamw_group": L.AdamwGroup, "qfx_sgd_group": L.SgdGroup, "qfx_lion_group": L.LionGroup, "qfx_adam8bit_group": L.Adam8bitGroup}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "qfx.h"', "int main(void) {", '  printf("%d\\n", QFX_MAX_PARAM_GROUPS);']
    for cname, ct in pairs.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        lines += [f'  printf(" %zu", offsetof({cname}, {f}));' for f, _ in ct._fields_] + ['  printf("\\n");']
    (tmp_path / "abi.c").write_text("\n".join(lines + ["  return 0;", "}"]))
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")], check=True)
    out = subprocess.run([str(tmp_path / "abi")], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert int(out[0]) == L.MAX_PARAM_GROUPS == 16
    for line in out[1:]:
        parts = line.split()
        ct = pairs[parts[0]]
        assert [int(v) for v in parts[1:]] == [C.sizeof(ct)] + [getattr(ct, f).offset for f, _ in ct._fields_], parts
