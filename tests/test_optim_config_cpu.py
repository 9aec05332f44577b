"""CPU: optimizer_kwargs_from_config pinned case by case against tests/golden/optimizer_kwargs_cases.json, which was recorded from
the function as it stood before it moved out of the train-step module.  The case list lives here; the fixture holds, per case id,
either the returned dict (tuples, None and non-finite floats tagged so that JSON keeps them apart) or the exception's type and
full message."""
import json
import math
import os

import pytest

COMMON = {"lr": 2e-4, "betas": [0.8, 0.95], "eps": 1e-6, "weight_decay": 0.05}
KNOBS = {"min_8bit_size": 1024, "percentile_clipping": 100, "block_wise": True, "optim_bits": 32, "is_paged": False, "amsgrad": False,
         "foreach": None, "fused": None}
# kind -> {case name: init_args}: "full*" = every keyword the kind accepts, every other name = one refused keyword (or refused pair)
KINDS = {
    "fp32": {"full": dict(COMMON, **KNOBS)},
    "blockwise": {"full": dict(COMMON, percentile_clipping=100, max_unorm=0.0, block_wise=True, skip_zeros=False, amsgrad=False,
                               min_8bit_size=2048, is_paged=True, optim_bits=32, foreach=None, fused=None),
                  "percentile_clipping": {"percentile_clipping": 5}, "max_unorm": {"max_unorm": 1.0}, "block_wise": {"block_wise": False},
                  "skip_zeros": {"skip_zeros": True}, "amsgrad": {"amsgrad": True}, "blocksize": {"blocksize": 2048},
                  "two_refused": {"amsgrad": True, "percentile_clipping": 5}, "refused_and_unknown": {"max_unorm": 1.0, "bogus": 1}},
    "lion": {"full": dict(COMMON, use_triton=True, decoupled_weight_decay=False, cautious_factor=1.0, foreach=None),
             "decoupled_weight_decay": {"decoupled_weight_decay": True}, "cautious_factor": {"cautious_factor": 0.5},
             "two_refused": {"cautious_factor": 0.5, "decoupled_weight_decay": True}, "refused_and_unknown": {"cautious_factor": 0.5, "bogus": 1}},
    "sgd": {"full": {"lr": 1e-3, "weight_decay": 1e-4, "momentum": 0.9, "dampening": 0.0, "nesterov": True, "maximize": False,
                     "differentiable": False, "foreach": None, "fused": None},
            "maximize": {"maximize": True}, "refused_and_unknown": {"maximize": True, "bogus": 1},
            "invalid_for_torch": {"momentum": 0.0, "nesterov": True}},
    "prodigy": {"full": dict(COMMON, lr=1.0, beta3=0.99, decouple=False, use_bias_correction=True, safeguard_warmup=True, d0=1e-5, d_coef=2.0,
                             growth_rate=float("inf"))},
    "adafactor": {"full": {"eps": [1e-30, 1e-3], "clip_threshold": 1.5, "decay_rate": -0.7, "beta1": 0.9, "scale_parameter": False,
                           "relative_step": True, "warmup_init": True, "weight_decay": 0.01, "lr": None},
                  "full_with_lr": {"lr": 1e-3, "relative_step": False, "scale_parameter": False, "eps": (1e-30, 1e-3), "foreach": None},
                  "betas": {"betas": [0.9, 0.999]}, "lr_with_relative_step": {"lr": 1e-3}, "warmup_without_relative_step":
                  {"lr": 1e-3, "relative_step": False, "warmup_init": True}, "no_lr_without_relative_step": {"relative_step": False},
                  "clip_threshold": {"clip_threshold": 0.0}, "beta1": {"beta1": 1.0}, "eps_not_a_pair": {"eps": [1e-30]},
                  "betas_and_unknown": {"betas": [0.9, 0.999], "bogus": 1}, "betas_and_lr": {"betas": [0.9, 0.999], "lr": 1e-3},
                  "lr_and_unknown": {"lr": 1e-3, "bogus": 1}},
    "muon": {"full": {"lr": 2e-2, "weight_decay": 0.05, "momentum": 0.9, "nesterov": False, "ns_coefficients": [3.0, -4.0, 2.0], "eps": 1e-6,
                      "ns_steps": 4, "adjust_lr_fn": "match_rms_adamw", "foreach": None},
             "betas": {"betas": [0.9, 0.95]}, "ns_steps": {"ns_steps": 100}, "adjust_lr_fn": {"adjust_lr_fn": "bogus"},
             "momentum": {"momentum": -0.1}, "ns_coefficients": {"ns_coefficients": [1.0, 2.0]}, "eps": {"eps": 0.0},
             "betas_and_unknown": {"betas": [0.9, 0.95], "bogus": 1}, "betas_and_ns_steps": {"betas": [0.9, 0.95], "ns_steps": 100},
             "ns_steps_and_unknown": {"ns_steps": 100, "bogus": 1}},
    "schedulefree": {"full": dict(COMMON, warmup_steps=10, r=0.5, weight_lr_power=1.0, foreach=True),
                     "warmup_steps": {"warmup_steps": -1}, "refused_and_unknown": {"warmup_steps": -1, "bogus": 1}},
}
# every class path the function accepts -> the kinds whose cases it is run with (both state_bits values each)
PATHS = {
    "torch.optim.AdamW": ["fp32"], "bitsandbytes.optim.AdamW": ["fp32"], "qflux_amd.optim.AdamW": ["fp32"],
    "torch.optim.Adam": ["fp32"], "bitsandbytes.optim.Adam": ["fp32"], "qflux_amd.optim.Adam": ["fp32"],
    "bitsandbytes.optim.Adam8bit": ["fp32", "blockwise"], "bitsandbytes.optim.PagedAdam8bit": ["fp32", "blockwise"],
    "bitsandbytes.optim.AdamW8bit": ["fp32", "blockwise"], "bitsandbytes.optim.PagedAdamW8bit": ["fp32", "blockwise"],
    "qflux_amd.optim.Adam8bit": ["fp32", "blockwise"], "qflux_amd.optim.AdamW8bit": ["fp32", "blockwise"],
    "lion_pytorch.Lion": ["lion"], "bitsandbytes.optim.Lion": ["lion"], "bitsandbytes.optim.Lion32bit": ["lion"],
    "bitsandbytes.optim.Lion8bit": ["lion", "blockwise"], "bitsandbytes.optim.PagedLion8bit": ["lion", "blockwise"],
    "qflux_amd.optim.Lion8bit": ["lion", "blockwise"], "qflux_amd.optim.PagedLion8bit": ["lion", "blockwise"],
    "prodigyopt.Prodigy": ["prodigy"], "qflux_amd.optim.Prodigy": ["prodigy"], "qflux_amd.optim.SGD": ["sgd"],
    "transformers.optimization.Adafactor": ["adafactor"], "transformers.Adafactor": ["adafactor"], "qflux_amd.optim.Adafactor": ["adafactor"],
    "torch.optim.Muon": ["muon"], "qflux_amd.optim.Muon": ["muon"],
    "schedulefree.AdamWScheduleFree": ["schedulefree"], "qflux_amd.optim.AdamWScheduleFree": ["schedulefree"],
    # not mapped: an unknown class, torch's own SGD, the package's own Lion path
    "somepackage.optim.Unknown": ["fp32"], "torch.optim.SGD": ["sgd"], "qflux_amd.optim.Lion": ["lion"],
}


def cases():
    """[(case id, class path, init_args, state_bits)]"""
    out = []
    for path, kinds in PATHS.items():
        for bits in (8, 32):
            sets = {"empty": {}, "none": None, "unknown": {"bogus": 1}, "unknown_two": {"zeta": 1, "alpha": 2}, "lr_only": {"lr": 1e-4},
                    "lr_not_a_number": {"lr": "fast", "bogus": 1}}
            for kind in kinds:
                sets.update({f"{kind}.{n}": a for n, a in KINDS[kind].items()})
            out += [(f"{path}|{bits}|{n}", path, a, bits) for n, a in sets.items()]
    out += [(f"{path}|{bits!r}|bad_state_bits", path, {"lr": 1e-4}, bits) for path in ("torch.optim.AdamW", "somepackage.optim.Unknown")
            for bits in (16, 0, None, "8")]
    return out


def encode(v):
    if isinstance(v, dict):
        return {k: encode(x) for k, x in v.items()}
    if isinstance(v, tuple):
        return {"tuple": [encode(x) for x in v]}
    if isinstance(v, list):
        return [encode(x) for x in v]
    if v is None:
        return {"py": "None"}
    if isinstance(v, float) and not math.isfinite(v):
        return {"py": repr(v)}
    return v


def run(path, init_args, bits):
    from qflux_amd.trainer import optimizer_kwargs_from_config
    given = None if init_args is None else dict(init_args)
    try:
        out = {"returns": encode(optimizer_kwargs_from_config(path, init_args, state_bits=bits))}
    except Exception as e:  # noqa: BLE001 -- the type and the message are what is recorded
        out = {"raises": type(e).__name__, "message": str(e)}
    assert init_args == given, "the caller's init_args were modified"
    return out


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "optimizer_kwargs_cases.json")) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases_listed_here(recorded):
    ids = [c[0] for c in cases()]
    assert len(ids) == len(set(ids)) and set(ids) == set(recorded)
    for path, kinds in PATHS.items():      # the coverage asked of the list: empty, full, every refusal alone, one unknown keyword
        assert all(f"{path}|{b}|{n}" in recorded for b in (8, 32) for n in ["empty", "unknown"] + [f"{k}.full" for k in kinds])


def test_every_case_equals_the_recorded_result(recorded):
    wrong = {}
    for cid, path, init_args, bits in cases():
        got = run(path, init_args, bits)
        if json.dumps(got, sort_keys=True) != json.dumps(recorded[cid], sort_keys=True):     # as text: 0 is not 0.0, 1 is not True
            wrong[cid] = (got, recorded[cid])
    assert not wrong, f"{len(wrong)} of {len(cases())} cases differ, the first: {next(iter(wrong.items()))}"
