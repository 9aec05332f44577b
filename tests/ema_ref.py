"""Pure-torch CPU restatement of diffusers.training_utils.EMAModel's decay schedule and step, written from the published class
without looking at qflux_amd.ema: fp32 tensors, `s.sub_(one_minus_decay * (s - p))` with one_minus_decay a Python float.  The GPU
kernel (qfx_ema_update) and the stock-loop class are compared with it bit for bit."""
import torch

KEYS = {"decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power", "shadow_params"}


def get_decay(optimization_step, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3):
    step = max(0, optimization_step - update_after_step - 1)
    if step <= 0:
        return 0.0
    if use_ema_warmup:
        cur_decay_value = 1 - (1 + step / inv_gamma) ** -power
    else:
        cur_decay_value = (1 + step) / (10 + step)
    cur_decay_value = min(cur_decay_value, decay)
    cur_decay_value = max(cur_decay_value, min_decay)
    return cur_decay_value


def update(shadow, params, one_minus_decay):
    """One step of one shadow (a list of fp32 CPU tensors, in place) towards params at a given 1 - decay (a Python float)."""
    for s, p in zip(shadow, params):
        assert s.dtype == torch.float32 and p.dtype == torch.float32 and s.device.type == "cpu"
        s.sub_(one_minus_decay * (s - p))


class Ema:
    """EMAModel over CPU clones of the parameters it is given."""

    def __init__(self, params, decay=0.9999, **kw):
        self.shadow = [p.detach().cpu().float().clone() for p in params]
        self.decay, self.kw, self.optimization_step = decay, kw, 0

    def step(self, params):
        self.optimization_step += 1
        d = get_decay(self.optimization_step, self.decay, **self.kw)
        update(self.shadow, [p.detach().cpu() for p in params], 1 - d)
        return d


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))
