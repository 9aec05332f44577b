"""GPU: qfx_sgd_step against the installed torch.optim.SGD in fp32 on the CPU (4 steps), its determinism and its argument checks.

Bar: max |d| <= 1e-5 of the tensor's maximum, the bar test_kernels_gpu.py::test_adamw_matches_torch applies to the fp32 AdamW kernel
against torch.  What separates the two sides is fused multiply-add contraction (one rounding less per product on the device) over 4
steps of fp32 arithmetic: a few 1e-7 (profiles/sgd_step.json records the observed maximum)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-5
SIZES = [1, 255, 257, 4096 * 256 + 3]          # tails around one block; the last: a second grid-stride trip past the 4096-block cap
CASES = {
    "plain": dict(),
    "momentum": dict(momentum=0.9),
    "dampening": dict(momentum=0.9, dampening=0.1),          # the first step applies no dampening
    "nesterov": dict(momentum=0.9, nesterov=True),
    "weight_decay": dict(momentum=0.9, weight_decay=1e-4),
    "no_buffer": dict(momentum=0.0, weight_decay=1e-4),       # buf = NULL
    "clip": dict(momentum=0.9, weight_decay=1e-4, max_norm=None, grad_scale=0.5),      # max_norm: half the smallest gradient norm
}
LR, STEPS = 0.05, 4


def _data(n):
    g = torch.Generator().manual_seed(1000 + n % 997)
    return torch.randn(n, generator=g), [torch.randn(n, generator=g) * (1 + s) for s in range(STEPS)]


def _run_kernel(p0, grads, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, max_norm=0.0, grad_scale=1.0):
    from qflux_amd import ops
    p = p0.clone().to(DEV)
    buf = torch.full_like(p, float("nan")) if momentum else None       # the first step must ignore what the buffer holds
    nsq, parts = torch.zeros((), device=DEV), torch.zeros(1024, device=DEV)
    for s, g in enumerate(grads):
        gd = g.to(DEV)
        if max_norm > 0:
            ops.sumsq_det(gd, nsq, parts)
        ops.sgd_step(p, gd, buf, LR, momentum, dampening, weight_decay, nesterov, first=(s == 0), gnorm_sq=nsq if max_norm > 0 else None,
                     max_norm=max_norm, grad_scale=grad_scale)
        assert torch.equal(gd.cpu(), g)          # the gradient is read only
    return p.cpu(), None if buf is None else buf.cpu()


def _run_torch(p0, grads, max_norm=0.0, grad_scale=1.0, **kw):
    """torch.optim.SGD on the CPU; with a clip, the step of the reference's loop restated: the summed gradient times grad_scale
    (the data-parallel mean), clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)), then optimizer.step().  The norm is
    formed in fp64 and rounded to fp32: torch's fp32 Tensor.norm() on the CPU is itself 1.0e-5 to 1.3e-5 below the true norm of these
    2^20-element gradients (measured against fp64), which is the whole bar and enters every element of the momentum buffer through
    the coefficient; qfx_sumsq_det's fixed-order sum is within 1e-7 of fp64."""
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([p], lr=LR, **kw)
    for g in grads:
        g = g * grad_scale
        if max_norm > 0:
            g = g * torch.clamp(max_norm / (g.double().norm().float() + 1e-6), max=1.0)
        p.grad = g
        opt.step()
    return p.detach(), opt.state[p].get("momentum_buffer")


def _with_max_norm(kw, grads):
    """A clip that is active at every step (coefficient <= 0.5) whatever the size, so that the update stays far above the bar."""
    if "max_norm" in kw:
        kw = dict(kw, max_norm=0.5 * min(float((g * kw["grad_scale"]).norm()) for g in grads))
    return kw


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("n", SIZES)
def test_sgd_step_matches_torch_sgd(n, case):
    p0, grads = _data(n)
    kw = _with_max_norm(CASES[case], grads)
    p, buf = _run_kernel(p0, grads, **kw)
    p_ref, buf_ref = _run_torch(p0, grads, **kw)
    assert torch.isfinite(p).all()
    rel = ((p - p_ref).abs().max() / p_ref.abs().max()).item()
    moved = ((p_ref - p0).abs().max() / p_ref.abs().max()).item()
    rel_b = 0.0
    if kw.get("momentum"):
        assert torch.isfinite(buf).all()
        rel_b = ((buf - buf_ref).abs().max() / buf_ref.abs().max()).item()
    else:
        assert buf is None and buf_ref is None
    print(f"sgd n={n} {case}: rel p {rel:.3e} buf {rel_b:.3e} (update {moved:.3e})")
    assert moved > 100 * BAR          # the bar is far below what a step changes
    assert rel <= BAR and rel_b <= BAR, (rel, rel_b)


def test_first_step_rule_is_what_separates_dampening():
    """With dampening the first step's buffer is g itself, not (1 - dampening) g: a kernel that ignored `first` would miss torch by
    ~dampening, five orders above the bar."""
    p0, grads = _data(257)
    _, buf = _run_kernel(p0, grads[:1], momentum=0.9, dampening=0.1)
    assert torch.equal(buf, grads[0])


def test_two_launches_on_equal_inputs_are_bit_identical():
    n = SIZES[-1]
    p0, grads = _data(n)
    kw = _with_max_norm(dict(momentum=0.9, weight_decay=1e-4, nesterov=True, max_norm=None, grad_scale=0.5), grads)
    a, b = _run_kernel(p0, grads[:2], **kw), _run_kernel(p0, grads[:2], **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_rejected_arguments_do_not_launch():
    from qflux_amd import _lib, ops
    p = torch.ones(300, device=DEV)
    g = torch.ones(300, device=DEV)
    buf = torch.zeros(300, device=DEV)
    f, s = _lib.lib.qfx_sgd_step, ops.stream_ptr()
    P, G, B = p.data_ptr(), g.data_ptr(), buf.data_ptr()
    bad = [(None, G, B, 300, 0.9, 0.0, 0), (P, None, B, 300, 0.9, 0.0, 0), (P, G, B, 0, 0.9, 0.0, 0), (P, G, B, -1, 0.9, 0.0, 0),
           (P, G, None, 300, 0.9, 0.0, 0), (P, G, B, 300, 0.0, 0.0, 1), (P, G, B, 300, -0.9, 0.0, 1), (P, G, B, 300, 0.9, 0.1, 1)]
    for pp, gg, bb, n, mom, damp, nest in bad:
        assert f(pp, gg, bb, n, 0.1, mom, damp, 0.0, nest, 0, None, 0.0, 1.0, s) == _lib.QFX_EINVAL
    with pytest.raises(_lib.QfxError):
        ops.sgd_step(p, g, None, 0.1, momentum=0.9)
    torch.cuda.synchronize()
    assert bool(p.eq(1).all()) and bool(buf.eq(0).all())
    ops.sgd_step(p, g, None, 0.5)            # momentum 0 without a buffer is legal
    assert bool(p.eq(0.5).all())
