"""GPU: the optimizer's four kernels (csrc/train.hip adamw_kernel, adamw_shared_kernel, adamw_frozen_kernel<false / true>) and its
two squared sums (sqsum_kernel, sqsum_frozen_kernel) tied to each other bit for bit: all of them run one update body
(adamw_update, sqsum_sweep), and a mask that freezes nothing must give exactly what no mask gives.  The gradients are the test's
own (a fixed RNG into FineTuner.grads), no backward pass runs.

Geometry: the smallest training vector with the encoder trained among tests/geometry_cases.py, "patch 4, image 32 (Kp = 128)" on
the MID base: n = 6 742 364 = 6 330 204 (hypernetwork group) + 412 160 (shared group).  AdamW's grid is 2048 x 256 = 524 288
threads: the first group's grid-stride loop makes 12 full trips and a partial one, the second group's one partial trip.  (Every entry
of geometry_cases has n % 4 == 0, this one too; these kernels have no vector form that a remainder could miss.)"""

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, N_HYPER = 6742364, 6330204
STATE = ("params", "mu", "nu", "ema")


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import geometry_cases as gc
    from hypervla.model import HyperVLA
    return HyperVLA.from_synthetic(gc._mid(**gc.ENCODER_P64["patch 4, image 32 (Kp = 128)"]), max_batch=1)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _tuner(model, mask, **kw):
    """A FineTuner on both optimizer groups (base_weight_decay > 0: the shared group's decay and its pull towards params0 are on)
    with a state that is nowhere zero, and `mask` (uint8 [n] on the device, or None) as its frozen mask."""
    from hypervla.train import FineTuner
    ft = FineTuner(model, 1, train_encoder=True, base_weight_decay=0.05, ema_decay=0.999, ema_start_step=0, **kw)
    assert ft.n == N and ft.n_hyper == N_HYPER and N > 2048 * 256 and ft.frozen is None and ft.params0 is not None
    gen = torch.Generator().manual_seed(1234)
    ft.mu.copy_((0.01 * torch.randn(N, generator=gen)).to(torch.bfloat16))
    ft.nu.copy_(1e-4 * torch.rand(N, generator=gen) + 1e-8)
    ft.ema.copy_(ft.params + 0.001 * torch.randn(N, generator=gen).to(ft.params.device))
    ft.params0.add_(0.01)                                    # the pull towards params0 is not zero
    ft.frozen = mask
    return ft


def _after_apply(model, mask, grads):
    ft = _tuner(model, mask, clip=1e30)                      # the clip's scale is exactly 1 whatever the norm is taken over
    before = {k: getattr(ft, k).clone() for k in STATE}
    ft.grads.copy_(grads)
    assert ft.apply(lr=1e-3, base_lr=1e-4)
    torch.cuda.synchronize()
    return before, {k: getattr(ft, k).clone() for k in STATE}


def test_a_mask_that_freezes_nothing_is_no_mask(model):
    """(a) all-zero mask == no mask, and (b) elements 0, n_hyper - 1, n_hyper, n - 1 and a random tenth frozen: those keep the bits
    of params, mu, nu and ema, every other element has the bits of run (a).  Both groups, ema on, one apply()."""
    gen = torch.Generator().manual_seed(99)
    grads = torch.randn(N, generator=gen).cuda()
    before, plain = _after_apply(model, None, grads)
    assert all(not torch.equal(_bits(plain[k]), _bits(before[k])) for k in STATE)
    _, zero = _after_apply(model, torch.zeros(N, dtype=torch.uint8, device="cuda"), grads)
    for k in STATE:
        assert torch.equal(_bits(zero[k]), _bits(plain[k])), k
    mask = (torch.rand(N, generator=gen) < 0.1).to(torch.uint8)
    mask[[0, N_HYPER - 1, N_HYPER, N - 1]] = 1
    mask = mask.cuda()
    before_b, part = _after_apply(model, mask, grads)
    fz = mask.bool()
    for k in STATE:
        assert torch.equal(_bits(before_b[k]), _bits(before[k])), k           # the runs start from the same state
        assert torch.equal(_bits(part[k])[fz], _bits(before[k])[fz]), k
        assert torch.equal(_bits(part[k])[~fz], _bits(plain[k])[~fz]), k
        assert not torch.equal(_bits(plain[k])[fz], _bits(before[k])[fz]), k  # ... which the optimizer would have moved


def test_accumulate_under_a_mask_that_freezes_nothing(model):
    """(c) train_accumulate at the default clip (1.0), which bites: the running mean and the squared norm with an all-zero mask are
    those without a mask, bitwise.  The squared sums add their partial sums with atomics in any order, so the gradients are 0 and
    +-2^-6: every partial sum is a count of units of 2^-12, at most n < 2^24 of them -- exact in f32 in whatever order, and the
    clip's scale is one number."""
    gen = torch.Generator().manual_seed(7)
    grads = (torch.randint(0, 2, (N,), generator=gen).float() * 2 - 1) * (torch.rand(N, generator=gen) < 0.75).float() * 2.0 ** -6
    assert N < 2 ** 24
    out = []
    for mask in (None, torch.zeros(N, dtype=torch.uint8, device="cuda")):
        ft = _tuner(model, mask, grad_accumulation_steps=2)
        ft.grads.copy_(grads)
        assert ft.apply() is False                           # the first micro-step: accumulate only
        torch.cuda.synchronize()
        out.append((ft.acc.clone(), ft.sqsum.clone()))
    (acc0, sq0), (acc1, sq1) = out
    assert float(sq0) == float((grads.double() ** 2).sum()) and float(sq0) > 1.0
    assert torch.equal(_bits(sq1), _bits(sq0)) and torch.equal(_bits(acc1), _bits(acc0))
    assert 0 < float(acc0.abs().max()) < 2.0 ** -6 / 2                       # the clip bit
