"""FusedAdamW clip mode (global-norm clipping + non-finite skip) and the
stand-alone ops.grad_norm / ops.clip_grad_norm_, on the plain-torch CPU path.
The GPU kernels are covered by test_grad_clip_gpu.py."""

import copy
import math

import pytest
import torch

HP = dict(lr=1e-2, betas=(0.9, 0.95), weight_decay=0.01, eps=1e-8)
SHAPES = [(200,), (7, 3)]


def _params(seed):
    torch.manual_seed(seed)
    return [torch.randn(*s, requires_grad=True) for s in SHAPES]


def _clones(params):
    return [p.detach().clone().requires_grad_(True) for p in params]


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = g.clone()


def _ref_step(ref, ref_opt, grads, max_norm):
    _set_grads(ref, grads)
    torch.nn.utils.clip_grad_norm_(ref, max_norm)
    ref_opt.step()


def _rand_grads(scale):
    return [torch.randn(*s) * scale for s in SHAPES]


def test_clip_matches_torch_clip_then_adamw():
    from torchft_amd.ops import FusedAdamW

    ps = _params(0)
    ref = _clones(ps)
    opt = FusedAdamW(ps, max_grad_norm=0.5, **HP)
    ref_opt = torch.optim.AdamW(ref, **HP)
    norms = []
    # randn grads of 221 elements have norm ~15; scaled by 1e-3, ~0.015
    for scale in (1.0, 1e-3, 1.0, 1e-3, 1.0):
        grads = _rand_grads(scale)
        _set_grads(ps, grads)
        opt.step()
        norms.append(float(opt.last_grad_norm))
        _ref_step(ref, ref_opt, grads, 0.5)
    assert any(n > 0.5 for n in norms) and any(n < 0.5 for n in norms), norms
    for p, r in zip(ps, ref):
        torch.testing.assert_close(p, r)
        assert opt.state[p]["step"].dtype == torch.int32
        assert opt.state[p]["step"].dim() == 0
        assert int(opt.state[p]["step"]) == 5
    assert int(opt.skipped_steps) == 0


@pytest.mark.parametrize("bad", [math.inf, math.nan])
def test_nonfinite_grad_skips_the_step(bad):
    from torchft_amd.ops import FusedAdamW

    ps = _params(1)
    ref = _clones(ps)
    opt = FusedAdamW(ps, max_grad_norm=0.5, **HP)
    ref_opt = torch.optim.AdamW(ref, **HP)
    for scale in (1.0, 1e-3):
        grads = _rand_grads(scale)
        _set_grads(ps, grads)
        opt.step()
        _ref_step(ref, ref_opt, grads, 0.5)

    before = [
        (p.detach().clone(), opt.state[p]["exp_avg"].clone(),
         opt.state[p]["exp_avg_sq"].clone(), opt.state[p]["step"].clone())
        for p in ps
    ]
    grads = _rand_grads(1.0)
    grads[1][2, 1] = bad
    _set_grads(ps, grads)
    opt.step()
    for p, (p0, m0, v0, s0) in zip(ps, before):
        assert torch.equal(p.detach(), p0)
        assert torch.equal(opt.state[p]["exp_avg"], m0)
        assert torch.equal(opt.state[p]["exp_avg_sq"], v0)
        assert torch.equal(opt.state[p]["step"], s0)
    assert int(opt.skipped_steps) == 1
    assert not math.isfinite(float(opt.last_grad_norm))

    # the reference never sees the bad step
    grads = _rand_grads(1.0)
    _set_grads(ps, grads)
    opt.step()
    _ref_step(ref, ref_opt, grads, 0.5)
    for p, r in zip(ps, ref):
        torch.testing.assert_close(p, r)
        assert int(opt.state[p]["step"]) == 3
    assert int(opt.skipped_steps) == 1
    assert math.isfinite(float(opt.last_grad_norm))


def test_norm_reduce_scales_the_sum_of_squares():
    from torchft_amd.ops import FusedAdamW

    a = _params(2)
    b = _clones(a)
    seen = []

    def reduce(t):
        seen.append((t.shape, t.dtype))
        t.mul_(4)

    opt_a = FusedAdamW(a, max_grad_norm=0.5, **HP)
    opt_b = FusedAdamW(b, max_grad_norm=0.5, norm_reduce=reduce, **HP)
    grads = _rand_grads(1.0)  # both clip
    _set_grads(a, grads)
    _set_grads(b, grads)
    opt_a.step()
    opt_b.step()
    assert seen == [(torch.Size([1]), torch.float32)]
    torch.testing.assert_close(opt_b.last_grad_norm, 2 * opt_a.last_grad_norm)
    # first step from zero moments: exp_avg = (1 - beta1) * coef * g
    for pa, pb in zip(a, b):
        torch.testing.assert_close(opt_b.state[pb]["exp_avg"],
                                   opt_a.state[pa]["exp_avg"] / 2)


def test_norm_reduce_needs_clip_mode():
    from torchft_amd.ops import FusedAdamW

    with pytest.raises(ValueError):
        FusedAdamW(_params(3), norm_reduce=lambda t: None)
    with pytest.raises(ValueError):
        FusedAdamW(_params(3), max_grad_norm=0.0)


def test_inf_max_norm_reports_without_scaling():
    from torchft_amd.ops import FusedAdamW

    ps = _params(4)
    ref = _clones(ps)
    opt = FusedAdamW(ps, max_grad_norm=math.inf, **HP)
    ref_opt = torch.optim.AdamW(ref, **HP)
    for _ in range(3):
        grads = _rand_grads(1.0)
        _set_grads(ps, grads)
        _set_grads(ref, grads)
        opt.step()
        ref_opt.step()
    expect = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads))
    assert float(opt.last_grad_norm) == pytest.approx(expect, rel=1e-6)
    for p, r in zip(ps, ref):
        torch.testing.assert_close(p, r)


def _run(opt, ps, steps, seed):
    gen = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()


def _checkpoint(opt):
    # as written to and read back from storage: shares nothing with opt
    return copy.deepcopy(opt.state_dict())


def test_state_dict_round_trip_in_clip_mode():
    from torchft_amd.ops import FusedAdamW

    a = _params(5)
    opt_a = FusedAdamW(a, max_grad_norm=0.5, **HP)
    _run(opt_a, a, 3, seed=50)
    b = _clones(a)
    opt_b = FusedAdamW(b, max_grad_norm=0.5, **HP)
    opt_b.load_state_dict(_checkpoint(opt_a))
    for pa, pb in zip(a, b):
        sb = opt_b.state[pb]["step"]
        assert isinstance(sb, torch.Tensor) and sb.dtype == torch.int32
        assert sb.dim() == 0 and sb.device == pb.device and int(sb) == 3
    _run(opt_a, a, 2, seed=51)
    _run(opt_b, b, 2, seed=51)
    for pa, pb in zip(a, b):
        assert torch.equal(pa, pb)
        assert int(opt_b.state[pb]["step"]) == 5


def test_int_step_checkpoint_loads_into_clip_mode_and_back():
    from torchft_amd.ops import FusedAdamW

    a = _params(6)
    opt_a = FusedAdamW(a, **HP)
    _run(opt_a, a, 3, seed=60)
    assert all(type(opt_a.state[p]["step"]) is int for p in a)

    # int steps -> clip mode
    b = _clones(a)
    opt_b = FusedAdamW(b, max_grad_norm=math.inf, **HP)
    opt_b.load_state_dict(_checkpoint(opt_a))
    for pb in b:
        sb = opt_b.state[pb]["step"]
        assert isinstance(sb, torch.Tensor) and sb.dtype == torch.int32
        assert sb.dim() == 0 and int(sb) == 3
    _run(opt_b, b, 1, seed=61)

    # tensor steps -> plain mode
    c = _clones(b)
    opt_c = FusedAdamW(c, **HP)
    opt_c.load_state_dict(_checkpoint(opt_b))
    for pc in c:
        assert type(opt_c.state[pc]["step"]) is int
        assert opt_c.state[pc]["step"] == 4

    # with no scaling both modes walk the same trajectory
    _run(opt_a, a, 1, seed=61)
    _run(opt_a, a, 1, seed=62)
    _run(opt_c, c, 1, seed=62)
    for pa, pc in zip(a, c):
        torch.testing.assert_close(pa, pc)
        assert opt_c.state[pc]["step"] == 5


def test_plain_mode_keeps_int_steps_and_has_no_clip_state():
    from torchft_amd.ops import FusedAdamW

    ps = _params(7)
    opt = FusedAdamW(ps, **HP)
    _run(opt, ps, 2, seed=70)
    for p in ps:
        assert type(opt.state[p]["step"]) is int and opt.state[p]["step"] == 2
    assert opt.max_grad_norm is None
    assert opt.last_grad_norm is None and opt.skipped_steps is None


def test_grad_none_params_keep_their_own_step():
    from torchft_amd.ops import FusedAdamW

    ps = _params(8)
    ref = _clones(ps)
    opt = FusedAdamW(ps, max_grad_norm=0.5, **HP)
    ref_opt = torch.optim.AdamW(ref, **HP)
    for it in range(5):
        grads = _rand_grads(1.0 if it % 2 else 1e-3)
        for params, o in ((ps, opt), (ref, ref_opt)):
            params[0].grad = grads[0].clone()
            params[1].grad = grads[1].clone() if it % 2 == 0 else None
            if o is ref_opt:
                torch.nn.utils.clip_grad_norm_(params, 0.5)
            o.step()
            o.zero_grad(set_to_none=True)
    assert int(opt.state[ps[0]]["step"]) == 5
    assert int(opt.state[ps[1]]["step"]) == 3
    for p, r in zip(ps, ref):
        torch.testing.assert_close(p, r)


def test_ops_grad_norm_cpu():
    from torchft_amd import ops

    torch.manual_seed(9)
    ts = [torch.randn(33), torch.randn(4, 5).bfloat16(), torch.randn(1)]
    expect = math.sqrt(sum(float(t.double().pow(2).sum()) for t in ts))
    n = ops.grad_norm(ts)
    assert n.dim() == 0 and n.dtype == torch.float32
    assert float(n) == pytest.approx(expect, rel=1e-6)
    # parameters contribute their .grad; those without one are skipped
    ps = [torch.zeros(33, requires_grad=True), torch.zeros(2, requires_grad=True)]
    ps[0].grad = ts[0].clone()
    assert float(ops.grad_norm(ps)) == pytest.approx(float(ts[0].norm()), rel=1e-6)
    doubled = ops.grad_norm(ts, norm_reduce=lambda t: t.mul_(4))
    assert float(doubled) == pytest.approx(2 * expect, rel=1e-6)


def test_ops_clip_grad_norm_cpu():
    from torchft_amd import ops

    ps = _params(10)
    ref = _clones(ps)
    grads = _rand_grads(1.0)
    _set_grads(ps, grads)
    _set_grads(ref, grads)
    n = ops.clip_grad_norm_(ps, 0.5)
    n_ref = torch.nn.utils.clip_grad_norm_(ref, 0.5)
    torch.testing.assert_close(n, n_ref)
    for p, r in zip(ps, ref):
        torch.testing.assert_close(p.grad, r.grad)
    # below the threshold nothing is scaled
    small = [g * 1e-3 for g in grads]
    _set_grads(ps, small)
    ops.clip_grad_norm_(ps, 0.5)
    for p, g in zip(ps, small):
        assert torch.equal(p.grad, g)
    # a non-finite norm leaves the gradients alone
    grads[0][5] = math.nan
    _set_grads(ps, grads)
    n = ops.clip_grad_norm_(ps, 0.5)
    assert not math.isfinite(float(n))
    for p, g in zip(ps, grads):
        assert torch.equal(p.grad.isnan(), g.isnan())
        assert torch.equal(p.grad.nan_to_num(), g.nan_to_num())
