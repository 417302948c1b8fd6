"""The state ``FusedAdamW`` gathers for a step, in all six combinations of
``rounding`` and clip, which share one routine: what is created on first sight
and in which representation, what a parameter without a gradient keeps, and
which stream of random bits a parameter draws."""
import pytest
import torch

from torchft_amd import ops
from torchft_amd.ops.adamw_ref import sr_bits, stochastic_round_bf16

ROUNDINGS = ["nearest", "stochastic", "master"]


def _bits(t):
    return t.detach().view(torch.int16)


def _step_count(state):
    return int(state["step"])


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("rounding", ROUNDINGS)
def test_state_of_the_first_two_steps(rounding, clip):
    gen = torch.Generator().manual_seed(11)
    shapes = [(5,), (3, 4), (9,), (2, 2)]
    params = [torch.randn(s, generator=gen).to(torch.bfloat16).requires_grad_(True)
              for s in shapes]
    never, late = params[1], params[2]  # no gradient at all / none on the 2nd step
    opt = ops.FusedAdamW(
        [dict(params=params[:2]), dict(params=params[2:], lr=3e-3)], lr=1e-2,
        max_grad_norm=1.0 if clip else None, rounding=rounding, sr_seed=7)

    def grads(skip):
        for p in params:
            p.grad = None if any(p is s for s in skip) else (
                torch.randn(p.shape, generator=gen).to(torch.bfloat16))

    grads(skip=[never])
    opt.step()
    assert len(opt.state[never]) == 0
    for p in params:
        if p is never:
            continue
        state = opt.state[p]
        for key in ("exp_avg", "exp_avg_sq"):
            assert state[key].dtype == torch.float32
            assert state[key].shape == p.shape
        if clip:
            assert isinstance(state["step"], torch.Tensor)
            assert state["step"].dtype == torch.int32 and state["step"].dim() == 0
        else:
            assert type(state["step"]) is int
        assert _step_count(state) == 1
        assert ("master" in state) == (rounding == "master")
        if rounding == "master":
            assert state["master"].dtype == torch.float32
            assert state["master"].shape == p.shape
            assert torch.equal(_bits(state["master"].to(torch.bfloat16)), _bits(p))

    grads(skip=[never, late])
    opt.step()
    assert len(opt.state[never]) == 0
    for p in params:
        if p is not never:
            assert _step_count(opt.state[p]) == (1 if p is late else 2)


@pytest.mark.parametrize("clip", [False, True])
def test_stream_id_counts_parameters_without_a_gradient(clip):
    # the exact step of tests/test_adamw_rounding_cpu.py: g = 0, so
    # p' = p * (1 - 2^-7) in fp32, then the stochastic store
    seed = 5
    gen = torch.Generator().manual_seed(3)
    host = torch.randn(2049, generator=gen).to(torch.bfloat16)
    params = [host.clone().requires_grad_(True) for _ in range(3)]
    opt = ops.FusedAdamW(params, lr=2.0 ** -3, weight_decay=2.0 ** -4,
                         max_grad_norm=1.0 if clip else None, rounding="stochastic",
                         sr_seed=seed)
    params[0].grad = torch.zeros_like(params[0])
    params[2].grad = torch.zeros_like(params[2])
    opt.step()

    x = host.float() * (127 / 128)

    def want(stream_id):
        r16 = sr_bits(x.numel(), seed=seed, step=1, stream_id=stream_id)
        return stochastic_round_bf16(x, r16)

    assert torch.equal(_bits(params[1]), _bits(host))  # untouched
    assert torch.equal(_bits(params[0]), _bits(want(0)))
    assert torch.equal(_bits(params[2]), _bits(want(2)))
    assert not torch.equal(_bits(params[2]), _bits(want(1)))
