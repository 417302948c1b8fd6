"""``FusedAdamW(rounding=...)`` on the torch path, and the step both paths are
held to exactly (tests/test_adamw_rounding_gpu.py runs ``exact_steps`` on the
HIP kernel): ``g = 0``, fresh state, ``lr = 2^-3``, ``weight_decay = 2^-4``. Then
``m' = v' = 0``, the quotient is exactly 0 and ``p' = p * (1 - 2^-7)``: 15
significant bits from a bf16 ``p`` (22 on the master copy's second step), exact
in fp32 whatever a compiler contracts."""
import pytest
import torch

from torchft_amd import ops
from torchft_amd.ops.adamw_ref import philox4x32_10, sr_bits, stochastic_round_bf16

SHAPES = [(1,), (7,), (8,), (2047,), (2049,), (100, 33)]


def exact_steps(dev, rounding, clip, seed):
    gen = torch.Generator().manual_seed(3)
    host = [torch.randn(s, generator=gen).to(torch.bfloat16) for s in SHAPES]
    host.append(host[4].clone())  # the contents of (2049,) again, another stream
    buf = torch.cat([torch.zeros(1, dtype=torch.bfloat16), host[4]]).to(dev)
    params = [t.to(dev) for t in host] + [buf[1:]]  # and off a 16 B boundary
    for p in params:
        p.requires_grad_(True)
    opt = ops.FusedAdamW(
        [dict(params=params[:4]), dict(params=params[4:])], lr=2.0 ** -3,
        weight_decay=2.0 ** -4, max_grad_norm=1.0 if clip else None,
        rounding=rounding, sr_seed=seed)
    truth = [p.detach().cpu().float() for p in params]
    for step in (1, 2):
        for p in params:
            p.grad = torch.zeros_like(p)
        opt.step()
        for i, p in enumerate(params):  # i is the stream id
            got = p.detach().cpu()
            x = truth[i] * (127 / 128)
            if rounding == "master":
                assert torch.equal(opt.state[p]["master"].cpu(), x)
                want, truth[i] = x.to(torch.bfloat16), x
            else:
                r16 = sr_bits(x.numel(), seed=seed, step=step, stream_id=i)
                want = stochastic_round_bf16(x.reshape(-1), r16).view_as(x)
                truth[i] = got.float()
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (step, i)
        if rounding == "stochastic":  # same contents, three streams
            assert not torch.equal(params[4], params[6])
            assert not torch.equal(params[4], params[7])
    # the step count enters the counter
    assert not torch.equal(sr_bits(64, seed=seed, step=1, stream_id=0),
                           sr_bits(64, seed=seed, step=2, stream_id=0))


def test_philox_known_answers():
    for counter, key, want in [
            ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
            ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
            ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
             "d16cfe09 94fdcceb 5001e420 24126ea1")]:
        out = philox4x32_10(torch.tensor(counter, dtype=torch.int64), key)
        assert " ".join(f"{int(w):08x}" for w in out) == want


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("rounding", ["stochastic", "master"])
def test_exact_step_on_the_torch_path(rounding, clip):
    exact_steps(torch.device("cpu"), rounding, clip, seed=5)


def test_unknown_rounding_is_refused():
    with pytest.raises(ValueError, match="rounding"):
        ops.FusedAdamW([torch.zeros(2, requires_grad=True)], rounding="up")
