"""What the outer step from an fp8 pack is held to (tests/test_diloco_fp8_pack*.py).
Ground truth: ``diloco_outer_step_ref`` in fp64 fed ``d64 = code * fl32(scale *
inv_div)``. Criteria: those derived in tests/test_diloco_fused_gpu.py with one
more fp32 rounding, ``d``'s own product, on every chain ``d`` enters: ``m'`` 5,
``g'`` 9, ``p`` 6 on ``|l| + |g'|`` plus ``g'``'s budget, each times ``2^-24 *
S``. bf16: within one ulp of the rounded fp64 value, at most 0.1 % differing."""

import torch

import fp8_check as fc
from torchft_amd import ops
from torchft_amd import quantization as Q
from torchft_amd.ops.diloco import diloco_outer_step_ref

U32 = 2.0 ** -24
GROUP = [0, 2, 4, 5]  # the param group, of fp8_check.SHAPES; pack blocks 0, 2, 4-5, 6-7
FIRST = [0, 2, 4, 6]
TOTAL = 8  # at world 3 the slices hold blocks 0-2, 3-5, 6-8: the group spans all three
LR = 0.7


def outer_inputs(dtype, world):
    """CPU inputs at the scales of a sync (never modified), and the
    reference's own pack of seeded fp32 differences."""
    gen = torch.Generator().manual_seed(4321)
    g = [torch.randn(s, generator=gen).to(dtype) for s in fc.SHAPES]
    l = [(x.float() + 0.01 * torch.randn(x.shape, generator=gen)).to(dtype) for x in g]
    m = [(0.02 * torch.randn(s, generator=gen)).to(dtype) for s in fc.SHAPES]
    diffs = [0.03 * torch.randn(s, generator=gen) for s in fc.SHAPES]
    return g, l, m, Q.quantize_pack_ref(diffs, world)


def run_outer(dev, dtype, world, momentum, nesterov, alpha, misalign_l=False):
    """The op on the GROUP tensors with num_participants = 3; returns the
    (g, l, m) lists. The pack and the tensors outside the group must not change."""
    g0, l0, m0, pack0 = outer_inputs(dtype, world)
    g, l, m = ([t.to(dev) for t in ts] for ts in (g0, l0, m0))
    if misalign_l:  # buf[1:] views: off a 16 B boundary
        bufs = [torch.zeros(t.numel() + 1, dtype=dtype, device=dev) for t in l0]
        l = [b[1:].view(t.shape).copy_(t) for b, t in zip(bufs, l0)]
    pack = pack0.to(dev)
    ops.diloco_outer_step_fp8_(
        [g[i] for i in GROUP], [l[i] for i in GROUP], pack, FIRST, TOTAL, world,
        [m[i] for i in GROUP] if momentum else None, lr=LR, momentum=momentum,
        nesterov=nesterov, alpha=alpha, num_participants=3)
    assert torch.equal(pack.cpu(), pack0), "pack modified"
    for i in set(range(len(fc.SHAPES))) - set(GROUP):
        assert all(torch.equal(x[i].cpu(), x0[i]) for x, x0 in ((g, g0), (l, l0), (m, m0)))
    return g, l, m


def decode64(pack: torch.Tensor, world: int, num_participants: int) -> torch.Tensor:
    """[padded_blocks, QBLOCK] fp64: code * fl32(scale * fl32(1 / num_participants))."""
    scales, codes = Q.split_slices(pack.cpu(), world)
    s = scales.reshape(-1) * (torch.tensor(1.0, dtype=torch.float32) / num_participants)
    return Q.e4m3_values(codes.reshape(-1, Q.QBLOCK)).double() * s.double()[:, None]


def _ordered(t: torch.Tensor) -> torch.Tensor:
    i = t.view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def check_outer(got, g0, d64, m0, l0, *, lr, momentum, nesterov, alpha, label):
    """got = (m, g, l) after the step, the rest the CPU inputs of one tensor.
    Asserts the fp32 bounds or the bf16 ulp; returns (differing, total)."""
    m_ref, g_ref, p_ref = diloco_outer_step_ref(
        g0, d64.view_as(g0), m0 if momentum else None, l0, lr=lr, momentum=momentum,
        nesterov=nesterov, alpha=alpha, compute_dtype=torch.float64)
    got_m, got_g, got_p = (x.detach().cpu() for x in got)
    assert alpha != 0.0 or torch.equal(got_p, got_g), f"{label}: alpha 0"
    assert alpha != 1.0 or torch.equal(got_p, l0), f"{label}: alpha 1"
    pairs = [(got_g, g_ref), (got_p, p_ref)]
    if momentum:
        pairs.append((got_m, m_ref))
    else:
        assert torch.equal(got_m, m0), f"{label}: momentum buffer touched"
    if g0.dtype == torch.bfloat16:
        for x, ref in pairs:
            assert ((_ordered(x) - _ordered(ref)).abs() <= 1).all(), f"{label}: > 1 ulp"
        return sum(int((x != ref).sum()) for x, ref in pairs), sum(x.numel() for x, _ in pairs)
    dd, mm, gg, ll = (x.double().abs() for x in (d64.view_as(g0), m0, g0, l0))
    s_u = dd
    if momentum:
        s_m = momentum * mm + dd
        assert ((got_m.double() - m_ref.double()).abs() <= 5 * U32 * s_m).all(), f"{label}: m'"
        s_u = dd + momentum * s_m if nesterov else s_m
    bound_g = 9 * U32 * (gg + lr * s_u)
    assert ((got_g.double() - g_ref.double()).abs() <= bound_g).all(), f"{label}: g'"
    bound_p = 6 * U32 * (ll + g_ref.double().abs()) + bound_g
    assert ((got_p.double() - p_ref.double()).abs() <= bound_p).all(), f"{label}: p"
    return 0, 0
