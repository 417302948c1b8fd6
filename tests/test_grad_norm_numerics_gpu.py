"""``grad_sumsq_partial_kernel``, ``grad_sumsq_finalize_kernel`` and
``grad_scale_kernel`` (csrc/kernels/grad_norm.hip) held to tests/grad_norm_check.py
(docs/KERNELS.md, grad_norm.hip): sums of squares that must come out exactly, on
lists sized to the loops (a second trip of the finalize loop, a second
grid-stride trip at the default cap, a last block of mostly empty lanes, three
dtypes with several blocks each), the derived bound where exactness is not to
be had, the overflow rule, and every clipped gradient bit for bit.

Nothing here allocates more than 8 MB, so the two 2049-block lists run in the
2-byte dtypes only; the kernel's loops are the same template for all three."""

import math

import pytest
import torch

from grad_norm_check import (BEACON_LOG2, BLOCK, DTYPES, FINALIZE_SECOND_TRIP, GRID_SECOND_TRIP,
                             ZOO, beacon_positions, bits, check_norm, clip_expected,
                             coef_from_sumsq32, depth, hold_clip_bits, hold_exact, staircase,
                             sumsq_and_norm)
from torchft_amd import ops

pytestmark = pytest.mark.gpu

ZOO_N = [math.prod(s) for s in ZOO]
SENTINEL = 12288.0  # exact in all three dtypes
PAD = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked test without a HIP device"
    assert ops.have_hip_ext(), "HIP kernel extension must be loadable on a GPU box"
    return torch.device("cuda:0")


def _views(numels, dtype, dev, off, fill=0.0):
    """Each tensor a view at element ``PAD + off`` of its own sentinel buffer:
    off 0 is 16 B-aligned, off 1 the ``buf[1:]`` case."""
    bufs = [torch.full((n + 2 * PAD + 8,), SENTINEL, dtype=dtype, device=dev) for n in numels]
    views = [b[PAD + off : PAD + off + n] for b, n in zip(bufs, numels)]
    for v in views:
        v.fill_(fill)
        assert (v.data_ptr() % 16 == 0) == (off == 0)
    return bufs, views


def _sentinels_hold(bufs, views, off):
    for b, v in zip(bufs, views):
        lo = PAD + off
        outside = torch.cat([b[:lo], b[lo + v.numel() :]])
        assert (outside == SENTINEL).all(), "sentinel: the clip wrote outside a view"


def _sumsq(ts, **kw):
    s, norm = sumsq_and_norm(ts, **kw)
    assert float(norm) == float(s.sqrt())
    return s.cpu()


def _big_lists(dtype):
    out = {"257 blocks": ([FINALIZE_SECOND_TRIP], (1, 2, 2048, 65536))}
    if dtype != torch.float32:
        out["2049 blocks"] = ([GRID_SECOND_TRIP], (2048,))
        out["2049 blocks + 5"] = ([GRID_SECOND_TRIP + 5], (2048,))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_ones_sum_to_numel(dev, dtype):
    for off in (0, 1):
        _, views = _views(ZOO_N, dtype, dev, off, fill=1.0)
        for mb in (1, 3, 2048):
            hold_exact(_sumsq(views, max_blocks=mb), float(sum(ZOO_N)), f"zoo off={off} mb={mb}")
    for name, (numels, caps) in _big_lists(dtype).items():
        _, views = _views(numels, dtype, dev, 0, fill=1.0)
        for mb in caps:
            hold_exact(_sumsq(views, max_blocks=mb), float(sum(numels)), f"{name} mb={mb}")


def _params_with_grads(views):
    params = [torch.zeros_like(v).requires_grad_(True) for v in views]
    for p, v in zip(params, views):
        p.grad = v
    return params


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_beacon_is_found_wherever_it_stands(dev, dtype):
    """Finite: the sum of squares is 2^2k exactly. NaN / +inf at the same
    places: a non-finite norm, and the clip leaves every bit alone."""
    k = BEACON_LOG2[dtype]
    for off in (0, 1):
        bufs, views = _views(ZOO_N, dtype, dev, off)
        params = _params_with_grads(views)
        for i, e in beacon_positions(ZOO_N):
            views[i].view(-1)[e] = 2.0 ** k
            hold_exact(_sumsq(views), 4.0 ** k, f"zoo off={off} beacon {i}:{e}")
            for bad in (math.nan, math.inf):
                views[i].view(-1)[e] = bad
                before = [b.clone() for b in bufs]
                norm = ops.clip_grad_norm_(params, 1e-3)
                assert not math.isfinite(float(norm)), f"{bad} at {i}:{e} gave a finite norm"
                for b, b0 in zip(bufs, before):
                    assert torch.equal(bits(b), bits(b0)), f"{bad} at {i}:{e}: the clip wrote"
            views[i].view(-1)[e] = 0
    for name, (numels, caps) in _big_lists(dtype).items():
        _, views = _views(numels, dtype, dev, 0)
        n = numels[0]
        for e in sorted({0, BLOCK - 1, 256 * BLOCK, n - 1, n - 1 - (n - 1) % 8}):
            views[0][e] = 2.0 ** k
            for mb in caps:
                hold_exact(_sumsq(views, max_blocks=mb), 4.0 ** k, f"{name} beacon {e} mb={mb}")
            views[0][e] = 0


def test_mixed_dtypes_with_several_blocks_each(dev):
    """One launch per dtype into one partials buffer: the ``at_partial``
    offsets, with and without a grid-stride trip."""
    numels = [3 * BLOCK + 5, 4 * BLOCK, 3 * BLOCK + 1]
    ts = [torch.zeros(n, dtype=dt, device=dev) for n, dt in zip(numels, DTYPES)]
    order = [ts[2], ts[0], ts[1]]  # the binding sorts by dtype, not the caller
    for mb in (2, 2048):
        for t in ts:
            t[t.numel() - 1] = 2.0 ** BEACON_LOG2[t.dtype]
            hold_exact(_sumsq(order, max_blocks=mb), 4.0 ** BEACON_LOG2[t.dtype],
                       f"mixed, beacon in the last block of {t.dtype}, mb={mb}")
            t[t.numel() - 1] = 0
        for t in ts:
            t.fill_(1.0)
        hold_exact(_sumsq(order, max_blocks=mb), float(sum(numels)), f"mixed ones mb={mb}")
        for t in ts:
            t.zero_()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=str)
def test_staircase_needs_the_double_finalize(dev, dtype):
    hold_exact(_sumsq([staircase(dtype, dev)]), 2.0 ** 24 + 2, "staircase")


def test_refusals(dev):
    t = torch.ones(100, device=dev)
    for mb in (0, 65537):
        with pytest.raises(RuntimeError, match="max_blocks"):
            ops.grad_norm([t], max_blocks=mb)
    with pytest.raises(ValueError, match="no gradients"):
        ops.grad_norm([])
    with pytest.raises(TypeError, match="dtype"):
        ops.grad_norm([torch.ones(100, dtype=torch.int32, device=dev)])


def _bounded(name, dtype, dev, numels):
    g = torch.Generator().manual_seed(5)
    if name == "one 2^60 among ones":
        ts = [torch.ones(n, dtype=dtype) for n in numels]
        ts[-1][-1] = 2.0 ** 60
        return [t.to(dev) for t in ts]
    scale = {"randn": 1.0, "randn 2^-10": 2.0 ** -10, "randn 2^40": 2.0 ** 40,
             "randn 2^-80": 2.0 ** -80}[name]
    return [(scale * torch.randn(n, generator=g)).to(dtype).to(dev) for n in numels]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=str)
@pytest.mark.parametrize("name", ["randn", "randn 2^-10", "randn 2^40", "randn 2^-80",
                                  "one 2^60 among ones"])
def test_bounded_families(dev, name, dtype):
    worst = 0.0
    for numels, mb in ((ZOO_N, 2048), (ZOO_N, 3), ([FINALIZE_SECOND_TRIP], 2048),
                       ([FINALIZE_SECOND_TRIP], 2)):
        ts = _bounded(name, dtype, dev, numels)
        norm = ops.grad_norm(ts, max_blocks=mb)
        cpu = [t.cpu() for t in ts]
        worst = max(worst, check_norm(norm, cpu, depth(numels, mb), f"{name} {dtype} mb={mb}"))
    print(f"{name} {dtype}: worst fraction of the norm bound {worst:.3f}")


def test_fp16_randn(dev):
    g = torch.Generator().manual_seed(6)
    ts = [torch.randn(n, generator=g).half().to(dev) for n in ZOO_N]
    check_norm(ops.grad_norm(ts), [t.cpu() for t in ts], depth(ZOO_N), "randn fp16")


def test_finite_gradients_can_overflow_the_sum(dev):
    """|g| = 2^64 is a finite bf16 number whose square is not an fp32 number:
    the norm is inf, the clip leaves the gradients alone, FusedAdamW skips the
    step and counts it. Stated as the rule in docs/KERNELS.md."""
    shapes = [(8,), (2049,)]
    grads = [torch.full(s, 2.0 ** 64, dtype=torch.bfloat16, device=dev) for s in shapes]
    assert all(torch.isfinite(g).all() for g in grads)
    assert float(ops.grad_norm(grads)) == math.inf
    params = [torch.ones(s, dtype=torch.bfloat16, device=dev, requires_grad=True) for s in shapes]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    assert float(ops.clip_grad_norm_(params, 1.0)) == math.inf
    for p, g in zip(params, grads):
        assert torch.equal(bits(p.grad), bits(g))
    opt = ops.FusedAdamW(params, lr=1e-2, max_grad_norm=1.0)
    opt.step()
    assert int(opt.skipped_steps) == 1 and float(opt.last_grad_norm) == math.inf
    for p in params:
        assert (p == 1).all(), "a skipped step moved a parameter"


# ---- the clip, bit for bit ----------------------------------------------------

CLIP_N = [7, 2049, 5000]


def _clip_once(views, bufs, off, max_norm, reduce=None):
    """clip_grad_norm_ on the views; returns (sum of squares the kernel
    produced, gradients before, gradients after), on the CPU."""
    before = [v.clone().cpu() for v in views]
    seen = []

    def hook(s):
        seen.append(s.clone())
        if reduce is not None:
            reduce(s)

    norm = ops.clip_grad_norm_(_params_with_grads(views), max_norm, norm_reduce=hook)
    torch.cuda.synchronize()
    _sentinels_hold(bufs, views, off)
    assert len(seen) == 1
    return seen[0].cpu().reshape(()), norm, before, [v.cpu() for v in views]


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "buf[1:]"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_clip_bits(dev, dtype, off):
    g = torch.Generator().manual_seed(9)
    for scale in (1.0, 2.0 ** -14):  # at the small norm the 1e-6 is felt
        src = [(scale * torch.randn(n, generator=g)).to(dtype) for n in CLIP_N]
        bufs, views = _views(CLIP_N, dtype, dev, off)
        norm0 = float(ops.grad_norm([s.to(dev) for s in src]))
        # the norm just above the threshold, just below it, on it, far above
        for name, max_norm in (("above", norm0 * (1 - 2.0 ** -12)),
                               ("below", norm0 * (1 + 2.0 ** -12)), ("equal", norm0),
                               ("far above", 0.37 * norm0)):
            for v, s in zip(views, src):
                v.copy_(s)
            sumsq, norm, before, after = _clip_once(views, bufs, off, max_norm)
            tag = f"{dtype} off={off} scale={scale:.3g} {name}"
            check_norm(norm, before, depth(CLIP_N), tag)
            assert float(norm) == float(sumsq.sqrt())
            hold_clip_bits(after, clip_expected(before, sumsq, max_norm), tag)
            coef = float(coef_from_sumsq32(sumsq, max_norm))
            if name == "below":
                assert coef == 1.0
                hold_clip_bits(after, before, tag + " untouched")
            if name in ("above", "far above"):
                assert coef < 1.0
            if name == "far above":
                assert any(not torch.equal(bits(a), bits(b)) for a, b in zip(after, before))


def test_norm_reduce_feeds_the_clip(dev):
    """A reduce hook that multiplies the sum of squares by 4 halves the
    coefficient: the clip reads what the hook left."""
    g = torch.Generator().manual_seed(10)
    src = [torch.randn(n, generator=g).bfloat16() for n in CLIP_N]
    bufs, views = _views(CLIP_N, torch.bfloat16, dev, 1)
    for v, s in zip(views, src):
        v.copy_(s)
    sumsq, norm, before, after = _clip_once(views, bufs, 1, 1.0, reduce=lambda s: s.mul_(4))
    assert float(norm) == 2 * float(sumsq.sqrt())
    hold_clip_bits(after, clip_expected(before, 4 * sumsq, 1.0), "norm_reduce x4")
    c1, c4 = coef_from_sumsq32(sumsq, 1.0), coef_from_sumsq32(4 * sumsq, 1.0)
    assert abs(float(c4) / float(c1) - 0.5) <= 2.0 ** -22
