"""What the global-norm kernels (csrc/kernels/grad_norm.hip) are held to, the
lists and families they are held to it on, and an emulation of their reduction
order and of the clip with switchable mistakes (docs/KERNELS.md, grad_norm.hip).
Shared by the CPU test of the checker itself and by the GPU tests.

Exact families need no tolerance. ``ones``: every element 1, the sum of squares
is ``numel`` (below 2^24 every partial sum is an integer fp32 holds). ``beacon``:
zeros and one ``2^k``, the sum of squares is ``2^2k`` wherever the beacon sits;
``beacon_positions`` walks it over the places an indexing mistake would lose.
``staircase``: ``2^12``, 1 and 1 in the blocks 0, 1 and 2 of one tensor, three
partials whose sum ``2^24 + 2`` an fp32 finalize cannot hold on the way.

Bounded families: all summands are non-negative, so the fp32 sum of squares is
off by at most ``depth * 2^-24`` relative (``depth``: 8 fma per block a
workgroup visits, 6 shuffle steps, 3 wave adds; the partials are summed in
double), which the root halves; the norm is held to ``depth * 2^-24`` relative
(twice the bound, as margin for the two roundings of the result) plus an
absolute floor: an fp32 result below ``2^-126`` may be flushed, each of the at
most ``2 N`` additions loses less than that, and ``|sqrt a - sqrt b| <=
sqrt |a - b|``: ``sqrt(2 N) * 2^-63``.

Clip: ``coef = min(1, max_norm / (sqrt(sumsq) + 1e-6))`` in fp32 from the sum of
squares the kernel itself produced, and every gradient ``(g.float() *
coef).to(dtype)`` bit for bit. fp32 ``/`` and ``sqrtf`` are correctly rounded
in the project's build (hipcc's default ``-fhip-fp32-correctly-rounded-
divide-sqrt``, no ``-ffast-math``, see docs/KERNELS.md), so the CPU's IEEE
operations give the same bits.
"""

from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

BLOCK, LANES, EPT = 2048, 256, 8
DTYPES = (torch.bfloat16, torch.float16, torch.float32)  # dtype_code order
BEACON_LOG2 = {torch.bfloat16: 20, torch.float16: 7, torch.float32: 30}

ZOO = [(1,), (7,), (8,), (2047,), (2048,), (2049,), (5000,), (100, 33)]
FINALIZE_SECOND_TRIP = 257 * BLOCK  # 257 partials
GRID_SECOND_TRIP = 2049 * BLOCK  # workgroup 0 visits two blocks at the default cap


def depth(numels: Sequence[int], max_blocks: int = 2048) -> int:
    blocks = sum((n + BLOCK - 1) // BLOCK for n in numels)
    grid = min(blocks, max_blocks)
    return 8 * math.ceil(blocks / grid) + 6 + 3


def ref_norm(tensors) -> float:
    return math.sqrt(sum(float(t.double().pow(2).sum()) for t in tensors))


def norm_bound(tensors, dep: int) -> float:
    n = sum(t.numel() for t in tensors)
    return dep * 2.0 ** -24 * ref_norm(tensors) + math.sqrt(2.0 * n) * 2.0 ** -63


def check_norm(norm, tensors, dep: int, tag: str = "") -> float:
    ref = ref_norm(tensors)
    err = abs(float(norm.double()) - ref)
    bound = norm_bound(tensors, dep)
    frac = err / bound if err else 0.0
    print(f"grad_norm {tag}: |err| {err:.3e} bound {bound:.3e} ratio {frac:.3f}")
    assert err <= bound, f"norm bound: {tag}: error {err:.3e} over {bound:.3e}"
    return frac


def beacon_positions(numels: Sequence[int]) -> List[Tuple[int, int]]:
    """(tensor, element) of every place the beacon is to stand in a list."""
    out = [(0, 0)]
    for i, n in enumerate(numels):
        out.append((i, n - 1))
        if n > BLOCK:
            out.append((i, BLOCK - 1))  # the last element of a 2048-block
        if n % EPT and n > EPT:
            out.append((i, n - n % EPT))  # the first element of a partial vector
    return sorted(set(out))


# ---- the reduction order, with switchable mistakes ----------------------------

SUMSQ_INJECTIONS = ("partials_beyond_256_dropped", "last_partial_vector_skipped",
                    "empty_lane_reads_one", "misaligned_skips_element_0", "finalize_fp32")
CLIP_INJECTIONS = ("no_1e-6", "truncating_store", "coef_twice_on_the_tail")


def _group_blocks(tensors, misaligned, inject) -> torch.Tensor:
    """One dtype's tensors as fp32 [blocks, 256, 8], zeros where a lane has
    no element (adding an exact zero is what skipping it does)."""
    parts = []
    for t, mis in zip(tensors, misaligned):
        x = t.detach().reshape(-1).float().clone()
        n = x.numel()
        if inject == "last_partial_vector_skipped" and n % EPT:
            x[n - n % EPT :] = 0
        if inject == "misaligned_skips_element_0" and mis:
            x[0::EPT] = 0  # the scalar loop started at 1
        padded = torch.zeros(-(-n // BLOCK) * BLOCK)
        padded[:n] = x
        if inject == "empty_lane_reads_one":
            first_empty = -(-n // EPT) * EPT
            padded[first_empty::EPT] = x[n - 1]  # whatever lies there: a copy
        parts.append(padded)
    return torch.cat(parts).view(-1, LANES, EPT)


def _partials(blocks: torch.Tensor, grid: int) -> torch.Tensor:
    nb = blocks.shape[0]
    acc = torch.zeros(grid, LANES, dtype=torch.float32)
    for lo in range(0, nb, grid):  # workgroup w visits blocks w, w + grid, ...
        chunk = blocks[lo : lo + grid].double()
        a = acc[: chunk.shape[0]].double()
        for i in range(EPT):  # fmaf(x, x, acc): x * x is exact in double
            a = (a + chunk[:, :, i] * chunk[:, :, i]).float().double()
        acc[: chunk.shape[0]] = a.float()
    w = acc.view(grid, LANES // 64, 64).clone()
    for o in (32, 16, 8, 4, 2, 1):  # __shfl_down: a lane past the end reads itself
        w = w + torch.cat([w[:, :, o:], w[:, :, 64 - o :]], dim=2)
    s = w[:, :, 0]
    return ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]


def _finalize(partials: torch.Tensor, inject) -> torch.Tensor:
    if inject == "partials_beyond_256_dropped":
        partials = partials[:LANES]
    dt = torch.float32 if inject == "finalize_fp32" else torch.float64
    n = partials.numel()
    padded = torch.zeros(-(-n // LANES) * LANES, dtype=dt)
    padded[:n] = partials.to(dt)
    red = torch.zeros(LANES, dtype=dt)
    for row in padded.view(-1, LANES):
        red = red + row
    w = LANES // 2
    while w:
        red = red[:w] + red[w : 2 * w]
        w //= 2
    return red[0].float()


def sumsq_emulated(tensors, max_blocks: int = 2048, misaligned=None,
                   inject: Optional[str] = None) -> torch.Tensor:
    """The fp32 sum of squares as the two kernels form it: per-lane fma over
    the blocks a workgroup visits, the shuffle tree, the wave adds in index
    order, one partial per workgroup and dtype, a double finalize."""
    assert inject is None or inject in SUMSQ_INJECTIONS
    tensors = [t for t in tensors if t.numel()]
    if misaligned is None:
        misaligned = [False] * len(tensors)
    partials = []
    for dt in DTYPES:
        group = [(t, m) for t, m in zip(tensors, misaligned) if t.dtype == dt]
        if not group:
            continue
        blocks = _group_blocks([t for t, _ in group], [m for _, m in group], inject)
        partials.append(_partials(blocks, min(blocks.shape[0], max_blocks)))
    return _finalize(torch.cat(partials), inject)


def coef_from_sumsq32(sumsq: torch.Tensor, max_norm: float, plus: float = 1e-6) -> torch.Tensor:
    """The clip coefficient in fp32 on the CPU, operation by operation as
    grad_scale_kernel and adamw_kernel<true> form it."""
    sumsq = sumsq.detach().cpu().float().reshape(())
    norm = torch.sqrt(sumsq)
    coef = torch.tensor(max_norm, dtype=torch.float32) / (norm + torch.tensor(plus, dtype=torch.float32))
    return torch.clamp(coef, max=1.0)


def _truncate(x32: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    drop = {torch.bfloat16: 16, torch.float16: 13}.get(dtype)
    if drop is None:
        return x32.clone()
    bits = x32.contiguous().view(torch.int32) & (-1 << drop)
    return bits.view(torch.float32).to(dtype)


def clip_expected(grads, sumsq: torch.Tensor, max_norm: float,
                  inject: Optional[str] = None) -> List[torch.Tensor]:
    """Every gradient after the clip, on the CPU: untouched when the norm is
    non-finite or the coefficient exactly 1."""
    assert inject is None or inject in CLIP_INJECTIONS
    grads = [g.detach().cpu() for g in grads]
    norm = torch.sqrt(sumsq.detach().cpu().float().reshape(()))
    coef = coef_from_sumsq32(sumsq, max_norm, plus=0.0 if inject == "no_1e-6" else 1e-6)
    if not torch.isfinite(norm) or float(coef) == 1.0:
        return [g.clone() for g in grads]
    out = []
    for g in grads:
        y = g.float() * coef
        n = g.numel()
        if inject == "coef_twice_on_the_tail" and n % EPT:
            flat = y.view(-1)
            flat[n - n % EPT :] *= coef
        out.append(_truncate(y, g.dtype) if inject == "truncating_store" else y.to(g.dtype))
    return out


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def hold_exact(sumsq, expected: float, tag: str = "") -> None:
    got = float(sumsq.detach().double().reshape(()))
    assert got == expected, f"exact: {tag}: sum of squares {got!r}, must be {expected!r}"


def hold_clip_bits(got, expected, tag: str = "") -> None:
    for i, (g, e) in enumerate(zip(got, expected)):
        g = g.detach().cpu()
        assert g.dtype == e.dtype and g.shape == e.shape
        differ = int((bits(g) != bits(e)).sum())
        assert differ == 0, (
            f"clip bits: {tag}: tensor {i} ({g.dtype}, {g.numel()} elements) differs from "
            f"(g.float() * coef).to(dtype) in {differ} elements")


def ones_list(numels, dtype, device="cpu"):
    return [torch.ones(n, dtype=dtype, device=device) for n in numels]


def staircase(dtype, device="cpu") -> torch.Tensor:
    t = torch.zeros(3 * BLOCK, dtype=dtype, device=device)
    t[5], t[BLOCK + 5], t[2 * BLOCK + 5] = 2.0 ** 12, 1.0, 1.0
    return t


def sumsq_and_norm(tensors, **kw):
    """(the sum of squares ``grad_norm`` hands to ``norm_reduce``, the norm)."""
    from torchft_amd import ops

    seen = []
    norm = ops.grad_norm(tensors, norm_reduce=lambda s: seen.append(s.clone()), **kw)
    assert len(seen) == 1 and seen[0].shape == (1,) and seen[0].dtype == torch.float32
    return seen[0].reshape(()), norm
