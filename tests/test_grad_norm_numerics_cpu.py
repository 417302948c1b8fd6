"""CPU tests of the grad-norm checker (tests/grad_norm_check.py) that
tests/test_grad_norm_numerics_gpu.py holds the kernels to: the emulation of
the reduction order is exact on the exact families and inside the bound on the
others, each mistake worth catching is refused by the criterion meant to see
it, and the plain-torch path of ``grad_norm`` / ``clip_grad_norm_`` meets the
same families."""

import math

import pytest
import torch

from grad_norm_check import (BEACON_LOG2, BLOCK, CLIP_INJECTIONS, DTYPES, FINALIZE_SECOND_TRIP,
                             SUMSQ_INJECTIONS, ZOO, beacon_positions, check_norm, clip_expected,
                             coef_from_sumsq32, depth, hold_clip_bits, hold_exact, ones_list,
                             staircase, sumsq_and_norm, sumsq_emulated)
from torchft_amd import ops

ZOO_N = [math.prod(s) for s in ZOO]
LISTS = {"zoo": ZOO_N, "257 blocks": [FINALIZE_SECOND_TRIP], "mostly empty last block":
         [3 * BLOCK + 5]}


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("name", sorted(LISTS))
def test_emulation_is_exact_on_ones_and_beacons(name, dtype):
    numels = LISTS[name]
    for mb in (1, 2, 2048):
        hold_exact(sumsq_emulated(ones_list(numels, dtype), mb), float(sum(numels)), f"ones {mb}")
    k = BEACON_LOG2[dtype]
    ts = [torch.zeros(n, dtype=dtype) for n in numels]
    for i, e in beacon_positions(numels):
        ts[i][e] = 2.0 ** k
        hold_exact(sumsq_emulated(ts), 4.0 ** k, f"beacon at {i}:{e}")
        ts[i][e] = 0
    hold_exact(sumsq_emulated([staircase(dtype)]), 2.0 ** 24 + 2, "staircase")


def _bounded(name, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(5)
    if name == "one 2^60 among ones":
        ts = ones_list(ZOO_N, dtype)
        ts[5][2048] = 2.0 ** 60
        return ts
    scale = {"randn": 1.0, "randn 2^-10": 2.0 ** -10, "randn 2^40": 2.0 ** 40,
             "randn 2^-80": 2.0 ** -80}[name]
    return [(scale * torch.randn(n, generator=g)).to(dtype) for n in ZOO_N]


BOUNDED = ("randn", "randn 2^-10", "randn 2^40", "randn 2^-80", "one 2^60 among ones")


@pytest.mark.parametrize("name", BOUNDED)
def test_emulation_is_inside_the_bound(name):
    ts = _bounded(name)
    for mb in (3, 2048):
        frac = check_norm(sumsq_emulated(ts, mb).sqrt(), ts, depth(ZOO_N, mb), f"{name} {mb}")
    if name == "randn 2^-80":  # every square is below the smallest fp32 number
        assert float(sumsq_emulated(ts)) == 0.0 and frac > 0


def test_overflow_is_an_inf_norm():
    ts = [torch.full((n,), 2.0 ** 64, dtype=torch.bfloat16) for n in (8, 2049)]
    assert torch.isfinite(torch.cat(ts)).all()
    assert float(sumsq_emulated(ts)) == math.inf
    assert float(ops.grad_norm(ts)) == math.inf  # the plain-torch path agrees


# (mistake, the criterion that refuses it)
def _refuse_partials_beyond_256_dropped(inject):
    hold_exact(sumsq_emulated(ones_list([FINALIZE_SECOND_TRIP], torch.bfloat16), inject=inject),
               float(FINALIZE_SECOND_TRIP), "ones, 257 blocks")


def _refuse_last_partial_vector_skipped(inject):
    hold_exact(sumsq_emulated(ones_list(ZOO_N, torch.bfloat16), inject=inject),
               float(sum(ZOO_N)), "ones, zoo")


def _refuse_misaligned_skips_element_0(inject):
    t = torch.zeros(4097, dtype=torch.bfloat16)
    t[0] = 2.0 ** 20
    hold_exact(sumsq_emulated([t], misaligned=[True], inject=inject), 2.0 ** 40, "beacon at 0")


def _refuse_finalize_fp32(inject):
    hold_exact(sumsq_emulated([staircase(torch.float32)], inject=inject), 2.0 ** 24 + 2,
               "staircase")


SUMSQ_REFUSALS = {
    "partials_beyond_256_dropped": _refuse_partials_beyond_256_dropped,
    "last_partial_vector_skipped": _refuse_last_partial_vector_skipped,
    "empty_lane_reads_one": _refuse_last_partial_vector_skipped,
    "misaligned_skips_element_0": _refuse_misaligned_skips_element_0,
    "finalize_fp32": _refuse_finalize_fp32,
}


@pytest.mark.parametrize("inject", SUMSQ_INJECTIONS)
def test_injected_reduction_mistake_is_refused_by_an_exact_family(inject):
    SUMSQ_REFUSALS[inject](None)  # the correct order passes the same call
    with pytest.raises(AssertionError, match="exact"):
        SUMSQ_REFUSALS[inject](inject)


def test_a_dropped_partial_passes_the_bound_on_randn_alone():
    """Why the exact families are the core: a lost partial of a quiet block
    stays inside the bound on randn; on ones it is 2048 short."""
    g = torch.Generator().manual_seed(1)
    t = torch.randn(FINALIZE_SECOND_TRIP, generator=g).bfloat16()
    t[-BLOCK:] *= 2.0 ** -8  # a quiet last block: 1.2e-7 of the sum
    got = sumsq_emulated([t], inject="partials_beyond_256_dropped").sqrt()
    check_norm(got, [t], depth([t.numel()]), "dropped quiet partial")


def _clip_case(dtype, scale=2.0 ** -14):
    """A norm of 5e-3: the 1e-6 moves the coefficient by 2e-4, which 5 % of
    7056 bf16 elements feel."""
    g = torch.Generator().manual_seed(9)
    grads = [(scale * torch.randn(n, generator=g)).to(dtype) for n in (7, 2049, 5000)]
    sumsq = sumsq_emulated(grads)
    # not a power of two: g * 0.5 is a bf16 number that a 2e-4 cannot move
    return grads, sumsq, 0.37 * float(sumsq.sqrt())


# an fp32 store rounds nothing: no truncation to refuse there
CLIP_REFUSED = [(i, d) for i in CLIP_INJECTIONS for d in DTYPES
                if not (i == "truncating_store" and d == torch.float32)]


@pytest.mark.parametrize("inject,dtype", CLIP_REFUSED, ids=str)
def test_injected_clip_mistake_is_refused_by_the_bits(inject, dtype):
    grads, sumsq, max_norm = _clip_case(dtype)
    want = clip_expected(grads, sumsq, max_norm)
    hold_clip_bits(clip_expected(grads, sumsq, max_norm), want, "correct")
    with pytest.raises(AssertionError, match="clip bits"):
        hold_clip_bits(clip_expected(grads, sumsq, max_norm, inject=inject), want, inject)


def test_coefficient_at_the_threshold():
    s = torch.tensor(4096.0)  # norm 64: 64 + 1e-6 rounds to 64
    assert float(coef_from_sumsq32(s, 64.0)) == 1.0
    assert float(coef_from_sumsq32(s, 64.0 * (1 - 2.0 ** -24))) < 1.0
    assert float(coef_from_sumsq32(s, 65.0)) == 1.0
    s = torch.tensor(1.0)  # norm 1: the 1e-6 is felt
    assert float(coef_from_sumsq32(s, 1.0)) < 1.0
    # four times the sum of squares halves the coefficient, up to the 1e-6
    assert float(coef_from_sumsq32(4 * torch.tensor(4096.0), 32.0)) == 0.25


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_plain_torch_path_on_the_same_families(dtype):
    hold_exact(sumsq_and_norm(ones_list(ZOO_N, dtype))[0], float(sum(ZOO_N)), "ones")
    k = BEACON_LOG2[dtype]
    ts = [torch.zeros(n, dtype=dtype) for n in ZOO_N]
    for i, e in beacon_positions(ZOO_N):
        ts[i][e] = 2.0 ** k
        assert float(ops.grad_norm(ts)) == 2.0 ** k
        ts[i][e] = 0
    for name in BOUNDED:
        if dtype == torch.float16 and name != "randn":
            continue  # outside fp16's range
        ts = _bounded(name, dtype)
        check_norm(ops.grad_norm(ts), ts, 1, f"plain torch {name}")
    # the clip: fp32 coefficient, one rounding into the gradient's dtype
    grads, _, _ = _clip_case(dtype)
    params = [torch.zeros_like(g).requires_grad_(True) for g in grads]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    max_norm = 0.5 * float(ops.grad_norm(grads))
    ops.clip_grad_norm_(params, max_norm)
    want = clip_expected(grads, sumsq_and_norm(grads)[0], max_norm)
    for p, w in zip(params, want):
        torch.testing.assert_close(p.grad.float(), w.float(), rtol=2.0 ** -7, atol=0)
    # a NaN leaves every bit alone
    grads[1][77] = math.nan
    for p, g in zip(params, grads):
        p.grad = g.clone()
    assert math.isnan(float(ops.clip_grad_norm_(params, 1e-3)))
    grads[1][77] = params[1].grad[77]  # NaN * 1.0 is a NaN, torch may quieten its bits
    hold_clip_bits([p.grad for p in params], grads, "NaN")
