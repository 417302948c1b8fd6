"""Inputs the MXFP4 trio (csrc/kernels/mxfp4_quant.hip) is held to bit for
bit, built on the CPU and shared by tests/test_mxfp4_cpu.py (the reference
against the definition) and tests/test_mxfp4_gpu.py (the kernels against the
reference). Shapes, worlds and dtypes are those of tests/fp8_check.py."""

import torch

from fp8_check import DTYPES, QBLOCK, SHAPES, SPECIAL, WORLDS, _step_magnitude  # noqa: F401

GROUP = 32
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
FAMILIES = ["randn", "enumeration", "zeros", "tiny", "wide", "nan", "inf"]


def enumeration_groups(dtype):
    """(2 * GROUP values of `dtype`, the e2m1 code each must get): per sign one
    group with amax exactly 6, so X = 0 and a code is the bare rounding, holding
    every e2m1 value, every midpoint between neighbours and each midpoint one
    ulp of the dtype up and down. The codes follow from the construction (a tie
    goes to the even code), not from any rounding routine."""
    vals, codes = [], []
    for sign in (0, 8):
        s = -1.0 if sign else 1.0
        group = [torch.tensor([s * g for g in GRID], dtype=torch.float64).to(dtype)]
        want = [sign | c for c in range(8)]
        for c in range(7):
            mid = torch.tensor([s * (GRID[c] + GRID[c + 1]) / 2], dtype=torch.float64).to(dtype)
            group += [mid, _step_magnitude(mid, +1), _step_magnitude(mid, -1)]
            want += [sign | (c if c % 2 == 0 else c + 1), sign | (c + 1), sign | c]
        v = torch.cat(group)
        assert v.double().abs().max().item() == 6.0
        vals += [v, torch.zeros(GROUP - v.numel(), dtype=dtype)]
        codes += want + [0] * (GROUP - v.numel())
    return torch.cat(vals), torch.tensor(codes, dtype=torch.uint8)


def family_list(family, dtype):
    """CPU tensors of SHAPES: randn, with the front of the SPECIAL tensor (one
    whole block) replaced by the family's groups."""
    gen = torch.Generator().manual_seed(177 + FAMILIES.index(family))
    ts = [torch.randn(s, generator=gen).to(dtype) for s in SHAPES]
    special = ts[SPECIAL]
    if family == "enumeration":
        special[: 2 * GROUP] = enumeration_groups(dtype)[0]
    elif family == "zeros":
        special[:] = 0
        special[5 * GROUP + 1] = -0.0
    elif family == "tiny":
        # amax below 2^-123: the lower clamp X = -125 holds, and values from
        # 2^-126 up still get non-zero codes. fp32 subnormals among them; all
        # zeros in fp16, whose smallest value is 2^-24.
        tiny = torch.randn(QBLOCK, generator=gen).double().clamp(-3, 3) * 2.0 ** -126
        tiny[GROUP : 2 * GROUP] *= 2.0 ** -12
        special[:] = tiny.to(dtype)
        assert special.float().abs().max().item() < 2.0 ** -123
    elif family == "wide":
        # neighbouring groups 40 binades apart (fp16: 32, finite below 2^16): a
        # scale taken over the wrong 32 lanes saturates one or zeroes the other
        top = 12 if dtype == torch.float16 else 20
        for g in range(0, 16, 2):
            special[g * GROUP : (g + 1) * GROUP] *= 2.0 ** top
            special[(g + 1) * GROUP : (g + 2) * GROUP] *= 2.0 ** -20
    elif family == "nan":
        special[GROUP + 8] = float("nan")
    elif family == "inf":
        special[2 * GROUP + 6] = -float("inf")
    return ts
