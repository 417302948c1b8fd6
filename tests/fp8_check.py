"""Inputs the fp8 trio (csrc/kernels/fp8_quant.hip) is held to bit for bit,
built on the CPU; shared by tests/test_quantization_cpu.py, which checks the
reference of torchft_amd/quantization.py on them, and tests/test_fp8_exact_gpu.py,
which checks the kernels against that reference.

The *enumeration block* has amax exactly 448, so both block scales are exactly
1 and the payload is the bare conversion. It holds every finite e4m3 value,
every midpoint between two neighbours of either sign (2^-10 and 3*2^-10 in
the subnormal range included) and each midpoint one ulp of the input dtype up
and down; the expected codes follow from the construction (a tie goes to the
even code), not from any cast.
"""

from __future__ import annotations

from typing import List, Tuple

import torch

QBLOCK = 2048
SHAPES = [(1,), (7,), (2047,), (2048,), (2049,), (17, 129), (0,)]  # 8 blocks
WORLDS = [1, 2, 3, 4]  # blocks_per_rank 8, 4, 3 (one padding slot), 2
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
SPECIAL = 3  # index into SHAPES of the whole-block tensor the families overwrite


def e4m3_value(code: int) -> float:
    """The value of a finite e4m3 code, from the format's definition."""
    assert code & 0x7F != 0x7F
    e, m = (code >> 3) & 0xF, code & 7
    mag = m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7)
    return -mag if code & 0x80 else mag


def _step_magnitude(t: torch.Tensor, by: int) -> torch.Tensor:
    """The next value of t's dtype further from (by=+1) or nearer to (by=-1) zero."""
    bits = {2: torch.int16, 4: torch.int32}[t.element_size()]
    return (t.view(bits) + by).view(t.dtype)


def enumeration_block(dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    """(QBLOCK values of `dtype`, the e4m3 code each must get)."""
    vals: List[torch.Tensor] = []
    codes: List[int] = []
    for sign in (0x00, 0x80):
        finite = [sign | c for c in range(0x7F)]
        vals.append(torch.tensor([e4m3_value(c) for c in finite], dtype=torch.float64).to(dtype))
        codes += finite
        for c in range(0x7E):
            lo, hi = e4m3_value(sign | c), e4m3_value(sign | (c + 1))
            mid = torch.tensor([(lo + hi) / 2], dtype=torch.float64).to(dtype)
            assert mid.double().item() == (lo + hi) / 2, "midpoint not representable"
            vals += [mid, _step_magnitude(mid, +1), _step_magnitude(mid, -1)]
            codes += [sign | (c if c % 2 == 0 else c + 1), sign | (c + 1), sign | c]
    v = torch.cat(vals)
    assert v.numel() == len(codes) <= QBLOCK
    block = torch.zeros(QBLOCK, dtype=dtype)
    block[: v.numel()] = v
    want = torch.zeros(QBLOCK, dtype=torch.uint8)
    want[: v.numel()] = torch.tensor(codes, dtype=torch.uint8)
    assert block.double().abs().max().item() == 448.0
    return block, want


FAMILIES = ["randn", "enumeration", "zeros", "subnormal", "wide"]


def family_list(family: str, dtype: torch.dtype) -> List[torch.Tensor]:
    """CPU tensors of SHAPES: randn, with the SPECIAL tensor (one whole block)
    replaced by the family's block. ``subnormal`` also makes the first block
    of the next tensor tiny but above the flush threshold."""
    gen = torch.Generator().manual_seed(77 + FAMILIES.index(family))
    ts = [torch.randn(s, generator=gen).to(dtype) for s in SHAPES]
    if family == "enumeration":
        ts[SPECIAL] = enumeration_block(dtype)[0]
    elif family == "zeros":
        ts[SPECIAL] = torch.zeros(QBLOCK, dtype=dtype)
    elif family == "subnormal":
        # fp32 subnormals (k * 2^-140); they are zeros in fp16, whose smallest
        # value is 2^-24. 448/amax overflows: the block is flushed to zero.
        k = torch.randint(-1000, 1001, (QBLOCK,), generator=gen).double()
        k[0] = 1000
        ts[SPECIAL] = (k * 2.0 ** -140).to(dtype)
        if dtype != torch.float16:
            assert 0 < ts[SPECIAL].float().abs().max().item() < 2.0 ** -126
            # amax 2^-119 > 448/FLT_MAX: live, with a subnormal dequant scale
            tiny = (torch.randn(QBLOCK, generator=gen).clamp(-3, 3) / 3 * 2.0 ** -119)
            tiny[1] = 2.0 ** -119
            ts[SPECIAL + 1][:QBLOCK] = tiny.to(dtype)
    elif family == "wide":
        # magnitudes 2^-20 ... 2^20 in one block (fp16: up to 2^14, below its largest value)
        top = 14 if dtype == torch.float16 else 20
        e = torch.randint(-20, top + 1, (QBLOCK,), generator=gen).double()
        ts[SPECIAL] = (torch.randn(QBLOCK, generator=gen).double().clamp(-2, 2) * 2.0 ** e
                       ).to(dtype)
    return ts


def same_codes(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Byte equality, except that a NaN code may carry either sign."""
    got, want = got.cpu(), want.cpu()
    nan = (want & 0x7F) == 0x7F
    return bool(torch.equal(got[~nan], want[~nan])
                and ((got[nan] & 0x7F) == 0x7F).all())
