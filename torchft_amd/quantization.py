"""fp8 (OCP e4m3) block quantization for gradient collectives.

Thin tensor-level wrapper over the CDNA4 kernels in
``csrc/kernels/fp8_quant.hip`` plus a pure-torch reference implementation of
the exact packed layout (ground truth for the GPU numerics tests and a CPU
way to reason about the format).

Packed wire layout (per all-reduce world of size W): W equal slices; slice r
= ``[fp32 dequant-scales of its blocks] ‖ [QBLOCK fp8 bytes per block]``.
Blocks are 2048 elements; each tensor is padded to whole blocks so a block
never straddles tensors. Reference analogue: torchft/quantization.py
(Triton, per-row striping) — re-designed block-wise for MI355X (see the .hip
header comment).
"""

from __future__ import annotations

from typing import List, Tuple

import torch

from torchft_amd.ops import hip_ext

QBLOCK = 2048
FP8_MAX = 448.0


def pack_geometry(tensors: List[torch.Tensor], world: int) -> Tuple[int, int, int, int]:
    """Returns (total_blocks, padded_blocks, blocks_per_rank, slice_bytes)."""
    total = sum((t.numel() + QBLOCK - 1) // QBLOCK for t in tensors)
    padded = ((total + world - 1) // world) * world
    bpr = padded // world
    slice_bytes = bpr * (4 + QBLOCK)
    return total, padded, bpr, slice_bytes


def allocate_pack(tensors: List[torch.Tensor], world: int) -> torch.Tensor:
    _, _, _, slice_bytes = pack_geometry(tensors, world)
    return torch.empty(world * slice_bytes, dtype=torch.uint8, device=tensors[0].device)


def quantize_pack(tensors: List[torch.Tensor], pack: torch.Tensor, world: int) -> None:
    hip_ext().fp8_quantize(tensors, pack, world)


def dequantize_pack(tensors: List[torch.Tensor], pack: torch.Tensor, world: int) -> None:
    hip_ext().fp8_dequantize(tensors, pack, world)


def reduce_slices(recv: torch.Tensor, out: torch.Tensor, world: int, avg: bool) -> None:
    hip_ext().fp8_reduce(recv, out, world, avg)


# --------------------------------------------------------------- reference
#
# What the kernels compute, operation for operation, in fp32 torch (meant for
# the CPU, where torch's float8_e4m3fn cast rounds to nearest, ties to even,
# like the hardware conversion). The GPU tests hold the kernels to these bytes.

E4M3_NAN = 0x7F  # the kernels' NaN code may also carry the sign bit (0xFF)


def e4m3_codes(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> OCP e4m3 bytes as the kernels convert: finite values are clamped
    to +-448 and rounded to nearest even, NaN and +-Inf become NaN."""
    x = x.float()
    finite = torch.isfinite(x)
    y = torch.where(finite, x.clamp(-FP8_MAX, FP8_MAX), torch.zeros_like(x))
    codes = y.to(torch.float8_e4m3fn).view(torch.uint8)
    return torch.where(finite, codes, torch.full_like(codes, E4M3_NAN))


def e4m3_values(codes: torch.Tensor) -> torch.Tensor:
    """e4m3 bytes -> fp32 (exact)."""
    return codes.view(torch.float8_e4m3fn).float()


def block_scales_ref(blocks: torch.Tensor, inv_div: float = 1.0):
    """(amax, q_scale, dq_scale) of [n, QBLOCK] fp32 blocks, the kernels'
    rule (block_scales, fp8_quant.hip): amax over the non-NaN elements
    (fmaxf drops a NaN), 448/amax and (amax/448)*inv_div in fp32, zeros for an
    all-zero block and for one whose 448/amax overflows (amax < 1.3e-36)."""
    a = blocks.abs()
    amax = torch.where(torch.isnan(a), torch.zeros_like(a), a).amax(dim=1)
    pos = amax > 0
    # tensor / tensor: torch evaluates scalar / tensor as scalar * reciprocal,
    # which is not the correctly rounded quotient the device computes
    top = torch.full_like(amax, FP8_MAX)
    q = torch.where(pos, top / torch.where(pos, amax, top), torch.zeros_like(amax))
    dq = torch.where(pos, (amax / top) * torch.full_like(amax, inv_div),
                     torch.zeros_like(amax))
    flush = torch.isinf(q)
    q = torch.where(flush, torch.zeros_like(q), q)
    dq = torch.where(flush, torch.zeros_like(dq), dq)
    return amax, q, dq


def _write_slices(scales: torch.Tensor, codes: torch.Tensor, world: int) -> torch.Tensor:
    """[world*bpr] fp32 scales + [world*bpr, QBLOCK] bytes -> the packed buffer."""
    bpr = scales.numel() // world if world else 0
    pack = torch.cat(
        [scales.contiguous().view(torch.uint8).view(world, bpr * 4),
         codes.contiguous().view(world, bpr * QBLOCK)], dim=1)
    return pack.reshape(-1)


def split_slices(pack: torch.Tensor, slices: int):
    """A buffer of `slices` equal slices -> ([slices, bpr] fp32 scales,
    [slices, bpr, QBLOCK] bytes)."""
    slice_bytes = pack.numel() // slices if slices else 0
    bpr = slice_bytes // (4 + QBLOCK)
    sl = pack.view(slices, slice_bytes)
    scales = sl[:, : bpr * 4].contiguous().view(torch.float32).view(slices, bpr)
    codes = sl[:, bpr * 4:].contiguous().view(slices, bpr, QBLOCK)
    return scales, codes


def quantize_pack_ref(tensors: List[torch.Tensor], world: int) -> torch.Tensor:
    """Pure-torch construction of the packed wire buffer, every byte of it:
    scales, payload, zero padding inside a tensor's last block, and padding
    slots (scale 0, zero payload). Non-finite input as the kernel treats it: a
    NaN element stays NaN and leaves its block's scale alone, a block holding
    +-Inf gets scale inf, zero codes for its finite elements and NaN for the
    rest, so it decodes to NaN everywhere."""
    total, padded, bpr, slice_bytes = pack_geometry(tensors, world)
    dev = tensors[0].device
    allb = torch.zeros(padded, QBLOCK, dtype=torch.float32, device=dev)
    b = 0
    for t in tensors:
        flat = t.detach().float().reshape(-1)
        nb = (flat.numel() + QBLOCK - 1) // QBLOCK
        allb[b : b + nb].view(-1)[: flat.numel()] = flat
        b += nb
    _, q, dq = block_scales_ref(allb)
    codes = e4m3_codes(allb * q[:, None])
    return _write_slices(dq, codes, world)


def dequantize_pack_ref(
    shapes_numels: List[int], pack: torch.Tensor, world: int
) -> List[torch.Tensor]:
    """Decode a packed buffer into flat fp32 tensors of the given numels:
    ``code * scale``, one fp32 product per element."""
    total = sum((n + QBLOCK - 1) // QBLOCK for n in shapes_numels)
    scales, codes = split_slices(pack, world)
    vals = e4m3_values(codes.reshape(-1, QBLOCK)) * scales.reshape(-1)[:, None]
    out = []
    b = 0
    for n in shapes_numels:
        nb = (n + QBLOCK - 1) // QBLOCK
        out.append(vals[b : b + nb].reshape(-1)[:n].clone())
        b += nb
    assert b == total
    return out


def reduce_slices_ref(recv: torch.Tensor, world: int, avg: bool,
                      fused: bool = False) -> torch.Tensor:
    """The fused reduce on `world` received slices: fp32 accumulation of
    ``code * scale`` in rank order from zero, then requantization with the
    quantizer's rule, AVG folding fl(1/world) into the stored scale.
    ``fused=False`` rounds the product and the sum separately; ``fused=True``
    is a fused multiply-add, evaluated in fp64 (the product is exact there,
    the sum too while the operands span fewer than 53 bits, which the caller
    has to ensure) and rounded to fp32 once."""
    scales, codes = split_slices(recv, world)
    acc = torch.zeros(codes.shape[1:], dtype=torch.float32, device=recv.device)
    for r in range(world):
        vals, sc = e4m3_values(codes[r]), scales[r][:, None]
        if fused:
            acc = (acc.double() + vals.double() * sc.double()).float()
        else:
            acc = acc + vals * sc
    inv_div = float(torch.tensor(1.0, dtype=torch.float32) / world) if avg else 1.0
    _, q, dq = block_scales_ref(acc, inv_div)
    return _write_slices(dq, e4m3_codes(acc * q[:, None]), 1)
