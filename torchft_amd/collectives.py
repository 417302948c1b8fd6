"""Quantized collective algorithms over RCCL.

``allreduce_quantized`` decomposes the allreduce into
quantize → **alltoall** of per-rank slices → fused local reduce →
**allgather** of the reduced slice → dequantize, cutting wire traffic ~4x
at fp8 vs bf16 (8x vs fp32). On MI355X xGMI is 7 point-to-point links per
GPU, so the alltoall+allgather decomposition engages all links instead of
serializing on a single ring. ``wire="mxfp4"`` sends e2m1 codes with one
power-of-two scale byte per 32 elements instead (``csrc/kernels/mxfp4_quant.hip``):
0.530 of the fp8 pack's bytes.

``allreduce_pack`` is the same exchange for a caller that already holds the
quantized pack and decodes the result itself (the fused DiLoCo outer sync,
``ops.pseudograd_fp8_`` / ``ops.diloco_outer_step_fp8_``): alltoall → fused
local reduce → allgather, in place on the pack, with no quantize or
dequantize step around it.

Reference parity (semantics): torchft/collectives.py:159-415.
"""

from __future__ import annotations

from datetime import timedelta
from typing import List, Optional

import torch
from torch.distributed import ReduceOp, Work
from torch.distributed.distributed_c10d import AllgatherOptions, AllToAllOptions
from torch.futures import Future

from torchft_amd import quantization as Q
from torchft_amd.process_group import ProcessGroup


class _QuantizedWork(Work):
    """Completes when the dequantize at the tail of the pipeline is enqueued;
    wait() makes the caller's current stream depend on the sync stream."""

    def __init__(
        self,
        fut: Future,
        sync_stream: torch.cuda.Stream,
        tensors: List[torch.Tensor],
    ) -> None:
        super().__init__()
        self._fut = fut
        self._sync_stream = sync_stream
        self._tensors = tensors
        self._event: Optional[torch.cuda.Event] = None

    def _ensure_event(self) -> None:
        if self._event is None:
            self._fut.wait()
            with torch.cuda.stream(self._sync_stream):
                self._event = torch.cuda.Event()
                self._event.record()

    def wait(self, timeout: Optional[timedelta] = None) -> bool:
        self._ensure_event()
        assert self._event is not None
        self._event.wait()  # current stream waits on the dequant tail
        return True

    def block_current_stream(self, timeout: Optional[timedelta] = None) -> None:
        self.wait()

    def get_future(self) -> Future:
        return self._fut


WIRES = {"fp8": "", "mxfp4": "mx_"}  # wire format -> prefix of its functions in quantization


def _wire(wire: str):
    """(geometry, quantize, reduce, dequantize) of a wire format, looked up in
    ``quantization`` at call time."""
    if wire not in WIRES:
        raise ValueError(f"unknown wire format {wire!r}: expected one of {sorted(WIRES)}")
    return tuple(getattr(Q, WIRES[wire] + name) for name in
                 ("pack_geometry", "quantize_pack", "reduce_slices", "dequantize_pack"))


def allreduce_quantized(
    tensors: List[torch.Tensor],
    op: ReduceOp,
    pg: ProcessGroup,
    sync_stream: Optional[torch.cuda.Stream] = None,
    wire: str = "fp8",
) -> Work:
    """Fault-tolerant quantized allreduce of ``tensors`` (in place).

    op must be SUM or AVG (the fused reduce kernel applies 1/world itself —
    no extra pass). ``wire`` is the format that travels: ``"fp8"`` (e4m3 in
    2048-element blocks, 8.02 bits per element) or ``"mxfp4"`` (e2m1 codes
    with one power-of-two scale byte per 32 elements, 4.25 bits per element).
    """
    assert torch.cuda.is_available(), "quantized allreduce requires a HIP device"
    world = pg.size()
    avg = op == ReduceOp.AVG
    geometry, quantize, reduce, dequantize = _wire(wire)

    _, _, _, slice_bytes = geometry(tensors, world)
    device = tensors[0].device

    if sync_stream is None:
        sync_stream = torch.cuda.Stream()

    # the comm/kernel pipeline runs on sync_stream, ordered after the
    # caller's current stream
    sync_stream.wait_stream(torch.cuda.current_stream())

    with torch.cuda.stream(sync_stream):
        pack = torch.empty(world * slice_bytes, dtype=torch.uint8, device=device)
        quantize(tensors, pack, world)

        recv = torch.empty_like(pack)  # world copies of OUR slice
        a2a_work = pg.alltoall_base(recv, pack, [], [], AllToAllOptions())
        a2a_work.wait()

        my_slice = pack.narrow(0, 0, slice_bytes)  # reuse pack's first slice slot
        reduce(recv.view(world, slice_bytes).view(-1), my_slice, world, avg)

        ag_work = pg.allgather_into_tensor_coalesced([pack], [my_slice.clone()],
                                                     AllgatherOptions())
        fut = ag_work.get_future()

        def _dequant(f: Future) -> List[torch.Tensor]:
            with torch.cuda.stream(sync_stream):
                f.wait()
                dequantize(tensors, pack, world)
            return tensors

        fut = fut.then(_dequant)

    return _QuantizedWork(fut, sync_stream, tensors)


def allreduce_pack(
    pack: torch.Tensor,
    world: int,
    op: ReduceOp,
    pg: ProcessGroup,
    sync_stream: Optional[torch.cuda.Stream] = None,
) -> Work:
    """The middle of ``allreduce_quantized`` on a pack the caller has already
    quantized for ``world`` ranks (``ops.pseudograd_fp8_``), in place:
    alltoall of the slices, fused reduce (requantizing) into the first slice
    slot, allgather back into ``pack``. Nothing is quantized from or
    dequantized into tensors; the caller decodes the pack
    (``ops.diloco_outer_step_fp8_``). ``op`` is SUM or AVG as above."""
    assert torch.cuda.is_available(), "the pack allreduce requires a HIP device"
    if world != pg.size():
        raise ValueError(
            f"allreduce_pack: the pack was laid out for world {world}, the process "
            f"group has {pg.size()} ranks"
        )
    slice_bytes = pack.numel() // world
    if (pack.dtype != torch.uint8 or not pack.is_contiguous() or not pack.is_cuda
            or slice_bytes * world != pack.numel() or slice_bytes % (4 + Q.QBLOCK)):
        raise ValueError(
            "allreduce_pack: pack must be a contiguous uint8 device tensor of "
            f"{world} slices of whole blocks, got {pack.numel()} bytes"
        )
    avg = op == ReduceOp.AVG

    if sync_stream is None:
        sync_stream = torch.cuda.Stream()
    sync_stream.wait_stream(torch.cuda.current_stream())

    with torch.cuda.stream(sync_stream):
        recv = torch.empty_like(pack)  # world copies of OUR slice
        pg.alltoall_base(recv, pack, [], [], AllToAllOptions()).wait()

        my_slice = pack.narrow(0, 0, slice_bytes)
        Q.reduce_slices(recv, my_slice, world, avg)

        ag_work = pg.allgather_into_tensor_coalesced([pack], [my_slice.clone()],
                                                     AllgatherOptions())
        fut = ag_work.get_future()

    return _QuantizedWork(fut, sync_stream, [pack])


def reduce_scatter_quantized(
    tensors: List[torch.Tensor],
    op: ReduceOp,
    pg: ProcessGroup,
    sync_stream: Optional[torch.cuda.Stream] = None,
    wire: str = "fp8",
) -> tuple[Work, torch.Tensor]:
    """Quantized reduce-scatter: returns (work, out) where ``out`` is this
    rank's reduced share — ``blocks_per_rank * QBLOCK`` elements of the
    block-padded concatenation of ``tensors``, dequantized to the input
    dtype (zero-padded tail). ``wire`` as in ``allreduce_quantized``."""
    assert torch.cuda.is_available(), "quantized reduce_scatter requires a HIP device"
    world = pg.size()
    avg = op == ReduceOp.AVG
    geometry, quantize, reduce, dequantize = _wire(wire)

    _, _, bpr, slice_bytes = geometry(tensors, world)
    device = tensors[0].device
    if sync_stream is None:
        sync_stream = torch.cuda.Stream()
    sync_stream.wait_stream(torch.cuda.current_stream())

    out = torch.empty(bpr * Q.QBLOCK, dtype=tensors[0].dtype, device=device)

    with torch.cuda.stream(sync_stream):
        pack = torch.empty(world * slice_bytes, dtype=torch.uint8, device=device)
        quantize(tensors, pack, world)

        recv = torch.empty_like(pack)
        pg.alltoall_base(recv, pack, [], [], AllToAllOptions()).wait()

        my_slice = torch.empty(slice_bytes, dtype=torch.uint8, device=device)
        reduce(recv, my_slice, world, avg)
        # dequantize only our slice into the flat output
        dequantize([out], my_slice, 1)

        fut: Future = Future()
        fut.set_result([out])

    return _QuantizedWork(fut, sync_stream, [out]), out
