"""Fused DiLoCo outer sync: multi-tensor pseudo-gradient and outer step.

Two in-place multi-tensor ops back ``DiLoCo(..., fused_sync=True)``
(csrc/kernels/diloco_sync.hip on a HIP device, one launch per call):

``pseudograd_(outs, minuends, subtrahends)``
    ``outs[i] = minuends[i] - subtrahends[i]`` with a single rounding, i.e.
    torch's ``a - b`` bit for bit. The outputs are arbitrary tensors — in
    DiLoCo, views into the flat allreduce buckets.

``diloco_outer_step_(snapshots, params, pseudograds, momentum_bufs, ...)``
    Per element, in fp32, from the global snapshot ``g``, the averaged
    pseudo-gradient ``d``, the momentum buffer ``m`` and the local
    parameter ``l``::

        m' = mu*m + d                       (mu == 0: u = d, no buffer)
        u  = d + mu*m' if nesterov else m'
        g' = g - lr*u
        m <- T(m');  g <- T(g');  gs = float(T(g'))
        p  = gs + alpha*(l - gs)        if alpha < 0.5      # torch.lerp's
             l - (l - gs)*(1 - alpha)   otherwise           # two branches
        l <- T(p)

    which is torch.optim.SGD (dampening 0, no weight decay) on the snapshot,
    a re-snapshot, and ``lerp_(local, alpha)`` on the parameter, with three
    roundings to the storage dtype ``T`` instead of one per torch op.
    ``alpha == 0`` leaves the parameter equal to the new snapshot and
    ``alpha == 1`` leaves it untouched, both exactly.

All tensors of one call share one dtype (bf16, fp16 or fp32) and are
contiguous; zero-numel tensors are skipped.

With the fp8-quantized allreduce two more ops put the wire pack of
``torchft_amd.quantization`` in place of the pseudo-gradient tensors, so the
pseudo-gradient is never stored in the parameters' dtype
(``DiLoCo(fused_sync=True, should_quantize=True, fused_fp8_pack=True)``):

``pseudograd_fp8_(pack, minuends, subtrahends, world)``
    ``pack = quantize_pack(float(minuends[i]) - float(subtrahends[i]))``: the
    fp32 difference goes through the quantizer's block math unrounded, every
    byte of the pack is written. On CPU this is ``quantize_pack_ref``.

``diloco_outer_step_fp8_(snapshots, params, pack, first_blocks, ...)``
    ``diloco_outer_step_`` with ``d = code * (scale * fl(1/num_participants))``
    read from the reduced pack; tensor ``i`` owns the pack blocks from
    ``first_blocks[i]`` on. On CPU: ``pack_values_ref`` and
    ``diloco_outer_step_ref``.
"""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from torchft_amd.ops import hip_ext

_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _check_lists(what: str, lists: Sequence[Sequence[torch.Tensor]]) -> None:
    n = len(lists[0])
    if n == 0:
        raise ValueError(f"{what}: need at least one tensor")
    dtype, device = lists[0][0].dtype, lists[0][0].device
    if dtype not in _DTYPES:
        raise TypeError(f"{what}: unsupported dtype {dtype}")
    for ts in lists:
        if len(ts) != n:
            raise ValueError(f"{what}: list lengths differ")
        for t, ref in zip(ts, lists[0]):
            if t.dtype != dtype:
                raise TypeError(f"{what}: mixed dtypes ({dtype} and {t.dtype})")
            if t.device != device:
                raise ValueError(f"{what}: all tensors must be on one device")
            if t.numel() != ref.numel():
                raise ValueError(f"{what}: size mismatch")
            if not t.is_contiguous():
                raise ValueError(f"{what}: tensors must be contiguous")


@torch.no_grad()
def pseudograd_(
    outs: Sequence[torch.Tensor],
    minuends: Sequence[torch.Tensor],
    subtrahends: Sequence[torch.Tensor],
) -> None:
    """``outs[i] = minuends[i] - subtrahends[i]`` for the whole list at once."""
    _check_lists("pseudograd_", (outs, minuends, subtrahends))
    if outs[0].is_cuda:
        hip_ext().diloco_pseudograd(list(outs), list(minuends), list(subtrahends))
        return
    for o, a, b in zip(outs, minuends, subtrahends):
        o.copy_((a.float() - b.float()).view_as(o))


def diloco_outer_step_ref(
    g: torch.Tensor,
    d: torch.Tensor,
    m: Optional[torch.Tensor],
    l: torch.Tensor,  # noqa: E741
    *,
    lr: float,
    momentum: float,
    nesterov: bool,
    alpha: float,
    compute_dtype: torch.dtype = torch.float32,
) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
    """Plain-torch definition of the fused outer step for one tensor:
    ``(m', g', p)`` in the storage dtype, nothing modified. The math runs in
    ``compute_dtype`` with the same three roundings to the storage dtype;
    fp32 is the CPU path of ``diloco_outer_step_``, fp64 the ground truth of
    the tests. It never calls the extension."""
    T = g.dtype
    gf, df, lf = g.to(compute_dtype), d.to(compute_dtype), l.to(compute_dtype)
    m_new = None
    u = df
    if momentum != 0:
        assert m is not None
        mf = momentum * m.to(compute_dtype) + df
        m_new = mf.to(T)
        u = df + momentum * mf if nesterov else mf
    g_new = (gf - lr * u).to(T)
    gs = g_new.to(compute_dtype)
    diff = lf - gs
    p = gs + alpha * diff if alpha < 0.5 else lf - diff * (1.0 - alpha)
    return m_new, g_new, p.to(T)


@torch.no_grad()
def diloco_outer_step_(
    snapshots: Sequence[torch.Tensor],
    params: Sequence[torch.Tensor],
    pseudograds: Sequence[torch.Tensor],
    momentum_bufs: Optional[Sequence[torch.Tensor]],
    *,
    lr: float,
    momentum: float,
    nesterov: bool,
    alpha: float,
) -> None:
    """The outer step of one param group, in place on ``snapshots``,
    ``momentum_bufs`` and ``params`` (see the module docstring).
    ``momentum_bufs`` is required when ``momentum != 0`` and ignored
    otherwise."""
    lr, momentum, alpha = float(lr), float(momentum), float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must be between 0 and 1, got {alpha}")
    lists: List[Sequence[torch.Tensor]] = [snapshots, params, pseudograds]
    if momentum != 0:
        if momentum_bufs is None:
            raise ValueError("diloco_outer_step_: momentum != 0 needs momentum_bufs")
        lists.append(momentum_bufs)
    else:
        momentum_bufs = None
    _check_lists("diloco_outer_step_", lists)
    if snapshots[0].is_cuda:
        hip_ext().diloco_outer_step(
            list(snapshots), list(params), list(pseudograds),
            list(momentum_bufs) if momentum_bufs is not None else [],
            lr, momentum, bool(nesterov), alpha,
        )
        return
    _outer_step_cpu(snapshots, params, pseudograds, momentum_bufs, lr, momentum,
                    bool(nesterov), alpha)


def _outer_step_cpu(snapshots, params, pseudograds, momentum_bufs, lr, momentum,
                    nesterov, alpha) -> None:
    """The definition, tensor by tensor, in place. ``pseudograds`` may be fp32
    whatever the storage dtype is (the decoded pack)."""
    for i, (g, l, d) in enumerate(zip(snapshots, params, pseudograds)):  # noqa: E741
        m = momentum_bufs[i] if momentum_bufs is not None else None
        m_new, g_new, p = diloco_outer_step_ref(
            g, d.view_as(g), m.view_as(g) if m is not None else None, l.view_as(g),
            lr=lr, momentum=momentum, nesterov=nesterov, alpha=alpha,
        )
        if m is not None:
            m.copy_(m_new.view_as(m))
        g.copy_(g_new)
        l.copy_(p.view_as(l))


# ----------------------------------------------------------- through the fp8 pack


def _blocks(t: torch.Tensor) -> int:
    from torchft_amd.quantization import QBLOCK

    return (t.numel() + QBLOCK - 1) // QBLOCK


def _check_pack(what: str, pack: torch.Tensor, like: torch.Tensor, total_blocks: int,
                world: int) -> int:
    """The rules of the bindings, for the CPU path too. Returns the bytes of
    the pack's ``world`` slices."""
    from torchft_amd.quantization import QBLOCK

    if world < 1:
        raise ValueError(f"{what}: world must be >= 1, got {world}")
    need = -(-total_blocks // world) * (4 + QBLOCK) * world
    if pack.dtype != torch.uint8 or not pack.is_contiguous() or pack.dim() != 1:
        raise ValueError(f"{what}: pack must be a contiguous 1-D uint8 tensor")
    if pack.device != like.device:
        raise ValueError(f"{what}: pack must be on the tensors' device ({like.device})")
    if pack.numel() < need:
        raise ValueError(f"{what}: pack holds {pack.numel()} bytes, needs {need}")
    return need


@torch.no_grad()
def pseudograd_fp8_(
    pack: torch.Tensor,
    minuends: Sequence[torch.Tensor],
    subtrahends: Sequence[torch.Tensor],
    world: int,
) -> None:
    """``pack`` = the fp8 wire pack (``quantization.allocate_pack(minuends,
    world)``) of ``minuends[i] - subtrahends[i]``, the difference taken in
    fp32 and quantized from there. On a HIP device every tensor must start on
    a 16 B boundary."""
    what = "pseudograd_fp8_"
    _check_lists(what, (minuends, subtrahends))
    need = _check_pack(what, pack, minuends[0], sum(_blocks(t) for t in minuends), world)
    if pack.is_cuda:
        hip_ext().diloco_pseudograd_fp8(list(minuends), list(subtrahends), pack, world)
        return
    from torchft_amd.quantization import quantize_pack_ref

    diffs = [a.float() - b.float() for a, b in zip(minuends, subtrahends)]
    pack[:need].copy_(quantize_pack_ref(diffs, world))


@torch.no_grad()
def diloco_outer_step_fp8_(
    snapshots: Sequence[torch.Tensor],
    params: Sequence[torch.Tensor],
    pack: torch.Tensor,
    first_blocks: Sequence[int],
    pack_total_blocks: int,
    world: int,
    momentum_bufs: Optional[Sequence[torch.Tensor]],
    *,
    lr: float,
    momentum: float,
    nesterov: bool,
    alpha: float,
    num_participants: int,
) -> None:
    """``diloco_outer_step_`` for one param group whose averaged
    pseudo-gradients are read from ``pack``, the SUM-reduced wire pack of
    ``pack_total_blocks`` blocks over ``world`` slices: tensor ``i`` owns the
    blocks from ``first_blocks[i]`` on, and its pseudo-gradient is
    ``code * (scale * fl(1 / num_participants))``. The pack is not modified."""
    what = "diloco_outer_step_fp8_"
    lr, momentum, alpha = float(lr), float(momentum), float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must be between 0 and 1, got {alpha}")
    if num_participants < 1:
        raise ValueError(f"{what}: num_participants must be >= 1, got {num_participants}")
    lists: List[Sequence[torch.Tensor]] = [snapshots, params]
    if momentum != 0:
        if momentum_bufs is None:
            raise ValueError(f"{what}: momentum != 0 needs momentum_bufs")
        lists.append(momentum_bufs)
    else:
        momentum_bufs = None
    _check_lists(what, lists)
    need = _check_pack(what, pack, snapshots[0], pack_total_blocks, world)
    first_blocks = [int(b) for b in first_blocks]
    if len(first_blocks) != len(snapshots):
        raise ValueError(f"{what}: first_blocks needs one entry per tensor")
    for i, (b, t) in enumerate(zip(first_blocks, snapshots)):
        if b < 0 or b + _blocks(t) > pack_total_blocks:
            raise ValueError(
                f"{what}: first_blocks[{i}] = {b} puts a tensor of {_blocks(t)} blocks "
                f"outside the pack's {pack_total_blocks}"
            )
    inv_div = float(torch.tensor(1.0, dtype=torch.float32) / num_participants)
    if pack.is_cuda:
        hip_ext().diloco_outer_step_fp8(
            list(snapshots), list(params), pack, first_blocks, pack_total_blocks, world,
            list(momentum_bufs) if momentum_bufs is not None else [],
            lr, momentum, bool(nesterov), alpha, inv_div,
        )
        return
    from torchft_amd.quantization import pack_values_ref

    vals = pack_values_ref(pack[:need], world, inv_div)
    ds = [vals[b : b + _blocks(t)].reshape(-1)[: t.numel()]
          for b, t in zip(first_blocks, snapshots)]
    _outer_step_cpu(snapshots, params, ds, momentum_bufs, lr, momentum, bool(nesterov),
                    alpha)
