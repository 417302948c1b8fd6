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
    for i, (g, l, d) in enumerate(zip(snapshots, params, pseudograds)):  # noqa: E741
        m = momentum_bufs[i] if momentum_bufs is not None else None
        m_new, g_new, p = diloco_outer_step_ref(
            g, d.view_as(g), m.view_as(g) if m is not None else None, l.view_as(g),
            lr=lr, momentum=momentum, nesterov=bool(nesterov), alpha=alpha,
        )
        if m is not None:
            m.copy_(m_new.view_as(m))
        g.copy_(g_new)
        l.copy_(p.view_as(l))
