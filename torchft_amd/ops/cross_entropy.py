"""Fused linear + cross-entropy loss head with bounded training memory.

``linear_cross_entropy(h, weight, targets)`` is the lm-head projection and
the mean cross-entropy in one autograd node. The logits are computed
``chunk_rows`` rows at a time; for each chunk one fused pass
(csrc/kernels/fused_cross_entropy.hip on a HIP device) produces the fp32
per-row loss and overwrites the logits in place with their gradient, and the
two backward GEMMs of that chunk run at once. Nothing of size
``[rows, vocab]`` outlives its chunk, in the forward pass or in training —
only ``dh`` and ``dW`` are kept for backward.

Per row, in fp32, with ``lse = logsumexp(x)``::

    row_loss = lse - x[t] + z * lse**2
    g[j]     = grad_scale * (softmax(x)[j] * (1 + 2*z*lse) - [j == t])

A row whose target equals ``ignore_index`` has loss 0 and a zero gradient.
A target outside ``[0, V)`` that is not ``ignore_index`` is an error made
loud: that row's loss and gradient are NaN. A row with a NaN or ``+inf`` logit,
or with no finite logit at all, has a non-finite loss and no finite gradient
element (the kernel gives NaN for a ``+inf`` logit where the definition gives
a ``+inf`` loss; docs/KERNELS.md, "Numerics"). ``-inf`` logits are fine; a
target on one gives a ``+inf`` loss and a finite gradient.
"""

from __future__ import annotations

from typing import Tuple, Union

import torch

from torchft_amd.ops import hip_ext


def cross_entropy_ref(
    logits: torch.Tensor,
    targets: torch.Tensor,
    ignore_index: int = -100,
    z_loss: float = 0.0,
    grad_scale: Union[float, torch.Tensor] = 1.0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Plain-torch definition of the fused op: ``(row_loss [R], grad [R, V])``.

    Math runs in fp32 (fp64 if the logits are fp64) and both results are
    returned in that dtype. This is the CPU path of ``fused_cross_entropy_``
    and the ground truth of the tests; it never calls the extension."""
    ct = torch.float64 if logits.dtype == torch.float64 else torch.float32
    x = logits.detach().to(ct)
    V = x.shape[-1]
    lse = torch.logsumexp(x, dim=-1)
    valid = targets != ignore_index
    in_range = (targets >= 0) & (targets < V)
    hit = valid & in_range
    safe_t = torch.where(hit, targets, torch.zeros_like(targets)).unsqueeze(1)
    xt = x.gather(1, safe_t).squeeze(1)
    loss = lse - xt + z_loss * lse * lse
    grad = torch.exp(x - lse.unsqueeze(1)) * (1.0 + 2.0 * z_loss * lse).unsqueeze(1)
    grad.scatter_add_(1, safe_t, -hit.to(ct).unsqueeze(1))
    if isinstance(grad_scale, torch.Tensor):
        grad_scale = grad_scale.detach().to(ct).reshape(())
    grad = grad * grad_scale
    zero = torch.zeros((), dtype=ct, device=x.device)
    nan = torch.full((), float("nan"), dtype=ct, device=x.device)
    loss = torch.where(valid, torch.where(in_range, loss, nan), zero)
    grad = torch.where(
        valid.unsqueeze(1), torch.where(in_range.unsqueeze(1), grad, nan), zero
    )
    return loss, grad


def fused_cross_entropy_(
    logits: torch.Tensor,
    targets: torch.Tensor,
    *,
    ignore_index: int = -100,
    z_loss: float = 0.0,
    grad_scale: Union[float, torch.Tensor] = 1.0,
    write_grad: bool = True,
) -> torch.Tensor:
    """fp32 per-row loss of ``logits`` [R, V]; with ``write_grad`` the logits
    are overwritten IN PLACE by ``grad_scale * d(row_loss)/d(logits)``.

    On a HIP device this is one launch of the gfx950 kernel (bf16,
    contiguous logits; ``grad_scale`` may be a 1-element device tensor so the
    caller never syncs). On CPU it is ``cross_entropy_ref`` with the gradient
    copied into ``logits``, so both paths have the same in-place contract."""
    if z_loss < 0:
        raise ValueError(f"z_loss must be >= 0, got {z_loss}")
    if logits.is_cuda:
        if not isinstance(grad_scale, torch.Tensor):
            grad_scale = torch.full(
                (1,), float(grad_scale), dtype=torch.float32, device=logits.device
            )
        if grad_scale.numel() != 1:
            raise ValueError(
                f"grad_scale must have one element, got {grad_scale.numel()}"
            )
        return hip_ext().cross_entropy_fwd_bwd(
            logits, targets, int(ignore_index), float(z_loss),
            grad_scale.reshape(1), bool(write_grad),
        )
    loss, grad = cross_entropy_ref(logits, targets, ignore_index, z_loss, grad_scale)
    if write_grad:
        logits.copy_(grad)
    return loss.float()


class _LinearCrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(  # type: ignore[override]
        ctx, h, weight, targets, chunk_rows, ignore_index, z_loss, need_h, need_w
    ):
        n = h.shape[0]
        n_valid = (targets != ignore_index).sum()
        # device-side 1 / max(n_valid, 1): no host sync, and the all-ignored
        # batch gets loss 0 and zero gradients instead of 0/0
        grad_scale = n_valid.clamp(min=1).to(torch.float32).reciprocal().reshape(1)
        dh = torch.empty_like(h) if need_h else None
        dw = torch.zeros_like(weight) if need_w else None
        write_grad = need_h or need_w
        row_losses = []
        for i in range(0, n, chunk_rows):
            h_c = h[i : i + chunk_rows]
            logits = torch.mm(h_c, weight.t())
            row_losses.append(
                fused_cross_entropy_(
                    logits, targets[i : i + chunk_rows], ignore_index=ignore_index,
                    z_loss=z_loss, grad_scale=grad_scale, write_grad=write_grad,
                )
            )
            # logits now holds dlogits for this chunk
            if need_h:
                torch.mm(logits, weight, out=dh[i : i + chunk_rows])
            if need_w:
                dw.addmm_(logits.t(), h_c)
            del logits
        if row_losses:
            total = torch.cat(row_losses).sum()
        else:
            total = torch.zeros((), dtype=torch.float32, device=h.device)
        ctx.save_for_backward(dh, dw)
        return total * grad_scale.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):  # type: ignore[override]
        dh, dw = ctx.saved_tensors
        # grad_out is a 0-dim fp32 tensor: the product keeps dh/dW's dtype
        gh = dh * grad_out if dh is not None else None
        gw = dw * grad_out if dw is not None else None
        return gh, gw, None, None, None, None, None, None


def linear_cross_entropy(
    h: torch.Tensor,
    weight: torch.Tensor,
    targets: torch.Tensor,
    *,
    chunk_rows: int = 4096,
    ignore_index: int = -100,
    z_loss: float = 0.0,
) -> torch.Tensor:
    """Mean cross-entropy of ``h @ weight.T`` against ``targets`` as a scalar
    fp32 loss, without ever holding more than ``chunk_rows`` rows of logits.

    ``h`` is ``[..., D]``, ``weight`` ``[V, D]``, ``targets`` ``[...]``
    (int64). The mean runs over the targets that differ from
    ``ignore_index`` (``F.cross_entropy(reduction="mean")`` semantics), with
    one exception: if EVERY target is ignored the loss is 0 and all
    gradients are 0, where torch returns NaN. ``z_loss`` adds
    ``z_loss * logsumexp(logits)**2`` per row.

    The gradients w.r.t. ``h`` and ``weight`` are computed during the
    forward pass, chunk by chunk, and are the only tensors kept for
    backward; backward scales them by the incoming gradient. With no input
    requiring grad (or under ``torch.no_grad()``) the gradient pass and both
    backward GEMMs are skipped. bf16 on a HIP device; fp32/bf16 on CPU."""
    if chunk_rows < 1:
        raise ValueError(f"chunk_rows must be >= 1, got {chunk_rows}")
    if z_loss < 0:
        raise ValueError(f"z_loss must be >= 0, got {z_loss}")
    if h.is_cuda and (h.dtype != torch.bfloat16 or weight.dtype != torch.bfloat16):
        raise TypeError("linear_cross_entropy on a device requires bf16 h and weight")
    h2 = h.reshape(-1, h.shape[-1])
    t = targets.reshape(-1)
    if t.shape[0] != h2.shape[0]:
        raise ValueError(
            f"targets has {t.shape[0]} elements for {h2.shape[0]} rows of h"
        )
    grad_on = torch.is_grad_enabled()
    return _LinearCrossEntropyFn.apply(
        h2, weight, t, int(chunk_rows), int(ignore_index), float(z_loss),
        grad_on and h.requires_grad, grad_on and weight.requires_grad,
    )
