"""Flash attention with a hand-written CDNA4 backward.

Forward: aten's flash kernel (fast on gfx950, and it hands us the
logsumexp). Backward: the MFMA kernels in csrc/kernels/flash_attn_bwd.hip —
the stock backward is the single largest kernel of the Llama-8B step
(profiles/SUMMARY.md).

Constraints of the custom backward: bf16, head_dim=128, seq % 128 == 0,
dropout 0. Anything else falls back to stock SDPA.

Status: the custom backward is ON by default (opt out with
TORCHFT_AMD_CUSTOM_FA=0); the hand-written forward (fa_fwd) is numerically
pinned against aten but still behind it, so it stays opt-in
(TORCHFT_AMD_CUSTOM_FA_FWD=1). Design, measured numbers and what was tried
and dropped: docs/KERNELS.md, "flash_attn_bwd.hip" and "flash_attn_fwd.hip".

Packed sequences: ``flash_attention(..., doc_mask=DocMask...)`` keeps every
token inside its own document (causal within the document). With a mask the
hand-written forward always runs, whatever TORCHFT_AMD_CUSTOM_FA_FWD says:
aten's flash forward takes no mask. docs/KERNELS.md, "document mask".
``DocMask.positions()`` gives the position of every token inside its document,
for ``ops.qkv_rope`` to restart the rotary positions at document starts.
"""

from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional, Sequence

import torch
import torch.nn.functional as F

from torchft_amd.ops import hip_ext

_ENV = "TORCHFT_AMD_CUSTOM_FA"
_ENV_FWD = "TORCHFT_AMD_CUSTOM_FA_FWD"


def custom_fa_enabled() -> bool:
    v = os.environ.get(_ENV, "1")
    return v in ("1", "true", "True")


def custom_fa_fwd_enabled() -> bool:
    """The hand-written forward (opt-in until it beats aotriton's)."""
    v = os.environ.get(_ENV_FWD, "0")
    return v in ("1", "true", "True")


@dataclass(frozen=True)
class DocMask:
    """Document boundaries of a batch of packed rows, built once per batch and
    shared by every layer.

    Key ``j`` is visible to query ``i`` of the same row iff
    ``doc_start[b, i] <= j <= i``, equally ``j <= i < doc_end[b, j]``:
    ``doc_start[b, i]`` is the first position of the document that holds
    position ``i`` and ``doc_end[b, j]`` the exclusive end of the document
    that holds ``j``. Both are int32 ``[B, S]``, non-decreasing along S and
    consistent with each other when one of the constructors built them; the
    kernels accept any contents without an out-of-range access, but the
    values are then unspecified."""

    doc_start: torch.Tensor
    doc_end: torch.Tensor

    @staticmethod
    def _from_starts(starts: torch.Tensor) -> "DocMask":
        """starts: bool [B, S], True where a document begins (column 0 is
        forced). Device-side, no host sync."""
        if starts.dim() != 2 or starts.shape[1] == 0:
            raise ValueError(f"expected a non-empty [B, S] tensor, got {tuple(starts.shape)}")
        S = starts.shape[1]
        starts = starts.clone()
        starts[:, 0] = True
        pos = torch.arange(S, device=starts.device, dtype=torch.int32).expand_as(starts)
        # the latest start at or before i
        doc_start = torch.where(starts, pos, torch.zeros_like(pos)).cummax(dim=1).values
        # the earliest start after j, S if none: a reversed running minimum
        nxt = torch.full_like(pos, S)
        nxt[:, :-1] = torch.where(starts[:, 1:], pos[:, 1:], nxt[:, 1:])
        doc_end = nxt.flip(1).cummin(dim=1).values.flip(1)
        return DocMask(doc_start.to(torch.int32).contiguous(),
                       doc_end.to(torch.int32).contiguous())

    @classmethod
    def from_doc_ids(cls, ids: torch.Tensor) -> "DocMask":
        """ids: integer [B, S]; a new document starts wherever the id differs
        from its left neighbour."""
        starts = torch.ones_like(ids, dtype=torch.bool)
        starts[:, 1:] = ids[:, 1:] != ids[:, :-1]
        return cls._from_starts(starts)

    @classmethod
    def from_eos(cls, tokens: torch.Tensor, eos_id: int) -> "DocMask":
        """tokens: integer [B, S]; a document ends with its EOS token and the
        next token starts a new one."""
        starts = torch.ones_like(tokens, dtype=torch.bool)
        starts[:, 1:] = tokens[:, :-1] == eos_id
        return cls._from_starts(starts)

    @classmethod
    def from_lengths(cls, lengths: Sequence[Sequence[int]], S: int,
                     device=None) -> "DocMask":
        """lengths: one list of document lengths per row, each list summing
        to S. Built on the host, then moved to ``device``."""
        rows = []
        for row in lengths:
            row = [int(n) for n in row]
            if any(n <= 0 for n in row) or sum(row) != S:
                raise ValueError(f"document lengths {row} must be positive and sum to {S}")
            rows.append(torch.repeat_interleave(
                torch.arange(len(row)), torch.tensor(row)))
        return cls.from_doc_ids(torch.stack(rows).to(device))

    def positions(self) -> torch.Tensor:
        """The position of every token inside its own document, int32
        ``[B, S]``: ``arange(S) - doc_start``, so positions restart at 0 where
        a document starts. What ``ops.qkv_rope`` takes to rotate a packed
        document as it would be rotated alone. Computed on the mask's device
        without a host sync, once: the result is kept on the instance."""
        cached = self.__dict__.get("_positions")
        if cached is None:
            S = self.doc_start.shape[1]
            pos = torch.arange(S, device=self.doc_start.device, dtype=torch.int32)
            cached = (pos - self.doc_start).to(torch.int32).contiguous()
            # frozen dataclass: the cache is no field and takes no part in ==
            object.__setattr__(self, "_positions", cached)
        return cached

    def dense(self) -> torch.Tensor:
        """The mask as bool [B, 1, S, S], True = visible. For fallbacks and
        tests: S*S bytes per row."""
        S = self.doc_start.shape[1]
        pos = torch.arange(S, device=self.doc_start.device)
        i, j = pos[:, None], pos[None, :]
        return ((j <= i) & (j >= self.doc_start[:, :, None])).unsqueeze(1)


class _FlashAttentionFn(torch.autograd.Function):
    """q,k,v: [B, H, S, D] (SDPA layout), causal, GQA-native. doc_start /
    doc_end: a DocMask's arrays; with them the hand-written forward runs
    whatever TORCHFT_AMD_CUSTOM_FA_FWD says (aten's takes no mask)."""

    @staticmethod
    def forward(ctx, q, k, v, causal: bool, scale: float, doc_start=None, doc_end=None):
        ctx.doc = doc_start is not None
        if ctx.doc:
            out, lse = hip_ext().fa_fwd(q, k, v, scale, causal, doc_start, doc_end)
            ctx.save_for_backward(q, k, v, out, lse, doc_start, doc_end)
            ctx.causal = causal
            ctx.scale = scale
            return out
        if custom_fa_fwd_enabled() and q.shape[2] % 256 == 0:
            out, lse = hip_ext().fa_fwd(q, k, v, scale, causal)
        else:
            out, lse, *_ = torch.ops.aten._scaled_dot_product_flash_attention(
                q, k, v, 0.0, causal, False, scale=scale
            )
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.causal = causal
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, *doc = ctx.saved_tensors
        # D_i = rowsum(dout * out), fused fp32 kernel (no fp32 temporaries;
        # handles the model's [B,S,H,D]-backed transpose views natively)
        delta = hip_ext().fa_delta(dout, out)
        dq, dk, dv = hip_ext().fa_bwd(
            q, k, v, dout, lse, delta, ctx.scale, ctx.causal, *doc
        )
        return dq, dk, dv, None, None, None, None


def _supported(q: torch.Tensor, k: torch.Tensor) -> bool:
    return (
        q.is_cuda
        and q.dtype == torch.bfloat16
        and q.shape[-1] == 128
        and q.shape[2] % 128 == 0
        and k.shape[2] == q.shape[2]
        and q.shape[1] % k.shape[1] == 0
        and custom_fa_enabled()
        and hip_ext() is not None
    )


def flash_attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    causal: bool = True,
    scale: Optional[float] = None,
    doc_mask: Optional[DocMask] = None,
) -> torch.Tensor:
    """SDPA-compatible attention ([B, H, S, D]) with the custom backward
    where supported, stock SDPA otherwise.

    ``doc_mask`` (packed sequences, ``causal=True`` only): every query sees
    the keys of its own document up to itself. Where the kernels apply (a HIP
    device, bf16, D = 128, S % 256 == 0, equal q and k lengths, heads
    dividing, TORCHFT_AMD_CUSTOM_FA not 0, the extension built) the
    hand-written forward and backward run and skip the tiles outside a
    document. Everywhere else the mask goes to stock SDPA as a dense
    [B, 1, S, S] boolean tensor: correct, but S*S bytes per row and off the
    flash path, so slow."""
    if scale is None:
        scale = q.shape[-1] ** -0.5
    if doc_mask is not None:
        if not causal:
            raise ValueError("doc_mask needs causal=True (non-causal document masks "
                             "are not supported)")
        if _supported(q, k) and q.shape[2] % 256 == 0:
            return _FlashAttentionFn.apply(
                q, k, v, True, scale, doc_mask.doc_start, doc_mask.doc_end
            )
        return F.scaled_dot_product_attention(
            q, k, v, attn_mask=doc_mask.dense(), scale=scale,
            enable_gqa=q.shape[1] != k.shape[1],
        )
    if _supported(q, k):
        # no .contiguous(): the kernels consume both the packed [B,H,S,D]
        # layout and the model's [B,S,H,D]-backed transpose views natively
        return _FlashAttentionFn.apply(q, k, v, causal, scale)
    return F.scaled_dot_product_attention(
        q, k, v, is_causal=causal, scale=scale, enable_gqa=q.shape[1] != k.shape[1]
    )
