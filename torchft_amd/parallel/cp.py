"""Context parallelism (sequence sharding) for long-context Llama training.

New scope relative to the reference: torchft has no sequence-parallel code
 — it treats everything inside a replica group as opaque.
This module supplies that slot natively so the Llama-3 long-context configs
run inside a replica group while the cross-replica FT dimension stays
unchanged.

Design (MI355X-first): **all-gather-KV context parallelism.** Each CP rank
holds a contiguous sequence shard of Q/K/V; K and V are all-gathered along
the sequence so every rank runs flash attention for its Q shard against the
full context. With Llama-3 GQA (8 KV heads × 128 dim) the gathered KV is
2 KB/token/layer — at 128k context that is ~256 MB/layer against 288 GB
HBM3E, and the gather is a large contiguous allgather that RCCL drives over
all 7 xGMI links. This is the scheme Llama-3's own long-context training
used; a ring-attention (block-rotating) variant saves the KV residency at
the cost of 2(W-1) p2p hops per layer and is the planned upgrade for
>512k contexts (``ring_attention`` below; with ``TORCHFT_AMD_RING_FA=1`` its
compute runs on the hand-written kernels, the softmax state carried from hop
to hop: docs/KERNELS.md, "Ring attention: carried state").

Backward: dK/dV are computed for the full context on every rank and
reduce-scattered (sum) back to the owning shard.

What a rank computes after the gather is :func:`cp_rank_attention`. By default
that is the flash + LSE merge below (``_MergedFlashAttn``); with
``TORCHFT_AMD_CP_RECT=1`` (or ``CPPlan(rect=True)``) it is one
``ops.flash_attention_rect`` call on the keys up to the rank's own: the
hand-written rectangular kernels (docs/KERNELS.md, "Rectangular attention").
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch.distributed.distributed_c10d import AllgatherOptions, AllreduceOptions, ReduceOp

from torchft_amd.ops import hip_ext
from torchft_amd.ops.flash_attention import (
    _fold_supported,
    _rect_supported,
    flash_attention_fold,
    flash_attention_rect,
)
from torchft_amd.process_group import ProcessGroup

_ENV_RECT = "TORCHFT_AMD_CP_RECT"
_ENV_RING_FA = "TORCHFT_AMD_RING_FA"


def cp_rect_enabled() -> bool:
    """The rectangular attention kernels under CP (opt-in)."""
    return os.environ.get(_ENV_RECT, "0") in ("1", "true", "True")


def ring_fa_enabled() -> bool:
    """The hand-written kernels under ring attention (opt-in)."""
    return os.environ.get(_ENV_RING_FA, "0") in ("1", "true", "True")


def shard_sequence(t: torch.Tensor, rank: int, world: int, dim: int = 1) -> torch.Tensor:
    """Slice this rank's contiguous sequence shard (seq % world == 0)."""
    seq = t.size(dim)
    assert seq % world == 0, f"sequence {seq} not divisible by cp world {world}"
    shard = seq // world
    return t.narrow(dim, rank * shard, shard).contiguous()


class _AllGatherSeq(torch.autograd.Function):
    """All-gather along dim 1 (sequence); backward reduce-scatters the sum."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, pg: ProcessGroup, rank: int, world: int):
        ctx.pg = pg
        ctx.rank = rank
        ctx.world = world
        ctx.in_shape = x.shape
        if world == 1:
            return x
        x = x.contiguous()
        out = torch.empty(
            (world,) + tuple(x.shape), dtype=x.dtype, device=x.device
        )
        pg.allgather_into_tensor_coalesced([out.view(-1)], [x.view(-1)],
                                           AllgatherOptions()).wait()
        # [world, B, s, H, D] -> [B, world*s, H, D]
        return out.movedim(0, 1).reshape(
            x.shape[0], world * x.shape[1], *x.shape[2:]
        )

    @staticmethod
    def backward(ctx, grad: torch.Tensor):
        if ctx.world == 1:
            return grad, None, None, None
        # sum the full-context gradient across ranks, keep own shard
        grad = grad.contiguous()
        opts = AllreduceOptions()
        opts.reduceOp = ReduceOp.SUM
        ctx.pg.allreduce([grad], opts).wait()
        s = ctx.in_shape[1]
        own = grad.narrow(1, ctx.rank * s, s).contiguous()
        return own, None, None, None


def cp_attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    pg: Optional[ProcessGroup],
    rank: int,
    world: int,
    causal: bool = True,
    rect: Optional[bool] = None,
) -> torch.Tensor:
    """Context-parallel attention.

    Args:
        q/k/v: this rank's sequence shard, [B, s, H, D] ([B, s, Hkv, D] for
            k/v with GQA), shard ``rank`` of ``world``.
        pg: the CP process group (None or world==1 -> plain attention).
        rect: run the rectangular kernels where they apply
            (:func:`cp_rank_attention`); None reads TORCHFT_AMD_CP_RECT.
    Returns:
        attention output for this rank's Q shard, [B, s, H, D].
    """
    B, s, H, D = q.shape
    if pg is None or world == 1:
        out = F.scaled_dot_product_attention(
            q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
            is_causal=causal, enable_gqa=True,
        )
        return out.transpose(1, 2)

    k_full = _AllGatherSeq.apply(k, pg, rank, world)
    v_full = _AllGatherSeq.apply(v, pg, rank, world)
    return cp_rank_attention(q, k_full, v_full, rank, world, causal, rect)


def cp_rank_attention(
    q: torch.Tensor,
    k_full: torch.Tensor,
    v_full: torch.Tensor,
    rank: int,
    world: int,
    causal: bool = True,
    rect: Optional[bool] = None,
) -> torch.Tensor:
    """What rank ``rank`` of ``world`` computes once K / V are gathered: its
    query shard q [B, s, H, D] against k_full / v_full [B, world*s, Hkv, D].
    No communication; the gradients of k_full / v_full cover the full context.

    ``rect`` (None: TORCHFT_AMD_CP_RECT): where the rectangular kernels apply,
    one ``flash_attention_rect`` call on the keys the shard can see, the first
    ``rank*s + s`` (all of them when not causal). The keys past them get their
    zero gradient from autograd's narrow. For B > 1 that key view is not one
    dense [B, S, H, D] block and the binding copies the call to contiguous
    [B, H, S, D] (docs/ROADMAP.md). Otherwise, and wherever the kernels do not
    apply, the flash + LSE merge runs."""
    s = q.shape[1]
    if cp_rect_enabled() if rect is None else rect:
        n = rank * s + s if causal else k_full.shape[1]
        qT = q.transpose(1, 2)
        kT = k_full[:, :n].transpose(1, 2)
        vT = v_full[:, :n].transpose(1, 2)
        if _rect_supported(qT, kT):
            return flash_attention_rect(qT, kT, vT, causal=causal).transpose(1, 2)

    if not causal:
        out = F.scaled_dot_product_attention(
            q.transpose(1, 2), k_full.transpose(1, 2), v_full.transpose(1, 2),
            is_causal=False, enable_gqa=True,
        )
        return out.transpose(1, 2)

    # causal with a sequence offset: queries at global positions
    # [rank*s, (rank+1)*s) attend to keys [0, rank*s + local_pos).
    # Split into the fully-visible prefix block (dense flash) and the
    # diagonal block (causal flash) and merge via log-sum-exp — flash speed
    # and flash memory at any context length (no materialized score matrix).
    prefix_len = rank * s
    qT = q.transpose(1, 2)
    if prefix_len > 0:
        out = _MergedFlashAttn.apply(
            qT.contiguous(),
            k_full.transpose(1, 2).contiguous(),
            v_full.transpose(1, 2).contiguous(),
            prefix_len,
        )
        return out.transpose(1, 2)

    out = F.scaled_dot_product_attention(
        qT, k_full[:, :s].transpose(1, 2), v_full[:, :s].transpose(1, 2),
        is_causal=True, enable_gqa=True,
    )
    return out.transpose(1, 2)


# ---------------------------------------------------------------------------
# flash-attention two-block merge
# ---------------------------------------------------------------------------

_NATIVE_GQA_CACHE: dict = {}


def _native_gqa_ok(device_type: str, dtype: torch.dtype) -> bool:
    """Probe whether the flash op accepts Hq != Hkv directly on this device."""
    key = (device_type, dtype)
    if key not in _NATIVE_GQA_CACHE:
        try:
            q = torch.zeros(1, 2, 8, 32, dtype=dtype, device=device_type)
            kv = torch.zeros(1, 1, 8, 32, dtype=dtype, device=device_type)
            _flash_fwd_raw(q, kv, kv, causal=False)
            _NATIVE_GQA_CACHE[key] = True
        except Exception:  # noqa: BLE001
            _NATIVE_GQA_CACHE[key] = False
    return _NATIVE_GQA_CACHE[key]


def _flash_fwd_raw(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool):
    """Flash forward returning (out, lse, aux) with lse [B,H,Sq] fp32.

    ``aux`` carries whatever the device-specific backward needs.
    """
    if q.is_cuda:
        (out, lse, cum_q, cum_k, max_q, max_k, seed, offset, _dbg) = (
            torch.ops.aten._scaled_dot_product_flash_attention(q, k, v, 0.0, causal)
        )
        return out, lse, (cum_q, cum_k, max_q, max_k, seed, offset)
    out, lse = torch.ops.aten._scaled_dot_product_flash_attention_for_cpu(
        q, k, v, 0.0, causal
    )
    return out, lse, None


def _flash_bwd_raw(
    dout: torch.Tensor,
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    out: torch.Tensor,
    lse: torch.Tensor,
    causal: bool,
    aux,
):
    if q.is_cuda:
        cum_q, cum_k, max_q, max_k, seed, offset = aux
        return torch.ops.aten._scaled_dot_product_flash_attention_backward(
            dout, q, k, v, out, lse, cum_q, cum_k, max_q, max_k, 0.0, causal,
            seed, offset,
        )
    return torch.ops.aten._scaled_dot_product_flash_attention_for_cpu_backward(
        dout, q, k, v, out, lse, 0.0, causal
    )


def _expand_kv(t: torch.Tensor, rep: int) -> torch.Tensor:
    return t.repeat_interleave(rep, dim=1) if rep > 1 else t


class _MergedFlashAttn(torch.autograd.Function):
    """Causal CP attention of one Q shard against [prefix | diagonal] KV.

    Forward runs flash on each block and merges by log-sum-exp. Backward
    re-enters each block's flash backward with the MERGED out and lse: with
    the merged lse, exp(S_block − lse) IS the global softmax restricted to
    the block's columns, and rowsum(dout·out_merged) is the global delta —
    so each block backward yields exactly its contribution to dq/dk/dv
    (the standard ring-attention backward identity).
    """

    @staticmethod
    def forward(ctx, q: torch.Tensor, k_full: torch.Tensor, v_full: torch.Tensor,
                prefix_len: int):
        # q [B,Hq,s,D]; k_full/v_full [B,Hkv,S,D], S >= prefix_len + s
        s = q.shape[2]
        Hq, Hkv = q.shape[1], k_full.shape[1]
        rep = Hq // Hkv
        if rep > 1 and _native_gqa_ok(q.device.type, q.dtype):
            rep = 1  # flash handles GQA natively; don't expand

        kp = _expand_kv(k_full[:, :, :prefix_len].contiguous(), rep)
        vp = _expand_kv(v_full[:, :, :prefix_len].contiguous(), rep)
        kd = _expand_kv(k_full[:, :, prefix_len : prefix_len + s].contiguous(), rep)
        vd = _expand_kv(v_full[:, :, prefix_len : prefix_len + s].contiguous(), rep)

        out_p, lse_p, aux_p = _flash_fwd_raw(q, kp, vp, causal=False)
        out_d, lse_d, aux_d = _flash_fwd_raw(q, kd, vd, causal=True)

        lse = torch.logaddexp(lse_p.float(), lse_d.float())  # [B,Hq,s]
        w_p = torch.exp(lse_p.float() - lse).unsqueeze(-1)
        w_d = torch.exp(lse_d.float() - lse).unsqueeze(-1)
        out = (out_p.float() * w_p + out_d.float() * w_d).to(q.dtype)

        ctx.save_for_backward(q, k_full, v_full, out, lse)
        ctx.prefix_len = prefix_len
        ctx.rep = rep
        ctx.aux = (aux_p, aux_d)
        return out

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        q, k_full, v_full, out, lse = ctx.saved_tensors
        prefix_len, rep = ctx.prefix_len, ctx.rep
        aux_p, aux_d = ctx.aux
        s = q.shape[2]
        dout = dout.contiguous()

        kp = _expand_kv(k_full[:, :, :prefix_len].contiguous(), rep)
        vp = _expand_kv(v_full[:, :, :prefix_len].contiguous(), rep)
        kd = _expand_kv(k_full[:, :, prefix_len : prefix_len + s].contiguous(), rep)
        vd = _expand_kv(v_full[:, :, prefix_len : prefix_len + s].contiguous(), rep)

        dq_p, dk_p, dv_p = _flash_bwd_raw(dout, q, kp, vp, out, lse, False, aux_p)
        dq_d, dk_d, dv_d = _flash_bwd_raw(dout, q, kd, vd, out, lse, True, aux_d)

        Hkv = k_full.shape[1]

        def fold(dk: torch.Tensor) -> torch.Tensor:
            # undo the GQA expansion: sum grads over the replicated heads
            if rep == 1:
                return dk
            B, _, S, D = dk.shape
            return dk.view(B, Hkv, rep, S, D).sum(2)

        dk_full = torch.zeros_like(k_full)
        dv_full = torch.zeros_like(v_full)
        dk_full[:, :, :prefix_len] = fold(dk_p)
        dv_full[:, :, :prefix_len] = fold(dv_p)
        dk_full[:, :, prefix_len : prefix_len + s] = fold(dk_d)
        dv_full[:, :, prefix_len : prefix_len + s] = fold(dv_d)
        return dq_p + dq_d, dk_full, dv_full, None


def _sdpa_with_lse(
    q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool
) -> Tuple[torch.Tensor, torch.Tensor]:
    """SDPA returning (out, logsumexp) — needed for block merging.

    Uses a numerically-stable explicit implementation (fp32 softmax); block
    sizes here are sequence shards so the score matrix is s×s_block, not
    S×S.
    """
    # expand GQA kv heads
    Hq, Hkv = q.shape[1], k.shape[1]
    if Hq != Hkv:
        rep = Hq // Hkv
        k = k.repeat_interleave(rep, dim=1)
        v = v.repeat_interleave(rep, dim=1)
    scale = q.shape[-1] ** -0.5
    scores = torch.matmul(q.float(), k.float().transpose(-2, -1)) * scale
    if causal:
        s_q, s_k = scores.shape[-2], scores.shape[-1]
        mask = torch.ones(s_q, s_k, dtype=torch.bool, device=scores.device).tril_()
        scores = scores.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(scores, dim=-1)  # [B, H, s_q]
    probs = torch.softmax(scores, dim=-1)
    out = torch.matmul(probs, v.float()).to(q.dtype)
    return out, lse


class ContextParallelAttention(torch.nn.Module):
    """Drop-in attention module computing CP attention over a PG."""

    def __init__(self, pg: Optional[ProcessGroup], rank: int, world: int,
                 causal: bool = True) -> None:
        super().__init__()
        self._pg = pg
        self._rank = rank
        self._world = world
        self._causal = causal

    def forward(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        return cp_attention(q, k, v, self._pg, self._rank, self._world, self._causal)


# ---------------------------------------------------------------------------
# ring attention (block-rotating KV)
# ---------------------------------------------------------------------------


def _merge_block(out_acc, lse_acc, out_b, lse_b):
    """Online LSE merge of one more KV block into the running (out, lse)."""
    lse_b = lse_b.float()
    new_lse = torch.logaddexp(lse_acc, lse_b)
    out_acc = out_acc * torch.exp(lse_acc - new_lse).unsqueeze(-1) + out_b.float() * torch.exp(
        lse_b - new_lse
    ).unsqueeze(-1)
    return out_acc, new_lse


def _ring_fused(fused: Optional[bool], q: torch.Tensor, k: torch.Tensor) -> bool:
    """Whether a ring's blocks run on the hand-written kernels: asked for
    (``fused``; None reads TORCHFT_AMD_RING_FA) and the kernels apply."""
    want = ring_fa_enabled() if fused is None else fused
    return bool(want) and _fold_supported(q, k)


def _ring_rep(fused: bool, q: torch.Tensor, k: torch.Tensor) -> int:
    """How often aten's flash needs a KV block repeated along the heads. The
    hand-written kernels are GQA-native: never."""
    rep = q.shape[1] // k.shape[1]
    if fused or (rep > 1 and _native_gqa_ok(q.device.type, q.dtype)):
        rep = 1
    return rep


def _ring_fold(fused, q, k_b, v_b, state, blk_causal, last, rep):
    """Fold one KV block into a rank's running state; returns (state, aux).

    Fused: ``flash_attention_fold``, the kernel's own state handed on raw, and
    ``(out, lse)`` comes back from the fold that is told it is the ``last``.
    Otherwise aten's flash forward on the block and ``_merge_block`` into
    ``(out_acc fp32, lse_acc)``; ``aux`` is what its backward wants back."""
    if fused:
        return flash_attention_fold(q, k_b, v_b, state, causal=blk_causal, last=last), None
    if state is None:
        B, Hq, s, D = q.shape
        state = (torch.zeros(B, Hq, s, D, dtype=torch.float32, device=q.device),
                 torch.full((B, Hq, s), float("-inf"), dtype=torch.float32, device=q.device))
    o_b, l_b, aux = _flash_fwd_raw(q, _expand_kv(k_b, rep), _expand_kv(v_b, rep),
                                   causal=blk_causal)
    return _merge_block(*state, o_b, l_b), aux


def _ring_bwd_prepare(fused, dout, out):
    """Once per backward, before the blocks: the fused path's delta."""
    return hip_ext().fa_delta(dout, out) if fused else None


def _ring_block_bwd(fused, dout, q, k_b, v_b, out, lse, delta, blk_causal, aux, rep, dq):
    """One block's backward with the MERGED out / lse (the identity
    ``_MergedFlashAttn`` states). Adds the block's dq into ``dq`` (fp32) and
    returns its (dk, dv) per KV head.

    Fused: dkdv + the accumulating dq kernel, which adds its unrounded fp32
    dq into ``dq`` itself: no per-block dq, no fp32 copy, no head expansion.
    Otherwise aten's flash backward and the sum over the repeated heads."""
    if fused:
        _, dk_b, dv_b = hip_ext().fa_bwd(q, k_b, v_b, dout, lse, delta,
                                         q.shape[-1] ** -0.5, blk_causal, dq_acc=dq)
        return dk_b, dv_b
    dq_b, dk_b, dv_b = _flash_bwd_raw(dout, q, _expand_kv(k_b, rep), _expand_kv(v_b, rep),
                                      out, lse, blk_causal, aux)
    dq += dq_b.float()
    if rep == 1:
        return dk_b.float(), dv_b.float()
    B, Hkv, s, D = k_b.shape
    return (dk_b.view(B, Hkv, rep, s, D).float().sum(2),
            dv_b.view(B, Hkv, rep, s, D).float().sum(2))


class _RingRank(torch.autograd.Function):
    """``ring_rank_attention``: q [B,Hq,s,D] against n KV blocks in hop order."""

    @staticmethod
    def forward(ctx, q, causal_block, fused, n, *kv):
        q = q.contiguous()
        ks, vs = [t.contiguous() for t in kv[:n]], [t.contiguous() for t in kv[n:]]
        fused = _ring_fused(fused, q, ks[0])
        rep = _ring_rep(fused, q, ks[0])
        state, auxs = None, []
        for i in range(n):
            state, aux = _ring_fold(fused, q, ks[i], vs[i], state, i == causal_block,
                                    i == n - 1, rep)
            auxs.append(aux)
        out, lse = state
        out = out.to(q.dtype)
        ctx.save_for_backward(q, out, lse, *ks, *vs)
        ctx.causal_block, ctx.fused, ctx.rep, ctx.n, ctx.auxs = causal_block, fused, rep, n, auxs
        return out

    @staticmethod
    def backward(ctx, dout):
        q, out, lse, *kv = ctx.saved_tensors
        n, fused = ctx.n, ctx.fused
        dout = dout.contiguous()
        delta = _ring_bwd_prepare(fused, dout, out)
        dq = torch.zeros_like(q, dtype=torch.float32)
        dks, dvs = [], []
        for i in range(n):
            dk_b, dv_b = _ring_block_bwd(fused, dout, q, kv[i], kv[n + i], out, lse, delta,
                                         i == ctx.causal_block, ctx.auxs[i], ctx.rep, dq)
            dks.append(dk_b.to(q.dtype))
            dvs.append(dv_b.to(q.dtype))
        return (dq.to(q.dtype), None, None, None, *dks, *dvs)


def ring_rank_attention(q, k_blocks, v_blocks, causal_block: Optional[int],
                        fused: Optional[bool] = None) -> torch.Tensor:
    """What one ring-attention rank computes from the KV blocks it meets, in
    hop order, without the ring: the counterpart of :func:`cp_rank_attention`.

    q [B, Hq, s, D]; k_blocks / v_blocks: lists of [B, Hkv, s, D], every one
    visible to the rank. ``causal_block`` is the index of the one block that is
    causal (the rank's own, index 0 in ring order), None for none. Returns
    ``out`` [B, Hq, s, D]; autograd gives q's gradient and every block's.

    ``fused`` (None: TORCHFT_AMD_RING_FA, default off): where the kernels
    apply (a HIP device, bf16, D = 128, s % 256 == 0, heads dividing,
    TORCHFT_AMD_CUSTOM_FA not 0, the extension built) every block is one
    ``flash_attention_fold`` launch with the softmax state carried raw, and
    the backward is ``fa_delta`` once, then dkdv + accumulating dq per block.
    Otherwise aten's flash per block with the LSE merge."""
    n = len(k_blocks)
    assert n > 0 and n == len(v_blocks), "one v block per k block, at least one"
    return _RingRank.apply(q, causal_block, fused, n, *k_blocks, *v_blocks)


class _RingAttention(torch.autograd.Function):
    """Causal CP attention with ring-rotated KV blocks.

    Forward: each rank streams the other shards' K/V around the ring
    (W-1 send/recv hops) and folds every visible block into its running
    (out, lse) by the online-softmax merge — peak KV residency is TWO
    shards instead of the full context, which is what makes >512k-token
    training fit. Causal note: rank r attends blocks 0..r only, so later
    ranks do more work per hop (the classic ring imbalance; a zigzag
    shard order is the known fix and is left for a later round).

    Backward: re-all-gathers K/V (one collective, no ring) and re-enters
    flash backward per visible block with the MERGED out/lse — the same
    identity _MergedFlashAttn uses — then sum-reduces dK/dV back to the
    owning shards. Peak memory in backward matches the all-gather-KV
    scheme; the ring saves the FORWARD residency, which is what persists
    across the whole layer stack of a training step.

    The compute of both is ``_ring_fold`` / ``_ring_block_bwd``; ``fused``
    puts them on the hand-written kernels (``ring_rank_attention``).
    """

    @staticmethod
    def forward(ctx, q, k_shard, v_shard, pg, rank, world, causal, fused=None):
        # layouts: q [B,Hq,s,D]; k_shard/v_shard [B,Hkv,s,D]
        q = q.contiguous()
        fused = _ring_fused(fused, q, k_shard)
        rep = _ring_rep(fused, q, k_shard)
        # the last hop whose block this rank sees
        last_hop = rank if causal else world - 1
        state = None

        cur_k, cur_v = k_shard.contiguous(), v_shard.contiguous()
        nxt = (rank + 1) % world
        prv = (rank - 1) % world
        aux_by_owner = {}
        for hop in range(world):
            owner = (rank - hop) % world
            if hop < world - 1:
                # rotate: pass the current block downstream, fetch upstream.
                # send first on even ranks, recv first on odd: no deadlock
                # on blocking transports.
                send_buf = torch.cat([cur_k.reshape(1, -1), cur_v.reshape(1, -1)], 0)
                recv_buf = torch.empty_like(send_buf)
                if rank % 2 == 0:
                    ws = pg.send([send_buf], nxt, tag=hop)
                    wr = pg.recv([recv_buf], prv, tag=hop)
                else:
                    wr = pg.recv([recv_buf], prv, tag=hop)
                    ws = pg.send([send_buf], nxt, tag=hop)
                ws.wait()
                wr.wait()
            if not causal or owner <= rank:
                blk_causal = causal and owner == rank
                state, aux_by_owner[owner] = _ring_fold(
                    fused, q, cur_k, cur_v, state, blk_causal, hop == last_hop, rep)
            if hop < world - 1:
                cur_k = recv_buf[0].view_as(cur_k).contiguous()
                cur_v = recv_buf[1].view_as(cur_v).contiguous()

        out_acc, lse_acc = state
        out = out_acc.to(q.dtype)
        ctx.save_for_backward(q, k_shard, v_shard, out, lse_acc)
        ctx.pg, ctx.rank, ctx.world, ctx.causal = pg, rank, world, causal
        ctx.rep, ctx.fused = rep, fused
        ctx.aux_by_owner = aux_by_owner  # dropout-0 flash bwd side args
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k_shard, v_shard, out, lse = ctx.saved_tensors
        pg, rank, world, causal = ctx.pg, ctx.rank, ctx.world, ctx.causal
        rep, fused = ctx.rep, ctx.fused
        B, Hkv, s, D = k_shard.shape
        dout = dout.contiguous()

        # one allgather instead of re-running the ring: [W,B,Hkv,s,D]
        flat = torch.cat([k_shard.reshape(1, -1), v_shard.reshape(1, -1)], 0)
        gath = torch.empty(world * flat.numel(), dtype=flat.dtype, device=flat.device)
        pg.allgather_into_tensor_coalesced(
            [gath], [flat.reshape(-1)], AllgatherOptions()
        ).wait()
        gath = gath.view(world, 2, B, Hkv, s, D)

        dq = torch.zeros_like(q, dtype=torch.float32)
        dk_full = torch.zeros(world, B, Hkv, s, D, dtype=torch.float32,
                              device=q.device)
        dv_full = torch.zeros_like(dk_full)
        delta = _ring_bwd_prepare(fused, dout, out)
        for o in range(world):
            if causal and o > rank:
                continue
            kb = gath[o, 0].to(q.dtype).contiguous()
            vb = gath[o, 1].to(q.dtype).contiguous()
            blk_causal = causal and o == rank
            # flash bwd consumes the MERGED out/lse: exp(S_b - lse) is the
            # global softmax restricted to block b's columns
            dk_full[o], dv_full[o] = _ring_block_bwd(
                fused, dout, q, kb, vb, out, lse, delta, blk_causal,
                ctx.aux_by_owner[o], rep, dq)

        # sum contributions from every rank, keep own shard
        opts = AllreduceOptions()
        opts.reduceOp = ReduceOp.SUM
        grads = torch.cat([dk_full.reshape(1, -1), dv_full.reshape(1, -1)], 0)
        pg.allreduce([grads], opts).wait()
        dk = grads[0].view(world, B, Hkv, s, D)[rank].to(k_shard.dtype)
        dv = grads[1].view(world, B, Hkv, s, D)[rank].to(v_shard.dtype)
        return dq.to(q.dtype), dk, dv, None, None, None, None, None


def ring_attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    pg: Optional[ProcessGroup],
    rank: int,
    world: int,
    causal: bool = True,
    fused: Optional[bool] = None,
) -> torch.Tensor:
    """Ring-attention CP: same contract as :func:`cp_attention` ([B, s, H, D]
    shards in/out) but with ring-rotated KV — forward KV residency is two
    shards instead of the full context. ``fused`` (None: TORCHFT_AMD_RING_FA):
    the hand-written kernels with the softmax state carried between hops,
    where they apply (:func:`ring_rank_attention`); the communication is the
    same either way."""
    if pg is None or world == 1:
        return cp_attention(q, k, v, None, rank, 1, causal)
    out = _RingAttention.apply(
        q.transpose(1, 2).contiguous(),
        k.transpose(1, 2).contiguous(),
        v.transpose(1, 2).contiguous(),
        pg, rank, world, causal, fused,
    )
    return out.transpose(1, 2)


# ---------------------------------------------------------------------------
# zigzag ring attention (balanced causal ring)
# ---------------------------------------------------------------------------


def shard_sequence_zigzag(
    t: torch.Tensor, rank: int, world: int, dim: int = 1
) -> torch.Tensor:
    """Zigzag shard: the sequence splits into 2W chunks and rank i owns
    chunks (i, 2W-1-i) concatenated — every rank then sees the same causal
    work per ring hop, fixing the plain ring's tail-heavy imbalance."""
    seq = t.size(dim)
    assert seq % (2 * world) == 0, (
        f"sequence {seq} not divisible by 2*world {2 * world}"
    )
    c = seq // (2 * world)
    lo = t.narrow(dim, rank * c, c)
    hi = t.narrow(dim, (2 * world - 1 - rank) * c, c)
    return torch.cat([lo, hi], dim=dim).contiguous()


def unshard_sequence_zigzag(
    parts: list, world: int, dim: int = 1
) -> torch.Tensor:
    """Inverse of :func:`shard_sequence_zigzag` given every rank's shard."""
    chunks = [None] * (2 * world)
    for r, p in enumerate(parts):
        c = p.size(dim) // 2
        chunks[r] = p.narrow(dim, 0, c)
        chunks[2 * world - 1 - r] = p.narrow(dim, c, c)
    return torch.cat(chunks, dim=dim)


class _ZigzagRingAttention(torch.autograd.Function):
    """Causal ring attention over zigzag shards.

    Each rank's Q/K/V shard is [low chunk i | high chunk 2W-1-i]. Per hop
    the owner's two KV chunks are tested against the rank's two Q chunks —
    chunk-causal visibility (kv chunk <= q chunk; equality = in-chunk
    causal) gives every rank the same number of visible blocks per hop.
    Forward streams KV around the ring with per-q-chunk online LSE merges;
    backward re-all-gathers KV and re-enters flash backward per visible
    block with the merged out/lse (same identity as _RingAttention).
    """

    @staticmethod
    def forward(ctx, q, k_shard, v_shard, pg, rank, world):
        B, Hq, s2, D = q.shape  # s2 = 2c
        c = s2 // 2
        q = q.contiguous()
        Hkv = k_shard.shape[1]
        rep = Hq // Hkv
        if rep > 1 and _native_gqa_ok(q.device.type, q.dtype):
            rep = 1

        my_chunks = (rank, 2 * world - 1 - rank)
        q_halves = (q[:, :, :c], q[:, :, c:])
        out_acc = [
            torch.zeros(B, Hq, c, D, dtype=torch.float32, device=q.device)
            for _ in range(2)
        ]
        lse_acc = [
            torch.full((B, Hq, c), float("-inf"), dtype=torch.float32,
                       device=q.device)
            for _ in range(2)
        ]

        cur_k, cur_v = k_shard.contiguous(), v_shard.contiguous()
        nxt, prv = (rank + 1) % world, (rank - 1) % world
        aux_by_block = {}
        for hop in range(world):
            owner = (rank - hop) % world
            if hop < world - 1:
                send_buf = torch.cat(
                    [cur_k.reshape(1, -1), cur_v.reshape(1, -1)], 0
                )
                recv_buf = torch.empty_like(send_buf)
                if rank % 2 == 0:
                    ws = pg.send([send_buf], nxt, tag=hop)
                    wr = pg.recv([recv_buf], prv, tag=hop)
                else:
                    wr = pg.recv([recv_buf], prv, tag=hop)
                    ws = pg.send([send_buf], nxt, tag=hop)
                ws.wait()
                wr.wait()

            owner_chunks = (owner, 2 * world - 1 - owner)
            for kh in range(2):
                kc = owner_chunks[kh]
                kb = _expand_kv(cur_k[:, :, kh * c : (kh + 1) * c].contiguous(), rep)
                vb = _expand_kv(cur_v[:, :, kh * c : (kh + 1) * c].contiguous(), rep)
                for qh in range(2):
                    qc = my_chunks[qh]
                    if kc > qc:
                        continue
                    blk_causal = kc == qc
                    o_b, l_b, aux = _flash_fwd_raw(
                        q_halves[qh].contiguous(), kb, vb, causal=blk_causal
                    )
                    aux_by_block[(qh, kc)] = aux
                    out_acc[qh], lse_acc[qh] = _merge_block(
                        out_acc[qh], lse_acc[qh], o_b, l_b
                    )
            if hop < world - 1:
                cur_k = recv_buf[0].view_as(cur_k).contiguous()
                cur_v = recv_buf[1].view_as(cur_v).contiguous()

        out = torch.cat([a.to(q.dtype) for a in out_acc], dim=2)
        ctx.save_for_backward(q, k_shard, v_shard, out, lse_acc[0], lse_acc[1])
        ctx.pg, ctx.rank, ctx.world, ctx.rep = pg, rank, world, rep
        ctx.aux_by_block = aux_by_block
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k_shard, v_shard, out, lse0, lse1 = ctx.saved_tensors
        pg, rank, world, rep = ctx.pg, ctx.rank, ctx.world, ctx.rep
        B, Hkv, s2, D = k_shard.shape
        c = s2 // 2
        Hq = q.shape[1]
        dout = dout.contiguous()

        flat = torch.cat([k_shard.reshape(1, -1), v_shard.reshape(1, -1)], 0)
        gath = torch.empty(world * flat.numel(), dtype=flat.dtype,
                           device=flat.device)
        pg.allgather_into_tensor_coalesced(
            [gath], [flat.reshape(-1)], AllgatherOptions()
        ).wait()
        gath = gath.view(world, 2, B, Hkv, 2, c, D)  # [owner][k/v][..][half]

        my_chunks = (rank, 2 * world - 1 - rank)
        q_halves = (q[:, :, :c].contiguous(), q[:, :, c:].contiguous())
        o_halves = (out[:, :, :c].contiguous(), out[:, :, c:].contiguous())
        d_halves = (dout[:, :, :c].contiguous(), dout[:, :, c:].contiguous())
        lses = (lse0, lse1)

        dq = torch.zeros_like(q, dtype=torch.float32)
        dkv_chunks = torch.zeros(2, 2 * world, B, Hkv, c, D,
                                 dtype=torch.float32, device=q.device)

        def fold(d):
            if rep == 1:
                return d.float()
            return d.view(B, Hkv, rep, c, D).float().sum(2)

        for o in range(world):
            owner_chunks = (o, 2 * world - 1 - o)
            for kh in range(2):
                kc = owner_chunks[kh]
                kb = _expand_kv(
                    gath[o, 0, :, :, kh].to(q.dtype).contiguous(), rep
                )
                vb = _expand_kv(
                    gath[o, 1, :, :, kh].to(q.dtype).contiguous(), rep
                )
                for qh in range(2):
                    qc = my_chunks[qh]
                    if kc > qc:
                        continue
                    dq_b, dk_b, dv_b = _flash_bwd_raw(
                        d_halves[qh], q_halves[qh], kb, vb, o_halves[qh],
                        lses[qh], kc == qc, ctx.aux_by_block[(qh, kc)]
                    )
                    dq[:, :, qh * c : (qh + 1) * c] += dq_b.float()
                    dkv_chunks[0, kc] += fold(dk_b)
                    dkv_chunks[1, kc] += fold(dv_b)

        opts = AllreduceOptions()
        opts.reduceOp = ReduceOp.SUM
        pg.allreduce([dkv_chunks.view(-1)], opts).wait()
        lo, hi = my_chunks
        dk = torch.cat([dkv_chunks[0, lo], dkv_chunks[0, hi]], dim=2).to(
            k_shard.dtype
        )
        dv = torch.cat([dkv_chunks[1, lo], dkv_chunks[1, hi]], dim=2).to(
            v_shard.dtype
        )
        return dq.to(q.dtype), dk, dv, None, None, None


def ring_attention_zigzag(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    pg: Optional[ProcessGroup],
    rank: int,
    world: int,
) -> torch.Tensor:
    """Balanced causal ring attention over :func:`shard_sequence_zigzag`
    shards ([B, 2c, H, D] in/out)."""
    if pg is None or world == 1:
        return cp_attention(q, k, v, None, rank, 1, True)
    out = _ZigzagRingAttention.apply(
        q.transpose(1, 2).contiguous(),
        k.transpose(1, 2).contiguous(),
        v.transpose(1, 2).contiguous(),
        pg, rank, world,
    )
    return out.transpose(1, 2)
