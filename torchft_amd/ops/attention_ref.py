"""Plain-torch yardsticks for the attention kernels (docs/KERNELS.md,
"Numerics" of the forward and the backward). Both run on CPU or GPU.

``attention_ref64``   the operation in fp64 from the bf16 inputs, with the
                      denominators of the elementwise error bounds.
``attention_emulated`` the kernels' rounding chain in fp32 torch: P rounded to
                      bf16 before P.V and P^T.dO, dS rounded to bf16 after the
                      ``scale`` factor, bf16 stores, ``delta`` from the bf16
                      ``out``. It is the measure of what a correct bf16 chain
                      costs, not a port of the kernels: no tiles, no deferred
                      maximum, torch's summation order.

Layout: q, dout [B, Hq, S, D]; k, v [B, Hkv, S, D] with Hkv dividing Hq; key j
is visible to query i under ``causal`` iff j <= i, under a mask iff the mask
says so. ``doc_mask`` is a ``DocMask`` or a dense bool tensor broadcastable to
[B, Hq, S, S] (True = visible).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

U_BF16 = 2.0 ** -8   # unit round-off of bf16
E_FP32 = 2.0 ** -24  # unit round-off of fp32
_FLOOR = 2.0 ** -60  # denominators are floored at this fraction of their maximum


@dataclass
class AttentionRef:
    """fp64 results and bound denominators. dk, dv, A_dk, A_dv are
    [B, Hkv, S, D]; out, dq, A_out, A_dq [B, Hq, S, D]; the rest [B, Hq, S].
    A_dq_ref / A_dk_ref are A_dq / A_dk without the P.E term of W: the
    denominators of a backward that is fed this reference's own lse / delta
    and so inherits no error of ``out``. They carry the fp32 rounding of
    dP - delta instead, which P.E otherwise hides."""

    out: torch.Tensor
    lse: torch.Tensor
    delta: torch.Tensor
    dq: torch.Tensor
    dk: torch.Tensor
    dv: torch.Tensor
    A_out: torch.Tensor
    A_dq: torch.Tensor
    A_dk: torch.Tensor
    A_dv: torch.Tensor
    A_dq_ref: torch.Tensor
    A_dk_ref: torch.Tensor
    A_delta: torch.Tensor
    Sqk: torch.Tensor
    n: torch.Tensor


@dataclass
class AttentionEmulated:
    """What the rounding chain stores: out, dq, dk, dv bf16; lse, delta fp32."""

    out: torch.Tensor
    lse: torch.Tensor
    delta: torch.Tensor
    dq: torch.Tensor
    dk: torch.Tensor
    dv: torch.Tensor


def visible(S: int, causal: bool, doc_mask, device) -> torch.Tensor:
    """The visibility mask, broadcastable to [B, Hq, S, S]."""
    if doc_mask is not None:
        dense = doc_mask if isinstance(doc_mask, torch.Tensor) else doc_mask.dense()
        return dense.to(device=device, dtype=torch.bool)
    pos = torch.arange(S, device=device)
    if causal:
        return (pos[None, :] <= pos[:, None])[None, None]
    return torch.ones(1, 1, S, S, dtype=torch.bool, device=device)


def _group_sum(t: torch.Tensor, Hkv: int) -> torch.Tensor:
    B, Hq, S, D = t.shape
    return t.reshape(B, Hkv, Hq // Hkv, S, D).sum(2)


def _floored(t: torch.Tensor) -> torch.Tensor:
    return t.clamp_min(_FLOOR * t.max())


def delta_ref64(dout: torch.Tensor, out: torch.Tensor):
    """delta = rowsum(dout * out) in fp64 and its bound denominator
    A_delta = rowsum |dout * out|, floored like the others."""
    prod = dout.double() * out.double()
    return prod.sum(-1), _floored(prod.abs().sum(-1))


def attention_ref64(q, k, v, dout, scale: float, causal: bool,
                    doc_mask=None) -> AttentionRef:
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    qd, dod = q.double(), dout.double()
    kr = k.double().repeat_interleave(G, dim=1)
    vr = v.double().repeat_interleave(G, dim=1)
    vis = visible(S, causal, doc_mask, q.device)

    s = (qd @ kr.transpose(-1, -2)) * scale
    s = s.masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    P = torch.exp(s - lse[..., None])
    out = P @ vr
    dP = dod @ vr.transpose(-1, -2)
    delta = (dod * out).sum(-1)
    dS = P * (dP - delta[..., None])
    dq = (dS @ kr) * scale
    dk = _group_sum(dS.transpose(-1, -2) @ qd, Hkv) * scale
    dv = _group_sum(P.transpose(-1, -2) @ dod, Hkv)

    A_out = P @ vr.abs()
    E = (dod.abs() * A_out).sum(-1)
    A_dv = _group_sum(P.transpose(-1, -2) @ dod.abs(), Hkv)
    W = dS.abs() + P * E[..., None]
    A_dq = (W @ kr.abs()) * scale
    A_dk = _group_sum(W.transpose(-1, -2) @ qd.abs(), Hkv) * scale
    # fed this lse / delta: W = |dS|, plus the fp32 rounding of dP (a 128-term
    # dot product) and of delta as fed (rounded to fp32), which u |dS| does not
    # cover where dP - delta cancels (row 0 of a causal head: dS = 0 exactly).
    # Scaled so that 3u A = 3u scale |dS|.|k| + e scale F.|k|.
    F = P * (D * (dod.abs() @ vr.abs().transpose(-1, -2)) + delta.abs()[..., None])
    W_ref = dS.abs() + (E_FP32 / (3.0 * U_BF16)) * F
    A_dq_ref = (W_ref @ kr.abs()) * scale
    A_dk_ref = _group_sum(W_ref.transpose(-1, -2) @ qd.abs(), Hkv) * scale
    A_delta = (dod * out).abs().sum(-1)
    absdot = (qd.abs() @ kr.abs().transpose(-1, -2)).masked_fill(~vis, 0.0)
    Sqk = absdot.amax(-1) * scale
    n = vis.sum(-1).expand(B, Hq, S).double()
    return AttentionRef(out=out, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv,
                        A_out=_floored(A_out), A_dq=_floored(A_dq),
                        A_dk=_floored(A_dk), A_dv=_floored(A_dv),
                        A_dq_ref=_floored(A_dq_ref), A_dk_ref=_floored(A_dk_ref),
                        A_delta=_floored(A_delta), Sqk=Sqk, n=n)


_LOG2E = 1.4426950408889634
_LN2 = 0.6931471805599453


def _bf(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 and come back: the value the MFMA reads."""
    return t.to(torch.bfloat16).float()


def attention_emulated(q, k, v, dout, scale: float, causal: bool, doc_mask=None, *,
                       lse: Optional[torch.Tensor] = None,
                       delta: Optional[torch.Tensor] = None) -> AttentionEmulated:
    """``lse`` / ``delta``, if given, feed the backward in place of the
    forward's own (rounded to fp32): the backward alone."""
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    qf, dof = q.float(), dout.float()
    kr = k.float().repeat_interleave(G, dim=1)
    vr = v.float().repeat_interleave(G, dim=1)
    vis = visible(S, causal, doc_mask, q.device)

    # forward: log2-domain softmax, P rounded to bf16 for P.V only
    raw = qf @ kr.transpose(-1, -2)
    c2 = torch.tensor(scale * _LOG2E, dtype=torch.float32).item()
    s2 = (raw * c2).masked_fill(~vis, float("-inf"))
    m = s2.amax(-1, keepdim=True)
    e = torch.exp2(s2 - m)
    l = e.sum(-1, keepdim=True)
    out = ((_bf(e) @ vr) * (1.0 / l)).to(torch.bfloat16)
    lse_fwd = (_LN2 * (m + torch.log2(l))).squeeze(-1)

    lse_b = lse_fwd if lse is None else lse.float()
    delta_fwd = (dof * out.float()).sum(-1)
    delta_b = delta_fwd if delta is None else delta.float()

    # backward: P recomputed from lse; scale folded before dS is rounded
    sc = torch.tensor(scale, dtype=torch.float32).item()
    p = torch.exp((raw * sc).masked_fill(~vis, float("-inf")) - lse_b[..., None])
    dP = dof @ vr.transpose(-1, -2)
    dS = _bf(p * (dP - delta_b[..., None]) * sc)
    dq = (dS @ kr).to(torch.bfloat16)
    dk = _group_sum(dS.transpose(-1, -2) @ qf, Hkv).to(torch.bfloat16)
    dv = _group_sum(_bf(p).transpose(-1, -2) @ dof, Hkv).to(torch.bfloat16)
    return AttentionEmulated(out=out, lse=lse_fwd, delta=delta_fwd, dq=dq, dk=dk, dv=dv)
