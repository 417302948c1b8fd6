"""CDNA4 fused ops: RMSNorm, RoPE, the fused QKV split + RoPE (``qkv_rope``,
with per-token positions for packed rows), SwiGLU, fused AdamW (with optional fused
global-norm clipping), gradient norm / clip, the fused loss head and the
fused DiLoCo outer sync (``pseudograd_``, ``diloco_outer_step_``, and
``pseudograd_fp8_`` / ``diloco_outer_step_fp8_`` around the fp8 wire pack).

On a HIP device these route through the in-tree gfx950 extension
(``torchft_amd/_hip_kernels.so``, sources in ``csrc/kernels/``) and FAIL
LOUDLY if it is missing — a silent eager fallback on the GPU would
invalidate every benchmark. On CPU they fall back to plain fp32 torch
reference implementations (used by the numerics tests as ground truth).
"""

from __future__ import annotations

import os
from typing import Optional

import torch

_EXT = None
_EXT_ERR: Optional[str] = None


def _load_ext():
    global _EXT, _EXT_ERR
    if _EXT is not None:
        return _EXT
    import importlib.util

    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                      "_hip_kernels.so")
    try:
        spec = importlib.util.spec_from_file_location("torchft_amd._hip_kernels", so)
        assert spec is not None and spec.loader is not None
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _EXT = mod
    except Exception as e:  # noqa: BLE001
        _EXT_ERR = f"{type(e).__name__}: {e}"
        _EXT = None
    return _EXT


def hip_ext():
    """The HIP kernel extension; raises on a GPU host if unavailable."""
    ext = _load_ext()
    if ext is None and torch.cuda.is_available():
        raise RuntimeError(
            f"torchft_amd HIP kernel extension not available on a GPU host "
            f"(build with `python -m torchft_amd._build`): {_EXT_ERR}"
        )
    return ext


def have_hip_ext() -> bool:
    return _load_ext() is not None


# ----------------------------------------------------------------- RMSNorm


def rmsnorm_ref(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """fp32 reference: y = x * rsqrt(mean(x^2)+eps) * w."""
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * inv * w.float()).to(x.dtype)


class _RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
        y, invrms = hip_ext().rmsnorm_fwd(x, w, eps)
        ctx.save_for_backward(x, w, invrms)
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, w, invrms = ctx.saved_tensors
        dx, dw = hip_ext().rmsnorm_bwd(dy, x, w, invrms)
        return dx, dw.to(w.dtype), None


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    if x.is_cuda:
        return _RMSNormFn.apply(x.contiguous(), w, eps)
    # CPU fallback keeps autograd via plain torch ops
    inv = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + eps)
    return (x.float() * inv * w.float()).to(x.dtype)


class RMSNorm(torch.nn.Module):
    def __init__(self, hidden: int, eps: float = 1e-5, dtype=torch.bfloat16) -> None:
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(hidden, dtype=dtype))
        self.eps = eps

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return rmsnorm(x, self.weight, self.eps)


# ----------------------------------------------------------------- RoPE


def rope_tables(
    seq_len: int, head_dim: int, theta: float = 500000.0, device="cpu"
) -> tuple[torch.Tensor, torch.Tensor]:
    """Llama-3 rotary tables: cos/sin [S, D/2] fp32 (rope theta 500k)."""
    inv_freq = 1.0 / (
        theta ** (torch.arange(0, head_dim, 2, device=device).float() / head_dim)
    )
    t = torch.arange(seq_len, device=device).float()
    freqs = torch.outer(t, inv_freq)  # [S, D/2]
    return freqs.cos(), freqs.sin()


def rope_ref(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """Reference rotate-half RoPE on [B, S, H, D]."""
    S, D = x.shape[1], x.shape[-1]
    c = cos[:S].view(1, S, 1, D // 2).float()
    s = sin[:S].view(1, S, 1, D // 2).float()
    x1, x2 = x.float().chunk(2, dim=-1)
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(x.dtype)


class _RopeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor):
        ctx.save_for_backward(cos, sin)
        return hip_ext().rope_apply(x, cos, sin, False)

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        cos, sin = ctx.saved_tensors
        return hip_ext().rope_apply(dy, cos, sin, True), None, None


def _rotate_half(x: torch.Tensor, c: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """The plain-torch rotation of [B, S, H, D] by tables that broadcast
    against [B, S, H, D/2]; autograd comes through the torch ops."""
    x1, x2 = x.chunk(2, dim=-1)
    return torch.cat(
        [x1 * c.to(x.dtype) - x2 * s.to(x.dtype), x2 * c.to(x.dtype) + x1 * s.to(x.dtype)],
        dim=-1,
    )


def rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """Apply rotary embedding to [B, S, H, D] (fused on HIP)."""
    if x.is_cuda:
        return _RopeFn.apply(x, cos, sin)
    S, D = x.shape[1], x.shape[-1]
    c = cos[:S].view(1, S, 1, D // 2)
    s = sin[:S].view(1, S, 1, D // 2)
    return _rotate_half(x, c, s)


# ----------------------------------------------------------------- QKV split + RoPE


class _QkvRopeFn(torch.autograd.Function):
    """csrc/kernels/qkv_rope.hip. The rotation needs no activations: only the
    tables and the positions are saved, so ``qkv`` is free as soon as the
    projection's own backward no longer needs it."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, n_heads: int, n_kv_heads: int, positions):
        ctx.save_for_backward(cos, sin, positions)
        q, k, v = hip_ext().qkv_rope_fwd(qkv, cos, sin, n_heads, n_kv_heads, positions)
        return q, k, v

    @staticmethod
    def backward(ctx, dq, dk, dv):
        # an output nobody used arrives as zeros (materialize_grads), so the
        # kernel always has its three inputs and writes all of dqkv
        cos, sin, positions = ctx.saved_tensors
        dqkv = hip_ext().qkv_rope_bwd(dq, dk, dv, cos, sin, positions)
        # the tables, the head counts and the positions take no gradient
        return dqkv, None, None, None, None, None


def qkv_rope(
    qkv: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    n_heads: int,
    n_kv_heads: int,
    positions: Optional[torch.Tensor] = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Split a fused projection ``qkv`` [B, S, (n_heads + 2 * n_kv_heads) * D]
    (q heads, then k heads, then v heads) into q [B, S, n_heads, D] and k, v
    [B, S, n_kv_heads, D] and apply the rotary embedding to q and k.

    ``positions`` (int32 [B, S], e.g. ``DocMask.positions()``): the row of
    ``cos`` / ``sin`` every token is rotated by; without it token ``s`` reads
    row ``s``. Values outside the tables give unspecified results.

    On a HIP device one kernel each way (bf16, ``D % 16 == 0``): the forward
    reads ``qkv`` once and writes three contiguous tensors, the backward
    writes the whole gradient of ``qkv`` from the three incoming ones. On CPU:
    slices plus the rotate-half math of :func:`rope`."""
    if qkv.is_cuda:
        return _QkvRopeFn.apply(qkv, cos, sin, n_heads, n_kv_heads, positions)
    B, S, W = qkv.shape
    D = W // (n_heads + 2 * n_kv_heads)
    if D * (n_heads + 2 * n_kv_heads) != W:
        raise ValueError(
            f"qkv_rope: the last dimension of qkv ({W}) must be divisible by "
            f"n_heads + 2 * n_kv_heads = {n_heads} + 2 * {n_kv_heads}"
        )
    nq, nkv = n_heads * D, n_kv_heads * D
    q = qkv[..., :nq].view(B, S, n_heads, D)
    k = qkv[..., nq : nq + nkv].view(B, S, n_kv_heads, D)
    v = qkv[..., nq + nkv :].view(B, S, n_kv_heads, D)
    if positions is None:
        return rope(q, cos, sin), rope(k, cos, sin), v
    if positions.shape != (B, S):
        raise ValueError(
            f"qkv_rope: positions must be [B, S] = {(B, S)}, got {tuple(positions.shape)}"
        )
    idx = positions.long()
    c = cos[idx].view(B, S, 1, D // 2)
    s = sin[idx].view(B, S, 1, D // 2)
    return _rotate_half(q, c, s), _rotate_half(k, c, s), v


# ----------------------------------------------------------------- SwiGLU


def swiglu_ref(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return (torch.nn.functional.silu(a.float()) * b.float()).to(a.dtype)


class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a: torch.Tensor, b: torch.Tensor):
        ctx.save_for_backward(a, b)
        return hip_ext().swiglu_fwd(a, b)

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        a, b = ctx.saved_tensors
        da, db = hip_ext().swiglu_bwd(dy, a, b)
        return da, db


def swiglu(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    if a.is_cuda:
        return _SwiGLUFn.apply(a, b)
    return torch.nn.functional.silu(a) * b


class _SwiGLUGluFn(torch.autograd.Function):
    """Packed-GLU SwiGLU: gu = [..., 2f] with gate = gu[..., :f], up =
    gu[..., f:] (the fused w13 projection's output) — the kernel reads the
    halves strided so no contiguous() copies of the activations happen."""

    @staticmethod
    def forward(ctx, gu: torch.Tensor):
        ctx.save_for_backward(gu)
        return hip_ext().swiglu_glu_fwd(gu)

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        (gu,) = ctx.saved_tensors
        return hip_ext().swiglu_glu_bwd(dy, gu)


def swiglu_glu(gu: torch.Tensor) -> torch.Tensor:
    """silu(gu[..., :f]) * gu[..., f:] for a packed [..., 2f] projection."""
    if gu.is_cuda:
        return _SwiGLUGluFn.apply(gu)
    f = gu.shape[-1] // 2
    return torch.nn.functional.silu(gu[..., :f]) * gu[..., f:]


# at the bottom: the modules below import hip_ext from this one

# ----------------------------------------------------------------- Fused AdamW, grad norm

from torchft_amd.ops.adamw import (  # noqa: E402,F401
    FusedAdamW,
    _as_grads,
    _local_view,
    _sumsq_torch,
    _use_hip_norm,
    clip_grad_norm_,
    grad_norm,
)

# ----------------------------------------------------------------- Cross-entropy

from torchft_amd.ops.cross_entropy import linear_cross_entropy  # noqa: E402,F401

# ----------------------------------------------------------------- DiLoCo outer sync

from torchft_amd.ops.diloco import (  # noqa: E402,F401
    diloco_outer_step_,
    diloco_outer_step_fp8_,
    pseudograd_,
    pseudograd_fp8_,
)

# ----------------------------------------------------------------- Flash attention

from torchft_amd.ops.flash_attention import (  # noqa: E402,F401
    DocMask,
    flash_attention,
    flash_attention_fold,
    flash_attention_rect,
)
