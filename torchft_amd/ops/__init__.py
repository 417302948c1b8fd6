"""CDNA4 fused ops: RMSNorm, RoPE, the fused QKV split + RoPE (``qkv_rope``,
with per-token positions for packed rows), SwiGLU, fused AdamW (with optional fused
global-norm clipping), gradient norm / clip, the fused loss head and the
fused DiLoCo outer sync (``pseudograd_``, ``diloco_outer_step_``).

On a HIP device these route through the in-tree gfx950 extension
(``torchft_amd/_hip_kernels.so``, sources in ``csrc/kernels/``) and FAIL
LOUDLY if it is missing — a silent eager fallback on the GPU would
invalidate every benchmark. On CPU they fall back to plain fp32 torch
reference implementations (used by the numerics tests as ground truth).
"""

from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional

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


# ----------------------------------------------------------------- Fused AdamW


def _local_view(t: torch.Tensor) -> torch.Tensor:
    """The local shard of a DTensor (FSDP2 sharded params/grads), else t.
    The update runs on the shard in place — mathematically identical for
    elementwise optimizers, and what lets the HSDP path use the fused
    kernel."""
    try:
        from torch.distributed.tensor import DTensor
    except ImportError:  # pragma: no cover
        return t
    return t.to_local() if isinstance(t, DTensor) else t


_GRAD_NORM_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _sumsq_torch(tensors: List[torch.Tensor]) -> torch.Tensor:
    """Plain-torch sum of squares (double accumulation) as fp32 [1]."""
    total = torch.zeros((), dtype=torch.float64, device=tensors[0].device)
    for t in tensors:
        total = total + t.detach().double().pow(2).sum()
    return total.float().reshape(1)


def _as_grads(tensors_or_params) -> List[torch.Tensor]:
    """Gradients to measure: a tensor that requires grad is a parameter and
    contributes its ``.grad`` (skipped if None); any other tensor is taken as
    a gradient itself. DTensors contribute their local shard."""
    if isinstance(tensors_or_params, torch.Tensor):
        tensors_or_params = [tensors_or_params]
    out = []
    for t in tensors_or_params:
        if t.requires_grad:
            t = t.grad
            if t is None:
                continue
        t = _local_view(t)
        if t.numel() > 0:
            out.append(t)
    return out


def _use_hip_norm(grads: List[torch.Tensor]) -> bool:
    if not grads[0].is_cuda:
        return False
    for g in grads:
        if g.dtype not in _GRAD_NORM_DTYPES:
            raise TypeError(f"grad norm kernel: unsupported dtype {g.dtype}")
    return True


def grad_norm(tensors_or_params, *, norm_reduce=None, max_blocks: int = 2048) -> torch.Tensor:
    """Global L2 norm of a list of gradients (or of the ``.grad`` of a list of
    parameters) as a 0-dim fp32 tensor on their device; no host sync.

    On a HIP device: csrc/kernels/grad_norm.hip, two launches and no atomics,
    so the value is bitwise reproducible for a given ``max_blocks`` (the cap
    on the reduction grid). ``norm_reduce``, if given, is called with the
    1-element fp32 sum of squares before the square root — sharded callers
    all-reduce (SUM) it there. On CPU: plain torch.

    The sum of squares is an fp32 number: finite gradients whose squares add
    up past 2**128 (``|g| >= 2**64`` in bf16 or fp32) give an ``inf`` norm.
    ``clip_grad_norm_`` then leaves the gradients untouched and
    ``FusedAdamW(max_grad_norm=...)`` skips the step and counts it, as for a
    non-finite gradient (docs/KERNELS.md, "Overflow rule").
    """
    grads = _as_grads(tensors_or_params)
    if not grads:
        raise ValueError("grad_norm: no gradients")
    if _use_hip_norm(grads):
        sumsq = hip_ext().grad_sumsq(grads, max_blocks)
    else:
        sumsq = _sumsq_torch(grads)
    if norm_reduce is not None:
        norm_reduce(sumsq)
    return sumsq.sqrt().reshape(())


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm: float, *, norm_reduce=None) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` for users of other optimizers:
    scales every ``.grad`` in place by ``min(1, max_norm / (norm + 1e-6))``
    and returns the pre-clip global norm as a 0-dim fp32 device tensor.
    Gradients are left untouched when the norm is non-finite, and nothing
    waits on the host. ``norm_reduce`` as in :func:`grad_norm`.
    """
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [_local_view(p.grad) for p in parameters if p.grad is not None]
    grads = [g for g in grads if g.numel() > 0]
    if not grads:
        raise ValueError("clip_grad_norm_: no gradients")
    max_norm = float(max_norm)
    if not max_norm > 0:
        raise ValueError(f"max_norm must be > 0, got {max_norm}")
    if _use_hip_norm(grads):
        sumsq = hip_ext().clip_grad_norm(grads, max_norm, 2048, norm_reduce)
        return sumsq.sqrt().reshape(())
    sumsq = _sumsq_torch(grads)
    if norm_reduce is not None:
        norm_reduce(sumsq)
    norm = sumsq.sqrt().reshape(())
    coef = (max_norm / (norm + 1e-6)).clamp(max=1.0)
    coef = torch.where(torch.isfinite(norm), coef, torch.ones_like(coef))
    for g in grads:
        g.mul_(coef)
    return norm


class FusedAdamW(torch.optim.Optimizer):
    """Single-kernel multi-tensor AdamW for bf16 params (fp32 moments).

    One launch per step updates every parameter (csrc/kernels/fused_adamw.hip);
    falls back to torch's foreach AdamW path on CPU. DTensor params (the
    FSDP2 sharded path) are updated on their local shards.

    ``max_grad_norm`` (opt-in; ``math.inf`` allowed) turns on the clip mode:
    the global L2 norm over all param groups is reduced on the device
    (csrc/kernels/grad_norm.hip), the clip coefficient is folded into the
    update's gradient read, and a non-finite norm skips the step on the
    device — ``p``, ``exp_avg``, ``exp_avg_sq`` and the bias-correction step
    stay untouched, with no host sync. In this mode ``state[p]["step"]`` is a
    0-dim int32 device tensor, ``last_grad_norm`` holds the pre-clip norm of
    the last step (non-finite if it was skipped) and ``skipped_steps`` counts
    the skips, both as device tensors. ``norm_reduce``, if given, is called
    with the 1-element fp32 sum of squares before the update; FSDP2/DTensor
    callers all-reduce (SUM) their shard's value there.
    """

    def __init__(
        self,
        params,
        lr: float = 1e-3,
        betas=(0.9, 0.95),
        eps: float = 1e-8,
        weight_decay: float = 0.01,
        max_grad_norm: Optional[float] = None,
        norm_reduce: Optional[Callable[[torch.Tensor], None]] = None,
    ) -> None:
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0:
                raise ValueError(f"max_grad_norm must be > 0, got {max_grad_norm}")
        elif norm_reduce is not None:
            raise ValueError("norm_reduce needs max_grad_norm (math.inf to only report)")
        self.max_grad_norm = max_grad_norm
        self.norm_reduce = norm_reduce
        self.last_grad_norm: Optional[torch.Tensor] = None
        self.skipped_steps: Optional[torch.Tensor] = None
        if max_grad_norm is not None:
            dev = _local_view(self.param_groups[0]["params"][0]).device
            self._clip_buffers(dev)

    def _clip_buffers(self, dev: torch.device) -> None:
        skipped = self.skipped_steps
        self._sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
        self.skipped_steps = torch.zeros((), dtype=torch.int32, device=dev)
        if skipped is not None:  # params moved since construction
            self.skipped_steps.copy_(skipped)

    def load_state_dict(self, state_dict) -> None:  # noqa: D102
        # torch leaves a "step" entry as it was saved (an int or a tensor on
        # any device); make it what this optimizer's mode steps with.
        super().load_state_dict(state_dict)
        for p, state in self.state.items():
            if "step" not in state:
                continue
            step = state["step"]
            if self.max_grad_norm is not None:
                dev = _local_view(p).device
                state["step"] = torch.as_tensor(step).to(
                    device=dev, dtype=torch.int32).reshape(()).clone()
            elif isinstance(step, torch.Tensor):
                state["step"] = int(step.item())

    @torch.no_grad()
    def _step_clip(self) -> None:
        params: List[torch.Tensor] = []
        grads: List[torch.Tensor] = []
        exp_avgs: List[torch.Tensor] = []
        exp_avg_sqs: List[torch.Tensor] = []
        steps: List[torch.Tensor] = []
        groups = []
        for group in self.param_groups:
            n0 = len(params)
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                p_loc = _local_view(p)
                if len(state) == 0:
                    # the step lives on the device: a skipped step must not
                    # advance it, and the host never learns which were skipped
                    state["step"] = torch.zeros((), dtype=torch.int32, device=p_loc.device)
                    state["exp_avg"] = torch.zeros_like(p_loc, dtype=torch.float32)
                    state["exp_avg_sq"] = torch.zeros_like(p_loc, dtype=torch.float32)
                params.append(p_loc)
                grads.append(_local_view(p.grad))
                exp_avgs.append(state["exp_avg"])
                exp_avg_sqs.append(state["exp_avg_sq"])
                steps.append(state["step"])
            groups.append((group, len(params) - n0))
        if not params:
            return
        dev = params[0].device
        if self._sumsq.device != dev:
            self._clip_buffers(dev)

        if dev.type == "cuda" and all(
            p.dtype == torch.bfloat16 and g.dtype == torch.bfloat16
            for p, g in zip(params, grads)
        ):
            # norm over everything, then one update launch per param group —
            # no bucketing by step count, the kernel reads each tensor's own
            hip_ext().adamw_clip_step(
                params, grads, exp_avgs, exp_avg_sqs, steps,
                [cnt for _, cnt in groups],
                [float(g["lr"]) for g, _ in groups],
                [float(g["betas"][0]) for g, _ in groups],
                [float(g["betas"][1]) for g, _ in groups],
                [float(g["eps"]) for g, _ in groups],
                [float(g["weight_decay"]) for g, _ in groups],
                self.max_grad_norm, 2048, self._sumsq, self.skipped_steps,
                self.last_grad_norm, self.norm_reduce,
            )
            return

        # plain-torch path, same semantics and still no host sync: every
        # tensor is rewritten through where(finite, new, old)
        self._sumsq.copy_(_sumsq_torch(grads))
        if self.norm_reduce is not None:
            self.norm_reduce(self._sumsq)
        norm = self._sumsq.sqrt().reshape(())
        finite = torch.isfinite(norm)
        coef = (self.max_grad_norm / (norm + 1e-6)).clamp(max=1.0)
        i = 0
        for group, cnt in groups:
            beta1, beta2 = group["betas"]
            for p, g, m, v, s in zip(params[i:i + cnt], grads[i:i + cnt],
                                     exp_avgs[i:i + cnt], exp_avg_sqs[i:i + cnt],
                                     steps[i:i + cnt]):
                gf = g.float() * coef
                s1 = (s + 1).double()
                bc1 = (1 - beta1 ** s1).float()
                bc2 = (1 - beta2 ** s1).float()
                m_new = m * beta1 + gf * (1 - beta1)
                v_new = v * beta2 + gf * gf * (1 - beta2)
                denom = (v_new / bc2).sqrt_().add_(group["eps"])
                update = (m_new / bc1) / denom + group["weight_decay"] * p.float()
                p_new = p + (-group["lr"] * update).to(p.dtype)
                p.copy_(torch.where(finite, p_new, p))
                m.copy_(torch.where(finite, m_new, m))
                v.copy_(torch.where(finite, v_new, v))
                s.add_(finite.to(s.dtype))
            i += cnt
        self.last_grad_norm.copy_(norm)
        self.skipped_steps.add_((~finite).to(torch.int32))

    @torch.no_grad()
    def step(self, closure=None):  # noqa: D102
        assert closure is None
        if self.max_grad_norm is not None:
            self._step_clip()
            return None
        for group in self.param_groups:
            # Params that intermittently have grad=None (e.g. unused-param
            # DDP) accumulate different step counts; the bias correction is
            # per step count, so bucket by it — one kernel launch per
            # distinct count (one in the common case).
            by_step: Dict[int, List[List[torch.Tensor]]] = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                p_loc = _local_view(p)
                g_loc = _local_view(p.grad)
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p_loc, dtype=torch.float32)
                    state["exp_avg_sq"] = torch.zeros_like(p_loc, dtype=torch.float32)
                state["step"] += 1
                bucket = by_step.setdefault(state["step"], [[], [], [], []])
                bucket[0].append(p_loc)
                bucket[1].append(g_loc)
                bucket[2].append(state["exp_avg"])
                bucket[3].append(state["exp_avg_sq"])

            beta1, beta2 = group["betas"]
            for step, (params, grads, exp_avgs, exp_avg_sqs) in by_step.items():
                if params[0].is_cuda and params[0].dtype == torch.bfloat16:
                    hip_ext().adamw_step(
                        params, grads, exp_avgs, exp_avg_sqs, group["lr"], beta1,
                        beta2, group["eps"], group["weight_decay"], step,
                    )
                else:
                    bc1 = 1 - beta1**step
                    bc2 = 1 - beta2**step
                    for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
                        gf = g.float()
                        m.mul_(beta1).add_(gf, alpha=1 - beta1)
                        v.mul_(beta2).addcmul_(gf, gf, value=1 - beta2)
                        denom = (v / bc2).sqrt_().add_(group["eps"])
                        update = (m / bc1) / denom + group["weight_decay"] * p.float()
                        p.add_((-group["lr"] * update).to(p.dtype))
        return None


# ----------------------------------------------------------------- Cross-entropy

# at the bottom: cross_entropy.py imports hip_ext from this module
from torchft_amd.ops.cross_entropy import linear_cross_entropy  # noqa: E402,F401

# ----------------------------------------------------------------- DiLoCo outer sync

from torchft_amd.ops.diloco import diloco_outer_step_, pseudograd_  # noqa: E402,F401

# ----------------------------------------------------------------- Flash attention

from torchft_amd.ops.flash_attention import DocMask, flash_attention  # noqa: E402,F401
