"""Plain fp64 yardstick for ``adamw_kernel`` (csrc/kernels/fused_adamw.hip;
docs/KERNELS.md, "Numerics" of fused_adamw.hip). Runs on CPU or GPU.

``adamw_ref64``  one decoupled-weight-decay Adam step in fp64 from the stored
                 ``p``, ``g`` (bf16) and ``m``, ``v`` (fp32), with the sums of
                 absolute values that the error bounds are multiples of.
``clip_coef64``  the clip coefficient of the clip mode, the norm taken in fp64.
``philox4x32_10`` / ``sr_bits`` / ``stochastic_round_bf16``  the random bits and
                 the rounding of ``rounding="stochastic"`` (csrc/kernels/philox.h)
                 on integer torch tensors, plain and slow.

The kernel receives its hyper-parameters as fp32, and ``1 - float(beta)`` is
not the true ``1 - beta``: it is off by ``2^-24 * beta / (1 - beta)`` relative,
about 1000 fp32 units at ``beta2 = 0.999``. The reference therefore rounds
every hyper-parameter to fp32 first (``round_hparams``), forms ``1 - beta``
from the rounded ``beta`` and the bias corrections ``1 - beta^step`` from it
too; what is left between it and the kernel is the kernel's own arithmetic.
With ``round_hparams=False`` it is ``torch.optim.AdamW``'s definition to the
last few fp64 units (tests/test_adamw_numerics_cpu.py).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import torch


@dataclass
class AdamWRef:
    """fp64 results of one step and the bound denominators.

    ``s_m = beta1|m| + (1-beta1)|g|`` (``g`` after the clip coefficient);
    ``s_p = |p| + lr * (t_q + wd|p|)`` with ``t_q = (s_m / bc1) / (sqrt(v' /
    bc2) + eps)``, the quotient ``m_hat / denom`` with ``|m'|`` replaced by
    ``s_m`` so that cancellation inside ``m'`` cannot hide its rounding.
    ``a1``, ``a2`` are ``beta^step / (1 - beta^step)``, the factor by which an
    error of ``beta^step`` shows in the bias correction."""

    m: torch.Tensor
    v: torch.Tensor
    p: torch.Tensor  # unrounded
    s_m: torch.Tensor
    s_p: torch.Tensor
    t_q: torch.Tensor
    g: torch.Tensor  # the gradient the moments saw (clipped), fp64
    one_minus_b1: float
    one_minus_b2: float
    bc1: float
    bc2: float
    a1: float
    a2: float


def _f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


def clip_coef64(grads: Sequence[torch.Tensor], max_norm: float,
                round_hparams: bool = True) -> float:
    """``min(1, max_norm / (norm + 1e-6))`` with the global L2 norm of
    ``grads`` in fp64 from their stored values."""
    sumsq = 0.0
    for g in grads:
        sumsq += float(g.detach().double().pow(2).sum())
    norm = sumsq ** 0.5
    if round_hparams:
        max_norm = _f32(max_norm)
    return min(1.0, max_norm / (norm + 1e-6))


def adamw_ref64(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, *,
                lr: float, beta1: float, beta2: float, eps: float, weight_decay: float,
                step: int, coef: float = 1.0, round_hparams: bool = True) -> AdamWRef:
    """The step that takes the state to step count ``step`` (1 for the first)."""
    if round_hparams:
        lr, beta1, beta2, eps, weight_decay = (
            _f32(x) for x in (lr, beta1, beta2, eps, weight_decay))
    p, g, m, v = (t.detach().double() for t in (p, g, m, v))
    g = g * coef
    pow1, pow2 = beta1 ** step, beta2 ** step
    bc1, bc2 = 1.0 - pow1, 1.0 - pow2
    m_new = beta1 * m + (1.0 - beta1) * g
    v_new = beta2 * v + (1.0 - beta2) * g * g
    denom = (v_new / bc2).sqrt() + eps
    p_new = p - lr * ((m_new / bc1) / denom + weight_decay * p)
    s_m = beta1 * m.abs() + (1.0 - beta1) * g.abs()
    t_q = (s_m / bc1) / denom
    s_p = p.abs() + lr * (t_q + weight_decay * p.abs())
    return AdamWRef(m=m_new, v=v_new, p=p_new, s_m=s_m, s_p=s_p, t_q=t_q, g=g,
                    one_minus_b1=1.0 - beta1, one_minus_b2=1.0 - beta2,
                    bc1=bc1, bc2=bc2, a1=pow1 / bc1, a2=pow2 / bc2)


# ---- rounding="stochastic" (csrc/kernels/philox.h) -----------------------------

_M32 = 0xFFFFFFFF
_PHILOX_M = (0xD2511F53, 0xCD9E8D57)
_PHILOX_W = (0x9E3779B9, 0xBB67AE85)


def _mulhilo(a: int, b: torch.Tensor):
    """High and low 32 bits of ``a * b``; ``b`` holds 32-bit values in int64.
    The product is taken in two 16-bit halves of ``a`` so that it fits int64."""
    lo_part = (a & 0xFFFF) * b  # < 2^48
    hi_part = (a >> 16) * b  # < 2^48, worth 2^16 times more
    low = (lo_part + ((hi_part & 0xFFFF) << 16))  # < 2^49
    return ((hi_part >> 16) + (low >> 32)) & _M32, low & _M32


def philox4x32_10(counter: torch.Tensor, key) -> torch.Tensor:
    """Philox4x32-10 of ``counter`` (int64 ``[..., 4]``, 32-bit values) under
    the two 32-bit key words ``key``: int64 ``[..., 4]`` of 32-bit outputs."""
    c = [counter[..., i].to(torch.int64) & _M32 for i in range(4)]
    k0, k1 = (int(k) & _M32 for k in key)
    for _ in range(10):
        hi0, lo0 = _mulhilo(_PHILOX_M[0], c[0])
        hi1, lo1 = _mulhilo(_PHILOX_M[1], c[2])
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + _PHILOX_W[0]) & _M32, (k1 + _PHILOX_W[1]) & _M32
    return torch.stack(c, dim=-1)


def sr_bits(numel: int, *, seed: int, step: int, stream_id: int) -> torch.Tensor:
    """The 16 random bits of every element of a tensor (int64 ``[numel]``, on
    the CPU) as the kernel draws them: elements ``8j .. 8j+7`` share the call
    with the counter ``{j low, j high, step, stream_id}`` under the key ``seed``;
    element ``i`` of the eight takes bits ``16*(i&1) .. +16`` of word ``i>>1``."""
    j = torch.arange((numel + 7) // 8, dtype=torch.int64)
    counter = torch.stack([j & _M32, j >> 32, torch.full_like(j, step & _M32),
                           torch.full_like(j, stream_id)], dim=-1)
    words = philox4x32_10(counter, (seed & _M32, (seed >> 32) & _M32))
    halves = torch.stack([words & 0xFFFF, words >> 16], dim=-1)  # [n, 4, 2]
    return halves.reshape(-1)[:numel]


def stochastic_round_bf16(x_fp32: torch.Tensor, r16: torch.Tensor) -> torch.Tensor:
    """``x_fp32`` rounded to bf16 with the 16 random bits ``r16`` (int64, same
    shape): ``(bits + r16) >> 16`` for a finite value, round to nearest for inf
    and NaN."""
    assert x_fp32.dtype == torch.float32
    bits = x_fp32.contiguous().view(torch.int32).to(torch.int64) & _M32
    out = ((bits + (r16.to(bits.device) & 0xFFFF)) >> 16) & 0xFFFF
    out = torch.where(out >= 0x8000, out - 0x10000, out).to(torch.int16).view(torch.bfloat16)
    return torch.where(torch.isfinite(x_fp32), out, x_fp32.to(torch.bfloat16))
