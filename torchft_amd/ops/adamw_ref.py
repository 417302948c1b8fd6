"""Plain fp64 yardstick for ``adamw_kernel`` (csrc/kernels/fused_adamw.hip;
docs/KERNELS.md, "Numerics" of fused_adamw.hip). Runs on CPU or GPU.

``adamw_ref64``  one decoupled-weight-decay Adam step in fp64 from the stored
                 ``p``, ``g`` (bf16) and ``m``, ``v`` (fp32), with the sums of
                 absolute values that the error bounds are multiples of.
``clip_coef64``  the clip coefficient of the clip mode, the norm taken in fp64.

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
