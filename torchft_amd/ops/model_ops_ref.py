"""Plain-torch yardsticks for the RMSNorm / RoPE / SwiGLU kernels of
csrc/kernels/fused_model_ops.hip (docs/KERNELS.md, "Numerics" of that file).
No kernel is called here; everything runs on CPU or GPU tensors alike.

``*_ref64``     the operation in fp64 from the bf16 inputs (fp32 ``invrms`` and
                rotary tables as the kernels are fed them), with the
                magnitudes the error bounds of tests/model_ops_check.py are
                stated against. ``eps`` is rounded to fp32 first: that is the
                value the kernel receives.
``*_emulated``  each kernel's rounding chain in fp32 torch, written from the
                formulas in the ``.hip`` file: the same order of products,
                ``ss / H + eps`` then ``rsqrt``, ``inv * inv * inv * s / H``
                (``inv * s / H * inv * inv`` where ``inv^3`` is no normal fp32
                number), ``1 / (1 + exp(-a))`` in fp32, one rounding to bf16 at the
                store. It is the measure of what a correct fp32 chain costs and
                the statement of what non-finite inputs give; it is not a port:
                torch's summation order, no fma, the host's ``exp`` and
                ``rsqrt``. ``inject`` switches on one mistake at a time
                (``INJECTIONS``); tests/test_model_ops_numerics_cpu.py shows
                that the checker refuses each.

Shapes: RMSNorm ``x``, ``dy`` [rows, H], ``w`` [H], ``invrms`` [rows]; the
rotation ``x`` [B, S, Hh, D] with rotate-half pairing (i, i + D/2) and tables
[at least S, D/2], position ``s`` reading row ``s``; SwiGLU any shape, the
packed form ``gu`` [..., 2f] with gate ``gu[..., :f]`` and up ``gu[..., f:]``.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

U_BF16 = 2.0 ** -8   # unit round-off of bf16
E_FP32 = 2.0 ** -24  # unit round-off of fp32

INJECTIONS = {
    "rmsnorm_fwd": ("eps_before_div", "no_eps", "h_minus_1", "ss_bf16", "y_bf16_before_w",
                    "inv_bf16"),
    "rmsnorm_bwd": ("inv2_in_k", "k_without_1_over_h", "s_without_w"),
    "swiglu_fwd": ("sig_bf16", "halves_swapped", "sig_clamped"),
    "swiglu_bwd": ("sig_bf16", "da_without_b", "one_plus_sig", "db_from_sig",
                   "halves_swapped", "sig_clamped"),
    "rope": ("sin_sign_second_half", "backward_not_flipped", "row_plus_1"),
}


def _inject_ok(kernel: str, inject: Optional[str]) -> None:
    assert inject is None or inject in INJECTIONS[kernel], (kernel, inject)


def fp32_value(v: float) -> float:
    """``v`` rounded to fp32, as a Python float."""
    return torch.tensor(v, dtype=torch.float32).item()


# ------------------------------------------------------------------ fp64


def rmsnorm_fwd_ref64(x: torch.Tensor, w: torch.Tensor,
                      eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(invrms [rows], y [rows, H]): invrms = 1 / sqrt(mean(x^2) + eps),
    y = x * invrms * w."""
    xd = x.double()
    inv = 1.0 / torch.sqrt(xd.pow(2).mean(-1) + fp32_value(eps))
    return inv, xd * inv[..., None] * w.double()


@dataclass
class RmsnormBwdRef:
    """dx = invrms * w * dy - invrms^3 / H * x * sum(dy * w * x) per row and
    dw = sum over rows of dy * x * invrms, both from the ``invrms`` given (the
    kernel's input). ``mag`` is the sum of the absolute values of what enters
    dx, ``dw_abs`` of what enters dw."""

    dx: torch.Tensor
    dw: torch.Tensor
    mag: torch.Tensor
    dw_abs: torch.Tensor


def rmsnorm_bwd_ref64(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor,
                      invrms: torch.Tensor) -> RmsnormBwdRef:
    H = x.shape[-1]
    dyd, xd, wd = dy.double(), x.double(), w.double()
    inv = invrms.double()[..., None]
    dwx = dyd * wd * xd
    s = dwx.sum(-1, keepdim=True)
    dx = inv * wd * dyd - inv ** 3 * s / H * xd
    mag = inv * (wd * dyd).abs() + inv ** 3 * dwx.abs().sum(-1, keepdim=True) / H * xd.abs()
    terms = (dyd * xd * inv).reshape(-1, H)
    return RmsnormBwdRef(dx=dx, dw=terms.sum(0), mag=mag, dw_abs=terms.abs().sum(0))


def rotate_ref64(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                 backward: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out, mag) of the rotation, or of its transpose with ``backward``:
    out1 = x1 c - x2 s, out2 = x2 c + x1 s (s negated for the transpose);
    mag = |x1 c| + |x2 s| resp. |x2 c| + |x1 s|."""
    S, D = x.shape[1], x.shape[-1]
    c = cos[:S].double().view(1, S, 1, D // 2)
    s = sin[:S].double().view(1, S, 1, D // 2) * (-1.0 if backward else 1.0)
    x1, x2 = x.double().chunk(2, dim=-1)
    out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    mag = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], dim=-1)
    return out, mag


def sigmoid_ref64(a: torch.Tensor) -> torch.Tensor:
    """1 / (1 + exp(-a)) in fp64; 0 where exp overflows."""
    return 1.0 / (1.0 + torch.exp(-a.double()))


def swiglu_fwd_ref64(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """silu(a) * b = a * sig(a) * b."""
    return a.double() * sigmoid_ref64(a) * b.double()


@dataclass
class SwigluBwdRef:
    """da = dy * b * sig * (1 + a * (1 - sig)), db = dy * a * sig;
    ``mag_da`` = |dy * b * sig| * (1 + |a| * (1 - sig)): silu' has a zero near
    a = -1.278, where da cancels and its bound cannot be relative."""

    da: torch.Tensor
    db: torch.Tensor
    mag_da: torch.Tensor


def swiglu_bwd_ref64(dy: torch.Tensor, a: torch.Tensor, b: torch.Tensor) -> SwigluBwdRef:
    dyd, ad, bd = dy.double(), a.double(), b.double()
    sig = sigmoid_ref64(a)
    p = dyd * bd * sig
    return SwigluBwdRef(da=p * (1.0 + ad * (1.0 - sig)), db=dyd * ad * sig,
                        mag_da=p.abs() * (1.0 + ad.abs() * (1.0 - sig)))


# ------------------------------------------------------------------ fp32 chains


def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).float()


def _out(t: torch.Tensor, store: bool) -> torch.Tensor:
    """The kernel's bf16 store, or with ``store=False`` the fp32 value ahead
    of it: what the fp32 part of a bound is measured on."""
    return t.to(torch.bfloat16) if store else t


def rmsnorm_fwd_emulated(x: torch.Tensor, w: torch.Tensor, eps: float, *, store: bool = True,
                         inject: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y bf16, invrms fp32) as ``rmsnorm_fwd_kernel`` computes them."""
    _inject_ok("rmsnorm_fwd", inject)
    H = x.shape[-1]
    xf, wf = x.float(), w.float()
    eps32 = torch.tensor(eps, dtype=torch.float32, device=x.device)
    sq = xf * xf
    ss = _bf(_bf(sq).sum(-1)) if inject == "ss_bf16" else sq.sum(-1)
    if inject == "eps_before_div":
        ms = (ss + eps32) / H
    elif inject == "no_eps":
        ms = ss / H
    elif inject == "h_minus_1":
        ms = ss / (H - 1) + eps32
    else:
        ms = ss / H + eps32
    inv = torch.rsqrt(ms)
    used = _bf(inv) if inject == "inv_bf16" else inv
    xn = xf * used[..., None]
    if inject == "y_bf16_before_w":
        xn = _bf(xn)
    return _out(xn * wf, store), inv


def rmsnorm_bwd_emulated(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor,
                         invrms: torch.Tensor, *, store: bool = True,
                         inject: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dx bf16, dw fp32 [H]) as ``rmsnorm_bwd_kernel`` computes them."""
    _inject_ok("rmsnorm_bwd", inject)
    H = x.shape[-1]
    d, v, g = dy.float(), x.float(), w.float()
    inv = invrms.float()[..., None]
    s = (d * v if inject == "s_without_w" else d * g * v).sum(-1, keepdim=True)
    if inject == "inv2_in_k":
        k = inv * s / H * inv
    elif inject == "k_without_1_over_h":
        k = inv * s * inv * inv
    else:
        # inv^3 first where it is a normal fp32 number, inv * s first elsewhere
        inv3 = inv * inv * inv
        k = torch.where(inv3 >= torch.finfo(torch.float32).tiny, inv3 * s / H,
                        inv * s / H * inv * inv)
    dx = _out(inv * g * d - k * v, store)
    dw = (d * v * inv).reshape(-1, H).sum(0)
    return dx, dw


def rope_emulated(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                  backward: bool = False, *, store: bool = True,
                  inject: Optional[str] = None) -> torch.Tensor:
    """``rope_kernel``: two fp32 products and a sum per output, the sign of
    the transpose multiplied into the sine first (exact)."""
    _inject_ok("rope", inject)
    S, D = x.shape[1], x.shape[-1]
    first = 1 if inject == "row_plus_1" else 0
    c = cos[first:first + S].float().view(1, S, 1, D // 2)
    s = sin[first:first + S].float().view(1, S, 1, D // 2)
    if backward and inject != "backward_not_flipped":
        s = s * -1.0
    x1, x2 = x.float().chunk(2, dim=-1)
    o1 = x1 * c - x2 * s
    o2 = x2 * c - x1 * s if inject == "sin_sign_second_half" else x2 * c + x1 * s
    return _out(torch.cat([o1, o2], dim=-1), store)


def _sigmoid32(a: torch.Tensor, inject: Optional[str]) -> torch.Tensor:
    sig = 1.0 / (1.0 + torch.exp(-a))
    if inject == "sig_bf16":
        sig = _bf(sig)
    if inject == "sig_clamped":
        sig = torch.where(a < -20.0, torch.zeros_like(sig), sig)
    return sig


def swiglu_fwd_emulated(a: torch.Tensor, b: torch.Tensor, *, store: bool = True,
                        inject: Optional[str] = None) -> torch.Tensor:
    """``swiglu_fwd8``: o = a * sig * b, bf16."""
    _inject_ok("swiglu_fwd", inject)
    af, bf = a.float(), b.float()
    if inject == "halves_swapped":
        af, bf = bf, af
    return _out(af * _sigmoid32(af, inject) * bf, store)


def swiglu_bwd_emulated(dy: torch.Tensor, a: torch.Tensor, b: torch.Tensor, *,
                        store: bool = True, inject: Optional[str] = None
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``swiglu_bwd1``: (da, db) bf16. With ``halves_swapped`` the gate and up
    are read, and their gradients written, in each other's place."""
    _inject_ok("swiglu_bwd", inject)
    d, af, bf = dy.float(), a.float(), b.float()
    if inject == "halves_swapped":
        af, bf = bf, af
    sig = _sigmoid32(af, inject)
    silu = af * sig
    da = d * sig if inject == "da_without_b" else d * bf * sig
    da = da * (1.0 + af * ((1.0 + sig) if inject == "one_plus_sig" else (1.0 - sig)))
    db = d * sig if inject == "db_from_sig" else d * silu
    if inject == "halves_swapped":
        da, db = db, da
    return _out(da, store), _out(db, store)


def swiglu_glu_fwd_emulated(gu: torch.Tensor, *, inject: Optional[str] = None) -> torch.Tensor:
    f = gu.shape[-1] // 2
    return swiglu_fwd_emulated(gu[..., :f], gu[..., f:], inject=inject)


def swiglu_glu_bwd_emulated(dy: torch.Tensor, gu: torch.Tensor, *,
                            inject: Optional[str] = None) -> torch.Tensor:
    """dgu [..., 2f]: dgate in the gate half, dup in the up half."""
    f = gu.shape[-1] // 2
    return torch.cat(swiglu_bwd_emulated(dy, gu[..., :f], gu[..., f:], inject=inject), dim=-1)
