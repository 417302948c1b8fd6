"""The criteria ``cross_entropy_kernel`` (csrc/kernels/fused_cross_entropy.hip)
is held to, the seeded input families it is held to them on, the sentinel
buffer its logits live in, and an fp32 evaluation of its chain with switchable
mistakes (docs/KERNELS.md, "Numerics" of fused_cross_entropy.hip). Shared by
the CPU test of the checker itself and by the GPU tests; plain torch on the CPU.

The reference is ``cross_entropy_ref`` on ``x.double()``. ``u = 2^-24`` is the
unit roundoff of an fp32 operation, ``2^-8`` that of the bf16 store. With ``m``
the row maximum, ``d = m - x[j]``, ``s = sum exp(x - m)``, ``p = softmax(x)``,
``lse = m + log s`` and ``A = 1 + 2 z |lse|``:

``__expf(a)``   is ``exp2(a * log2(e))`` (clang's ``__clang_hip_math.h``): the
    product is rounded once, which moves the result by ``|a| u`` relative, the
    constant is off by less than that again, and ``V_EXP_F32`` is good to 1 ulp
    ``= 2u`` (CDNA ISA guide): ``(2 + 2|a|) u``. The argument ``a = x - m`` is a
    difference of two bf16 values, exact when they are close and rounded by at
    most ``|a| u`` otherwise: ``(2 + 3|a|) u`` in all.
``s``   every summand is a product of ``__expf`` factors whose arguments add up
    to ``-d``: its own, one rescaling per trip of the vector loop (``T`` trips,
    ``T <= V // 8192 + 1``), one in the scalar combine and one in each of the
    6 + 15 combines across the workgroup, ``T + 23`` factors, ``2 (T + 23) + 3d``
    units, one product per rescaling (``T + 22``) and ``8T + 22`` additions.
    All summands are positive, so the error is relative to ``s``, and ``sum p d
    = H - log s <= ln V`` (``H`` the entropy):
    ``S_UNITS = 11 T + 90 + 3 ln V``.
``lse``  ``logf`` 1 ulp, the sum one rounding: ``u (|lse| + 2 |log s| + S_UNITS)``.
``coef = gs (1 + 2 z lse) / s``   ``float(z)``, ``2z * lse``, ``1 +``, ``gs *``
    one rounding each at magnitude ``A`` or below, the quotient one ulp, ``lse``'s
    own error ``2z`` times the line above, ``1 / s`` its ``S_UNITS``.
``g[j] = coef * __expf(x[j] - m)``   the exponential ``(2 + 3d) u``, the
    product one rounding.

Off the target that is ``F = u gs p A (12 + 3d + (1 + 2z) S_UNITS)``: 2 for the
exponential, 2 for the quotient, 5 single roundings, 2 for ``lse`` and ``log
s``'s share at ``z <= 1e-2``, 1 for second order. ``gs p A`` is ``|g_ref|``
whenever ``lse >= 0``; where ``1 + 2 z lse`` cancels (``lse`` near ``-1 / 2z``)
the error does not shrink with it, so the bound is on magnitude. At the target
the subtraction ``g - gs`` rounds once more on a result no larger than ``gs``,
and the ``gs`` subtracted is the fp32 rounding of the caller's value:
``+ 2 u gs``. The floor: ``V_EXP_F32`` flushes a result below ``2^-126`` to zero,
which costs up to ``coef 2^-126``, an fp32 product below the normal range may be
flushed likewise, and bf16's subnormal step is ``2^-133``:
``2^-126 (1 + gs A / s) + 2^-134``.

    |g - g_ref| <= 2^-8 |g_ref| + F

Row loss: ``4 eps max(max|x|, |loss_ref|)`` as before (``eps = 2u``), and for
``T_z = z lse^2``: ``float(z)``, two products, the sum and twice ``lse``'s
relative rounding are ``6 u T_z``; the rest of ``lse``'s error enters with
``2 z |lse|``: ``+ u (6 T_z + 2 z |lse| (2 |log s| + S_UNITS))``.

Rows are held by class. Ignored: loss ``+0`` and every gradient bit zero. A row
with a NaN or ``+inf`` logit, an all ``-inf`` row or an out-of-range target:
non-finite loss and no finite gradient element (the kernel gives NaN for
``+inf`` where the definition gives ``+inf``: ``inf - inf`` in the running
maximum's subtraction; stated as intended in docs/KERNELS.md). A target on a
``-inf`` logit: loss exactly ``+inf``, gradient under the bound.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from torchft_amd.ops.cross_entropy import cross_entropy_ref

IGNORE = -100
U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
EPS32 = 2.0 ** -23
NINF = float("-inf")

PAD = 64  # sentinel elements on either side; a multiple of 8, so that the
# element offset o is the view's misalignment
SENTINEL_BITS = 0x4B4B  # bf16 13303808.0: finite, and no gradient looks like it

Z_GRID = (0.0, 1e-4, 1e-2)
GS_GRID = (1.0, 1.0 / 29, 2.0 ** -20, 0.0)
FAMILIES = ("randn4", "randn3000", "flat", "needle", "neg_inf", "nonfinite")


def s_units(V: int) -> float:
    return 11 * (V // 8192 + 1) + 90 + 3 * math.log(V)


# ---- logits inside a sentinel buffer ------------------------------------------


@dataclass
class Case:
    """bf16 logits as a contiguous [R, V] view at element ``PAD + o`` of a
    sentinel-filled 1-D buffer, and int64 targets."""

    buf: torch.Tensor
    R: int
    V: int
    o: int
    t: torch.Tensor

    def view(self) -> torch.Tensor:
        lo = PAD + self.o
        return self.buf[lo : lo + self.R * self.V].view(self.R, self.V)

    def to(self, device) -> "Case":
        """A fresh copy on ``device``: the kernel writes into it."""
        return Case(self.buf.clone().to(device), self.R, self.V, self.o, self.t.to(device))

    def assert_sentinels(self, what: str = "") -> None:
        bits = self.buf.cpu().view(torch.int16)
        lo = PAD + self.o
        outside = torch.cat([bits[:lo], bits[lo + self.R * self.V :]])
        bad = int((outside != SENTINEL_BITS).sum())
        assert bad == 0, f"sentinel: {bad} elements outside the view were written {what}"


def make_case(x: torch.Tensor, t: torch.Tensor, o: int = 0) -> Case:
    R, V = x.shape
    assert 0 <= o < 8
    buf = torch.full((PAD + o + R * V + PAD + 8,), SENTINEL_BITS, dtype=torch.int16)
    buf = buf.view(torch.bfloat16)
    case = Case(buf, R, V, o, t.clone())
    case.view().copy_(x.to(torch.bfloat16))
    return case


def family(name: str, R: int = 6, V: int = 1003, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(bf16 logits [R, V], targets [R]) of one family; R >= 6, V >= 4."""
    assert name in FAMILIES and R >= 6 and V >= 4
    g = torch.Generator().manual_seed(7919 * FAMILIES.index(name) + 1000 * R + V + seed)
    noise = torch.randn(R, V, generator=g)
    t = torch.randint(0, V, (R,), generator=g)
    t[0], t[1] = 0, V - 1
    run = min(16, V - 1)  # covers the scalar head and lane 0's first vector
    if name == "randn4":
        x = 4.0 * noise
        t[2] = IGNORE
    elif name == "randn3000":  # with the -inf run of the older test_extremes
        x = 3000.0 * noise
        x[4, V // 10 : 7 * V // 10] = NINF
        t[4] = V // 20
        t[2] = IGNORE
    elif name == "flat":
        # -57: lse = -50.09 at V = 1003, where 1 + 2 z lse cancels for z = 1e-2
        vals = torch.tensor([0.0, 1.0, 5.0, 88.0, -3000.0, -57.0])
        x = vals[torch.arange(R) % 6].unsqueeze(1).expand(R, V).clone()
        t[2] = IGNORE
    elif name == "needle":
        x = noise.clone()
        for r in range(R):
            # even rows: the target is the needle, g[t] = gs (p - 1) cancels;
            # odd rows: the mirror, a needle elsewhere
            col = int(t[r]) if r % 2 == 0 else (int(t[r]) + V // 2) % V
            x[r, col] += 40.0
    elif name == "neg_inf":
        x = 4.0 * noise
        x[0, :run] = NINF  # lane 0 starts on -inf, finite afterwards
        t[0] = V - 2
        keep = x[1, V - 1].clone()
        x[1] = NINF  # the target is the only finite logit
        x[1, V - 1] = keep
        x[2] = NINF  # the only finite logit is not the target
        x[2, V // 2] = 3.25
        t[2] = V // 2 - 1
        x[3, int(t[3])] = NINF  # a target on a -inf logit
        x[4, ::3] = NINF
        t[4] = IGNORE
    else:  # nonfinite
        x = 4.0 * noise
        x[0, V // 2] = float("nan")
        x[1, 3] = float("inf")
        x[2] = NINF
        x[3, int(t[3])] = float("nan")
        x[4, 1] = float("nan")
        t[4] = IGNORE
    return x.to(torch.bfloat16), t


# ---- the bounds and the class rules -------------------------------------------


def _frac(err: torch.Tensor, bound: torch.Tensor) -> float:
    # a NaN error or a zero bound with a non-zero error must fail
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    if ratio.numel() == 0:
        return 0.0
    worst = float(ratio.max())
    return math.inf if (ratio != ratio).any() else worst


class Bounds:
    """Reference, row classes and bounds of one (x, t, z, gs), all fp64 on the
    CPU. ``F`` is the fp32 part of the gradient bound."""

    def __init__(self, x: torch.Tensor, t: torch.Tensor, z: float, gs: float) -> None:
        x, t = x.detach().cpu(), t.detach().cpu()
        assert x.dtype == torch.bfloat16
        R, V = x.shape
        xd = x.double()
        self.ref_loss, self.ref_grad = cross_entropy_ref(xd, t, IGNORE, z, gs)
        self.ignored = t == IGNORE
        oob = ~self.ignored & ((t < 0) | (t >= V))
        broken = torch.isnan(xd).any(1) | (xd == math.inf).any(1) | (xd == NINF).all(1)
        self.nonfinite = ~self.ignored & (oob | broken)
        self.finite = ~self.ignored & ~self.nonfinite
        self.inf_loss = self.finite & (self.ref_loss == math.inf)

        f = self.finite
        xf = torch.where(f.unsqueeze(1), xd, torch.zeros_like(xd))
        m = xf.amax(dim=1, keepdim=True)
        lse = torch.logsumexp(xf, dim=1, keepdim=True)
        log_s = lse - m
        p = torch.exp(xf - lse)
        d = torch.where(torch.isfinite(xf), m - xf, torch.zeros_like(xf))
        A = 1.0 + 2.0 * z * lse.abs()
        su = s_units(V)
        units = 12.0 + 3.0 * d + (1.0 + 2.0 * z) * su
        F = U32 * gs * p * A * units
        safe_t = torch.where(f, t, torch.zeros_like(t)).unsqueeze(1)
        F.scatter_add_(1, safe_t, torch.full((R, 1), 2 * U32 * gs, dtype=torch.float64))
        F = F + 2.0 ** -126 * (1.0 + gs * A / torch.exp(log_s)) + 2.0 ** -134
        self.F = F
        self.grad_bound = U_BF16 * self.ref_grad.abs() + F

        xmax = torch.where(torch.isfinite(xf), xf.abs(), torch.zeros_like(xf)).amax(dim=1)
        lse, log_s = lse.squeeze(1), log_s.squeeze(1)
        t_z = z * lse * lse
        self.loss_bound = (4 * EPS32 * torch.maximum(xmax, self.ref_loss.abs())
                           + U32 * (6 * t_z + 2 * z * lse.abs() * (2 * log_s.abs() + su)))


def check(x: torch.Tensor, t: torch.Tensor, row_loss: torch.Tensor, grad: Optional[torch.Tensor],
          z: float, gs: float, tag: str = "", rows: Optional[torch.Tensor] = None,
          F_share: Optional[float] = None) -> Dict[str, float]:
    """Hold one launch's results to every criterion; print and return the worst
    fractions. ``grad`` None: a loss-only launch. ``rows``: hold only these.
    ``F_share``: ``grad`` is the fp32 value ahead of the bf16 store and must
    stay under this share of ``F`` alone."""
    b = Bounds(x, t, z, gs)
    row_loss = row_loss.detach().cpu()
    assert row_loss.dtype == torch.float32 and row_loss.shape == (x.shape[0],)
    sel = torch.ones_like(b.finite) if rows is None else torch.zeros_like(b.finite)
    if rows is not None:
        sel[rows.cpu()] = True
    out: Dict[str, float] = {}

    ign = b.ignored & sel
    assert (row_loss[ign].view(torch.int32) == 0).all(), f"{tag}: ignored row: loss is not +0"
    bad = b.nonfinite & sel
    assert not torch.isfinite(row_loss[bad]).any(), (
        f"{tag}: class: finite loss in a row with a NaN / +inf logit, no finite logit or "
        "a target out of range")
    fin = b.finite & sel
    inf_rows = b.inf_loss & sel
    assert (row_loss[inf_rows] == math.inf).all(), (
        f"{tag}: class: a target on a -inf logit must give a +inf loss")
    held = fin & ~b.inf_loss
    assert torch.isfinite(row_loss[held]).all(), f"{tag}: loss bound: non-finite loss"
    out["loss"] = _frac((row_loss.double() - b.ref_loss)[held].abs(), b.loss_bound[held])

    if grad is not None:
        grad = grad.detach().cpu()
        if F_share is None:
            assert grad.dtype == torch.bfloat16
            zero_bits = grad.view(torch.int16) == 0
        else:
            zero_bits = grad.view(torch.int32) == 0
        assert zero_bits[ign].all(), f"{tag}: ignored row: a gradient element is not +0"
        assert not torch.isfinite(grad[bad]).any(), (
            f"{tag}: class: finite gradient element in a non-finite row")
        assert torch.isfinite(grad[fin]).all(), f"{tag}: gradient bound: non-finite gradient"
        err = (grad.double() - b.ref_grad)[fin].abs()
        if F_share is None:
            out["grad"] = _frac(err, b.grad_bound[fin])
            # what the bf16 term does not explain, as a fraction of F
            out["F"] = _frac((err - U_BF16 * b.ref_grad[fin].abs()).clamp(min=0), b.F[fin])
        else:
            out["F"] = _frac(err, b.F[fin])

    print(f"{tag} shape={tuple(x.shape)} z={z} gs={gs:.3g}: worst error / bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in out.items()))
    assert out["loss"] <= 1.0, f"{tag}: loss bound: off by {out['loss']:.3f} x bound"
    if grad is not None and F_share is None:
        assert out["grad"] <= 1.0, f"{tag}: gradient bound: off by {out['grad']:.3f} x bound"
    if grad is not None and F_share is not None:
        assert out["F"] <= F_share, (
            f"{tag}: gradient bound: fp32 chain at {out['F']:.3f} of F, over {F_share:.3f}")
    return out


# ---- the kernel's chain in fp32 torch, with switchable mistakes ---------------

INJECTIONS = ("z_dropped", "z_halved", "truncating_store", "tail_out_of_sum",
              "head_out_of_sum", "onehot_unscaled", "onehot_shifted", "bf16_x_minus_lse",
              "ignored_not_zeroed", "loss_without_z")


def _truncate_bf16(g: torch.Tensor) -> torch.Tensor:
    bits = g.contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(torch.bfloat16)


def ce_chain32(x: torch.Tensor, t: torch.Tensor, z: float, gs: float,
               inject: Optional[str] = None, store: bool = True):
    """(row_loss fp32, gradient) as the kernel forms them, every operation a
    separate fp32 torch op on the CPU: row maximum, ``exp(x - m)``, the sum,
    ``logf``, ``coef = gs (1 + 2 z lse) / s``, the product and ``- gs`` at the
    target. ``store`` False returns the fp32 gradient ahead of the bf16 store."""
    assert inject is None or inject in INJECTIONS
    R, V = x.shape
    xf = x.float()
    z32, gs32 = torch.tensor(z, dtype=torch.float32), torch.tensor(gs, dtype=torch.float32)
    ignored = t == IGNORE
    ok = ~ignored & (t >= 0) & (t < V)
    safe_t = torch.where(ok, t, torch.zeros_like(t)).unsqueeze(1)
    m = xf.amax(dim=1, keepdim=True)
    e = torch.exp(xf - m)
    e_sum = e
    if inject == "tail_out_of_sum":
        e_sum = e[:, :-1]
    elif inject == "head_out_of_sum":
        e_sum = e[:, 1:]
    s = e_sum.sum(dim=1, keepdim=True)
    log_s = torch.log(s)
    lse = m + log_s
    xt = xf.gather(1, safe_t)
    loss = (m - xt) + log_s
    if inject != "loss_without_z":
        loss = loss + z32 * lse * lse
    if inject == "z_dropped":
        factor = torch.ones_like(lse)
    elif inject == "z_halved":
        factor = 1.0 + z32 * lse
    else:
        factor = 1.0 + 2.0 * z32 * lse
    if inject == "bf16_x_minus_lse":
        g = gs32 * factor * torch.exp((xf - lse).to(torch.bfloat16).float())
    else:
        g = (gs32 * factor / s) * e
    hot_col = safe_t + 1 if inject == "onehot_shifted" else safe_t
    hot = torch.zeros_like(g)
    inside = ok.unsqueeze(1) & (hot_col < V)
    hot.scatter_(1, hot_col.clamp(max=V - 1), inside.float())
    g = g - hot * (1.0 if inject == "onehot_unscaled" else gs32)
    nan = torch.tensor(float("nan"))
    loss = torch.where(ok, loss.squeeze(1), nan)
    g = torch.where(ok.unsqueeze(1), g, nan)
    loss = torch.where(ignored, torch.zeros(()), loss)
    if inject == "ignored_not_zeroed":
        g = torch.where(ignored.unsqueeze(1), xf, g)
    else:
        g = torch.where(ignored.unsqueeze(1), torch.zeros(()), g)
    if not store:
        return loss, g
    return loss, (_truncate_bf16(g) if inject == "truncating_store" else g.to(torch.bfloat16))
