"""The criteria the kernels of csrc/kernels/fused_model_ops.hip are held to
against torchft_amd/ops/model_ops_ref.py, and the seeded input families they
are held to them on (docs/KERNELS.md, "Numerics" of that file). Shared by the
checker's own CPU test and by the GPU tests; plain torch, the arithmetic on the
CPU in fp64. Every ``check_*`` prints its worst error over bound, raises an
``AssertionError`` that begins with the criterion's name, and returns the worst
fractions by name.

Every bound counts roundings: ``u = 2^-8`` is the unit round-off of the one
bf16 store, ``e = 2^-24`` that of an fp32 operation, and an error of one ulp
(a hardware approximation) is ``2e``. Nothing is tuned on kernel output.

``invrms``   ``|got - ref| <= (depth/2 + 3) e |ref|``. ``depth(H)`` counts the
    fp32 roundings on a partial sum of squares, all of one sign, the way
    ``_depth`` of tests/test_grad_clip_gpu.py does: the product, ``8 *
    ceil(H / 2048)`` adds in the lane, 6 shuffle steps, 3 wave adds. The root
    halves that. Then the division by ``H`` and the sum with ``eps`` (``e``
    each on the mean, halved: ``e`` together; ``H < 2^24`` converts exactly,
    ``eps`` is taken as the fp32 value the kernel receives) and ``rsqrtf``, one
    ulp ``= 2e``: 3. The figure for ``rsqrtf`` is the "1 ULP" of the table of
    single-precision device functions in the HIP documentation ("HIP math
    API"); that table is not in the ROCm tree this was written against, and
    the CDNA ISA guide gives ``V_RSQ_F32`` the same 1 ulp.
``y``   ``|got - ref| <= (u + k e) |ref|`` with ``k = depth/2 + 3 + 3``:
    ``inv``, the two products, and one unit for the products of these terms
    with ``u``. In addition ``y`` is never more than one bf16 ulp from the
    fp64 value rounded to bf16 and differs from it in at most 0.1 % of the
    elements of a case (a tie broken the other way; the project's cap, as for
    DiLoCo and AdamW).
``dx``  ``T1 - T2`` with ``T1 = inv w dy`` and ``T2 = inv^3 s / H x``, ``s =
    sum(dy w x)``, cancels, so the bound is on ``mag = inv |w dy| + inv^3
    sum|dy w x| / H |x|``: ``u |ref| + k e mag``. The reference takes the
    ``invrms`` the kernel is fed, so ``inv`` is exact. ``T1``: two products and
    the subtraction, 3. ``T2``: ``s`` has two products and ``depth - 1`` adds,
    then three products and a division for ``k`` (in either order of the
    kernel's), ``k * x`` and the subtraction: ``depth + 7``. One unit for
    second order: ``k = depth + 8``.
``dw``  per column ``(rows + 8) 2^-23 sum|dy x invrms|``: each term is rounded
    in two products and the rows are added one at a time in some order, at
    most ``rows + 1`` roundings of partial sums below ``sum|term|``, with a
    factor of two left (unchanged from tests/test_model_ops_gpu.py).
rotation    ``(u + 3e) (|x1 c| + |x2 s|)``: two products, one sum, one store
    (tests/test_qkv_rope_gpu.py).
``o``, ``db``   ``o = a sig b``, ``sig = 1 / (1 + E)``, ``E = exp(-a)``. ``E``
    carries ``|a| e`` for the rounding of ``a log2(e)`` ahead of the hardware
    exponential and ``2e`` for that instruction (1 ulp); its share in ``sig``
    is ``(1 - sig) <= 1`` of that. The sum ``1 + E`` is ``e``, the quotient
    ``2e`` (one ulp allowed), the two products ``2e``, second order 1:
    ``(u + (8 + |a|) e) |ref| + 2^-126 |a b| + 2^-133``. The ``2^-126`` floor
    covers ``sig`` flushed or rounded below the fp32 normal range (``a`` from
    -87.3 down; at -88.8 ``E`` is inf and ``sig`` 0 while the true product is
    still a normal bf16 number); ``2^-133`` is the bf16 subnormal step.
    ``db = dy a sig`` likewise with ``dy a`` in the floor.
``da``  ``da = P Q``, ``P = dy b sig``, ``Q = 1 + a (1 - sig)``; on magnitude,
    because ``silu'`` has a zero near ``a = -1.278``: ``u |ref| + (c + |a|) e
    mag + 2^-126 |dy b| (1 + |a|) + 2^-133``, ``mag = |P| (1 + |a| (1 - sig))``.
    ``sig`` is off by ``d = ((1 - sig)(2 + |a|) + 3) e`` relative; ``P`` adds
    two products. In ``Q`` the absolute error ``sig d`` of ``sig`` is
    multiplied by ``|a|``: the part ``|a| sig (1 - sig)(2 + |a|) e`` is at most
    ``sig (2 + |a|) e`` of ``Q``'s magnitude, which with the ``(1 - sig)(2 +
    |a|) e`` in ``P`` makes ``(2 + |a|) e``; the part ``3 |a| sig e`` is not
    small against ``Q ~ 1`` for positive ``a``, but from ``a = 17.33`` on ``E <
    2^-25``, ``1 + E`` rounds to 1, ``sig`` is exactly 1 and what is lost is
    ``a E <= a e``: ``3 * 17.33 = 52``. ``1 - sig``, ``a * ()`` and ``1 + ()``
    are 3, the last product 1, second order 1: ``c = 2 + 3 + 2 + 52 + 3 + 1 +
    1 = 64``.
class   where the fp32 emulation gives NaN, +inf or -inf the kernel gives the
    same, and where it is finite the kernel is finite.
"""

from __future__ import annotations

import math
from typing import Dict, Tuple

import torch

from torchft_amd.ops import model_ops_ref as ref

U = ref.U_BF16
E = ref.E_FP32
BF16 = torch.bfloat16
FLIP_CAP = 1e-3
C_INV = 3
C_SWIGLU = 8
C_SWIGLU_DA = 64
NORMAL_FLOOR = 2.0 ** -126  # the smallest normal fp32 and bf16 number
BF16_STEP = 2.0 ** -133     # the bf16 subnormal step


def depth(H: int) -> int:
    return 1 + 8 * math.ceil(H / 2048) + 6 + 3


def k_invrms(H: int) -> float:
    return depth(H) / 2 + C_INV


def k_y(H: int) -> float:
    return k_invrms(H) + 3


def k_dx(H: int) -> int:
    return depth(H) + 8


def ordered(t: torch.Tensor) -> torch.Tensor:
    """bf16 bit patterns as integers ordered like the values (+0 == -0)."""
    i = t.view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _hold(name: str, label: str, err: torch.Tensor, bound: torch.Tensor) -> float:
    # a NaN error or a zero bound with a non-zero error must fail
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = ~(err <= bound)
    print(f"{label}: {name} worst error / bound {worst:.4f}")
    assert not bad.any() and worst == worst, (
        f"{name}: {label}: outside its bound in {int(bad.sum())} of {err.numel()} "
        f"elements, worst error / bound {worst:.3g}")
    return worst


def _hold_bf16(name: str, label: str, got: torch.Tensor, want64: torch.Tensor) -> float:
    """The two-part bf16 criterion; returns the differing fraction over the cap."""
    assert got.dtype == BF16
    steps = (ordered(got) - ordered(want64.to(BF16))).abs()
    differing, total = int((steps != 0).sum()), got.numel()
    frac = differing / max(total, 1)
    print(f"{label}: {name} differs from the rounded fp64 value in {differing} of {total} "
          f"elements ({100 * frac:.4f} %), at most {int(steps.max()) if total else 0} ulp")
    assert not (steps > 1).any(), (
        f"{name} bf16: {label}: {int((steps > 1).sum())} elements more than one bf16 ulp "
        "from the rounded fp64 value")
    assert differing <= FLIP_CAP * total, (
        f"{name} bf16: {label}: {differing} of {total} elements differ from the rounded "
        "fp64 value, more than 0.1 %")
    return frac / FLIP_CAP


def _store(t: torch.Tensor, stored: bool) -> Tuple[float, float]:
    """(u, bf16 subnormal step) of the bound: those of the bf16 store for a
    kernel's output, zero for an fp32 chain taken before its store, which is
    then held to the fp32 part of the bound alone."""
    assert t.dtype == (BF16 if stored else torch.float32), t.dtype
    return (U, BF16_STEP) if stored else (0.0, 0.0)


def _class(t: torch.Tensor) -> torch.Tensor:
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    t = t.float()
    return (torch.isnan(t) * 1 + (t == float("inf")) * 2 + (t == float("-inf")) * 3)


def check_class(name: str, label: str, got: torch.Tensor, emulated: torch.Tensor) -> None:
    bad = _class(got.cpu()) != _class(emulated.cpu())
    assert not bad.any(), (
        f"class: {label}: {name} is NaN / +inf / -inf / finite where the fp32 chain is "
        f"not, in {int(bad.sum())} elements, first at {bad.flatten().nonzero()[0].item()}")


# ---- RMSNorm ------------------------------------------------------------------


def check_rmsnorm_fwd(label: str, y: torch.Tensor, invrms: torch.Tensor, x: torch.Tensor,
                      w: torch.Tensor, eps: float, stored: bool = True) -> Dict[str, float]:
    y, invrms, x, w = y.cpu(), invrms.cpu(), x.cpu(), w.cpu()
    H = x.shape[-1]
    u, _ = _store(y, stored)
    assert y.shape == x.shape
    assert invrms.dtype == torch.float32 and invrms.shape == x.shape[:-1]
    inv64, y64 = ref.rmsnorm_fwd_ref64(x, w, eps)
    out = {"invrms": _hold("invrms", label, (invrms.double() - inv64).abs(),
                           k_invrms(H) * E * inv64)}
    out["y"] = _hold("y", label, (y.double() - y64).abs(), (u + k_y(H) * E) * y64.abs())
    if stored:
        out["y bf16"] = _hold_bf16("y", label, y, y64)
    return out


def check_rmsnorm_bwd(label: str, dx: torch.Tensor, dw: torch.Tensor, dy: torch.Tensor,
                      x: torch.Tensor, w: torch.Tensor, invrms: torch.Tensor,
                      stored: bool = True) -> Dict[str, float]:
    """``invrms`` is what the kernel was fed; ``dw`` its fp32 sum."""
    dx, dw, dy, x, w, invrms = (t.cpu() for t in (dx, dw, dy, x, w, invrms))
    H = x.shape[-1]
    rows = x.numel() // H
    u, _ = _store(dx, stored)
    assert dx.shape == x.shape
    assert dw.dtype == torch.float32 and dw.shape == (H,)
    r = ref.rmsnorm_bwd_ref64(dy, x, w, invrms)
    out = {"dx": _hold("dx", label, (dx.double() - r.dx).abs(),
                       u * r.dx.abs() + k_dx(H) * E * r.mag)}
    out["dw"] = _hold("dw", label, (dw.double() - r.dw).abs(),
                      (rows + 8) * 2.0 ** -23 * r.dw_abs)
    return out


RMSNORM_SHAPES = [(1, 8), (3, 2048), (3, 2056), (5, 4104), (2049, 8)]
RMSNORM_FAMILIES = ["randn", "small", "large", "zero_row", "one_hot", "w_zeros", "eps6"]
_X_SCALE = {"small": 2.0 ** -10, "large": 2.0 ** 40}


def rmsnorm_inputs(rows: int, H: int, family: str = "randn"
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, float]:
    """(x, w, dy, eps) on the CPU, bf16. ``small``: eps dominates mean(x^2);
    ``zero_row`` / ``one_hot``: row 0 is zeros, resp. zeros but for one 2^60."""
    gen = torch.Generator().manual_seed(
        7919 * RMSNORM_FAMILIES.index(family) + 31 * rows + H)
    x = (_X_SCALE.get(family, 1.0) * torch.randn(rows, H, generator=gen)).to(BF16)
    w = torch.randn(H, generator=gen).to(BF16)
    dy = torch.randn(rows, H, generator=gen).to(BF16)
    if family in ("zero_row", "one_hot"):
        x[0] = 0
    if family == "one_hot":
        x[0, (5 * H) // 8 - 1] = -(2.0 ** 60)
    if family == "w_zeros":
        w[::3] = 0
    return x, w, dy, (1e-6 if family == "eps6" else 1e-5)


# ---- rotation -----------------------------------------------------------------

ROPE_SHAPES = [((1, 3, 1, 8), 3), ((2, 5, 3, 16), 9)]


def check_rope(label: str, out: torch.Tensor, x: torch.Tensor, cos: torch.Tensor,
               sin: torch.Tensor, backward: bool, stored: bool = True) -> Dict[str, float]:
    out, x, cos, sin = out.cpu(), x.cpu(), cos.cpu(), sin.cpu()
    u, _ = _store(out, stored)
    assert out.shape == x.shape
    want, mag = ref.rotate_ref64(x, cos, sin, backward)
    return {"rotation": _hold("rotation", label, (out.double() - want).abs(),
                              (u + 3 * E) * mag)}


# ---- SwiGLU -------------------------------------------------------------------

GLU_EVERY_GATE = (249, 264)  # rows, f of the packed every_gate case


def every_gate(n: int = 65536) -> torch.Tensor:
    """All 65,536 bf16 bit patterns, cycled to n elements."""
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    return bits.view(BF16)[torch.arange(n) % 65536]


def clamped_randn(n: int, seed: int) -> torch.Tensor:
    """bf16 randn with 2^-4 <= |.| <= 1, signs kept: no product with a finite
    gate overflows and none is zero."""
    t = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    return (torch.where(t < 0, -1.0, 1.0) * t.abs().clamp(2.0 ** -4, 1.0)).to(BF16)


def swiglu_inputs(family: str, n: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(a, b, dy) flat on the CPU, bf16."""
    if family == "every_gate":
        return every_gate(n), clamped_randn(n, 101), clamped_randn(n, 102)
    assert family == "randn"
    gen = torch.Generator().manual_seed(200 + n)
    return tuple(torch.randn(n, generator=gen).to(BF16) for _ in range(3))


def pack_glu(a: torch.Tensor, b: torch.Tensor, rows: int, f: int) -> torch.Tensor:
    return torch.cat([a.view(rows, f), b.view(rows, f)], dim=-1).contiguous()


def check_swiglu_fwd(label: str, o: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
                     stored: bool = True) -> Dict[str, float]:
    o, a, b = o.cpu(), a.cpu(), b.cpu()
    u, step = _store(o, stored)
    assert o.shape == a.shape
    check_class("o", label, o, ref.swiglu_fwd_emulated(a, b))
    fin = torch.isfinite(a)
    want = ref.swiglu_fwd_ref64(a, b)[fin]
    ad, bd = a.double()[fin], b.double()[fin]
    bound = ((u + (C_SWIGLU + ad.abs()) * E) * want.abs()
             + NORMAL_FLOOR * (ad * bd).abs() + step)
    return {"o": _hold("o", label, (o.double()[fin] - want).abs(), bound)}


def check_swiglu_bwd(label: str, da: torch.Tensor, db: torch.Tensor, dy: torch.Tensor,
                     a: torch.Tensor, b: torch.Tensor, stored: bool = True) -> Dict[str, float]:
    da, db, dy, a, b = (t.cpu() for t in (da, db, dy, a, b))
    u, step = _store(da, stored)
    assert db.dtype == da.dtype and da.shape == a.shape == db.shape
    emu_da, emu_db = ref.swiglu_bwd_emulated(dy, a, b)
    check_class("da", label, da, emu_da)
    check_class("db", label, db, emu_db)
    fin = torch.isfinite(a)
    r = ref.swiglu_bwd_ref64(dy, a, b)
    dyd, ad, bd = dy.double()[fin], a.double()[fin], b.double()[fin]
    units = ad.abs() * E
    bound_da = (u * r.da[fin].abs() + (C_SWIGLU_DA * E + units) * r.mag_da[fin]
                + NORMAL_FLOOR * (dyd * bd).abs() * (1 + ad.abs()) + step)
    bound_db = ((u + C_SWIGLU * E + units) * r.db[fin].abs()
                + NORMAL_FLOOR * (dyd * ad).abs() + step)
    return {"da": _hold("da", label, (da.double()[fin] - r.da[fin]).abs(), bound_da),
            "db": _hold("db", label, (db.double()[fin] - r.db[fin]).abs(), bound_db)}


def check_swiglu_glu_bwd(label: str, dgu: torch.Tensor, dy: torch.Tensor,
                         gu: torch.Tensor, stored: bool = True) -> Dict[str, float]:
    f = gu.shape[-1] // 2
    assert dgu.shape == gu.shape
    return check_swiglu_bwd(label, dgu[..., :f].contiguous(), dgu[..., f:].contiguous(), dy,
                            gu[..., :f].contiguous(), gu[..., f:].contiguous(), stored)


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Equal bit patterns, NaN payloads included."""
    view = torch.int16 if got.element_size() == 2 else torch.int32
    return (got.shape == want.shape and got.dtype == want.dtype
            and torch.equal(got.contiguous().view(view), want.contiguous().view(view)))
