"""The criteria ``adamw_kernel`` is held to, the seeded input families it is
held to them on, and an fp32 evaluation of its rounding chain with switchable
mistakes (docs/KERNELS.md, "Numerics" of fused_adamw.hip). Shared by the CPU
test of the checker itself and by the GPU tests; plain torch on the CPU.

Every bound is a count of fp32 roundings times ``u = 2^-24`` times the sum of
the absolute values of the terms entering the output (``adamw_ref64`` returns
the sums), each rounding being at most ``u`` times a value that never exceeds
that sum:

``m' = b1*m + (1-b1)*g``   ``1 - float(b1)`` is exact (Sterbenz, b in [0.5, 1]);
    each term is rounded as a product and again in the sum; counted as two
    products and a sum: ``3 u S_m``, ``S_m = b1|m| + (1-b1)|g|``.
``v' = b2*v + ((1-b2)*g)*g``   the g term is rounded in two products and in the
    sum, the v term in one product and the sum, all terms non-negative, so the
    error is relative to ``v'`` itself; counted as three products and a sum:
    ``4 u v'``.
clip mode, coefficient below 1   the gradient is ``g*coef`` with ``coef =
    max_norm / (norm + 1e-6)``: the norm is within ``depth`` units (grad_norm.hip:
    8 adds in the lane, 6 shuffle steps, 3 wave adds = 17 while every workgroup
    visits one block; that bound already covers ``sqrtf``), then the sum with
    1e-6, the division and the product ``g*coef``: ``CLIP_UNITS = depth + 3 = 20``
    on ``(1-b1)|g|`` in ``m'`` and twice that on ``(1-b2)g^2`` in ``v'``. A
    coefficient of exactly 1 adds nothing.
``p' = p - lr*(m_hat/(sqrt(v_hat) + eps) + wd*p)``, ``S_p = |p| + lr*(T_q +
    wd|p|)``, ``T_q`` the quotient with ``S_m`` in place of ``|m'|``. Along the
    quotient's chain: ``m'`` 3; ``bc1 = 1 - b1^s`` one rounding plus ``A1 =
    b1^s/(1-b1^s)`` times ``powf``'s error of ``E_POW`` units; ``m'/bc1`` 1;
    ``v'`` 4, ``bc2`` ``1 + A2*E_POW``, ``v'/bc2`` 1, all halved by the root,
    which then rounds once: ``4 + A2*E_POW/2``; the sum with ``eps`` 1; the
    division 1; then ``+ wd*p``, ``lr*``, ``p -`` one each: 14. The ``wd*p``
    chain has 4 and ``p`` itself 1, so ``k = 14 + E_POW*(A1 + A2/2)``, plus
    ``2*CLIP_UNITS`` in clip mode (once through ``m'``, twice and halved through
    ``v'``).

The stored parameter is bf16: ``|p_kernel - p'| <= 2^-8 |p'| + k u S_p``, and in
addition it may differ from ``bf16(p')`` in at most 0.1 % of the parameters of
a case and never by more than one bf16 ulp. The fp32 errors above are far
below the bf16 step, so only a rounding tie broken the other way may differ.
The one-ulp rule presumes that: it is applied where ``k u S_p <= 2^-9 |p'|``,
half the smallest bf16 step at ``p'``. Where ``p`` and the update cancel below
that (a few parameters per million at ``lr = 0.1``, ``wd = 0.5``) a correct
fp32 chain already lands several bf16 steps from ``bf16(p')``; such a parameter
stays under the absolute bound and counts towards the 0.1 %.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from grad_norm_check import coef_from_sumsq32
from torchft_amd.ops.adamw_ref import AdamWRef

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
M_UNITS = 3
V_UNITS = 4
P_UNITS = 14
E_POW = 1  # powf, host (libm) and device (HIP's documented accuracy): 1 ulp
NORM_DEPTH = 17
CLIP_UNITS = NORM_DEPTH + 3
FLIP_CAP = 1e-3

SHAPES = [(1,), (7,), (8,), (2047,), (2048,), (2049,), (5000,), (100, 33)]
STEPS = 3

# p scale, g scale, lr, beta1, beta2, eps, weight decay, step count preset
FAMILIES: Dict[str, dict] = {
    "default": dict(p=1.0, g=1.0, lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.01, step0=0),
    # the update dominates p', so the bf16 store resolves it
    "smallp": dict(p=1e-3, g=1.0, lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.01, step0=0),
    # sqrt(v_hat) ~ eps
    "epsreg": dict(p=1e-3, g=1e-8, lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.0, step0=0),
    "decay": dict(p=1.0, g=1.0, lr=0.1, b1=0.9, b2=0.999, eps=1e-8, wd=0.5, step0=0),
    # powf far from its trivial arguments, bc far from both 0 and 1
    "latestep": dict(p=1.0, g=1.0, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, step0=1000),
}


def family_tensors(name: str, shapes: Sequence[Tuple[int, ...]], seed: int = 0):
    """(p, [g of step 0, 1, ...], m, v) on the CPU: p and g bf16, m and v fp32.
    m and v are zeros except where the family presets a step count, where
    they are what a run would have left (m ~ 0.1 g, v ~ g^2 / 4)."""
    fam = FAMILIES[name]
    gen = torch.Generator().manual_seed(1000 + 17 * sorted(FAMILIES).index(name) + seed)
    p = [(fam["p"] * torch.randn(s, generator=gen)).to(torch.bfloat16) for s in shapes]
    gs = [[(fam["g"] * torch.randn(s, generator=gen)).to(torch.bfloat16) for s in shapes]
          for _ in range(STEPS)]
    if fam["step0"]:
        m = [0.1 * fam["g"] * torch.randn(s, generator=gen) for s in shapes]
        v = [(0.5 * fam["g"] * torch.randn(s, generator=gen)) ** 2 for s in shapes]
    else:
        m = [torch.zeros(s) for s in shapes]
        v = [torch.zeros(s) for s in shapes]
    return p, gs, m, v


def ordered(t: torch.Tensor) -> torch.Tensor:
    """bf16 bit patterns as integers ordered like the values (+0 == -0)."""
    i = t.view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


class Case:
    """Holds every tensor of one case (family x mode, all steps) to the
    bounds, then the case to the cap on differing bf16 parameters."""

    def __init__(self, label: str) -> None:
        self.label = label
        self.worst = {"m": 0.0, "v": 0.0, "p": 0.0}
        self.differing = 0
        self.total = 0
        self.unresolved = 0

    def _hold(self, name: str, err: torch.Tensor, bound: torch.Tensor) -> None:
        # a NaN error or a zero bound with a non-zero error must fail
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
        worst = float(ratio.max()) if ratio.numel() else 0.0
        bad = ~(err <= bound)
        if not bad.any() and worst == worst:
            self.worst[name] = max(self.worst[name], worst)
        assert not bad.any(), (
            f"{self.label}: {name}' outside its bound in {int(bad.sum())} of "
            f"{err.numel()} elements, worst error / bound {worst:.3g}")

    def check(self, got_p: torch.Tensor, got_m: torch.Tensor, got_v: torch.Tensor,
              ref: AdamWRef, clipped: bool = False) -> None:
        """``clipped``: the clip mode ran with a coefficient below 1."""
        got_p, got_m, got_v = got_p.cpu(), got_m.cpu(), got_v.cpu()
        assert got_p.dtype == torch.bfloat16 and got_m.dtype == torch.float32
        cu = CLIP_UNITS if clipped else 0
        g_m = ref.one_minus_b1 * ref.g.abs()  # the gradient's share of S_m
        g_v = ref.one_minus_b2 * ref.g * ref.g  # and of v'
        self._hold("m", (got_m.double() - ref.m).abs(),
                   M_UNITS * U32 * ref.s_m + cu * U32 * g_m)
        self._hold("v", (got_v.double() - ref.v).abs(),
                   V_UNITS * U32 * ref.v + 2 * cu * U32 * g_v)
        k = P_UNITS + E_POW * (ref.a1 + ref.a2 / 2) + 2 * cu
        self._hold("p", (got_p.double() - ref.p).abs(),
                   U_BF16 * ref.p.abs() + k * U32 * ref.s_p)
        want = ref.p.to(torch.bfloat16)
        steps = (ordered(got_p) - ordered(want)).abs()
        # where p' cancels to less than 2^9 times the fp32 budget, that budget
        # alone spans bf16 steps of p': such a parameter is held to the bound
        # above and counts as differing, but not to the one-ulp rule
        resolved = k * U32 * ref.s_p <= (U_BF16 / 2) * ref.p.abs()
        far = (steps > 1) & resolved
        assert not far.any(), (
            f"{self.label}: {int(far.sum())} parameters more than one bf16 "
            "ulp from the rounded fp64 value")
        self.unresolved += int((~resolved).sum())
        self.differing += int((steps != 0).sum())
        self.total += got_p.numel()

    def finish(self) -> None:
        frac = self.differing / max(self.total, 1)
        print(f"{self.label}: worst error / bound m' {self.worst['m']:.3f}, "
              f"v' {self.worst['v']:.3f}, p' {self.worst['p']:.3f}; "
              f"{self.differing} of {self.total} parameters ({100 * frac:.3f} %) "
              f"differ from the rounded fp64 value, {self.unresolved} below the "
              "one-ulp rule's reach")
        assert self.differing <= FLIP_CAP * self.total, (
            f"{self.label}: {self.differing} of {self.total} parameters differ from "
            "the rounded fp64 value, more than 0.1 %")


# ---- the kernel's chain in fp32 torch, with switchable mistakes ---------------

INJECTIONS = ("bc_swapped", "step_off_by_one", "eps_in_sqrt", "no_decay",
              "coupled_decay", "g_not_g2")


def _t32(x: float) -> torch.Tensor:
    return torch.tensor(x, dtype=torch.float32)


def adamw_chain32(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, *,
                  lr: float, beta1: float, beta2: float, eps: float, weight_decay: float,
                  step: int, coef: Optional[torch.Tensor] = None,
                  inject: Optional[str] = None):
    """One step as the kernel writes it, every operation a separate fp32
    torch op on the CPU (no fma). Returns (p' bf16, m', v')."""
    assert inject is None or inject in INJECTIONS
    lr32, b1, b2, eps32, wd = (_t32(x) for x in (lr, beta1, beta2, eps, weight_decay))
    s = _t32(float(step + (1 if inject == "step_off_by_one" else 0)))
    bc1 = 1.0 - torch.pow(b1, s)
    bc2 = 1.0 - torch.pow(b2, s)
    if inject == "bc_swapped":
        bc1, bc2 = bc2, bc1
    pf, gf = p.float(), g.float()
    if coef is not None:
        gf = gf * coef
    if inject == "coupled_decay":
        gf = gf + wd * pf
    m2 = b1 * m + (1.0 - b1) * gf
    v2 = b2 * v + ((1.0 - b2) * gf if inject == "g_not_g2" else (1.0 - b2) * gf * gf)
    mhat, vhat = m2 / bc1, v2 / bc2
    denom = torch.sqrt(vhat + eps32) if inject == "eps_in_sqrt" else torch.sqrt(vhat) + eps32
    upd = mhat / denom
    if inject not in ("no_decay", "coupled_decay"):
        upd = upd + wd * pf
    return (pf - lr32 * upd).to(torch.bfloat16), m2, v2


def clip_coef32(grads: List[torch.Tensor], max_norm: float) -> torch.Tensor:
    """The clip coefficient as fp32 torch computes it."""
    sumsq = torch.zeros((), dtype=torch.float32)
    for g in grads:
        sumsq = sumsq + g.float().pow(2).sum()
    return coef_from_sumsq32(sumsq, max_norm)
