"""The two criteria the attention kernels are held to, and the seeded input
families they are held to them on (docs/KERNELS.md, "Numerics" of
flash_attn_fwd.hip and flash_attn_bwd.hip). Shared by the CPU test of the
checker itself and by the GPU tests; plain torch, any device.

Hard bound   elementwise, derived: |got - ref64| <= factor * u * A with the
             denominators of ``attention_ref64``. Never exceeded by a correct
             kernel.
Sharp        relative to ``attention_emulated``: per (batch, head, 32 rows) the
             relative L2 error of the kernel is at most 3x the emulation's
             (lse: the maximum absolute error, at most 4x).
"""

from __future__ import annotations

import math
import os
import re

import torch

from torchft_amd.ops.attention_ref import E_FP32, U_BF16, delta_ref64

D = 128
SCALE0 = D ** -0.5


def _fwd_threshold() -> float:
    """kFwdThr as flash_attn_fwd.hip has it, in log2 units (11.54 = 8 nats):
    the ramp family is built around the kernel's own constant."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "csrc", "kernels", "flash_attn_fwd.hip")
    with open(src) as f:
        m = re.search(r"constexpr\s+float\s+kFwdThr\s*=\s*([0-9.]+)f\s*;", f.read())
    assert m is not None, "kFwdThr not found in flash_attn_fwd.hip"
    return float(m.group(1))


FWD_THR_LOG2 = _fwd_threshold()

# factor of u * A per output, and the denominator of attention_ref64 it goes
# with. Fed the reference's own lse / delta the backward inherits nothing from
# `out`: the P.E term leaves W (A_dq_ref / A_dk_ref) and the factor is 3.
HARD = {"out": (3.0, "A_out"), "dv": (3.0, "A_dv"),
        "dq": (5.0, "A_dq"), "dk": (5.0, "A_dk")}
HARD_REF_FED = {"dv": (3.0, "A_dv"), "dq": (3.0, "A_dq_ref"), "dk": (3.0, "A_dk_ref")}
# fa_delta_kernel: the bf16 x bf16 products are exact in fp32, one add in the
# lane, six __shfl_down levels
DELTA_DEPTH = 7
SHARP = 3.0
SHARP_LSE = 4.0
BLOCK = 32


# ---- input families ---------------------------------------------------------

def _randn(shape, gen, device):
    return torch.randn(shape, generator=gen, device=device, dtype=torch.float32)


def _views(t):
    """[B,S,H,D] storage seen as [B,H,S,D]: the model's layout."""
    return t.to(torch.bfloat16).contiguous().transpose(1, 2)


def needle_map(S: int, h: int) -> torch.Tensor:
    """pi(i) <= i that reaches every 32-key block at or below the diagonal
    from every 32-row block (while there are at most 32 of them), different
    for every head h."""
    i = torch.arange(S)
    r, t = i // BLOCK, i % BLOCK
    blk = (t + h) % (r + 1)
    off = (5 * t + 3 * h + 1) % BLOCK
    off = torch.where(blk == r, off % (t + 1), off)
    pi = blk * BLOCK + off
    assert bool((pi <= i).all())
    return pi


def ramp_nats(S: int, variant: str) -> tuple[torch.Tensor, torch.Tensor]:
    """(a_i, c_j): query i's score against key j is moved by a_i * c_j nats.
    c rises by a fixed amount per 32-key block over the first eight blocks and
    is flat after them, so that |a_i * c_j| <= 34.
      a  9.5 nats per block for every row: each of the first eight blocks
         exceeds the running maximum by more than the threshold.
      b  6.5 nats over the whole row: below the threshold, nothing rescales
         after the first block and P reaches e^6.5 and more.
      c  odd rows as a, even rows flat: the wave-wide vote fails because of
         some rows only."""
    blk = (torch.arange(S) // BLOCK).clamp(max=7).double()
    a = torch.ones(S, dtype=torch.float64)
    if variant == "b":
        c = 6.5 * blk / 7.0
    else:
        c = 9.5 * (blk - 3.5)
        if variant == "c":
            a[0::2] = 0.0
    return a, c


def make_inputs(family: str, B: int, Hq: int, Hkv: int, S: int, scale: float,
                device="cpu", seed: int = 7):
    """q, k, v, dout as bf16 [B,S,H,D]-backed views. Seeded on the CPU so that
    a case is the same tensor wherever it is built."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    q = _randn((B, S, Hq, D), gen, "cpu")
    k = _randn((B, S, Hkv, D), gen, "cpu")
    v = _randn((B, S, Hkv, D), gen, "cpu")
    dout = _randn((B, S, Hq, D), gen, "cpu")
    G = Hq // Hkv
    if family == "randn":
        pass
    elif family == "offset":
        v = v + 8.0
    elif family == "needle":
        # rows of norm^2 = 128, q_i = mult * k_pi(i): score 45 at the needle
        k = k * (math.sqrt(D) / k.norm(dim=-1, keepdim=True))
        mult = 4.0 * SCALE0 / scale
        for h in range(Hq):
            q[:, :, h] = mult * k[:, needle_map(S, h), h // G]
    elif family.startswith("ramp_"):
        a, c = ramp_nats(S, family[-1])
        w = torch.ones(D)
        w[1::2] = -1.0
        w[::3] *= -1.0
        w = w / w.norm()
        # noise of ~0.25 nats, with w projected out so the cross terms vanish
        q, k = 0.5 * q * math.sqrt(SCALE0 / scale), 0.5 * k * math.sqrt(SCALE0 / scale)
        q = q - (q @ w)[..., None] * w
        k = k - (k @ w)[..., None] * w
        unit = 1.0 / math.sqrt(scale)
        q = q + (a.float() * unit)[None, :, None, None] * w
        k = k + (c.float() * unit)[None, :, None, None] * w
    else:
        raise ValueError(family)
    return tuple(_views(t.to(device)) for t in (q, k, v, dout))


# document-mask layouts, B = 2 with different documents in the two rows
DOC_LAYOUTS = {
    # boundaries inside a wave, on a 32 edge, on a 64 edge, a document of one
    # token | rows 5-31 of wave 0 start a document inside its first block
    "mixed256": (256, ([1, 31, 32, 33, 63, 96], [5, 251])),
    "single256": (256, ([256], [1, 31, 32, 33, 63, 96])),
    # two workgroups: the second skips the first's keys | a boundary inside
    # the second workgroup
    "halves512": (512, ([256, 256], [300, 212])),
    "eighths512": (512, ([64] * 8, [300, 212])),
}


def doc_mask(name: str, device="cuda"):
    from torchft_amd.ops import DocMask

    S, rows = DOC_LAYOUTS[name]
    return DocMask.from_lengths(rows, S, device=device)


FAMILIES = ("randn", "offset", "needle", "ramp_a", "ramp_b", "ramp_c")
SHARP_FAMILIES = ("randn", "offset", "ramp_a", "ramp_b", "ramp_c")


# ---- the criteria -----------------------------------------------------------

def hard_ratio(got, ref, A, factor, unit=U_BF16) -> float:
    """max |got - ref| / (factor * unit * A): at most 1 for a correct kernel."""
    return ((got.double() - ref).abs() / (factor * unit * A)).max().item()


def lse_ratio(got, ref) -> float:
    bound = E_FP32 * (D * ref.Sqk + ref.n + 8.0 * (1.0 + ref.lse.abs()))
    return ((got.double() - ref.lse).abs() / bound).max().item()


def delta_ratio(got, dout, out) -> float:
    """fa_delta against fp64 of the SAME bf16 out."""
    want, A = delta_ref64(dout, out)
    return hard_ratio(got, want, A, DELTA_DEPTH, unit=E_FP32)


def block_rho(got, ref) -> torch.Tensor:
    """Relative L2 error per (batch, head, 32 consecutive rows)."""
    B, H, S, Dh = ref.shape
    err = (got.double() - ref).reshape(B, H, S // BLOCK, BLOCK * Dh)
    return err.norm(dim=-1) / ref.reshape(B, H, S // BLOCK, BLOCK * Dh).norm(dim=-1)


def block_maxerr(got, ref) -> torch.Tensor:
    B, H, S = ref.shape
    return (got.double() - ref).abs().reshape(B, H, S // BLOCK, BLOCK).amax(-1)


def sharp_ratio(got, emu, ref, lse: bool = False) -> float:
    """max over blocks of (kernel's error) / (emulation's error): at most
    SHARP (SHARP_LSE for lse). A block the emulation gets exactly right must
    be exactly right."""
    f = block_maxerr if lse else block_rho
    rk, re = f(got, ref), f(emu, ref)
    ratio = torch.where(rk == 0, torch.zeros_like(rk), rk / re)  # x / 0 = inf
    return ratio.max().item()


class Report:
    """Collects the worst ratio of every comparison, prints each, and fails at
    the end with all of them so that one run shows the whole picture."""

    def __init__(self, what: str):
        self.what = what
        self.rows: list[tuple[str, float, float]] = []

    def add(self, name: str, ratio: float, limit: float) -> None:
        self.rows.append((name, ratio, limit))
        print(f"{self.what}: {name} {ratio:.3f} (limit {limit:g})")

    def failures(self) -> list[str]:
        return [f"{n}: {r:.3f} > {lim:g}" for n, r, lim in self.rows
                if not r <= lim]

    def check(self) -> None:
        bad = self.failures()
        assert not bad, f"{self.what}: " + "; ".join(bad)


def check_hard(rep: Report, got: dict, ref, factors=HARD) -> None:
    """got: name -> tensor, each name `lse` or a key of `factors`."""
    for n, t in got.items():
        assert torch.isfinite(t).all(), f"{rep.what}: non-finite {n}"
        if n == "lse":
            rep.add("hard lse", lse_ratio(t, ref), 1.0)
            continue
        assert n in factors, f"{rep.what}: no hard bound for {n!r}"
        factor, denom = factors[n]
        rep.add(f"hard {n}", hard_ratio(t, getattr(ref, n), getattr(ref, denom), factor), 1.0)


def check_sharp(rep: Report, got: dict, emu, ref) -> None:
    for n, t in got.items():
        if n == "lse":
            rep.add("sharp lse", sharp_ratio(t, emu.lse, ref.lse, lse=True), SHARP_LSE)
        else:
            assert n in ("out", "dq", "dk", "dv"), f"{rep.what}: no sharp criterion for {n!r}"
            rep.add(f"sharp {n}", sharp_ratio(t, getattr(emu, n), getattr(ref, n)), SHARP)
