"""``adamw_kernel``'s ``stochastic`` and ``master`` modes (docs/KERNELS.md, "Rounding
modes"): the exact step of tests/test_adamw_rounding_cpu.py bit for bit, the
families of tests/adamw_check.py under its ``k u S_p``, and the stall they cure."""
import copy

import pytest
import torch

from adamw_check import (CLIP_UNITS, E_POW, FAMILIES, P_UNITS, SHAPES, STEPS, U32, Case,
                         family_tensors)
from test_adamw_numerics_gpu import MODES, dev  # noqa: F401  (the fixture)
from test_adamw_rounding_cpu import exact_steps
from torchft_amd import ops
from torchft_amd.ops.adamw_ref import adamw_ref64, clip_coef64

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [0, 0x1234_5678_9ABC_DEF0])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("rounding", ["stochastic", "master"])
def test_exact_step(dev, rounding, clip, seed):
    exact_steps(dev, rounding, clip, seed)


def bf16_floor(x: torch.Tensor) -> torch.Tensor:
    """The largest bf16 value (8 significant bits; subnormals) not above fp64 x."""
    _, e = torch.frexp(x)
    q = torch.ldexp(torch.ones_like(x), e.clamp(min=-125) - 8)
    return torch.floor(x / q) * q


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("family", ["decay", "default", "smallp"])
@pytest.mark.parametrize("rounding", ["stochastic", "master"])
def test_every_step_against_fp64(dev, rounding, family, mode):
    """Each step is one step from the kernel's own previous state. In master
    mode the odd elements of every ``p`` are doubled before the second step:
    those start from ``float(p)``, the others from ``master``. The last step is
    also taken by a fresh optimizer loaded from ``state_dict()``."""
    fam = FAMILIES[family]
    hp = dict(lr=fam["lr"], betas=(fam["b1"], fam["b2"]), eps=fam["eps"],
              weight_decay=fam["wd"])
    p0, gs, _, _ = family_tensors(family, SHAPES)
    params = [t.to(dev).requires_grad_(True) for t in p0]
    norm0 = sum(float(g.double().pow(2).sum()) for g in gs[0]) ** 0.5
    extra = dict(max_grad_norm=MODES[mode] and MODES[mode] * norm0, rounding=rounding,
                 sr_seed=7)
    opt = ops.FusedAdamW(params, **hp, **extra)
    case = Case(f"{rounding}, {family}, {mode}")
    for it in range(STEPS):
        start = []
        for p, g in zip(params, gs[it]):
            st = opt.state.get(p, {})
            if "master" in st and it == 1:
                p.detach().view(-1)[1::2].mul_(2)
            s = p.detach().cpu().float()
            if "master" in st:
                odd = torch.zeros(s.numel(), dtype=torch.bool)
                odd[1::2] = it == 1
                s = torch.where(odd.view_as(s), s, st["master"].cpu())
            start.append((s, *(st[key].cpu().clone() if st else torch.zeros_like(s)
                               for key in ("exp_avg", "exp_avg_sq"))))
            p.grad = g.to(dev)
        coef = clip_coef64(gs[it], extra["max_grad_norm"]) if MODES[mode] else 1.0
        if it == STEPS - 1:
            twins = [p.detach().clone().requires_grad_(True) for p in params]
            twin_opt = ops.FusedAdamW(twins, **hp, **extra)
            twin_opt.load_state_dict(copy.deepcopy(opt.state_dict()))
            for t, p in zip(twins, params):
                t.grad = p.grad.clone()
            twin_opt.step()
        opt.step()
        for i, p in enumerate(params):
            st, got = opt.state[p], p.detach().cpu()
            s, m, v = start[i]
            ref = adamw_ref64(s, gs[it][i], m, v, lr=hp["lr"], beta1=fam["b1"],
                              beta2=fam["b2"], eps=hp["eps"], weight_decay=fam["wd"],
                              step=it + 1, coef=coef)
            # m' and v' under the checker's bounds; its rules for a nearest p do
            # not apply, so it is shown the reference's own rounding
            case.check(ref.p.to(torch.bfloat16), st["exp_avg"], st["exp_avg_sq"], ref,
                       clipped=coef < 1.0)
            k = P_UNITS + E_POW * (ref.a1 + ref.a2 / 2) + (2 * CLIP_UNITS if coef < 1.0 else 0)
            bound = k * U32 * ref.s_p
            if rounding == "master":
                assert ((st["master"].cpu().double() - ref.p).abs() <= bound).all()
                assert torch.equal(got, st["master"].cpu().to(torch.bfloat16))
            else:
                assert (got.double() >= bf16_floor(ref.p - bound)).all()
                assert (got.double() <= -bf16_floor(-(ref.p + bound))).all()
            if it == STEPS - 1:
                assert torch.equal(got, twins[i].detach().cpu())
                for key in set(st) - {"step"}:
                    assert torch.equal(st[key], twin_opt.state[twins[i]][key])


@pytest.mark.parametrize("rounding", ["nearest", "stochastic", "master"])
def test_small_updates_act(dev, rounding):
    """p = 1.0, ``g = 0``, ``lr * wd = 2^-12``, 16 steps: the fp64 value is ``(1 -
    2^-12)^16``, 1.0 * 2^-8 below 1. ``nearest`` drops every update. ``master``
    follows in fp32: ``m' = 0`` makes the quotient exactly 0, so ``k = 14`` a step.
    ``stochastic`` follows in the mean (unbiased rounding, linear step): per step
    and element the variance is ``(2^-8)^2 f (1 - f)``, ``f = 1/16`` (below 1.0 the
    bf16 step is 2^-9 and ``f = 1/8``: less), so over 16 steps and 65536 elements
    ``sigma_mean = 2^-8 sqrt(16 * 15/256 / 65536) = 0.0038 * 2^-8``."""
    p = torch.ones(65536, dtype=torch.bfloat16, device=dev, requires_grad=True)
    opt = ops.FusedAdamW([p], lr=2.0 ** -6, weight_decay=2.0 ** -6, rounding=rounding)
    for _ in range(16):
        p.grad = torch.zeros_like(p)
        opt.step()
    want, got = (1 - 2.0 ** -12) ** 16, p.detach().cpu()
    if rounding == "nearest":
        assert (got == 1.0).all()
    elif rounding == "master":
        master = opt.state[p]["master"].cpu()
        assert ((master.double() - want).abs() <= 16 * P_UNITS * U32).all()
        assert torch.equal(got, master.to(torch.bfloat16)) and (got == 1 - 2.0 ** -8).all()
    else:
        sigma = 2.0 ** -8 * (16 * (15 / 256) / 65536) ** 0.5
        assert abs(float(got.double().mean()) - want) <= 6 * sigma
