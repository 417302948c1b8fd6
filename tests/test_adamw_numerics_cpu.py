"""CPU tests of the AdamW yardstick and checker (torchft_amd/ops/adamw_ref.py,
tests/adamw_check.py) that tests/test_adamw_numerics_gpu.py holds the kernel
to: the fp64 definition is torch's, a correct fp32 chain passes every
criterion, and each mistake worth catching is refused on the family built to
show it."""

import pytest
import torch

from adamw_check import (FAMILIES, INJECTIONS, STEPS, Case, adamw_chain32, clip_coef32,
                         family_tensors)
from torchft_amd.ops.adamw_ref import adamw_ref64, clip_coef64

N = 200_000


def test_ref64_is_torch_adamw_in_fp64():
    """Unrounded hyper-parameters: the reference chained over 5 steps equals
    torch.optim.AdamW on fp64 tensors to 1e-12 relative, over three param
    groups and a parameter whose grad is None on odd steps."""
    gen = torch.Generator().manual_seed(3)
    shapes = [(33,), (100, 7), (5,), (2049,)]
    groups_hp = [dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01),
                 dict(lr=0.1, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.5),
                 dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0)]
    owner = [0, 0, 1, 2]  # param -> group
    ps = [torch.randn(s, generator=gen, dtype=torch.float64).requires_grad_(True)
          for s in shapes]
    opt = torch.optim.AdamW(
        [dict(params=[p for p, o in zip(ps, owner) if o == gi], **hp)
         for gi, hp in enumerate(groups_hp)])
    mine = [dict(p=p.detach().clone(), m=torch.zeros_like(p), v=torch.zeros_like(p), step=0)
            for p in ps]
    for it in range(5):
        for i, p in enumerate(ps):
            if i == 1 and it % 2 == 1:
                p.grad = None
                continue
            p.grad = torch.randn(p.shape, generator=gen, dtype=torch.float64)
            st, hp = mine[i], groups_hp[owner[i]]
            st["step"] += 1
            r = adamw_ref64(st["p"], p.grad, st["m"], st["v"], lr=hp["lr"],
                            beta1=hp["betas"][0], beta2=hp["betas"][1], eps=hp["eps"],
                            weight_decay=hp["weight_decay"], step=st["step"],
                            round_hparams=False)
            st["p"], st["m"], st["v"] = r.p, r.m, r.v
        opt.step()
    assert mine[1]["step"] == 3 and mine[0]["step"] == 5
    for i, p in enumerate(ps):
        for got, want in ((mine[i]["p"], p.detach()),
                          (mine[i]["m"], opt.state[p]["exp_avg"]),
                          (mine[i]["v"], opt.state[p]["exp_avg_sq"])):
            assert ((got - want).abs() <= 1e-12 * want.abs()).all()


def test_rounded_hparams_are_what_the_kernel_receives():
    """1 - float(beta2) is far from 1 - beta2: the reason the reference
    rounds first."""
    b2 = 0.999
    b2f = float(torch.tensor(b2, dtype=torch.float32))
    rel = abs((1 - b2f) - (1 - b2)) / (1 - b2)
    assert 100 * 2.0 ** -24 < rel <= 2.0 ** -24 * b2 / (1 - b2)
    p, g = torch.ones(4, dtype=torch.bfloat16), torch.ones(4, dtype=torch.bfloat16)
    z = torch.zeros(4)
    kw = dict(lr=0.1, beta1=0.9, beta2=b2, eps=1e-8, weight_decay=0.0, step=1)
    a = adamw_ref64(p, g, z, z, **kw)
    b = adamw_ref64(p, g, z, z, round_hparams=False, **kw)
    assert a.one_minus_b2 == 1 - b2f and b.one_minus_b2 == 1 - b2
    assert ((a.v - b.v).abs() > 100 * 2.0 ** -24 * b.v).all()


def _run_chain(family, mode, inject=None, n=N):
    """STEPS steps of the fp32 chain on one n-element parameter, each checked
    as one step from the chain's own previous state. mode: None (plain), or
    the factor of the first step's norm that max_grad_norm is set to."""
    fam = FAMILIES[family]
    (p,), gs, (m,), (v,) = family_tensors(family, [(n,)])
    hp = dict(lr=fam["lr"], beta1=fam["b1"], beta2=fam["b2"], eps=fam["eps"],
              weight_decay=fam["wd"])
    max_norm = None if mode is None else mode * float(gs[0][0].double().norm())
    case = Case(f"fp32 chain, {family}, {'plain' if mode is None else f'clip x{mode}'}"
                + (f", {inject}" if inject else ""))
    for it in range(STEPS):
        g = gs[it][0]
        step = fam["step0"] + it + 1
        coef32 = coef64 = None
        if max_norm is not None:
            coef32 = clip_coef32([g], max_norm)
            coef64 = clip_coef64([g], max_norm)
            assert (coef64 < 1) == (mode < 1) and (float(coef32) < 1) == (mode < 1)
        ref = adamw_ref64(p, g, m, v, step=step, coef=1.0 if coef64 is None else coef64, **hp)
        p, m, v = adamw_chain32(p, g, m, v, step=step, coef=coef32, inject=inject, **hp)
        case.check(p, m, v, ref, clipped=coef64 is not None and coef64 < 1)
    case.finish()
    return case


@pytest.mark.parametrize("mode", [None, 0.5, 2.0])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_fp32_chain_is_inside_every_bound_and_cap(family, mode):
    _run_chain(family, mode)


# (mistake, family built to show it)
REFUSED_ON = [
    ("bc_swapped", "default"), ("bc_swapped", "smallp"), ("bc_swapped", "decay"),
    ("step_off_by_one", "default"), ("step_off_by_one", "smallp"),
    ("step_off_by_one", "decay"),
    ("eps_in_sqrt", "epsreg"),
    ("no_decay", "decay"),
    ("coupled_decay", "decay"),
    ("g_not_g2", "default"), ("g_not_g2", "smallp"),
]


def test_every_injection_has_a_family():
    assert {i for i, _ in REFUSED_ON} == set(INJECTIONS)


@pytest.mark.parametrize("inject,family", REFUSED_ON)
def test_injected_error_is_refused(inject, family):
    # at the GPU tests' size: the criteria must see it there
    with pytest.raises(AssertionError):
        _run_chain(family, None, inject=inject, n=14_411)
