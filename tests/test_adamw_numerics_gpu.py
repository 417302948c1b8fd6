"""``adamw_kernel`` (csrc/kernels/fused_adamw.hip), plain and clip mode, against
the fp64 definition under the derived bounds of tests/adamw_check.py
(docs/KERNELS.md, "Numerics" of fused_adamw.hip): ``exp_avg``, ``exp_avg_sq``
and the parameter after every step, each step checked as one step from the
kernel's own previous state so that the bounds do not compound.

Every case runs one FusedAdamW over the eight shapes (a partial vector, one
vector, a block boundary from both sides, several blocks) in two param groups
with different lr / weight decay / beta1, and two parameters whose grad is None
on the middle step: the plain mode then buckets by step count and the clip
mode reads per-tensor device step counts that differ."""

import pytest
import torch

from adamw_check import FAMILIES, SHAPES, STEPS, Case, family_tensors
from torchft_amd import ops
from torchft_amd.ops.adamw_ref import adamw_ref64, clip_coef64

pytestmark = pytest.mark.gpu

NO_GRAD_ON_ODD_STEPS = (2, 5)  # indices into SHAPES: (8,) and (2049,)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked test without a HIP device"
    assert ops.have_hip_ext(), "HIP kernel extension must be loadable on a GPU box"
    return torch.device("cuda:0")


def _group_hp(fam, gi):
    """Group 0 has the family's hyper-parameters, group 1 twice the lr and
    weight decay and another beta1."""
    if gi == 0:
        return dict(lr=fam["lr"], betas=(fam["b1"], fam["b2"]), eps=fam["eps"],
                    weight_decay=fam["wd"])
    return dict(lr=2 * fam["lr"], betas=(0.8, fam["b2"]), eps=fam["eps"],
                weight_decay=2 * fam["wd"])


# None: plain mode; else max_grad_norm as a factor of the first step's norm
MODES = {"plain": None, "clip_below": 0.5, "clip_above": 2.0}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_step_against_fp64(dev, family, mode):
    fam = FAMILIES[family]
    p0, gs, m0, v0 = family_tensors(family, SHAPES)
    params = [t.to(dev).requires_grad_(True) for t in p0]
    owner = [i % 2 for i in range(len(SHAPES))]
    groups = [dict(params=[p for p, o in zip(params, owner) if o == gi], **_group_hp(fam, gi))
              for gi in (0, 1)]
    factor = MODES[mode]
    max_norm = None
    if factor is not None:
        max_norm = factor * clip_coef_norm([g for g in gs[0]])
    opt = ops.FusedAdamW(groups, max_grad_norm=max_norm)
    steps_taken = [fam["step0"]] * len(params)
    if fam["step0"]:
        for p, m, v in zip(params, m0, v0):
            step = (torch.tensor(fam["step0"], dtype=torch.int32, device=dev)
                    if max_norm is not None else fam["step0"])
            opt.state[p] = {"step": step, "exp_avg": m.to(dev), "exp_avg_sq": v.to(dev)}

    case = Case(f"{family}, {mode}")
    for it in range(STEPS):
        live = [i for i in range(len(params))
                if not (it % 2 == 1 and i in NO_GRAD_ON_ODD_STEPS)]
        before = []
        for i, p in enumerate(params):
            st = opt.state.get(p, {})
            before.append((p.detach().cpu().clone(),
                           st["exp_avg"].cpu().clone() if st else torch.zeros(SHAPES[i]),
                           st["exp_avg_sq"].cpu().clone() if st else torch.zeros(SHAPES[i])))
            p.grad = gs[it][i].to(dev) if i in live else None
        coef = 1.0
        if max_norm is not None:
            coef = clip_coef64([gs[it][i] for i in live], max_norm)
            assert (coef < 1.0) == (factor < 1.0)
        opt.step()
        torch.cuda.synchronize()
        for i, p in enumerate(params):
            bp, bm, bv = before[i]
            st = opt.state.get(p, {})
            if i not in live:
                assert torch.equal(p.detach().cpu(), bp), "parameter without grad moved"
                if st:
                    assert torch.equal(st["exp_avg"].cpu(), bm)
                    assert torch.equal(st["exp_avg_sq"].cpu(), bv)
                    assert int(st["step"]) == steps_taken[i]
                continue
            steps_taken[i] += 1
            assert int(st["step"]) == steps_taken[i]
            hp = _group_hp(fam, owner[i])
            ref = adamw_ref64(bp, gs[it][i], bm, bv, lr=hp["lr"], beta1=hp["betas"][0],
                              beta2=hp["betas"][1], eps=hp["eps"],
                              weight_decay=hp["weight_decay"], step=steps_taken[i], coef=coef)
            case.check(p.detach(), st["exp_avg"], st["exp_avg_sq"], ref, clipped=coef < 1.0)
    assert steps_taken[NO_GRAD_ON_ODD_STEPS[0]] == fam["step0"] + 2
    assert steps_taken[0] == fam["step0"] + 3
    if max_norm is not None:
        assert int(opt.skipped_steps) == 0
    case.finish()


def clip_coef_norm(grads) -> float:
    """fp64 global norm of the stored gradients."""
    return sum(float(g.double().pow(2).sum()) for g in grads) ** 0.5
