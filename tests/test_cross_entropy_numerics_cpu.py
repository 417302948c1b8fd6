"""CPU tests of the cross-entropy checker (tests/ce_check.py) that
tests/test_cross_entropy_numerics_gpu.py holds the kernel to: a correct fp32
chain is inside every bound on every family and, ahead of the bf16 store,
under two thirds of the fp32 part ``F``; each mistake worth catching is refused
by the criterion meant to see it; the sentinel buffer sees a stray write. That
``cross_entropy_ref`` is torch's cross-entropy on randn is
tests/test_cross_entropy_cpu.py's business; here only the rows the families
add to it, against fp64 autograd."""

import math

import pytest
import torch

import ce_check
from ce_check import (FAMILIES, GS_GRID, IGNORE, INJECTIONS, Z_GRID, ce_chain32, check, family,
                      make_case)
from torchft_amd.ops.cross_entropy import cross_entropy_ref

SMALL_V = (4, 7, 8, 9, 15, 16, 22, 23)


@pytest.mark.parametrize("gs", GS_GRID)
@pytest.mark.parametrize("z", Z_GRID)
@pytest.mark.parametrize("name", FAMILIES)
def test_fp32_chain_is_inside_every_bound(name, z, gs):
    x, t = family(name)
    loss, g = ce_chain32(x, t, z, gs)
    check(x, t, loss, g, z, gs, tag=f"fp32 chain, {name}")
    # ahead of the store: the two thirds that F's margin rests on
    loss, g32 = ce_chain32(x, t, z, gs, store=False)
    check(x, t, loss, g32, z, gs, tag=f"fp32 chain unrounded, {name}", F_share=2 / 3)


@pytest.mark.parametrize("V", SMALL_V + (8207,))
def test_fp32_chain_at_the_gpu_tests_other_widths(V):
    for name in ("randn4", "needle", "neg_inf"):
        x, t = family(name, V=V)
        loss, g = ce_chain32(x, t, 1e-4, 1 / 29)
        check(x, t, loss, g, 1e-4, 1 / 29, tag=f"fp32 chain, {name}")


# (mistake, family, z, gs, V, the criterion that refuses it)
REFUSED = [
    ("z_dropped", "randn4", 1e-4, 1.0, 1003, "gradient bound"),
    ("z_dropped", "randn4", 1e-4, 1 / 29, 9, "gradient bound"),
    ("z_dropped", "randn3000", 1e-2, 1.0, 1003, "gradient bound"),
    ("z_halved", "randn4", 1e-4, 1.0, 1003, "gradient bound"),
    ("z_halved", "flat", 1e-2, 1.0, 1003, "gradient bound"),
    ("truncating_store", "randn4", 1e-4, 1.0, 1003, "gradient bound"),
    ("truncating_store", "randn4", 0.0, 1 / 29, 22, "gradient bound"),
    ("tail_out_of_sum", "flat", 1e-4, 1.0, 1003, "loss bound"),
    ("tail_out_of_sum", "randn4", 1e-4, 1.0, 9, "gradient bound"),
    ("head_out_of_sum", "flat", 1e-4, 1.0, 1003, "loss bound"),
    ("head_out_of_sum", "randn4", 1e-4, 1.0, 9, "gradient bound"),
    ("onehot_unscaled", "randn4", 1e-4, 1 / 29, 1003, "gradient bound"),
    ("onehot_unscaled", "needle", 1e-4, 2.0 ** -20, 1003, "gradient bound"),
    ("onehot_shifted", "randn4", 1e-4, 1.0, 1003, "gradient bound"),
    ("onehot_shifted", "needle", 1e-4, 1.0, 22, "gradient bound"),
    ("bf16_x_minus_lse", "randn4", 1e-4, 1.0, 1003, "gradient bound"),
    ("ignored_not_zeroed", "randn4", 1e-4, 1.0, 1003, "ignored row"),
    ("ignored_not_zeroed", "neg_inf", 1e-4, 1.0, 1003, "ignored row"),
    ("loss_without_z", "randn4", 1e-4, 1.0, 1003, "loss bound"),
    ("loss_without_z", "randn3000", 1e-2, 1.0, 1003, "loss bound"),
]


def test_every_injection_is_tried():
    assert {r[0] for r in REFUSED} == set(INJECTIONS)


@pytest.mark.parametrize("inject,name,z,gs,V,criterion", REFUSED)
def test_injected_mistake_is_refused(inject, name, z, gs, V, criterion):
    x, t = family(name, V=V)
    loss, g = ce_chain32(x, t, z, gs, inject=inject)
    # the named criterion alone must refuse it: the other output is a correct one
    good_loss, good_g = ce_chain32(x, t, z, gs)
    if criterion == "loss bound":
        g = good_g
    else:
        loss = good_loss
    with pytest.raises(AssertionError, match=criterion):
        check(x, t, loss, g, z, gs, tag=inject)


def test_old_gradient_bound_passes_what_the_new_one_refuses():
    """The reason for the 2^-8 term: under 2^-7 |g_ref| + 1e-6 gs a kernel
    without the z factor, or one that truncates, passes at z = 1e-4."""
    x, t = family("randn4")
    _, ref = cross_entropy_ref(x.double(), t, IGNORE, 1e-4, 1.0)
    for inject in ("z_dropped", "truncating_store"):
        _, g = ce_chain32(x, t, 1e-4, 1.0, inject=inject)
        old = ((g.double() - ref).abs() / (2.0 ** -7 * ref.abs() + 1e-6)).max()
        assert float(old) <= 1.0, inject


def test_class_rules_refuse_a_lost_nan_and_a_finite_inf():
    x, t = family("nonfinite")
    loss, g = ce_chain32(x, t, 1e-4, 1.0)
    # a kernel whose sum never saw the NaN: the row comes out finite
    clean = x.clone()
    clean[0, x.shape[1] // 2] = 0.0
    loss2, g2 = ce_chain32(clean, t, 1e-4, 1.0)
    bad_loss = loss.clone()
    bad_loss[0] = loss2[0]
    with pytest.raises(AssertionError, match="class"):
        check(x, t, bad_loss, g, 1e-4, 1.0, tag="lost NaN")
    bad_g = g.clone()
    bad_g[0] = g2[0]
    with pytest.raises(AssertionError, match="class"):
        check(x, t, loss, bad_g, 1e-4, 1.0, tag="lost NaN")
    # a target on a -inf logit must be +inf, not merely large
    x, t = family("neg_inf")
    loss, g = ce_chain32(x, t, 0.0, 1.0)
    assert loss[2] == math.inf and loss[3] == math.inf
    loss[3] = 3e38
    with pytest.raises(AssertionError, match="class"):
        check(x, t, loss, g, 0.0, 1.0, tag="finite for +inf")


def test_only_finite_logit_is_the_target():
    """The loss is z x[t]^2 and the gradient is zero off the target, in the
    reference the families are held to."""
    x, t = family("neg_inf")
    for z in Z_GRID:
        loss, grad = cross_entropy_ref(x.double(), t, IGNORE, z, 1.0)
        xt = float(x[1, -1])
        assert abs(float(loss[1]) - z * xt * xt) <= 1e-15 * max(1.0, z * xt * xt)
        assert torch.count_nonzero(grad[1, :-1]).item() == 0
        assert abs(float(grad[1, -1]) - 2 * z * xt) <= 1e-15


def test_sentinels_see_a_stray_write():
    x, t = family("randn4", V=22)
    for o in range(8):
        case = make_case(x, t, o)
        assert case.view().data_ptr() % 16 == (2 * o) % 16
        assert torch.equal(case.view(), x)
        case.assert_sentinels()
        case.view().zero_()
        case.assert_sentinels()
        for where in (ce_check.PAD + o - 1, ce_check.PAD + o + x.numel()):
            broken = make_case(x, t, o)
            broken.buf[where] = 0.0
            with pytest.raises(AssertionError, match="sentinel"):
                broken.assert_sentinels()


@pytest.mark.parametrize("name", [f for f in FAMILIES if f != "nonfinite"])
def test_reference_is_fp64_autograd_on_the_families(name):
    """tests/test_cross_entropy_cpu.py holds ``cross_entropy_ref`` to torch on
    randn; here the rows the families add (needles, -inf runs, a lone finite
    logit), in fp64, wherever the loss is finite."""
    x, t = family(name)
    z, gs = 1e-2, 1.0 / 29
    loss, grad = cross_entropy_ref(x.double(), t, IGNORE, z, gs)
    rows = torch.isfinite(loss) & (t != IGNORE)
    xa = x.double().requires_grad_(True)
    lse = torch.logsumexp(xa, dim=1)
    xt = xa.gather(1, t.clamp(min=0).unsqueeze(1)).squeeze(1)
    per_row = lse - xt + z * lse * lse
    (gs * per_row[rows].sum()).backward()
    assert rows.sum() >= 3
    assert ((per_row.detach() - loss)[rows].abs() <= 1e-12 * loss[rows].abs().clamp(min=1)).all()
    err = (xa.grad - grad)[rows].abs()
    assert (err <= 1e-12 * grad[rows].abs() + 1e-18).all()
