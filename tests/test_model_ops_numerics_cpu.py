"""The model-ops checker checked (tests/model_ops_check.py against
torchft_amd/ops/model_ops_ref.py): the fp32 emulation of each kernel's rounding
chain passes every criterion on every family tests/test_model_ops_numerics_gpu.py
uses, its worst fraction of every bound is at most two thirds, and each
injected mistake is refused by the criterion named next to it. This is the
evidence that the GPU tests would fail on a subtly wrong kernel. No GPU.

Where a bound has the term ``u |ref|`` of the bf16 store, rounding a correct
value to bf16 alone reaches 0.99 of it, so the two thirds are asked of the fp32
part: of the chain's value ahead of its store against the bound without ``u``
and without the bf16 subnormal step. The stored value is held to the whole
bound as the kernels are. This departs from the letter of "two thirds of every
bound", which no chain that ends in a bf16 store can meet; docs/KERNELS.md
says so above its table of fractions."""

import functools

import pytest
import torch

import model_ops_check as mc
from torchft_amd.ops import model_ops_ref as ref
from torchft_amd.ops import rope_tables

TWO_THIRDS = 2.0 / 3.0
H_MAX = 40952  # the largest H rmsnorm_bwd accepts (kernels.h)
RMSNORM_CASES = [(rows, H, fam) for rows, H in mc.RMSNORM_SHAPES + [(2, H_MAX)]
                 for fam in (mc.RMSNORM_FAMILIES if rows <= 5 else ["randn"])]


def _under_two_thirds(fractions):
    print({k: round(v, 4) for k, v in fractions.items()})
    bad = {k: v for k, v in fractions.items() if not v <= TWO_THIRDS}
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def _rope_case(shape, table_rows):
    cos, sin = rope_tables(table_rows, shape[3])
    gen = torch.Generator().manual_seed(6)
    return torch.randn(*shape, generator=gen).to(torch.bfloat16), cos, sin


# ---- the emulation under the bounds ------------------------------------------------


@pytest.mark.parametrize("rows,H,family", RMSNORM_CASES)
def test_rmsnorm_emulation_two_thirds(rows, H, family):
    x, w, dy, eps = mc.rmsnorm_inputs(rows, H, family)
    label = f"fp32 chain ({rows}, {H}) {family}"
    y, inv = ref.rmsnorm_fwd_emulated(x, w, eps)
    stored = mc.check_rmsnorm_fwd(label, y, inv, x, w, eps)
    dx, dw = ref.rmsnorm_bwd_emulated(dy, x, w, inv)
    stored.update(mc.check_rmsnorm_bwd(label, dx, dw, dy, x, w, inv))
    if family == "zero_row":
        inv0 = ref.fp32_value(eps) ** -0.5
        assert not y[0].any()
        assert abs(float(inv[0]) - inv0) <= mc.k_invrms(H) * mc.E * inv0

    label += ", ahead of the store"
    y32, _ = ref.rmsnorm_fwd_emulated(x, w, eps, store=False)
    dx32, _ = ref.rmsnorm_bwd_emulated(dy, x, w, inv, store=False)
    part = mc.check_rmsnorm_fwd(label, y32, inv, x, w, eps, stored=False)
    part.update(mc.check_rmsnorm_bwd(label, dx32, dw, dy, x, w, inv, stored=False))
    part["y bf16"] = stored["y bf16"]
    _under_two_thirds(part)


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "transpose"])
@pytest.mark.parametrize("shape,table_rows", mc.ROPE_SHAPES)
def test_rope_emulation_two_thirds(shape, table_rows, backward):
    x, cos, sin = _rope_case(shape, table_rows)
    label = f"fp32 chain {shape} backward={backward}"
    mc.check_rope(label, ref.rope_emulated(x, cos, sin, backward), x, cos, sin, backward)
    _under_two_thirds(mc.check_rope(
        label + ", ahead of the store", ref.rope_emulated(x, cos, sin, backward, store=False),
        x, cos, sin, backward, stored=False))


SWIGLU_CASES = [("every_gate", 65536), ("every_gate", 249 * 264), ("randn", 8),
                ("randn", 2056), ("randn", 3 * 264)]


@pytest.mark.parametrize("family,n", SWIGLU_CASES)
def test_swiglu_emulation_two_thirds(family, n):
    a, b, dy = mc.swiglu_inputs(family, n)
    label = f"fp32 chain {family} n={n}"
    mc.check_swiglu_fwd(label, ref.swiglu_fwd_emulated(a, b), a, b)
    mc.check_swiglu_bwd(label, *ref.swiglu_bwd_emulated(dy, a, b), dy, a, b)
    label += ", ahead of the store"
    part = mc.check_swiglu_fwd(label, ref.swiglu_fwd_emulated(a, b, store=False), a, b,
                               stored=False)
    part.update(mc.check_swiglu_bwd(label, *ref.swiglu_bwd_emulated(dy, a, b, store=False),
                                    dy, a, b, stored=False))
    _under_two_thirds(part)


def test_every_gate_holds_every_pattern_and_the_clamp_holds():
    a, b, dy = mc.swiglu_inputs("every_gate", 65536)
    assert len(set(a.view(torch.int16).tolist())) == 65536
    assert int(torch.isnan(a).sum()) == 2 * 127 and int(torch.isinf(a).sum()) == 2
    for t in (b, dy):
        assert ((t.abs() >= 2.0 ** -4) & (t.abs() <= 1.0)).all()
        assert (t < 0).any() and (t > 0).any()
    rows, f = mc.GLU_EVERY_GATE
    assert len(set(mc.every_gate(rows * f).view(torch.int16).tolist())) == 65536


def test_non_finite_gates_of_the_emulation():
    """What docs/KERNELS.md tabulates: a NaN gate gives NaN everywhere, +inf
    gives o and db = +-inf and da NaN (inf * 0), -inf gives NaN everywhere
    (-inf * 0); the largest finite gates give finite results."""
    big = torch.finfo(torch.bfloat16).max
    a = torch.tensor([float("nan"), float("inf"), float("-inf"), big, -big],
                     dtype=torch.bfloat16)
    b = torch.full_like(a, 0.5)
    dy = torch.full_like(a, -0.25)
    o = ref.swiglu_fwd_emulated(a, b).float()
    da, db = (t.float() for t in ref.swiglu_bwd_emulated(dy, a, b))
    inf = float("inf")
    assert torch.isnan(o[0]) and torch.isnan(da[0]) and torch.isnan(db[0])
    assert o[1] == inf and torch.isnan(da[1]) and db[1] == -inf
    assert torch.isnan(o[2]) and torch.isnan(da[2]) and torch.isnan(db[2])
    assert torch.isfinite(o[3:]).all() and torch.isfinite(da[3:]).all()
    assert torch.isfinite(db[3:]).all()
    assert o[4] == 0 and da[4] == 0 and db[4] == 0 and da[3] == dy[3].float() * 0.5


def test_class_criterion_refuses_a_finite_value_for_nan_and_the_reverse():
    a, b, _ = mc.swiglu_inputs("every_gate", 65536)
    o = ref.swiglu_fwd_emulated(a, b)
    nan_at = int(torch.isnan(o).nonzero()[0])
    for at, value in ((nan_at, 0.0), (40000, float("nan")), (40000, float("inf"))):
        wrong = o.clone()
        wrong[at] = value
        with pytest.raises(AssertionError, match=r"^class: "):
            mc.check_swiglu_fwd("class", wrong, a, b)


# ---- injected mistakes ---------------------------------------------------------------

# (mistake, family that shows it, criterion meant to see it)
RMSNORM_FWD_REFUSED = [
    ("eps_before_div", "small", "invrms"), ("eps_before_div", "randn", "invrms"),
    ("no_eps", "small", "invrms"), ("no_eps", "randn", "invrms"),
    ("h_minus_1", "randn", "invrms"), ("h_minus_1", "large", "invrms"),
    ("ss_bf16", "randn", "invrms"),
    ("y_bf16_before_w", "randn", "y"), ("y_bf16_before_w", "randn", "y bf16"),
    ("inv_bf16", "randn", "y bf16"), ("inv_bf16", "large", "y"),
]
RMSNORM_BWD_REFUSED = [
    ("inv2_in_k", "small", "dx"), ("inv2_in_k", "large", "dx"),
    ("k_without_1_over_h", "randn", "dx"), ("k_without_1_over_h", "small", "dx"),
    ("s_without_w", "randn", "dx"), ("s_without_w", "w_zeros", "dx"),
]
INJECTION_SHAPES = [(3, 2056), (5, 4104)]


def _only(criterion, fractions_fn):
    """The checks run to the criterion named; the ones before it pass."""
    with pytest.raises(AssertionError, match=rf"^{criterion}: "):
        fractions_fn()


@pytest.mark.parametrize("rows,H", INJECTION_SHAPES)
@pytest.mark.parametrize("inject,family,criterion", RMSNORM_FWD_REFUSED)
def test_rmsnorm_fwd_mistake_is_refused(inject, family, criterion, rows, H):
    x, w, _, eps = mc.rmsnorm_inputs(rows, H, family)
    y, inv = ref.rmsnorm_fwd_emulated(x, w, eps, inject=inject)
    if criterion != "invrms":
        # the mistake is in how y is formed: invrms itself is right
        _, inv = ref.rmsnorm_fwd_emulated(x, w, eps)
    if criterion == "y bf16":
        _, y64 = ref.rmsnorm_fwd_ref64(x, w, eps)
        _only(criterion, lambda: mc._hold_bf16("y", inject, y, y64))
    else:
        _only(criterion, lambda: mc.check_rmsnorm_fwd(inject, y, inv, x, w, eps))


@pytest.mark.parametrize("rows,H", INJECTION_SHAPES)
@pytest.mark.parametrize("inject,family,criterion", RMSNORM_BWD_REFUSED)
def test_rmsnorm_bwd_mistake_is_refused(inject, family, criterion, rows, H):
    x, w, dy, eps = mc.rmsnorm_inputs(rows, H, family)
    _, inv = ref.rmsnorm_fwd_emulated(x, w, eps)
    dx, dw = ref.rmsnorm_bwd_emulated(dy, x, w, inv, inject=inject)
    _only(criterion, lambda: mc.check_rmsnorm_bwd(inject, dx, dw, dy, x, w, inv))


def test_inv_cubed_alone_is_refused_on_the_one_hot_row():
    """``inv * inv * inv * s / H``, the order the kernel had: ``inv^3`` leaves
    the fp32 range for the row whose one element is 2^60, ``k`` is 0 and dx of
    that element keeps its whole first term."""
    for rows, H in mc.RMSNORM_SHAPES[:4]:
        x, w, dy, eps = mc.rmsnorm_inputs(rows, H, "one_hot")
        _, inv = ref.rmsnorm_fwd_emulated(x, w, eps)
        _, dw = ref.rmsnorm_bwd_emulated(dy, x, w, inv)
        i, d, v, g = inv[:, None], dy.float(), x.float(), w.float()
        k = i * i * i * (d * g * v).sum(-1, keepdim=True) / H
        assert k[0] == 0
        dx = (i * g * d - k * v).to(torch.bfloat16)
        _only("dx", lambda: mc.check_rmsnorm_bwd("inv^3 first", dx, dw, dy, x, w, inv))


SWIGLU_REFUSED = [
    ("swiglu_fwd", "sig_bf16", "o"), ("swiglu_fwd", "halves_swapped", "o"),
    ("swiglu_fwd", "sig_clamped", "o"),
    ("swiglu_bwd", "sig_bf16", "da"), ("swiglu_bwd", "da_without_b", "da"),
    ("swiglu_bwd", "one_plus_sig", "da"), ("swiglu_bwd", "db_from_sig", "db"),
    ("swiglu_bwd", "halves_swapped", "da"), ("swiglu_bwd", "sig_clamped", "da"),
]


# no randn gate is below -20: every_gate alone shows the clamp. On every_gate
# a * (1 + sig) overflows for the largest gates, which the class criterion,
# the first to run, reports
SWIGLU_REFUSED_ON = [
    (k, i, "class" if (i, fam) == ("one_plus_sig", "every_gate") else c, fam, n)
    for k, i, c in SWIGLU_REFUSED for fam, n in [("every_gate", 65536), ("randn", 2056)]
    if not (i == "sig_clamped" and fam == "randn")]


@pytest.mark.parametrize("kernel,inject,criterion,family,n", SWIGLU_REFUSED_ON)
def test_swiglu_mistake_is_refused(kernel, inject, criterion, family, n):
    a, b, dy = mc.swiglu_inputs(family, n)
    # the finite gates: a mistake also changes what NaN and inf gates give, and
    # the class criterion, which has its own test, would report that first
    keep = torch.isfinite(a)
    a, b, dy = a[keep], b[keep], dy[keep]
    if kernel == "swiglu_fwd":
        o = ref.swiglu_fwd_emulated(a, b, inject=inject)
        _only(criterion, lambda: mc.check_swiglu_fwd(inject, o, a, b))
    else:
        da, db = ref.swiglu_bwd_emulated(dy, a, b, inject=inject)
        if criterion == "db":
            da, _ = ref.swiglu_bwd_emulated(dy, a, b)
        _only(criterion, lambda: mc.check_swiglu_bwd(inject, da, db, dy, a, b))


def test_packed_halves_swapped_is_refused():
    rows, f = 3, 264
    a, b, dy = mc.swiglu_inputs("randn", rows * f)
    gu = mc.pack_glu(a, b, rows, f)
    o = ref.swiglu_glu_fwd_emulated(gu, inject="halves_swapped")
    _only("o", lambda: mc.check_swiglu_fwd("packed swapped", o.view(-1), a, b))
    dgu = ref.swiglu_glu_bwd_emulated(dy.view(rows, f), gu, inject="halves_swapped")
    _only("da", lambda: mc.check_swiglu_glu_bwd("packed swapped", dgu, dy.view(rows, f), gu))
    # and unswapped the packed chain is the plain one
    assert mc.same_bits(ref.swiglu_glu_fwd_emulated(gu).view(-1),
                        ref.swiglu_fwd_emulated(a, b))


ROPE_REFUSED = [
    ("sin_sign_second_half", False), ("sin_sign_second_half", True),
    ("backward_not_flipped", True), ("row_plus_1", False), ("row_plus_1", True),
]


@pytest.mark.parametrize("inject,backward", ROPE_REFUSED)
def test_rope_mistake_is_refused(inject, backward):
    for shape, table_rows in mc.ROPE_SHAPES:
        if inject == "row_plus_1" and table_rows <= shape[1]:
            continue  # the table has no row S
        x, cos, sin = _rope_case(shape, table_rows)
        out = ref.rope_emulated(x, cos, sin, backward, inject=inject)
        _only("rotation", lambda: mc.check_rope(inject, out, x, cos, sin, backward))


def test_every_injection_is_exercised():
    seen = {k: set() for k in ref.INJECTIONS}
    seen["rmsnorm_fwd"] = {i for i, _, _ in RMSNORM_FWD_REFUSED}
    seen["rmsnorm_bwd"] = {i for i, _, _ in RMSNORM_BWD_REFUSED}
    for kernel, inject, _ in SWIGLU_REFUSED:
        seen[kernel].add(inject)
    seen["rope"] = {i for i, _ in ROPE_REFUSED}
    assert seen == {k: set(v) for k, v in ref.INJECTIONS.items()}


# ---- the definitions ---------------------------------------------------------------


def test_ref64_is_autograd_of_the_definition():
    """dx, dw, da, db of the reference are torch autograd's of y and o in fp64."""
    x, w, dy, eps = mc.rmsnorm_inputs(3, 2056, "randn")
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    inv = torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + ref.fp32_value(eps))
    y = xd * inv * wd
    y.backward(dy.double())
    inv64, y64 = ref.rmsnorm_fwd_ref64(x, w, eps)
    r = ref.rmsnorm_bwd_ref64(dy, x, w, inv64)
    assert torch.allclose(y64, y.detach(), rtol=1e-13, atol=0)
    assert ((r.dx - xd.grad).abs() <= 1e-13 * r.mag).all()
    assert ((r.dw - wd.grad).abs() <= 1e-13 * r.dw_abs).all()

    a, b, g = mc.swiglu_inputs("randn", 2056)
    ad = a.double().requires_grad_(True)
    bd = b.double().requires_grad_(True)
    o = torch.nn.functional.silu(ad) * bd
    o.backward(g.double())
    s = ref.swiglu_bwd_ref64(g, a, b)
    assert torch.allclose(ref.swiglu_fwd_ref64(a, b), o.detach(), rtol=1e-13, atol=0)
    assert ((s.da - ad.grad).abs() <= 1e-13 * s.mag_da).all()
    assert torch.allclose(s.db, bd.grad, rtol=1e-13, atol=0)


def test_transpose_ref_undoes_the_rotation():
    shape, table_rows = mc.ROPE_SHAPES[1]
    x, cos, sin = _rope_case(shape, table_rows)
    out, _ = ref.rotate_ref64(x, cos, sin)
    cd, sd = cos[:shape[1]].double().view(1, -1, 1, 8), sin[:shape[1]].double().view(1, -1, 1, 8)
    o1, o2 = out.chunk(2, dim=-1)
    back = torch.cat([o1 * cd + o2 * sd, o2 * cd - o1 * sd], dim=-1)
    assert torch.allclose(back, x.double(), rtol=0, atol=1e-6)  # cos^2 + sin^2 in fp32 tables
