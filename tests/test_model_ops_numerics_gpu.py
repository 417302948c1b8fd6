"""The kernels of csrc/kernels/fused_model_ops.hip against fp64 under the
derived bounds of tests/model_ops_check.py (docs/KERNELS.md, "Numerics" of that
file; the checker's own test is tests/test_model_ops_numerics_cpu.py). Inputs
are made on the CPU from seeds, the kernels run through the bindings, and the
outputs go back to the CPU, where every check prints its worst error over
bound before it asserts."""

import pytest
import torch

import model_ops_check as mc

pytestmark = pytest.mark.gpu

H_MAX = 40952  # the largest H rmsnorm_bwd accepts (kernels.h)


@pytest.fixture
def dev():
    return torch.device("cuda:0")


@pytest.fixture
def ext():
    from torchft_amd.ops import hip_ext

    return hip_ext()


# ---- SwiGLU ---------------------------------------------------------------------


@pytest.mark.parametrize("family,n", [("every_gate", 65536), ("randn", 8), ("randn", 2056)])
def test_swiglu_plain(dev, ext, family, n):
    a, b, dy = mc.swiglu_inputs(family, n)
    label = f"swiglu {family} n={n}"
    o = ext.swiglu_fwd(a.to(dev), b.to(dev))
    da, db = ext.swiglu_bwd(dy.to(dev), a.to(dev), b.to(dev))
    mc.check_swiglu_fwd(label, o, a, b)
    mc.check_swiglu_bwd(label, da, db, dy, a, b)


# (249, 264): all 65,536 gate patterns with a row boundary inside a workgroup
# and 2f = 528 not a power of two
@pytest.mark.parametrize("family,rows,f", [("every_gate",) + mc.GLU_EVERY_GATE,
                                           ("randn", 1, 8), ("randn", 3, 264)])
def test_swiglu_packed(dev, ext, family, rows, f):
    a, b, dy = mc.swiglu_inputs(family, rows * f)
    gu = mc.pack_glu(a, b, rows, f)
    dy2 = dy.view(rows, f)
    label = f"swiglu_glu {family} ({rows}, {f})"
    o = ext.swiglu_glu_fwd(gu.to(dev))
    dgu = ext.swiglu_glu_bwd(dy2.to(dev), gu.to(dev))
    assert o.shape == (rows, f) and dgu.shape == (rows, 2 * f)
    mc.check_swiglu_fwd(label, o.view(-1), a, b)
    mc.check_swiglu_glu_bwd(label, dgu, dy2, gu)

    # the plain kernels share swiglu_fwd8 / swiglu_bwd1: the same bits
    o_plain = ext.swiglu_fwd(a.to(dev), b.to(dev))
    da, db = ext.swiglu_bwd(dy.to(dev), a.to(dev), b.to(dev))
    assert mc.same_bits(o.view(-1), o_plain)
    assert mc.same_bits(dgu[:, :f].reshape(-1), da)
    assert mc.same_bits(dgu[:, f:].reshape(-1), db)


# ---- RMSNorm --------------------------------------------------------------------

# (3, 2048): exactly one trip; (3, 2056): lane 0's second; (5, 4104): its third;
# (2049, 8): more rows than the 2048-workgroup grid of the backward; (2, H_MAX):
# the whole LDS
RMSNORM_CASES = [(rows, H, fam) for rows, H in mc.RMSNORM_SHAPES + [(2, H_MAX)]
                 for fam in (mc.RMSNORM_FAMILIES if rows <= 5 else ["randn"])]


@pytest.mark.parametrize("rows,H,family", RMSNORM_CASES)
def test_rmsnorm(dev, ext, rows, H, family):
    x, w, dy, eps = mc.rmsnorm_inputs(rows, H, family)
    label = f"rmsnorm ({rows}, {H}) {family}"
    xg, wg, dyg = x.to(dev), w.to(dev), dy.to(dev)
    y, invrms = ext.rmsnorm_fwd(xg, wg, eps)
    mc.check_rmsnorm_fwd(label, y, invrms, x, w, eps)
    if family == "zero_row":
        assert not y[0].any()

    dx, dw = ext.rmsnorm_bwd(dyg, xg, wg, invrms)
    mc.check_rmsnorm_bwd(label, dx, dw, dy, x, w, invrms)
    dx2, _ = ext.rmsnorm_bwd(dyg, xg, wg, invrms)
    assert mc.same_bits(dx, dx2)


# ---- rope_apply -----------------------------------------------------------------


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "transpose"])
@pytest.mark.parametrize("shape,table_rows", mc.ROPE_SHAPES)
def test_rope_apply(dev, ext, shape, table_rows, backward):
    from torchft_amd.ops import rope_tables

    cos, sin = rope_tables(table_rows, shape[3], device=dev)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(6)).to(torch.bfloat16)
    out = ext.rope_apply(x.to(dev), cos, sin, backward)
    # the fp64 side reads the very table values the kernel read
    mc.check_rope(f"rope_apply {shape} backward={backward}", out, x, cos, sin, backward)


# ---- the autograd wrappers --------------------------------------------------------


def test_wrappers_return_the_bindings_outputs(dev, ext):
    from torchft_amd.ops import rmsnorm, swiglu, swiglu_glu

    x, w, dy, eps = (t.to(dev) if isinstance(t, torch.Tensor) else t
                     for t in mc.rmsnorm_inputs(2, 2056, "randn"))
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = rmsnorm(xr, wr, eps)
    y.backward(dy)
    y_b, invrms = ext.rmsnorm_fwd(x, w, eps)
    dx_b, dw_b = ext.rmsnorm_bwd(dy, x, w, invrms)
    assert mc.same_bits(y.detach(), y_b) and mc.same_bits(xr.grad, dx_b)
    # two rows: each dw column is two atomic adds onto zero, and a two-term sum
    # does not depend on the order, so dw is the same from call to call
    assert dw_b.dtype == torch.float32
    assert mc.same_bits(wr.grad, dw_b.to(torch.bfloat16))

    a, b, g = (t.to(dev) for t in mc.swiglu_inputs("randn", 2056))
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    o = swiglu(ar, br)
    o.backward(g)
    da_b, db_b = ext.swiglu_bwd(g, a, b)
    assert mc.same_bits(o.detach(), ext.swiglu_fwd(a, b))
    assert mc.same_bits(ar.grad, da_b) and mc.same_bits(br.grad, db_b)

    gu = mc.pack_glu(a[:792].clone(), b[:792].clone(), 3, 264).requires_grad_(True)
    g2 = g[:792].view(3, 264)
    o = swiglu_glu(gu)
    o.backward(g2)
    assert mc.same_bits(o.detach(), ext.swiglu_glu_fwd(gu.detach()))
    assert mc.same_bits(gu.grad, ext.swiglu_glu_bwd(g2, gu.detach()))
