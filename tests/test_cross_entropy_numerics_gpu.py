"""``cross_entropy_kernel`` (csrc/kernels/fused_cross_entropy.hip) and
``linear_cross_entropy`` on the device against the fp64 definition under the
derived bounds of tests/ce_check.py (docs/KERNELS.md, "Numerics" of
fused_cross_entropy.hip), at the smallest shapes that reach each path of the
kernel's indexing. The logits are always a view inside a sentinel buffer, and
after every launch every byte outside the view must be unchanged. Every check
prints its worst fraction of each bound."""

import math

import pytest
import torch

import ce_check
from ce_check import (FAMILIES, GS_GRID, IGNORE, U32, U_BF16, Z_GRID, Bounds, check, family,
                      make_case)
from torchft_amd import ops
from torchft_amd.ops.cross_entropy import fused_cross_entropy_

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked test without a HIP device"
    assert ops.have_hip_ext(), "HIP kernel extension must be loadable on a GPU box"
    return torch.device("cuda:0")


def _launch(case, dev, z, gs, write_grad=True):
    """One kernel call on a device copy of ``case``: (row_loss, the view's
    content afterwards), both on the CPU, the sentinels checked."""
    d = case.to(dev)
    view = d.view()
    assert view.is_contiguous()
    assert case.R == 0 or view.data_ptr() % 16 == (2 * case.o) % 16
    gs_t = torch.full((1,), gs, dtype=torch.float32, device=dev)
    loss = fused_cross_entropy_(view, d.t, ignore_index=IGNORE, z_loss=z, grad_scale=gs_t,
                                write_grad=write_grad)
    torch.cuda.synchronize()
    d.assert_sentinels(f"(R={case.R} V={case.V} o={case.o} write_grad={write_grad})")
    return loss.cpu(), d.view().cpu()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _both_ways(x, t, o, dev, z, gs, tag):
    """Gradient launch held to the checker, loss-only launch held to the
    gradient launch's loss bits and to untouched logits."""
    case = make_case(x, t, o)
    loss, grad = _launch(case, dev, z, gs)
    out = check(x, t, loss, grad, z, gs, tag=f"{tag} o={o}")
    loss_only, left = _launch(case, dev, z, gs, write_grad=False)
    assert torch.equal(_bits(loss_only), _bits(loss)), f"{tag}: loss differs without write_grad"
    assert torch.equal(_bits(left), _bits(x)), f"{tag}: write_grad=False changed a logit"
    if gs == 0.0:
        rows = Bounds(x, t, z, gs).finite
        assert (grad[rows] == 0).all(), f"{tag}: grad_scale 0 left a non-zero gradient"
    return out


def _walk(V, seed=0):
    """R = V rows whose one-hot visits every column, and one ignored row."""
    g = torch.Generator().manual_seed(100 + V + seed)
    x = (4.0 * torch.randn(V + 1, V, generator=g)).to(torch.bfloat16)
    t = torch.arange(V + 1)
    t[V] = IGNORE
    return x, t


@pytest.mark.parametrize("V", [1, 2, 7, 8, 9, 15, 16, 22, 23])
def test_every_column_at_every_alignment(dev, V):
    """V below the head (the ``head < V`` clip), no vector at all, 14 scalar
    elements (V = 22 at o = 1); the target in the head, in each slot of a
    vector and in the tail."""
    x, t = _walk(V)
    for o in range(8):
        _both_ways(x, t, o, dev, 1e-4, 1.0 / 29, f"walk V={V}")


@pytest.mark.parametrize("o", [0, 3])
@pytest.mark.parametrize("V", [8192, 8200, 8207])
def test_second_trip_of_the_vector_loop(dev, V, o):
    """1024 vectors exactly, lane 0's second trip, and that with a tail.
    Targets in the second-trip vector and in the tail; row 1 starts lane 0 on
    a -inf vector and is finite on its second trip."""
    g = torch.Generator().manual_seed(V + o)
    x = (4.0 * torch.randn(3, V, generator=g)).to(torch.bfloat16)
    x[1, :16] = float("-inf")
    t = torch.tensor([V - 1, min(8192 + 4, V - 1), 8191])
    _both_ways(x, t, o, dev, 1e-4, 1.0 / 29, f"second trip V={V}")


@pytest.mark.parametrize("name", FAMILIES)
def test_value_families(dev, name):
    """V = 1003, R = 6: rows with differing heads, every family over the
    z / grad_scale grid."""
    x, t = family(name)
    worst = {}
    for z in Z_GRID:
        for gs in GS_GRID:
            out = _both_ways(x, t, 0, dev, z, gs, name)
            for k, v in out.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"{name}: worst over the grid " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_only_finite_logit_is_the_target(dev):
    x, t = family("neg_inf")
    for z in Z_GRID:
        loss, grad = _launch(make_case(x, t, 5), dev, z, 1.0)
        xt = float(x[1, -1])
        b = Bounds(x, t, z, 1.0)
        assert abs(float(loss[1]) - z * xt * xt) <= float(b.loss_bound[1])
        assert (grad[1, :-1] == 0).all()


def test_nan_in_a_lane_without_a_vector(dev):
    """V = 22 at o = 1: one vector, and lanes 1..13 hold a scalar element
    only. A NaN there must reach the sum like any other."""
    V = 22
    x, t = _walk(V)
    t[:V] = 0
    for r in range(V):
        x[r, r] = float("nan")
    case = make_case(x, t, 1)
    loss, grad = _launch(case, dev, 1e-4, 1.0)
    check(x, t, loss, grad, 1e-4, 1.0, tag="NaN walk V=22 o=1")
    assert torch.isnan(loss[:V]).all()


def test_ignored_rows_at_every_alignment(dev):
    """Loss +0, every element +0, sentinels intact; the logits of the ignored
    rows are sentinels' look-alikes, NaN and -inf, which zeroing must not
    depend on."""
    for V in (5, 22, 1003):
        g = torch.Generator().manual_seed(V)
        x = (4.0 * torch.randn(4, V, generator=g)).to(torch.bfloat16)
        x[1, 0] = float("nan")
        x[2, ::2] = float("-inf")
        t = torch.tensor([IGNORE, IGNORE, IGNORE, 1])
        for o in range(8):
            loss, grad = _launch(make_case(x, t, o), dev, 1e-4, 1.0)
            assert (_bits(loss[:3]) == 0).all()
            assert (_bits(grad[:3]) == 0).all()
            check(x, t, loss, grad, 1e-4, 1.0, tag=f"ignored V={V} o={o}")


def test_no_rows(dev):
    case = make_case(torch.zeros(0, 16, dtype=torch.bfloat16), torch.zeros(0, dtype=torch.int64), 3)
    loss, grad = _launch(case, dev, 1e-4, 1.0)
    assert loss.shape == (0,) and loss.dtype == torch.float32 and grad.shape == (0, 16)


def test_bitwise_equal_from_call_to_call(dev):
    x, t = family("randn4", V=8207)
    case = make_case(x, t, 3)
    la, ga = _launch(case, dev, 1e-4, 0.37)
    lb, gb = _launch(case, dev, 1e-4, 0.37)
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(ga), _bits(gb))


def _refusals(dev):
    x, t = family("randn4", V=40)
    xd, td = x.to(dev), t.to(dev)
    gs = torch.ones(1, device=dev)
    wide = torch.zeros(6, 80, dtype=torch.bfloat16, device=dev)
    return xd, [
        ("fp32 logits", "logits", lambda b: (b.float(), td, gs, 0.0)),
        ("fp16 logits", "logits", lambda b: (b.half(), td, gs, 0.0)),
        ("1-D logits", "logits", lambda b: (b.reshape(-1), td, gs, 0.0)),
        ("3-D logits", "logits", lambda b: (b.reshape(6, 4, 10), td, gs, 0.0)),
        ("non-contiguous logits", "logits", lambda b: (wide[:, ::2], td, gs, 0.0)),
        ("int32 targets", "targets", lambda b: (b, td.int(), gs, 0.0)),
        ("wrong-length targets", "targets", lambda b: (b, td[:5], gs, 0.0)),
        ("CPU targets", "targets", lambda b: (b, t, gs, 0.0)),
        ("fp64 grad_scale", "grad_scale", lambda b: (b, td, gs.double(), 0.0)),
        ("two-element grad_scale", "grad_scale", lambda b: (b, td, torch.ones(2, device=dev), 0.0)),
        ("CPU grad_scale", "grad_scale", lambda b: (b, td, torch.ones(1), 0.0)),
        ("negative z_loss", "z_loss", lambda b: (b, td, gs, -1e-4)),
    ]


def test_refusals_name_their_argument_and_touch_nothing(dev):
    xd, cases = _refusals(dev)
    for label, arg, make in cases:
        buf = xd.clone()
        logits, targets, gs, z = make(buf)
        with pytest.raises((RuntimeError, ValueError, TypeError), match=arg):
            fused_cross_entropy_(logits, targets, ignore_index=IGNORE, z_loss=z, grad_scale=gs)
        torch.cuda.synchronize()
        assert torch.equal(_bits(buf), _bits(xd)), f"{label}: refused, yet the logits changed"


# ---- linear_cross_entropy on the device ------------------------------------------

N, D, V_HEAD, CHUNK = 300, 256, 1003, 128


def _head_inputs(dev, ignore=None):
    g = torch.Generator().manual_seed(11)
    h = torch.randn(N, D, generator=g).to(torch.bfloat16)
    w = (torch.randn(V_HEAD, D, generator=g) * D ** -0.5).to(torch.bfloat16)
    t = torch.randint(0, V_HEAD, (N,), generator=g)
    if ignore == "some":  # 20 %: the whole last chunk (44 rows) and 16 others
        t[2 * CHUNK :] = IGNORE
        t[torch.randperm(2 * CHUNK, generator=g)[:16]] = IGNORE
    elif ignore == "all":
        t[:] = IGNORE
    return h.to(dev), w.to(dev), t.to(dev)


def _run_head(h, w, t, z, h_grad=True, w_grad=True):
    ha = h.clone().requires_grad_(h_grad)
    wa = w.clone().requires_grad_(w_grad)
    loss = ops.linear_cross_entropy(ha, wa, t, chunk_rows=CHUNK, z_loss=z)
    loss.backward()
    return loss.detach(), ha.grad, wa.grad


def _head_reference(h, w, t, z):
    """fp64 from the bf16 logits the function itself forms (bf16 mm on the
    device, chunk by chunk), and the bounds that follow from them."""
    n_valid = max(int((t != IGNORE).sum()), 1)
    gs = float(torch.tensor(1.0 / n_valid, dtype=torch.float32))
    logits = torch.cat([torch.mm(h[i : i + CHUNK], w.t()) for i in range(0, N, CHUNK)]).cpu()
    b = Bounds(logits, t.cpu(), z, gs)
    assert b.finite.sum() + b.ignored.sum() == N
    hd, wd = h.cpu().double(), w.cpu().double()
    dl, dl_bound = b.ref_grad, b.grad_bound
    loss_ref = float(b.ref_loss.sum()) * gs
    # the fp32 sum of N row losses and the product with gs: N + 1 roundings
    loss_bound = float(b.loss_bound.sum()) * gs + (N + 1) * U32 * float(b.ref_loss.abs().sum()) * gs
    dh_ref = dl @ wd
    dh_bound = (U_BF16 * dh_ref.abs() + V_HEAD * U32 * (dl.abs() @ wd.abs())
                + dl_bound @ wd.abs())
    # dW: addmm_ accumulates into a bf16 dW, so the running sum is rounded to
    # bf16 once per chunk (the last of them is the result's own rounding;
    # 2^-7 on top for the earlier roundings inside the later sums), each
    # chunk's GEMM accumulates its rows in fp32
    mag = dl.abs().t() @ hd.abs()
    running = torch.zeros(V_HEAD, D, dtype=torch.float64)
    rounded = torch.zeros_like(running)
    for i in range(0, N, CHUNK):
        running = running + dl[i : i + CHUNK].t() @ hd[i : i + CHUNK]
        rounded = rounded + running.abs()
    dw_ref = running
    dw_bound = (U_BF16 * (1 + 2 * U_BF16) * rounded + N * U32 * mag
                + dl_bound.t() @ hd.abs())
    return loss_ref, loss_bound, dh_ref, dh_bound, dw_ref, dw_bound


def _hold(name, got, ref, bound):
    err = (got.cpu().double() - ref).abs()
    frac = ce_check._frac(err, bound)
    print(f"linear_cross_entropy {name}: worst error / bound {frac:.3f}")
    assert frac <= 1.0, f"{name} off by {frac:.3f} x bound"


@pytest.mark.parametrize("ignore,z", [(None, 0.0), ("some", 0.0), (None, 1e-3), ("some", 1e-3)])
def test_head_against_fp64_of_its_own_logits(dev, ignore, z):
    h, w, t = _head_inputs(dev, ignore)
    if ignore == "some":
        assert (t[2 * CHUNK :] == IGNORE).all() and int((t == IGNORE).sum()) == N // 5
    loss, dh, dw = _run_head(h, w, t, z)
    assert loss.dtype == torch.float32 and dh.dtype == dw.dtype == torch.bfloat16
    loss_ref, loss_bound, dh_ref, dh_bound, dw_ref, dw_bound = _head_reference(h, w, t, z)
    lf = abs(float(loss) - loss_ref) / loss_bound
    print(f"linear_cross_entropy loss {float(loss):.7f} ref {loss_ref:.7f}: error / bound {lf:.3f}")
    assert lf <= 1.0
    _hold("dh", dh, dh_ref, dh_bound)
    _hold("dW", dw, dw_ref, dw_bound)
    if ignore == "some":
        assert (dh[2 * CHUNK :] == 0).all(), "ignored rows with a gradient"


def test_head_all_ignored(dev):
    h, w, t = _head_inputs(dev, "all")
    loss, dh, dw = _run_head(h, w, t, 1e-3)
    assert float(loss) == 0.0 and (dh == 0).all() and (dw == 0).all()


def test_head_one_sided_grad_and_no_grad_are_bitwise_the_same(dev):
    h, w, t = _head_inputs(dev, "some")
    loss, dh, dw = _run_head(h, w, t, 1e-3)
    loss_h, dh_only, none_w = _run_head(h, w, t, 1e-3, w_grad=False)
    loss_w, none_h, dw_only = _run_head(h, w, t, 1e-3, h_grad=False)
    assert none_w is None and none_h is None
    assert torch.equal(_bits(dh_only), _bits(dh)) and torch.equal(_bits(dw_only), _bits(dw))
    with torch.no_grad():
        loss_ng = ops.linear_cross_entropy(h, w, t, chunk_rows=CHUNK, z_loss=1e-3)
    for other in (loss_h, loss_w, loss_ng):
        assert torch.equal(_bits(other.reshape(1)), _bits(loss.reshape(1)))
