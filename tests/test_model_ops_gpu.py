"""GPU tests of the RMSNorm / RoPE / SwiGLU bindings (csrc/kernels/
fused_model_ops.hip, `OpArgs` in bindings.cpp) at the smallest shapes at which
each kernel's indexing can still go wrong, and of the one argument rule the
seven bindings share: any layout and any alignment give the bits of a fresh
contiguous copy, zero-sized inputs launch nothing, and everything else is
refused by name before a launch."""

import pytest
import torch

import model_ops_check as mc

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
EPS = 1e-5


@pytest.fixture
def dev():
    return torch.device("cuda:0")


@pytest.fixture
def ext():
    from torchft_amd.ops import hip_ext

    return hip_ext()


def _randn(dev, *shape, seed=0, dtype=BF16):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(*shape, device=dev, dtype=torch.float32, generator=g).to(dtype)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _assert_same_bits(got, want):
    got = got if isinstance(got, (list, tuple)) else [got]
    want = want if isinstance(want, (list, tuple)) else [want]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        assert torch.equal(_bits(g.contiguous()), _bits(w.contiguous()))


# ---------------------------------------------------------------- numerics


# Held to fp64 under the derived bounds of tests/model_ops_check.py; the families
# built to show a wrong kernel are in tests/test_model_ops_numerics_gpu.py.


# (1, 8): one vector, 255 idle lanes; 2056 = 256*8 + 8: one lane's second trip
@pytest.mark.parametrize("rows,H", [(1, 8), (3, 2056)])
def test_rmsnorm_forward(dev, ext, rows, H):
    x = _randn(dev, rows, H, seed=1)
    w = _randn(dev, H, seed=2)
    y, invrms = ext.rmsnorm_fwd(x, w, EPS)
    assert invrms.shape == (rows,) and invrms.dtype == torch.float32
    mc.check_rmsnorm_fwd(f"rmsnorm_fwd ({rows}, {H})", y, invrms, x, w, EPS)


def test_rmsnorm_backward_more_rows_than_workgroups(dev, ext):
    """2049 rows on a grid capped at 2048: one workgroup takes two rows and the
    dw atomics see all 2048 workgroups."""
    from torchft_amd.ops import rmsnorm
    from torchft_amd.ops.model_ops_ref import rmsnorm_bwd_ref64

    rows, H = 2049, 8
    x = _randn(dev, rows, H, seed=3).requires_grad_(True)
    w = _randn(dev, H, seed=4).requires_grad_(True)
    dy = _randn(dev, rows, H, seed=5)
    rmsnorm(x, w, EPS).backward(dy)

    # the binding's bf16 dx under u |ref| + k e mag and its fp32 dw against
    # sum_rows dy * x * invrms in fp64, from the kernel's own invrms. Per column
    # the kernel rounds each product twice (two fp32 multiplies) and adds the
    # rows one at a time in some order: at most rows + 1 roundings of partial
    # sums that never exceed sum |term|, each 2^-24 relative; (rows + 8) * 2^-23
    # leaves a factor of two.
    xd, wd = x.detach(), w.detach()
    _, invrms = ext.rmsnorm_fwd(xd, wd, EPS)
    dx, dw = ext.rmsnorm_bwd(dy, xd, wd, invrms)
    assert dw.shape == (H,) and dw.dtype == torch.float32
    mc.check_rmsnorm_bwd("rmsnorm_bwd (2049, 8)", dx, dw, dy, xd, wd, invrms)
    # autograd's dx is the binding's; its dw is one more rounding, to bf16
    _assert_same_bits(x.grad, dx)
    r = rmsnorm_bwd_ref64(dy.cpu(), xd.cpu(), wd.cpu(), invrms.cpu())
    bound = (rows + 8) * 2.0 ** -23 * r.dw_abs
    assert w.grad.dtype == BF16
    err = (w.grad.cpu().double() - r.dw).abs()
    assert torch.all(err <= mc.U * r.dw.abs() + (1 + mc.U) * bound)


# (1, 3, 1, 8): halfD = 4, one thread per row; (2, 5, 3, 16) with 9 table rows:
# the table is longer than S and a row takes two threads
@pytest.mark.parametrize("shape,table_rows", [((1, 3, 1, 8), 3), ((2, 5, 3, 16), 9)])
def test_rope_forward_backward(dev, ext, shape, table_rows):
    from torchft_amd.ops import rope, rope_tables
    from torchft_amd.ops.model_ops_ref import rotate_ref64

    S, D = shape[1], shape[3]
    cos, sin = rope_tables(table_rows, D, device=dev)
    x = _randn(dev, *shape, seed=6).requires_grad_(True)
    out = rope(x, cos, sin)
    mc.check_rope(f"rope {shape}", out.detach(), x.detach(), cos, sin, False)

    dy = _randn(dev, *shape, seed=7)
    out.backward(dy)
    mc.check_rope(f"rope {shape} grad", x.grad, dy, cos, sin, True)

    # the rotation's transpose undoes it: back = R^T out carries its own
    # roundings, (u + 3e) mag, the forward's, (u + 3e) mag, taken through
    # |R^T|, and c^2 + s^2 = 1 only as far as the tables go: cos and sin within
    # 2 ulp = 4e each, doubled in the squares, 8e |x|
    back = ext.rope_apply(out.detach(), cos, sin, True)
    mc.check_rope(f"rope {shape} transpose", back, out.detach(), cos, sin, True)
    xc, oc = x.detach().cpu(), out.detach().cpu()
    _, mag_f = rotate_ref64(xc, cos.cpu(), sin.cpu(), False)
    _, mag_b = rotate_ref64(oc, cos.cpu(), sin.cpu(), True)
    c = cos[:S].cpu().double().abs().view(1, S, 1, D // 2)
    s = sin[:S].cpu().double().abs().view(1, S, 1, D // 2)
    f1, f2 = mag_f.chunk(2, dim=-1)
    through = torch.cat([c * f1 + s * f2, c * f2 + s * f1], dim=-1)
    x1, x2 = xc.double().abs().chunk(2, dim=-1)
    bound = (mc.U + 3 * mc.E) * (mag_b + through) + 8 * mc.E * torch.cat([x1 + x2, x1 + x2], -1)
    assert torch.all((back.cpu().double() - xc.double()).abs() <= bound)


@pytest.mark.parametrize("n", [8, 2056])
def test_swiglu_plain(dev, n):
    from torchft_amd.ops import swiglu

    a = _randn(dev, n, seed=8).requires_grad_(True)
    b = _randn(dev, n, seed=9).requires_grad_(True)
    dy = _randn(dev, n, seed=10)
    y = swiglu(a, b)
    y.backward(dy)
    mc.check_swiglu_fwd(f"swiglu n={n}", y.detach(), a.detach(), b.detach())
    mc.check_swiglu_bwd(f"swiglu n={n}", a.grad, b.grad, dy, a.detach(), b.detach())


# (3, 264): a row boundary inside a workgroup, 2f = 528 not a power of two
@pytest.mark.parametrize("rows,f", [(1, 8), (3, 264)])
def test_swiglu_packed(dev, rows, f):
    from torchft_amd.ops import swiglu_glu

    gu = _randn(dev, rows, 2 * f, seed=11).requires_grad_(True)
    dy = _randn(dev, rows, f, seed=12)
    y = swiglu_glu(gu)
    assert y.shape == (rows, f)
    y.backward(dy)
    g = gu.detach()
    mc.check_swiglu_fwd(f"swiglu_glu ({rows}, {f})", y.detach(), g[:, :f].contiguous(),
                        g[:, f:].contiguous())
    mc.check_swiglu_glu_bwd(f"swiglu_glu ({rows}, {f})", gu.grad, dy, g)


# ---------------------------------------------------------------- the argument rule

# binding -> call; the tensors go in by position, in _valid_args' order
CALLS = {
    "rmsnorm_fwd": lambda e, x, w: e.rmsnorm_fwd(x, w, EPS),
    "rmsnorm_bwd": lambda e, dy, x, w, invrms: e.rmsnorm_bwd(dy, x, w, invrms),
    "rope_apply": lambda e, x, cos_tab, sin_tab: e.rope_apply(x, cos_tab, sin_tab, False),
    "swiglu_fwd": lambda e, a, b: e.swiglu_fwd(a, b),
    "swiglu_bwd": lambda e, dy, a, b: e.swiglu_bwd(dy, a, b),
    "swiglu_glu_fwd": lambda e, gu: e.swiglu_glu_fwd(gu),
    "swiglu_glu_bwd": lambda e, dy, gu: e.swiglu_glu_bwd(dy, gu),
}


def _valid_args(dev, name):
    """Fresh, contiguous, valid arguments of binding `name`, by argument name.
    No dimension is 1, so every tensor has a non-contiguous twin. Two RMSNorm
    rows: each dw column is one atomic add per row onto zero, and a two-term
    sum does not depend on the order."""
    from torchft_amd.ops import rope_tables

    rows, H = 2, 16
    if name.startswith("rmsnorm"):
        x, w = _randn(dev, rows, H, seed=20), _randn(dev, H, seed=21)
        if name == "rmsnorm_fwd":
            return dict(x=x, w=w)
        invrms = torch.rsqrt(x.float().pow(2).mean(-1) + EPS)
        return dict(dy=_randn(dev, rows, H, seed=22), x=x, w=w, invrms=invrms)
    if name == "rope_apply":
        cos, sin = rope_tables(4, 8, device=dev)
        return dict(x=_randn(dev, 2, 3, 2, 8, seed=23), cos_tab=cos, sin_tab=sin)
    if name == "swiglu_fwd":
        return dict(a=_randn(dev, 4, 16, seed=24), b=_randn(dev, 4, 16, seed=25))
    if name == "swiglu_bwd":
        return dict(dy=_randn(dev, 4, 16, seed=26), a=_randn(dev, 4, 16, seed=24),
                    b=_randn(dev, 4, 16, seed=25))
    if name == "swiglu_glu_fwd":
        return dict(gu=_randn(dev, 4, 32, seed=27))
    assert name == "swiglu_glu_bwd"
    return dict(dy=_randn(dev, 4, 16, seed=28), gu=_randn(dev, 4, 32, seed=27))


def _call(ext, name, args):
    return CALLS[name](ext, *args.values())


def _strided(t):
    """The values of t behind strides that are not contiguous."""
    if t.dim() == 1:
        s = torch.stack([t, torch.zeros_like(t)], dim=1)[:, 0]
    else:
        s = t.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not s.is_contiguous() and torch.equal(s, t)
    return s


def _off_boundary(t):
    """A contiguous view of t's values one element into a fresh buffer."""
    buf = torch.zeros(t.numel() + 9, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("name", list(CALLS))
def test_any_layout_gives_the_bits_of_a_contiguous_copy(dev, ext, name):
    args = _valid_args(dev, name)
    want = _call(ext, name, args)
    got = _call(ext, name, {k: _strided(t) for k, t in args.items()})
    _assert_same_bits(got, want)
    for o in got if isinstance(got, (list, tuple)) else [got]:
        assert o.is_contiguous()


@pytest.mark.parametrize("name,arg", [
    ("rmsnorm_fwd", "x"), ("rope_apply", "x"), ("swiglu_fwd", "a"),
    ("swiglu_bwd", "dy"), ("swiglu_glu_bwd", "dy"), ("rope_apply", "cos_tab"),
])
def test_view_off_a_16_byte_boundary_gives_the_bits_of_a_copy(dev, ext, name, arg):
    args = _valid_args(dev, name)
    want = _call(ext, name, args)
    got = _call(ext, name, dict(args, **{arg: _off_boundary(args[arg])}))
    _assert_same_bits(got, want)


def test_zero_sized_inputs_launch_nothing(dev, ext):
    def empty(*shape, dtype=BF16):
        return torch.empty(*shape, device=dev, dtype=dtype)

    w = _randn(dev, 8, seed=30)
    y, invrms = ext.rmsnorm_fwd(empty(0, 8), w, EPS)
    assert y.shape == (0, 8) and y.dtype == BF16
    assert invrms.shape == (0,) and invrms.dtype == torch.float32
    dx, dw = ext.rmsnorm_bwd(empty(0, 8), empty(0, 8), w, invrms)
    assert dx.shape == (0, 8) and dx.dtype == BF16
    assert dw.dtype == torch.float32 and torch.equal(dw, torch.zeros(8, device=dev))

    out = ext.swiglu_fwd(empty(0), empty(0))
    assert out.shape == (0,) and out.dtype == BF16
    da, db = ext.swiglu_bwd(empty(0), empty(0), empty(0))
    assert da.shape == (0,) and db.shape == (0,) and da.dtype == BF16

    out = ext.swiglu_glu_fwd(empty(0, 16))
    assert out.shape == (0, 8) and out.dtype == BF16
    dgu = ext.swiglu_glu_bwd(empty(0, 8), empty(0, 16))
    assert dgu.shape == (0, 16) and dgu.dtype == BF16

    cos = torch.ones(3, 4, device=dev)
    out = ext.rope_apply(empty(0, 3, 1, 8), cos, cos, False)
    assert out.shape == (0, 3, 1, 8) and out.dtype == BF16

    torch.cuda.synchronize()
    assert (torch.ones(4, device=dev) + 1).sum().item() == 8.0


H_MAX = 40952  # the largest H rmsnorm_bwd accepts (kernels.h)


def _rmsnorm_bwd_args(dev, H):
    z = torch.zeros(2, H, device=dev, dtype=BF16)
    return dict(dy=z, x=z, w=z[0], invrms=torch.ones(2, device=dev))


def _refusals(dev):
    """(binding, argument named in the message, arguments) of every refusal."""
    def args(name, **changed):
        return dict(_valid_args(dev, name), **changed)

    x12 = _randn(dev, 2, 12, seed=40)
    return [
        ("rope_apply", "cos_tab", args("rope_apply", cos_tab=torch.ones(4, 4))),
        ("rope_apply", "sin_tab", args("rope_apply", sin_tab=torch.ones(4, 3, device=dev))),
        ("rmsnorm_bwd", "dy",
         args("rmsnorm_bwd", dy=_randn(dev, 2, 16, seed=41, dtype=torch.float16))),
        ("rmsnorm_bwd", "invrms", args("rmsnorm_bwd", invrms=torch.ones(1, device=dev))),
        ("rmsnorm_fwd", "w", args("rmsnorm_fwd", w=_randn(dev, 24, seed=42))),
        ("swiglu_fwd", "b", args("swiglu_fwd", b=_randn(dev, 56, seed=43))),
        ("swiglu_glu_bwd", "dy", args("swiglu_glu_bwd", dy=_randn(dev, 4, 32, seed=44))),
        ("rmsnorm_fwd", "x", dict(x=x12, w=_randn(dev, 12, seed=45))),
        ("swiglu_glu_fwd", "gu", dict(gu=_randn(dev, 4, 17, seed=46))),
        ("rmsnorm_fwd", "x", args("rmsnorm_fwd", x=torch.ones(2, 16, device=dev))),
        # dw[H] and the 16 static bytes of the block reduction fill the LDS at H_MAX
        # the first H past the limit, which is 40960 and named in the message,
        # and one further out
        ("rmsnorm_bwd", "x", _rmsnorm_bwd_args(dev, H_MAX + 16)),
        ("rmsnorm_bwd", "40960", _rmsnorm_bwd_args(dev, H_MAX + 8)),
    ]


REFUSAL_IDS = ["cpu-cos_tab", "sin_tab-one-column-short", "fp16-dy", "invrms-rows-minus-1",
               "w-H-plus-8", "b-8-short", "dy-full-2f-width", "H-12", "odd-gu", "fp32-x",
               "H_MAX-plus-16", "H-40960"]


@pytest.mark.parametrize("case", range(len(REFUSAL_IDS)), ids=REFUSAL_IDS)
def test_refusals_name_the_binding_and_the_argument(dev, ext, case):
    name, arg, args = _refusals(dev)[case]
    with pytest.raises(RuntimeError, match=rf"{name}: .*\b{arg}\b"):
        _call(ext, name, args)
    torch.cuda.synchronize()
