"""GPU tests of what the shared multi-tensor addressing (csrc/kernels/
multi_tensor.h, the table builder of bindings.cpp) gives FusedAdamW and the
fp8 pack: FusedAdamW sends tensors off a 16 B boundary down the element path
with the same bits, the fp8 pack refuses them, zero-numel tensors cost
nothing, and every binding validates alike. Everything here is bitwise: no
path reorders an operation."""

import pytest
import torch

pytestmark = pytest.mark.gpu

HP = dict(lr=1e-2, betas=(0.9, 0.95), weight_decay=0.01, eps=1e-8)
MODES = [None, 0.5]  # plain step, clip mode with an active coefficient
PAD = 8  # elements kept around a misaligned view


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _bits(t):
    t = t.detach()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _misaligned(values):
    """(buffer, view): the view holds `values` one element into the buffer."""
    n = values.numel()
    buf = torch.full((n + 1 + PAD,), 3.0, device=values.device, dtype=values.dtype)
    view = buf[1:1 + n]
    view.copy_(values)
    assert view.data_ptr() % 16 != 0
    return buf, view


def _assert_padding_untouched(buf, n):
    assert torch.all(buf[0] == 3.0) and torch.all(buf[1 + n:] == 3.0)


def _adamw_run(params, grads_per_step, max_grad_norm):
    """Steps FusedAdamW over leaf tensors `params`; returns (p, m, v) bits."""
    from torchft_amd.ops import FusedAdamW

    kw = dict(HP) if max_grad_norm is None else dict(HP, max_grad_norm=max_grad_norm)
    opt = FusedAdamW(params, **kw)
    for grads in grads_per_step:
        for p, g in zip(params, grads):
            p.grad = g
        opt.step()
    torch.cuda.synchronize()
    return [(_bits(p).clone(), _bits(opt.state[p]["exp_avg"]).clone(),
             _bits(opt.state[p]["exp_avg_sq"]).clone()) if p.numel() else None
            for p in params]


@pytest.mark.parametrize("max_grad_norm", MODES)
@pytest.mark.parametrize("n", [7, 2049])
def test_adamw_misaligned_views_match_aligned(dev, n, max_grad_norm):
    torch.manual_seed(n)
    p0 = torch.randn(n, device=dev).bfloat16()
    grads = [torch.randn(n, device=dev).bfloat16() for _ in range(3)]

    pbuf, pview = _misaligned(p0)
    gbufs = [_misaligned(g) for g in grads]
    got = _adamw_run([pview.requires_grad_(True)], [[gv] for _, gv in gbufs],
                     max_grad_norm)
    want = _adamw_run([p0.clone().requires_grad_(True)], [[g.clone()] for g in grads],
                      max_grad_norm)
    for a, b in zip(got[0], want[0]):
        assert torch.equal(a, b)
    _assert_padding_untouched(pbuf, n)
    for (gbuf, gview), g in zip(gbufs, grads):
        _assert_padding_untouched(gbuf, n)
        assert torch.equal(_bits(gview), _bits(g))


@pytest.mark.parametrize("max_grad_norm", MODES)
def test_adamw_with_zero_numel_parameter(dev, max_grad_norm):
    torch.manual_seed(3)
    shapes = [(5000,), (0,), (100, 33)]
    ps = [torch.randn(*s, device=dev).bfloat16() for s in shapes]
    grads = [[torch.randn(*s, device=dev).bfloat16() for s in shapes] for _ in range(3)]

    with_empty = [p.clone().requires_grad_(True) for p in ps]
    got = _adamw_run(with_empty, grads, max_grad_norm)
    want = _adamw_run([ps[0].clone().requires_grad_(True), ps[2].clone().requires_grad_(True)],
                      [[g[0], g[2]] for g in grads], max_grad_norm)
    assert got[1] is None
    for g, w in zip((got[0], got[2]), want):
        for a, b in zip(g, w):
            assert torch.equal(a, b)


@pytest.mark.parametrize("max_grad_norm", MODES)
def test_adamw_over_only_zero_numel_parameters(dev, max_grad_norm):
    from torchft_amd.ops import FusedAdamW

    ps = [torch.zeros(0, device=dev, dtype=torch.bfloat16, requires_grad=True),
          torch.zeros(0, 4, device=dev, dtype=torch.bfloat16, requires_grad=True)]
    kw = dict(HP) if max_grad_norm is None else dict(HP, max_grad_norm=max_grad_norm)
    opt = FusedAdamW(ps, **kw)
    for _ in range(2):
        for p in ps:
            p.grad = torch.zeros_like(p)
        opt.step()
    torch.cuda.synchronize()
    if max_grad_norm is not None:
        # a finite (zero) norm still advances an empty parameter's step count
        assert [int(opt.state[p]["step"]) for p in ps] == [2, 2]
        assert int(opt.skipped_steps) == 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", [7, 2049])
def test_fp8_pack_rejects_misaligned_views(dev, n, dtype):
    """The fp8 kernels have no element path for a tensor off a 16 B boundary
    (it would cost their aligned path 3-4 %), so the bindings refuse one
    before anything is launched: pack, view and its neighbours stay as they
    were. Aligned clones of the same values still go through."""
    from torchft_amd.ops import hip_ext
    from torchft_amd.quantization import allocate_pack

    world = 2
    torch.manual_seed(n)
    x = torch.randn(n, device=dev).to(dtype)
    buf, view = _misaligned(x)

    pack = allocate_pack([view], world).fill_(7)
    with pytest.raises(RuntimeError, match="16-byte boundary"):
        hip_ext().fp8_quantize([view], pack, world)
    with pytest.raises(RuntimeError, match="16-byte boundary"):
        hip_ext().fp8_quantize([x, view], allocate_pack([x, view], world), world)
    torch.cuda.synchronize()
    assert torch.all(pack == 7)

    hip_ext().fp8_quantize([x], pack, world)
    with pytest.raises(RuntimeError, match="16-byte boundary"):
        hip_ext().fp8_dequantize([view], pack, world)
    torch.cuda.synchronize()
    _assert_padding_untouched(buf, n)
    assert torch.equal(_bits(view), _bits(x))

    out = torch.zeros_like(x)
    hip_ext().fp8_dequantize([out], pack, world)
    assert out.abs().max() > 0


class TestValidation:
    def _lists(self, dev, n=64):
        p = torch.zeros(n, device=dev, dtype=torch.bfloat16)
        return [p], [torch.zeros_like(p)], [torch.zeros(n, device=dev)], \
            [torch.zeros(n, device=dev)]

    def _step(self, p, g, m, v):
        from torchft_amd.ops import hip_ext

        hip_ext().adamw_step(p, g, m, v, 1e-2, 0.9, 0.95, 1e-8, 0.01, 1)
        torch.cuda.synchronize()

    def test_adamw_step_rejects_fp32_gradient(self, dev):
        p, g, m, v = self._lists(dev)
        with pytest.raises(RuntimeError, match="mixed dtypes"):
            self._step(p, [g[0].float()], m, v)

    def test_adamw_step_rejects_numel_mismatch(self, dev):
        p, g, m, v = self._lists(dev)
        with pytest.raises(RuntimeError, match="size mismatch"):
            self._step(p, [torch.zeros(63, device=dev, dtype=torch.bfloat16)], m, v)
        with pytest.raises(RuntimeError, match="size mismatch"):
            self._step(p, g, m, [torch.zeros(65, device=dev)])
        with pytest.raises(RuntimeError, match="list lengths"):
            self._step(p, g + g, m, v)

    def test_adamw_step_rejects_cpu_tensor(self, dev):
        p, g, m, v = self._lists(dev)
        with pytest.raises(RuntimeError, match="one device"):
            self._step(p, [g[0].cpu()], m, v)

    def test_fp8_dequantize_rejects_mixed_dtypes(self, dev):
        from torchft_amd.ops import hip_ext
        from torchft_amd.quantization import allocate_pack

        ts = [torch.zeros(64, device=dev, dtype=torch.bfloat16),
              torch.zeros(64, device=dev, dtype=torch.float32)]
        pack = allocate_pack(ts, 1).zero_()
        with pytest.raises(RuntimeError, match="mixed dtypes"):
            hip_ext().fp8_dequantize(ts, pack, 1)
        with pytest.raises(RuntimeError, match="mixed dtypes"):
            hip_ext().fp8_quantize(ts, pack, 1)
