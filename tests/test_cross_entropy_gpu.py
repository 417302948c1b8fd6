"""GPU tests of the fused cross-entropy kernel
(csrc/kernels/fused_cross_entropy.hip) and of ``linear_cross_entropy`` on
the device.

Ground truth is the same definition (``cross_entropy_ref``) evaluated in
fp64 from the same bf16 logits. The bounds are derived, not tuned:

* row loss: ``4 * eps_fp32 * max(max|x|, |row_loss_ref|)`` — a few fp32 ulps
  at the magnitude the subtraction happens at;
* gradient: ``|g - g_ref| <= 2**-8 * |g_ref| + F`` — one correctly rounded
  bf16 store and the fp32 part ``F`` derived in tests/ce_check.py, which
  tests/test_cross_entropy_numerics_gpu.py holds the kernel to at its edges.

Every check prints its worst figure as a fraction of its bound before it
asserts.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

from ce_check import Bounds

pytestmark = pytest.mark.gpu

IGNORE = -100
EPS32 = torch.finfo(torch.float32).eps


def setup_module(module):
    if torch.cuda.is_available():
        torch.cuda.init()


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _kernel(logits, targets, *, z_loss=0.0, grad_scale=1.0, write_grad=True):
    from torchft_amd.ops.cross_entropy import fused_cross_entropy_

    gs = torch.full((1,), grad_scale, dtype=torch.float32, device=logits.device)
    return fused_cross_entropy_(
        logits, targets, ignore_index=IGNORE, z_loss=z_loss, grad_scale=gs,
        write_grad=write_grad,
    )


@functools.lru_cache(maxsize=None)
def _case(R, V, sigma=4.0, seed=0):
    """Seeded bf16 logits [R, V] ~ N(0, sigma^2) on the device and targets
    that force column 0, column V-1 and one ignored row (as far as R
    allows). Cached: callers clone the logits and never write to these."""
    g = torch.Generator().manual_seed(seed + 1000 * R + V)
    x = (torch.randn(R, V, generator=g) * sigma).to(torch.bfloat16).cuda()
    t = torch.randint(0, V, (R,), generator=g)
    if R == 1:
        t[0] = V - 1
    else:
        t[0] = 0
        t[1] = V - 1
    if R >= 3:
        t[2] = IGNORE
    return x, t.cuda()


def _truth(x, t, z_loss, grad_scale):
    from torchft_amd.ops.cross_entropy import cross_entropy_ref

    return cross_entropy_ref(x.double(), t, IGNORE, z_loss, grad_scale)


def _check(x, t, row_loss, grad, z_loss, grad_scale, rows=None, tag=""):
    ref_loss, ref_grad = _truth(x, t, z_loss, grad_scale)
    if rows is None:
        rows = torch.arange(x.shape[0], device=x.device)
    xd = x.double()
    xmax = torch.where(torch.isfinite(xd), xd.abs(), torch.zeros_like(xd)).amax(dim=1)
    loss_bound = 4 * EPS32 * torch.maximum(xmax, ref_loss.abs())
    loss_err = (row_loss.double() - ref_loss).abs()
    grad_bound = Bounds(x, t, z_loss, grad_scale).grad_bound.to(x.device)
    grad_err = (grad.double() - ref_grad).abs()
    lf = (loss_err[rows] / loss_bound[rows]).max().item()
    gf = (grad_err[rows] / grad_bound[rows]).max().item()
    print(
        f"{tag} shape={tuple(x.shape)} z={z_loss} gs={grad_scale}: "
        f"loss err/bound={lf:.3f} grad err/bound={gf:.3f}"
    )
    assert torch.isfinite(row_loss[rows]).all() and torch.isfinite(grad[rows]).all()
    assert lf <= 1.0, f"row loss off by {lf:.3f} x bound"
    assert gf <= 1.0, f"gradient off by {gf:.3f} x bound"


class TestKernel:
    @pytest.mark.parametrize(
        "R,V",
        [
            (5, 40),  # narrower than a workgroup
            (5, 1003),  # V % 8 != 0: misaligned rows, head and tail
            (33, 4096),  # exact multiple
            (4, 128256),  # the real vocab, partial last iteration
            (1, 8),  # the smallest vector row
        ],
    )
    def test_shapes(self, dev, R, V):
        x, t = _case(R, V)
        buf = x.clone()
        row_loss = _kernel(buf, t)
        assert row_loss.dtype == torch.float32 and row_loss.shape == (R,)
        if R >= 3:
            assert row_loss[2].item() == 0.0
            assert torch.count_nonzero(buf[2]).item() == 0
        _check(x, t, row_loss, buf, 0.0, 1.0, tag="shapes")

    @pytest.mark.parametrize("z_loss,grad_scale", [(1e-4, 1.0), (0.0, 1.0 / 29), (1e-4, 0.37)])
    def test_z_loss_and_grad_scale(self, dev, z_loss, grad_scale):
        x, t = _case(33, 4096)
        buf = x.clone()
        row_loss = _kernel(buf, t, z_loss=z_loss, grad_scale=grad_scale)
        _check(x, t, row_loss, buf, z_loss, grad_scale, tag="z/gs")

    @pytest.mark.parametrize("z_loss", [0.0, 1e-4])
    def test_extremes(self, dev, z_loss):
        x, t = _case(6, 1003, sigma=3000.0, seed=7)
        x = x.clone()
        x[4, 100:700] = float("-inf")
        t = t.clone()
        t[4] = 50
        buf = x.clone()
        row_loss = _kernel(buf, t, z_loss=z_loss)
        assert torch.isfinite(row_loss).all() and torch.isfinite(buf).all()
        assert torch.count_nonzero(buf[4, 100:700]).item() == 0
        _check(x, t, row_loss, buf, z_loss, 1.0, tag="extremes")

    def test_out_of_range_target_is_nan(self, dev):
        # the bad target sits in a non-last row on purpose: x[V] of that row
        # is inside the allocation whatever the kernel does with it
        V = 1003
        x, t = _case(4, V, seed=3)
        t = t.clone()
        t[1] = V
        buf = x.clone()
        row_loss = _kernel(buf, t)
        assert torch.isnan(row_loss[1]).item()
        keep = torch.tensor([0, 2, 3], device=dev)
        _check(x, t, row_loss, buf, 0.0, 1.0, rows=keep, tag="oob")

    @pytest.mark.parametrize("R,V", [(5, 1003), (4, 128256)])
    def test_loss_only_leaves_logits(self, dev, R, V):
        x, t = _case(R, V)
        buf = x.clone()
        with_grad = _kernel(buf, t, z_loss=1e-4)
        buf2 = x.clone()
        loss_only = _kernel(buf2, t, z_loss=1e-4, write_grad=False)
        assert torch.equal(loss_only, with_grad)
        assert torch.equal(buf2.view(torch.int16), x.view(torch.int16))

    def test_bitwise_reproducible(self, dev):
        x, t = _case(4, 128256)
        a, b = x.clone(), x.clone()
        la = _kernel(a, t, z_loss=1e-4, grad_scale=0.37)
        lb = _kernel(b, t, z_loss=1e-4, grad_scale=0.37)
        assert torch.equal(la, lb)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))

    def test_non_contiguous_logits_raise(self, dev):
        x, t = _case(5, 40)
        with pytest.raises(RuntimeError):
            _kernel(x.clone()[:, ::2], t)
        with pytest.raises(RuntimeError):
            _kernel(x.clone().t()[:5], t)


def _unfused_head(h, w, t, chunk_rows):
    """The loop ``Llama.forward_loss`` runs without the fused head."""
    n = h.shape[0]
    losses = []
    for i in range(0, n, chunk_rows):
        logits = F.linear(h[i : i + chunk_rows], w)
        losses.append(
            F.cross_entropy(logits, t[i : i + chunk_rows], reduction="sum").float()
        )
    return torch.stack(losses).sum() / n


class TestLinearCrossEntropy:
    def test_matches_fp32_and_beats_unfused(self, dev):
        from torchft_amd.ops import linear_cross_entropy

        N, D, V, chunk = 300, 256, 1003, 128
        g = torch.Generator().manual_seed(11)
        h = torch.randn(N, D, generator=g).to(torch.bfloat16).to(dev)
        w = (torch.randn(V, D, generator=g) * D**-0.5).to(torch.bfloat16).to(dev)
        t = torch.randint(0, V, (N,), generator=g).to(dev)

        hr = h.float().requires_grad_(True)
        wr = w.float().requires_grad_(True)
        ref = F.cross_entropy(F.linear(hr, wr), t)
        ref.backward()

        ha = h.clone().requires_grad_(True)
        wa = w.clone().requires_grad_(True)
        loss = linear_cross_entropy(ha, wa, t, chunk_rows=chunk)
        loss.backward()
        assert loss.dtype == torch.float32
        assert ha.grad.dtype == torch.bfloat16 and wa.grad.dtype == torch.bfloat16

        with torch.no_grad():
            unfused = _unfused_head(h, w, t, chunk)
        e_fused = (loss.detach() - ref.detach()).abs().item()
        e_unfused = (unfused - ref.detach()).abs().item()
        print(
            f"loss ref={ref.item():.6f} fused err={e_fused:.3e} "
            f"unfused err={e_unfused:.3e}"
        )
        torch.testing.assert_close(loss.detach(), ref.detach(), rtol=2e-3, atol=0)
        for name, got, want in (("dh", ha.grad, hr.grad), ("dW", wa.grad, wr.grad)):
            err = (got.float() - want).abs().max().item()
            print(f"{name}: max err={err:.3e} max|ref|={want.abs().max().item():.3e}")
            torch.testing.assert_close(
                got.float(), want, rtol=3e-2, atol=3e-2 * want.abs().max().item()
            )
        assert e_fused <= e_unfused

    def test_bounded_memory(self, dev):
        from torchft_amd.ops import linear_cross_entropy

        N, D, V, chunk = 4096, 256, 16384, 512
        MB = 1 << 20
        assert N * V * 2 == 128 * MB
        g = torch.Generator().manual_seed(12)
        h = torch.randn(N, D, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
        w = (torch.randn(V, D, generator=g) * D**-0.5).to(torch.bfloat16).to(dev)
        w.requires_grad_(True)
        t = torch.randint(0, V, (N,), generator=g).to(dev)

        def peak_over_baseline(head):
            def step():
                head().backward()
                h.grad = w.grad = None

            step()  # warm-up: GEMM workspaces, code objects
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step()
            torch.cuda.synchronize()
            return torch.cuda.max_memory_allocated() - base

        fused = peak_over_baseline(lambda: linear_cross_entropy(h, w, t, chunk_rows=chunk))
        unfused = peak_over_baseline(lambda: _unfused_head(h, w, t, chunk))
        print(f"peak over baseline: fused {fused / MB:.1f} MB, unfused {unfused / MB:.1f} MB")
        assert fused < 64 * MB
        assert unfused >= 128 * MB

    def test_llama_debug_bf16(self, dev):
        from torchft_amd.models.llama import LLAMA_DEBUG, Llama

        torch.manual_seed(0)
        model = Llama(LLAMA_DEBUG, dtype=torch.bfloat16, checkpoint_activations=False)
        model = model.to(dev).train()
        toks = torch.randint(0, LLAMA_DEBUG.vocab_size, (2, 129), device=dev)
        x, y = toks[:, :-1].contiguous(), toks[:, 1:].contiguous()
        y[0, :16] = IGNORE
        loss = model.forward_loss(x, y, chunk_rows=100, fused=True)
        loss.backward()
        assert loss.dtype == torch.float32 and torch.isfinite(loss).item()
        for n, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
        with torch.no_grad():
            hid = model.forward_hidden(x).reshape(-1, LLAMA_DEBUG.dim)
            ref = F.cross_entropy(
                F.linear(hid.float(), model.output.weight.float()), y.reshape(-1),
                ignore_index=IGNORE,
            )
        print(f"llama debug loss fused={loss.item():.6f} fp32 ref={ref.item():.6f}")
        torch.testing.assert_close(loss.detach(), ref, rtol=2e-3, atol=0)
