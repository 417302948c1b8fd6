"""GPU tests for the global-norm kernels (csrc/kernels/grad_norm.hip) and
FusedAdamW's clip mode (adamw_kernel<true>, adamw_bump_steps_kernel).

Norm bound: every summand g*g is non-negative, so the relative error of the
fp32 sum of squares is at most depth * 2^-24, depth being the longest fp32
addition chain: 8 adds per logical 2048-element block a workgroup visits
(ceil(blocks / grid) of them), 6 shuffle steps and 3 wave adds; the partials
are summed in double. The square root halves the relative error, so the norm
is held to |norm - ref| / ref <= depth * 2^-24 (twice the bound, as margin
for the two fp32 roundings of the result).
"""

import math

import pytest
import torch

from grad_norm_check import depth as _depth

pytestmark = pytest.mark.gpu

HP = dict(lr=1e-2, betas=(0.9, 0.95), weight_decay=0.01, eps=1e-8)
SHAPES = [(5000,), (100, 33)]  # as TestFusedAdamW
BF16_ULP = dict(rtol=2**-7, atol=0)


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _ref_norm(tensors):
    return math.sqrt(sum(float(t.double().pow(2).sum()) for t in tensors))


def _check_norm(norm, tensors, depth):
    ref = _ref_norm(tensors)
    err = abs(float(norm.double()) - ref) / ref
    bound = depth * 2.0**-24
    print(f"grad_norm rel err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert err <= bound, (err, bound)


class TestGradNorm:
    def test_bf16_zoo_in_one_call(self, dev):
        from torchft_amd import ops

        torch.manual_seed(0)
        shapes = [(1,), (7,), (8,), (2047,), (2048,), (2049,), (5000,), (100, 33)]
        ts = [torch.randn(*s, device=dev).bfloat16() for s in shapes]
        n = ops.grad_norm(ts)
        assert n.dim() == 0 and n.dtype == torch.float32 and n.is_cuda
        _check_norm(n, ts, _depth([t.numel() for t in ts]))

    def test_misaligned_view(self, dev):
        from torchft_amd import ops

        torch.manual_seed(1)
        buf = torch.randn(4100, device=dev).bfloat16()
        view = buf[1:4098]
        assert view.data_ptr() % 16 != 0
        _check_norm(ops.grad_norm([view]), [view], _depth([view.numel()]))

    def test_fp32(self, dev):
        from torchft_amd import ops

        torch.manual_seed(2)
        t = torch.randn(3001, device=dev)
        _check_norm(ops.grad_norm([t]), [t], _depth([3001]))

    def test_mixed_dtypes_and_params(self, dev):
        from torchft_amd import ops

        torch.manual_seed(3)
        a = torch.randn(2500, device=dev).bfloat16()
        b = torch.randn(700, device=dev)
        p = torch.zeros(9, device=dev, requires_grad=True)
        p.grad = torch.randn(9, device=dev)
        no_grad = torch.zeros(4, device=dev, requires_grad=True)
        n = ops.grad_norm([a, b, p, no_grad])
        # one reduction per dtype, each a single block per workgroup
        _check_norm(n, [a, b, p.grad], 8 + 6 + 3)

    def test_grid_stride_and_multi_partial_finalize(self, dev):
        from torchft_amd import ops

        torch.manual_seed(4)
        t = torch.randn(40_000, device=dev).bfloat16()
        depth = _depth([40_000], max_blocks=3)
        assert depth == 8 * 7 + 9  # 20 blocks over 3 workgroups
        _check_norm(ops.grad_norm([t], max_blocks=3), [t], depth)

    def test_bitwise_reproducible(self, dev):
        from torchft_amd import ops

        torch.manual_seed(5)
        ts = [torch.randn(n, device=dev).bfloat16() for n in (40_000, 2049, 7)]
        for mb in (3, 2048):
            a = ops.grad_norm(ts, max_blocks=mb)
            b = ops.grad_norm(ts, max_blocks=mb)
            assert torch.equal(a, b)

    def test_norm_reduce_sees_the_sum_of_squares(self, dev):
        from torchft_amd import ops

        torch.manual_seed(6)
        t = torch.randn(5000, device=dev).bfloat16()
        seen = []

        def reduce(s):
            seen.append((tuple(s.shape), s.dtype, s.is_cuda))
            s.mul_(4)

        n = ops.grad_norm([t])
        n2 = ops.grad_norm([t], norm_reduce=reduce)
        assert seen == [((1,), torch.float32, True)]
        assert float(n2) == 2 * float(n)


def _bf16_params(dev, seed):
    torch.manual_seed(seed)
    return [torch.randn(*s, device=dev, dtype=torch.bfloat16, requires_grad=True)
            for s in SHAPES]


def _clones(ps, dtype=None):
    return [p.detach().to(dtype or p.dtype).clone().requires_grad_(True) for p in ps]


def _rand_grads(dev, scale):
    return [(torch.randn(*s, device=dev) * scale).bfloat16() for s in SHAPES]


def _set_grads(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = g.to(p.dtype).clone()


def _ref_step(ref, ref_opt, grads, max_norm):
    _set_grads(ref, grads)
    torch.nn.utils.clip_grad_norm_(ref, max_norm)
    ref_opt.step()


def _bits(t):
    return t.detach().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class TestFusedAdamWClip:
    def test_inf_max_norm_matches_plain_kernel(self, dev):
        from torchft_amd.ops import FusedAdamW

        a = _bf16_params(dev, 10)
        b = _clones(a)
        plain = FusedAdamW(a, **HP)
        clip = FusedAdamW(b, max_grad_norm=math.inf, **HP)
        for _ in range(5):
            grads = _rand_grads(dev, 1.0)
            _set_grads(a, grads)
            _set_grads(b, grads)
            plain.step()
            clip.step()
        for pa, pb, g in zip(a, b, grads):
            # a coefficient of exactly 1.0 changes no bit of the moments
            assert torch.equal(plain.state[pa]["exp_avg"], clip.state[pb]["exp_avg"])
            assert torch.equal(plain.state[pa]["exp_avg_sq"],
                               clip.state[pb]["exp_avg_sq"])
            # device powf vs host pow in the bias correction: one bf16 ulp
            torch.testing.assert_close(pb.float(), pa.float(), **BF16_ULP)
            step = clip.state[pb]["step"]
            assert step.dtype == torch.int32 and step.dim() == 0 and step.is_cuda
            assert int(step) == 5 and plain.state[pa]["step"] == 5
        _check_norm(clip.last_grad_norm, grads, _depth([g.numel() for g in grads]))
        assert int(clip.skipped_steps) == 0

    def test_clip_matches_fp32_clip_then_adamw(self, dev):
        from torchft_amd.ops import FusedAdamW

        ps = _bf16_params(dev, 11)
        ref = _clones(ps, torch.float32)
        opt = FusedAdamW(ps, max_grad_norm=0.5, **HP)
        ref_opt = torch.optim.AdamW(ref, **HP)
        norms = []
        # 8300 randn elements: norm ~91; scaled by 1e-3, ~0.09
        for scale in (1.0, 1e-3, 1.0, 1e-3, 1.0):
            grads = _rand_grads(dev, scale)
            _set_grads(ps, grads)
            opt.step()
            norms.append(float(opt.last_grad_norm))
            _ref_step(ref, ref_opt, grads, 0.5)
        assert any(n > 0.5 for n in norms) and any(n < 0.5 for n in norms), norms
        for p, r in zip(ps, ref):
            torch.testing.assert_close(p.float(), r.detach(), rtol=2e-2, atol=2e-2)

    def test_nonfinite_grads_skip_on_device(self, dev):
        from torchft_amd.ops import FusedAdamW

        ps = _bf16_params(dev, 12)
        ref = _clones(ps, torch.float32)
        opt = FusedAdamW(ps, max_grad_norm=0.5, **HP)
        ref_opt = torch.optim.AdamW(ref, **HP)
        for scale in (1.0, 1e-3):
            grads = _rand_grads(dev, scale)
            _set_grads(ps, grads)
            opt.step()
            _ref_step(ref, ref_opt, grads, 0.5)

        before = [
            (_bits(p).clone(), opt.state[p]["exp_avg"].clone(),
             opt.state[p]["exp_avg_sq"].clone())
            for p in ps
        ]
        for skipped, bad in ((1, math.inf), (2, math.nan)):
            grads = _rand_grads(dev, 1.0)
            grads[1][50, 7] = bad
            _set_grads(ps, grads)
            opt.step()
            for p, (p0, m0, v0) in zip(ps, before):
                assert torch.equal(_bits(p), p0)
                assert torch.equal(_bits(opt.state[p]["exp_avg"]), _bits(m0))
                assert torch.equal(_bits(opt.state[p]["exp_avg_sq"]), _bits(v0))
                assert int(opt.state[p]["step"]) == 2
            assert int(opt.skipped_steps) == skipped
            assert not math.isfinite(float(opt.last_grad_norm))

        grads = _rand_grads(dev, 1.0)
        _set_grads(ps, grads)
        opt.step()
        _ref_step(ref, ref_opt, grads, 0.5)
        for p, r in zip(ps, ref):
            torch.testing.assert_close(p.float(), r.detach(), rtol=2e-2, atol=2e-2)
            assert int(opt.state[p]["step"]) == 3
        assert int(opt.skipped_steps) == 2
        assert math.isfinite(float(opt.last_grad_norm))

    def test_grad_none_mix_keeps_per_tensor_steps(self, dev):
        from torchft_amd.ops import FusedAdamW

        ps = _bf16_params(dev, 13)
        ref = _clones(ps, torch.float32)
        opt = FusedAdamW(ps, max_grad_norm=0.5, **HP)
        ref_opt = torch.optim.AdamW(ref, **HP)
        for it in range(5):
            grads = _rand_grads(dev, 1e-3 if it == 1 else 1.0)
            for params, o in ((ps, opt), (ref, ref_opt)):
                params[0].grad = grads[0].to(params[0].dtype).clone()
                # the second param only gets a grad on even iterations
                params[1].grad = (grads[1].to(params[1].dtype).clone()
                                  if it % 2 == 0 else None)
                if o is ref_opt:
                    torch.nn.utils.clip_grad_norm_(params, 0.5)
                o.step()
                o.zero_grad(set_to_none=True)
        assert int(opt.state[ps[0]]["step"]) == 5
        assert int(opt.state[ps[1]]["step"]) == 3
        for p, r in zip(ps, ref):
            torch.testing.assert_close(p.float(), r.detach(), rtol=2e-2, atol=2e-2)

    def test_param_groups_share_one_norm(self, dev):
        from torchft_amd.ops import FusedAdamW

        ps = _bf16_params(dev, 14)
        ref = _clones(ps, torch.float32)
        hp = {k: v for k, v in HP.items() if k != "lr"}
        opt = FusedAdamW([{"params": [ps[0]], "lr": 1e-2},
                          {"params": [ps[1]], "lr": 3e-2, "weight_decay": 0.0}],
                         max_grad_norm=0.5, **hp)
        ref_opt = torch.optim.AdamW([{"params": [ref[0]], "lr": 1e-2},
                                     {"params": [ref[1]], "lr": 3e-2,
                                      "weight_decay": 0.0}], **hp)
        for _ in range(3):
            grads = _rand_grads(dev, 1.0)
            _set_grads(ps, grads)
            opt.step()
            _ref_step(ref, ref_opt, grads, 0.5)
        _check_norm(opt.last_grad_norm, grads, _depth([g.numel() for g in grads]))
        for p, r in zip(ps, ref):
            torch.testing.assert_close(p.float(), r.detach(), rtol=2e-2, atol=2e-2)


class TestClipGradNorm:
    def test_matches_torch_on_fp32_clones(self, dev):
        from torchft_amd import ops

        ps = _bf16_params(dev, 20)
        ref = _clones(ps, torch.float32)
        grads = _rand_grads(dev, 1.0)
        _set_grads(ps, grads)
        _set_grads(ref, grads)
        n = ops.clip_grad_norm_(ps, 0.5)
        torch.nn.utils.clip_grad_norm_(ref, 0.5)
        assert n.dim() == 0 and n.dtype == torch.float32 and n.is_cuda
        _check_norm(n, grads, _depth([g.numel() for g in grads]))
        for p, r, g in zip(ps, ref, grads):
            assert not torch.equal(p.grad, g)
            torch.testing.assert_close(p.grad.float(), r.grad, **BF16_ULP)

    def test_below_threshold_and_nan_leave_grads_alone(self, dev):
        from torchft_amd import ops

        ps = _bf16_params(dev, 21)
        grads = _rand_grads(dev, 1e-3)
        _set_grads(ps, grads)
        n = ops.clip_grad_norm_(ps, 0.5)
        assert float(n) < 0.5
        for p, g in zip(ps, grads):
            assert torch.equal(_bits(p.grad), _bits(g))

        grads = _rand_grads(dev, 1.0)
        grads[0][1234] = math.nan
        _set_grads(ps, grads)
        n = ops.clip_grad_norm_(ps, 0.5)
        assert math.isnan(float(n))
        for p, g in zip(ps, grads):
            assert torch.equal(_bits(p.grad), _bits(g))
