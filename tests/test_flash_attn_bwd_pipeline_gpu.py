"""Flash-attention backward, software-pipelined tile stream (GPU).

The smallest shapes at which the prefetch pipeline of fa_bwd_dkdv_kernel /
fa_bwd_dq_kernel can go wrong, each in the packed [B,H,S,D] layout and
through transpose views of [B,S,H,D] buffers:

* (1,2,2,128): one workgroup, waves 4-7 inactive, the shortest streams
  (dq T=2, dkdv T=4) — prologue, one prefetch, unguarded last tile;
* (1,4,1,384) causal: G=4, the dkdv prefetch crosses query heads; the
  second workgroup is half active and starts at i_min > 0;
* (2,8,2,512): several workgroups per head in both grid dimensions, batch
  stride;
* (1,4,2,1024) causal: every wave of the causal diagonal group, reversed dq
  block order over 4 blocks.

Checked per case: gradients against SDPA autograd on the same bf16 inputs
(the tolerances of test_flash_attn_gpu.py), and — the race detectors — the
two layouts and two repeated calls give bit-identical gradients.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128

CASES = [
    (1, 2, 2, 128, True),
    (1, 2, 2, 128, False),
    (1, 4, 1, 384, True),
    (2, 8, 2, 512, True),
    (2, 8, 2, 512, False),
    (1, 4, 2, 1024, True),
]


def _run(q, k, v, dout, causal, bshd):
    """out, dq, dk, dv (logical [B,H,S,D]) of the custom path in one layout."""
    from torchft_amd.ops.flash_attention import _FlashAttentionFn

    def leaf(t):
        if bshd:  # [B,S,H,D] storage, handed over as a transpose view
            return t.transpose(1, 2).contiguous().requires_grad_(True)
        return t.clone().requires_grad_(True)

    def view(t):
        return t.transpose(1, 2) if bshd else t

    ql, kl, vl = leaf(q), leaf(k), leaf(v)
    do = view(dout.transpose(1, 2).contiguous()) if bshd else dout
    out = _FlashAttentionFn.apply(view(ql), view(kl), view(vl), causal, D ** -0.5)
    out.backward(do)
    torch.cuda.synchronize()
    return (out.detach(),) + tuple(view(t.grad) for t in (ql, kl, vl))


@functools.lru_cache(maxsize=None)
def _results(B, Hq, Hkv, S, causal):
    """Everything the three assertions of one case need, computed once."""
    torch.manual_seed(41)
    dev = "cuda"
    q = torch.randn(B, Hq, S, D, device=dev, dtype=torch.bfloat16)
    k = torch.randn(B, Hkv, S, D, device=dev, dtype=torch.bfloat16)
    v = torch.randn(B, Hkv, S, D, device=dev, dtype=torch.bfloat16)
    dout = torch.randn(B, Hq, S, D, device=dev, dtype=torch.bfloat16)

    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref_out = torch.nn.functional.scaled_dot_product_attention(
        qr, kr, vr, is_causal=causal, enable_gqa=Hq != Hkv)
    ref_out.backward(dout)
    ref = (ref_out.detach(), qr.grad, kr.grad, vr.grad)

    packed = _run(q, k, v, dout, causal, bshd=False)
    packed_again = _run(q, k, v, dout, causal, bshd=False)
    bshd = _run(q, k, v, dout, causal, bshd=True)
    bshd_again = _run(q, k, v, dout, causal, bshd=True)
    return ref, packed, packed_again, bshd, bshd_again


@pytest.mark.parametrize("B,Hq,Hkv,S,causal", CASES)
class TestBwdPipeline:
    def test_matches_sdpa_autograd(self, B, Hq, Hkv, S, causal):
        ref, packed, _, bshd, _ = _results(B, Hq, Hkv, S, causal)
        for got in (packed, bshd):
            torch.testing.assert_close(got[0], ref[0], rtol=2e-2, atol=2e-2)
            for g, r in zip(got[1:], ref[1:]):
                torch.testing.assert_close(g, r, rtol=5e-2, atol=5e-2)

    def test_layouts_bit_identical(self, B, Hq, Hkv, S, causal):
        _, packed, _, bshd, _ = _results(B, Hq, Hkv, S, causal)
        for name, g, h in zip(("dq", "dk", "dv"), packed[1:], bshd[1:]):
            assert torch.equal(g, h), f"{name}: packed and [B,S,H,D] differ"

    def test_repeatable(self, B, Hq, Hkv, S, causal):
        _, packed, packed_again, bshd, bshd_again = _results(B, Hq, Hkv, S, causal)
        for name, g, h in zip(("dq", "dk", "dv"), packed[1:], packed_again[1:]):
            assert torch.equal(g, h), f"{name}: two packed calls differ"
        for name, g, h in zip(("dq", "dk", "dv"), bshd[1:], bshd_again[1:]):
            assert torch.equal(g, h), f"{name}: two [B,S,H,D] calls differ"
