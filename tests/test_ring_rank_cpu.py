"""``cp.ring_rank_attention`` and ``ops.flash_attention_fold`` on the CPU (their
torch paths), fp32, against one-shot attention over the whole key range at the
tolerance tests/test_cp.py::TestRingAttention uses."""

import pytest
import torch
import torch.nn.functional as F

from torchft_amd.ops import flash_attention_fold
from torchft_amd.parallel.cp import ring_rank_attention

TOL = dict(rtol=2e-4, atol=2e-4)
B, S, D, s = 2, 64, 32, 32


def _inputs(Hq, Hkv):
    torch.manual_seed(5)
    return (torch.randn(B, Hq, s, D), torch.randn(B, Hkv, S, D), torch.randn(B, Hkv, S, D),
            torch.randn(B, Hq, s, D))


def _rank1_reference(q, k, v):
    """Rank 1 of world 2: the last s rows of causal attention over S keys."""
    mask = torch.ones(s, S, dtype=torch.bool).tril_(S - s)
    return F.scaled_dot_product_attention(q, k, v, attn_mask=mask, enable_gqa=True)


@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (4, 2)], ids=["mha", "gqa"])
def test_ring_rank_attention(Hq, Hkv):
    q, k, v, g = _inputs(Hq, Hkv)
    want, got = [], []
    for fn, dst in ((_rank1_reference, want),
                    # hop order: the rank's own block (causal), then block 0
                    (lambda q_, k_, v_: ring_rank_attention(
                        q_, [k_[:, :, s:], k_[:, :, :s]], [v_[:, :, s:], v_[:, :, :s]], 0), got)):
        leaves = [t.clone().requires_grad_() for t in (q, k, v)]
        out = fn(*leaves)
        out.backward(g)
        dst += [out.detach()] + [t.grad for t in leaves]
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, **TOL)


@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (4, 2)], ids=["mha", "gqa"])
def test_fold_recurrence(Hq, Hkv):
    q, k, v, _ = _inputs(Hq, Hkv)
    state = flash_attention_fold(q, k[:, :, :s], v[:, :, :s])
    assert len(state) == 3
    out, lse = flash_attention_fold(q, k[:, :, s:], v[:, :, s:], state, causal=True, last=True)
    torch.testing.assert_close(out, _rank1_reference(q, k, v), **TOL)
    scores = torch.einsum("bhqd,bhkd->bhqk", q, k.repeat_interleave(Hq // Hkv, 1)) * D ** -0.5
    scores = scores.masked_fill(~torch.ones(s, S, dtype=torch.bool).tril_(S - s), float("-inf"))
    torch.testing.assert_close(lse, torch.logsumexp(scores, -1), **TOL)
