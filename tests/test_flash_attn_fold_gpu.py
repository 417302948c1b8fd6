"""The carried softmax state (``fa_fwd(state=, last=)``, ``ops.flash_attention_fold``),
the accumulating dq (``fa_bwd(dq_acc=)``) and ``cp.ring_rank_attention`` on them.

A chain of folds never converts its state, so in key order it performs the
operations of ONE launch over the concatenated keys in the same order: it is
compared with ``torch.equal`` against the rectangular kernel. In ring order
(own block first) it is held to the fp64 reference as the rectangular test
holds its kernels: the square reference at S = (rank + 1) * s with ``dout``
zeroed above the rank's rows.
"""

import functools

import pytest
import torch

import attention_check as ac
from test_flash_attn_rect_gpu import _case, _grads, _hold
from torchft_amd.ops import flash_attention_fold, hip_ext
from torchft_amd.parallel import cp

pytestmark = pytest.mark.gpu

S0 = ac.SCALE0
s = 256


def _blocks(t, order):
    return [t[:, :, o * s:(o + 1) * s] for o in order]


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("bh", [(1, 2, 2), (2, 4, 1)], ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("nblk", [2, 3])
@pytest.mark.parametrize("family", ["randn", "ramp_a"])
def test_one_stream_bit_for_bit(family, nblk, bh, causal):
    Sk = nblk * s
    q, k, v, _ = ac.make_inputs(family, *bh, Sk, S0, "cuda")
    q = q[:, :, Sk - s:]
    want = hip_ext().fa_fwd(q, k, v, S0, causal)
    state = None
    for i, (kb, vb) in enumerate(zip(_blocks(k, range(nblk)), _blocks(v, range(nblk)))):
        last = i == nblk - 1
        state = flash_attention_fold(q, kb, vb, state, causal=causal and last, last=last,
                                     scale=S0)
    assert torch.equal(state[0], want[0]) and torch.equal(state[1], want[1])


@pytest.mark.parametrize("bh", [(1, 4, 2), (2, 2, 1)], ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("rank", [1, 2])  # of world rank + 1
@pytest.mark.parametrize("family", ["randn", "needle", "ramp_c"])
def test_ring_order(family, rank, bh):
    n, off = (rank + 1) * s, rank * s
    (q, k, v, dout), ref, emu = _case(family, *bh, n, off, n, True)
    order = [rank - hop for hop in range(rank + 1)]  # own block first, then the older ones
    ks, vs = _blocks(k, order), _blocks(v, order)

    def run(q_, k_, v_):
        return cp.ring_rank_attention(q_, _blocks(k_, order), _blocks(v_, order), 0, fused=True)

    got = _grads(run, q[:, :, off:], k, v, dout[:, :, off:])
    state = None
    for i in range(rank + 1):
        state = flash_attention_fold(q[:, :, off:], ks[i], vs[i], state, causal=i == 0,
                                     last=i == rank, scale=S0)
    assert torch.equal(state[0], got["out"])
    got["lse"] = state[1]
    _hold(f"ring-{family}-rank{rank}-{bh}", family, got, ref, emu)


@functools.lru_cache(maxsize=None)
def _square(B, Hq, Hkv, S, causal):
    q, k, v, dout = ac.make_inputs("randn", B, Hq, Hkv, S, S0, "cuda")
    out, lse = hip_ext().fa_fwd(q, k, v, S0, causal)
    return q, k, v, dout, lse, hip_ext().fa_delta(dout, out)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("shape", [(1, 2, 2, 256), (2, 4, 1, 512)],
                         ids=lambda t: "x".join(map(str, t)))
def test_dq_acc(shape, causal):
    args = (*_square(*shape, causal), S0, causal)
    dq, dk, dv = hip_ext().fa_bwd(*args)
    acc = torch.zeros(shape[0], shape[1], shape[3], ac.D, device="cuda")
    got, dk1, dv1 = hip_ext().fa_bwd(*args, dq_acc=acc)
    assert got.data_ptr() == acc.data_ptr()
    assert torch.equal(acc.to(torch.bfloat16), dq)
    assert torch.equal(dk1, dk) and torch.equal(dv1, dv)
    once = acc.clone()
    hip_ext().fa_bwd(*args, dq_acc=acc)
    assert torch.equal(acc, 2 * once)


@pytest.mark.parametrize("what,msg", [
    ("doc", "state does not go with doc_start / doc_end"),
    ("rect", "state needs k of q's sequence length"),
    ("acc_shape", "acc must be a contiguous"),
    ("dq_acc_dtype", "dq_acc must be an fp32 tensor"),
])
def test_refusals(what, msg):
    def z(*shape, dtype=torch.float32):
        return torch.zeros(*shape, device="cuda", dtype=dtype)

    q = z(1, 2, s, ac.D, dtype=torch.bfloat16)
    k = z(1, 2, 2 * s if what == "rect" else s, ac.D, dtype=torch.bfloat16)
    state = (z(1, 2, s, 64 if what == "acc_shape" else ac.D), z(1, 2, s), z(1, 2, s))
    ds = (z(1, s, dtype=torch.int32),) * 2 if what == "doc" else ()
    with pytest.raises(RuntimeError, match=msg):
        if what == "dq_acc_dtype":
            hip_ext().fa_bwd(q, k, k, q, state[1], state[1], S0, True, dq_acc=q.clone())
        else:
            hip_ext().fa_fwd(q, k, k, S0, True, *ds, state=state, last=False)
