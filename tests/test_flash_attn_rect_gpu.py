"""``flash_attention_rect`` (Sq rows against Sk >= Sq keys, bottom-right causal)
and the CP wiring against the square fp64 reference at S = Sk with ``dout``
zeroed on rows [0, off): dP, delta and dS of those rows are exactly 0, so it
gives the rectangular dk / dv in full and out / lse / dq on rows [off, Sk),
with their bound denominators. Shapes (B, Hq, Hkv, Sq, Sk):

    (1, 2, 2, 256, 512)    one query block, i_min clamped at 0, shifted diagonal
    (1, 4, 1, 512, 768)    dkdv grid 3 against dq grid 2, G = 4, i_min 0, 0, 8
    (2, 2, 1, 256, 1024)   a long prefix; B = 2 takes the contiguous-copy layout
"""

import functools
from types import SimpleNamespace

import pytest
import torch

import attention_check as ac
from torchft_amd.ops import flash_attention_rect, hip_ext
from torchft_amd.ops.attention_ref import attention_emulated, attention_ref64
from torchft_amd.parallel import cp

pytestmark = pytest.mark.gpu

S0 = ac.SCALE0
SHAPES = [(1, 2, 2, 256, 512), (1, 4, 1, 512, 768), (2, 2, 1, 256, 1024)]
Q_SIDE = ("out", "lse", "dq", "A_out", "A_dq", "Sqk", "n")


@functools.lru_cache(maxsize=None)
def _case(family, B, Hq, Hkv, S, off, Sk, causal):
    """Inputs of S positions as [B,S,H,D] views, cut to the first Sk, and the
    square reference / emulation there for query rows [off, Sk). Built once."""
    q, k, v, dout = (t[:, :, :Sk] for t in ac.make_inputs(family, B, Hq, Hkv, S, S0, "cuda"))
    dout[:, :, :off] = 0

    def rows(r):
        return SimpleNamespace(**{n: t[:, :, off:] if n in Q_SIDE else t
                                  for n, t in vars(r).items()})

    return ((q, k, v, dout), rows(attention_ref64(q, k, v, dout, S0, causal)),
            rows(attention_emulated(q, k, v, dout, S0, causal)))


def _hold(what, family, got, ref, emu):
    rep = ac.Report(what)
    ac.check_hard(rep, got, ref)
    if family in ac.SHARP_FAMILIES:
        ac.check_sharp(rep, got, emu, ref)
    rep.check()


def _grads(fn, q, k, v, dout):
    q, k, v = (t.detach().requires_grad_() for t in (q, k, v))
    out = fn(q, k, v)
    out.backward(dout)
    return dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", ["randn", "needle", "ramp_c"])
def test_rect(family, shape, causal):
    B, Hq, Hkv, Sq, Sk = shape
    off = Sk - Sq
    (q, k, v, dout), ref, emu = _case(family, B, Hq, Hkv, Sk, off, Sk, causal)
    qs, ds = q[:, :, off:], dout[:, :, off:]
    got = _grads(lambda q_, k_, v_: flash_attention_rect(q_, k_, v_, causal), qs, k, v, ds)
    got["lse"] = hip_ext().fa_fwd(qs, k, v, S0, causal)[1]
    _hold(f"rect-{family}-{shape}-{causal}", family, got, ref, emu)


@pytest.mark.parametrize("sq,sk,doc,msg", [
    (512, 256, False, "k must have q's batch and its sequence length"),
    (256, 384, False, "k's sequence length 384 must be a multiple of 256"),
    (256, 512, True, "doc_start / doc_end need k of q's sequence length"),
])
def test_refusals(sq, sk, doc, msg):
    q = torch.zeros(1, 2, sq, ac.D, device="cuda", dtype=torch.bfloat16)
    k = torch.zeros(1, 2, sk, ac.D, device="cuda", dtype=torch.bfloat16)
    ds = (torch.zeros(1, sq, device="cuda", dtype=torch.int32),) * 2 if doc else ()
    with pytest.raises(RuntimeError, match=msg):
        hip_ext().fa_fwd(q, k, k, S0, True, *ds)
    with pytest.raises(RuntimeError, match=msg):
        hip_ext().fa_bwd(q, k, k, q, q[..., 0].float(), q[..., 0].float(), S0, True, *ds)


@pytest.mark.parametrize("rank", [0, 1])
def test_cp_rank_attention(rank, monkeypatch):
    """Ranks 0 and 1 of world 2 on slices of one sequence, no process group."""
    s, n = 256, (rank + 1) * 256
    (q, k, v, dout), ref, emu = _case("randn", 1, 4, 2, 512, rank * s, n, True)
    full = ac.make_inputs("randn", 1, 4, 2, 512, S0, "cuda")
    shard = [t.transpose(1, 2)
             for t in (q[:, :, rank * s:], full[1], full[2], dout[:, :, rank * s:])]

    def run(rect):
        got = _grads(lambda q_, k_, v_: cp.cp_rank_attention(q_, k_, v_, rank, 2, True, rect),
                     *shard)
        return {n_: t.transpose(1, 2) for n_, t in got.items()}

    got = run(True)
    for name in ("dk", "dv"):  # the keys past the shard: autograd's narrow
        assert not got[name][:, :, n:].any()
        got[name] = got[name][:, :, :n]
    _hold(f"cp-rank{rank}", "randn", got, ref, emu)

    def refuse(*a, **kw):
        raise AssertionError("flash_attention_rect called")

    monkeypatch.setattr(cp, "flash_attention_rect", refuse)
    monkeypatch.delenv("TORCHFT_AMD_CP_RECT", raising=False)
    assert torch.isfinite(run(None)["out"]).all()  # flag off: the merge path
    with pytest.raises(AssertionError, match="flash_attention_rect called"):
        run(True)
