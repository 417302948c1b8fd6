"""The attention kernels take their block from fa_wg_order (fa_layout.h), which
reorders a causal launch. A transposed or off-by-one decode of the block id is
an O(1) error only where the grid has nx >= 2, ny >= 2 and nx != ny, so the
shapes here are the smallest with such grids in both backward launches:

    (B, Hq, Hkv, S)    dkdv grid   dq / forward grid
    (1, 4, 2, 768)     3 x 2       3 x 4
    (3, 2, 1, 512)     2 x 3       2 x 6
    (2, 8, 2, 1280)    5 x 4       5 x 16

Each runs causal and full as [B,S,H,D] views, one also packed, one under a
document mask of two unequal documents, on the needle family (a mis-addressed
block or head is an O(1) error) and on randn. fa_fwd takes every shape here
(S is a multiple of 256). Outputs are held to the two criteria of
tests/attention_check.py with its limits; the map itself is checked on the
host by tests/test_fa_wg_order.py."""

import functools

import pytest
import torch

import attention_check as ac
from torchft_amd.ops import DocMask, hip_ext
from torchft_amd.ops.attention_ref import attention_emulated, attention_ref64

pytestmark = pytest.mark.gpu

S0 = ac.SCALE0
SHAPES = [(1, 4, 2, 768), (3, 2, 1, 512), (2, 8, 2, 1280)]
DOCS_768 = [[300, 468]]  # a boundary inside the second of three blocks


def _id(val):
    if isinstance(val, tuple):
        return "x".join(str(v) for v in val)
    if isinstance(val, bool):
        return "causal" if val else "full"
    return str(val)


@functools.lru_cache(maxsize=None)
def _case(family, shape, causal, docs=False):
    """Inputs as [B,S,H,D]-backed views, the fp64 reference and the two
    emulations, built once on the device and left unchanged."""
    B, Hq, Hkv, S = shape
    tensors = ac.make_inputs(family, B, Hq, Hkv, S, S0, device="cuda")
    m = DocMask.from_lengths(DOCS_768, S, device="cuda") if docs else None
    ref = attention_ref64(*tensors, S0, causal, m)
    emu = attention_emulated(*tensors, S0, causal, m)
    emu_ref = attention_emulated(*tensors, S0, causal, m, lse=ref.lse.float(),
                                 delta=ref.delta.float())
    return tensors, m, ref, emu, emu_ref


def _check(what, family, shape, causal, docs=False, packed=False):
    """fa_fwd, then fa_bwd fed fa_fwd's out / lse and fed the reference's own
    lse / delta: the hard bound always, the sharp criterion outside needle."""
    tensors, m, ref, emu, emu_ref = _case(family, shape, causal, docs)
    if packed:
        tensors = tuple(t.contiguous() for t in tensors)
    q, k, v, dout = tensors
    ext = hip_ext()
    doc = () if m is None else (m.doc_start, m.doc_end)
    sharp = family in ac.SHARP_FAMILIES
    rep = ac.Report(what)

    def hold(tag, got, emu_x, factors):
        sub = ac.Report(f"{what} [{tag}]")
        ac.check_hard(sub, got, ref, factors)
        if sharp:
            ac.check_sharp(sub, got, emu_x, ref)
        rep.rows += [(f"{tag} {n}", r, lim) for n, r, lim in sub.rows]

    out, lse = ext.fa_fwd(q, k, v, S0, causal, *doc)
    hold("fa_fwd", dict(out=out, lse=lse), emu, ac.HARD)
    delta = ext.fa_delta(dout, out)
    dq, dk, dv = ext.fa_bwd(q, k, v, dout, lse, delta, S0, causal, *doc)
    hold("fwd-fed", dict(dq=dq, dk=dk, dv=dv), emu, ac.HARD)
    dq, dk, dv = ext.fa_bwd(q, k, v, dout, ref.lse.float(), ref.delta.float(), S0,
                            causal, *doc)
    hold("ref-fed", dict(dq=dq, dk=dk, dv=dv), emu_ref, ac.HARD_REF_FED)
    rep.check()


@pytest.mark.parametrize("causal", [True, False], ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("family", ["needle", "randn"])
def test_views(family, shape, causal):
    _check(f"{family}-{_id(shape)}-{_id(causal)}", family, shape, causal)


@pytest.mark.parametrize("family", ["needle", "randn"])
def test_packed(family):
    _check(f"{family}-packed", family, (2, 8, 2, 1280), True, packed=True)


@pytest.mark.parametrize("family", ["needle", "randn"])
def test_document_mask(family):
    _check(f"{family}-docs", family, (1, 4, 2, 768), True, docs=True)


def test_block_of_another_head_is_seen():
    """What the cases above rest on: dq of the needle family with two heads
    swapped is refused by the hard bound."""
    shape = (1, 4, 2, 768)
    (q, k, v, dout), _, ref, _, _ = _case("needle", shape, True)
    dq, _, _ = hip_ext().fa_bwd(q, k, v, dout, ref.lse.float(), ref.delta.float(),
                                S0, True)
    swapped = dq[:, [1, 0, 2, 3]]
    factor, denom = ac.HARD_REF_FED["dq"]
    assert ac.hard_ratio(dq, ref.dq, getattr(ref, denom), factor) <= 1.0
    wrong = ac.hard_ratio(swapped, ref.dq, getattr(ref, denom), factor)
    print(f"heads 0 and 1 of dq swapped: {wrong:.1f} of the hard bound")
    assert wrong > 1.0
