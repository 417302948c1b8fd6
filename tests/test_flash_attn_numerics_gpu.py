"""The attention kernels against fp64 under derived bounds (docs/KERNELS.md,
"Numerics"): fa_fwd, fa_delta and fa_bwd fed three ways (aten flash's out /
lse, fa_fwd's, the reference's own lse / delta), on seeded input families that
aim at scale, the delta cancellation, addressing and both sides of the
forward's defer-max branch. tests/test_attention_numerics_cpu.py shows that
the two criteria used here refuse subtly wrong results. Also what the bindings
do with empty inputs and with more batch * heads than a launch covers."""

import functools

import pytest
import torch

import attention_check as ac
from torchft_amd.ops.attention_ref import attention_emulated, attention_ref64

pytestmark = pytest.mark.gpu

S0 = ac.SCALE0
# (B, Hq, Hkv, S)
BWD_ONLY = [(1, 2, 2, 128), (2, 4, 1, 384)]
FWD_BWD = [(1, 2, 1, 256), (2, 8, 1, 256), (1, 4, 2, 512), (2, 4, 4, 768)]

CASES = (
    [("randn", *sh, c, S0) for sh in BWD_ONLY + FWD_BWD for c in (True, False)]
    + [("randn", 1, 4, 2, 512, True, s) for s in (0.25, 2.0 ** -5)]
    + [("randn", 1, 2, 1, 256, False, s) for s in (0.25, 2.0 ** -5)]
    + [("offset", 2, 4, 1, 384, True, S0), ("offset", 2, 4, 1, 384, False, S0),
       ("offset", 1, 4, 2, 512, True, S0), ("offset", 2, 4, 4, 768, False, S0)]
    + [("needle", 1, 2, 2, 128, True, S0), ("needle", 2, 4, 1, 384, True, S0),
       ("needle", 2, 8, 1, 256, False, S0), ("needle", 2, 4, 4, 768, True, S0)]
    + [(f, *sh, c, S0) for f in ("ramp_a", "ramp_b", "ramp_c")
       for sh, c in (((1, 2, 1, 256), True), ((1, 2, 1, 256), False),
                     ((1, 4, 2, 512), True))]
)


def _id(case):
    f, B, Hq, Hkv, S, causal, scale = case
    return f"{f}-{B}x{Hq}x{Hkv}x{S}-{'causal' if causal else 'full'}-s{scale:.4f}"


def _ext():
    from torchft_amd.ops import hip_ext

    return hip_ext()


@functools.lru_cache(maxsize=None)
def _case(case, mask_name=None):
    """Inputs as [B,S,H,D]-backed views, the fp64 reference and the two
    emulations (whole chain; backward fed the reference's lse / delta), built
    once on the device and left unchanged."""
    family, B, Hq, Hkv, S, causal, scale = case
    q, k, v, dout = ac.make_inputs(family, B, Hq, Hkv, S, scale, device="cuda")
    m = None if mask_name is None else ac.doc_mask(mask_name)
    ref = attention_ref64(q, k, v, dout, scale, causal, m)
    emu = attention_emulated(q, k, v, dout, scale, causal, m)
    emu_ref = attention_emulated(q, k, v, dout, scale, causal, m,
                                 lse=ref.lse.float(), delta=ref.delta.float())
    return (q, k, v, dout), m, ref, emu, emu_ref


def _check_chain(what, case, tensors, m, ref, emu, emu_ref, feeds):
    """Run the kernels the ways `feeds` names and hold each result to the hard
    bound, and outside the needle family to the sharp criterion."""
    family, B, Hq, Hkv, S, causal, scale = case
    q, k, v, dout = tensors
    ext = _ext()
    doc = () if m is None else (m.doc_start, m.doc_end)
    sharp = family in ac.SHARP_FAMILIES
    rep = ac.Report(what)

    def backward(tag, lse, delta, emu_b, factors):
        dq, dk, dv = ext.fa_bwd(q, k, v, dout, lse, delta, scale, causal, *doc)
        got = dict(dq=dq, dk=dk, dv=dv)
        sub = ac.Report(f"{what} [{tag}]")
        ac.check_hard(sub, got, ref, factors)
        if sharp:
            ac.check_sharp(sub, got, emu_b, ref)
        rep.rows += [(f"{tag} {n}", r, lim) for n, r, lim in sub.rows]

    def delta_of(tag, out):
        delta = ext.fa_delta(dout, out)
        assert torch.isfinite(delta).all()
        rep.add(f"{tag} hard delta", ac.delta_ratio(delta, dout, out), 1.0)
        return delta

    if "aten" in feeds:
        out, lse, *_ = torch.ops.aten._scaled_dot_product_flash_attention(
            q, k, v, 0.0, causal, False, scale=scale)
        print(f"{what}: aten out at {ac.hard_ratio(out, ref.out, ref.A_out, 3.0):.3f} "
              f"of 3 u A, lse at {ac.lse_ratio(lse, ref):.3f} of its bound")
        backward("aten-fed", lse, delta_of("aten-fed", out), emu, ac.HARD)
    if "fwd" in feeds:
        out, lse = ext.fa_fwd(q, k, v, scale, causal, *doc)
        got = dict(out=out, lse=lse)
        sub = ac.Report(f"{what} [fa_fwd]")
        ac.check_hard(sub, got, ref)
        if sharp:
            ac.check_sharp(sub, got, emu, ref)
        rep.rows += [(f"fa_fwd {n}", r, lim) for n, r, lim in sub.rows]
        backward("fwd-fed", lse, delta_of("fwd-fed", out), emu, ac.HARD)
    if "ref" in feeds:
        backward("ref-fed", ref.lse.float(), ref.delta.float(), emu_ref, ac.HARD_REF_FED)
    rep.check()


class TestAgainstFp64:
    @pytest.mark.parametrize("case", CASES, ids=_id)
    def test_views(self, case):
        tensors, m, ref, emu, emu_ref = _case(case)
        feeds = ("aten", "ref") + (("fwd",) if case[4] % 256 == 0 else ())
        _check_chain(_id(case), case, tensors, m, ref, emu, emu_ref, feeds)

    @pytest.mark.parametrize("family", ac.FAMILIES)
    def test_packed(self, family):
        """One packed case per family: the layouts' bitwise equality is tested
        elsewhere, this holds the packed path to the same bounds."""
        case = (family, 1, 4, 2, 512, True, S0)
        tensors, m, ref, emu, emu_ref = _case(case)
        tensors = tuple(t.contiguous() for t in tensors)
        _check_chain(_id(case) + "-packed", case, tensors, m, ref, emu, emu_ref,
                     ("aten", "fwd", "ref"))

    @pytest.mark.parametrize("name", ["mixed256", "halves512"])
    def test_document_mask(self, name):
        """Two layouts of tests/test_doc_mask_gpu.py under the two criteria."""
        S, rows = ac.DOC_LAYOUTS[name]
        case = ("randn", len(rows), 8, 2, S, True, S0)
        tensors, m, ref, emu, emu_ref = _case(case, name)
        _check_chain(f"doc-{name}", case, tensors, m, ref, emu, emu_ref, ("fwd", "ref"))


class TestStatDtype:
    def test_fp64_lse_and_delta_give_the_fp32_bits(self):
        case = ("offset", 2, 4, 1, 384, True, S0)
        (q, k, v, dout), _, ref, _, _ = _case(case)
        ext = _ext()
        a = ext.fa_bwd(q, k, v, dout, ref.lse.float(), ref.delta.float(), S0, True)
        b = ext.fa_bwd(q, k, v, dout, ref.lse.float().double(),
                       ref.delta.float().double(), S0, True)
        for n, x, y in zip(("dq", "dk", "dv"), a, b):
            assert torch.isfinite(x).all(), n
            assert torch.equal(x, y), n


class TestBindingEdges:
    """Empty inputs come back as empty outputs of the right shape, dtype and
    layout without a launch; batch * heads above gridDim.y's limit is refused
    before anything is allocated or launched."""

    @staticmethod
    def _args(B, Hq, Hkv, S, views):
        def mk(H):
            if views:
                return torch.zeros(B, S, H, 128, device="cuda",
                                   dtype=torch.bfloat16).transpose(1, 2)
            return torch.zeros(B, H, S, 128, device="cuda", dtype=torch.bfloat16)

        stat = torch.zeros(B, Hq, S, device="cuda")
        return mk(Hq), mk(Hkv), mk(Hkv), mk(Hq), stat, stat.clone()

    @pytest.mark.parametrize("views", [True, False], ids=["bshd", "packed"])
    @pytest.mark.parametrize("B,S", [(0, 256), (2, 0), (0, 0)])
    def test_empty_inputs(self, B, S, views):
        Hq, Hkv = 4, 2
        q, k, v, dout, lse, delta = self._args(B, Hq, Hkv, S, views)
        ext = _ext()
        out, lse_o = ext.fa_fwd(q, k, v, S0, True)
        d = ext.fa_delta(dout, out)
        dq, dk, dv = ext.fa_bwd(q, k, v, dout, lse, delta, S0, True)
        torch.cuda.synchronize()
        for t, like in ((out, q), (dq, q), (dk, k), (dv, v)):
            assert t.shape == like.shape and t.dtype == torch.bfloat16
            assert t.device == like.device and t.numel() == 0
            assert (t.transpose(1, 2) if views else t).is_contiguous()
        for t in (lse_o, d):
            assert t.shape == (B, Hq, S) and t.dtype == torch.float32

    @pytest.mark.parametrize("call", ["fa_fwd", "fa_bwd"])
    def test_grid_limit(self, call):
        """65536 batch rows as an expanded view: nothing large exists, and the
        refusal comes before the binding would make one contiguous."""
        B, S = 65536, 256

        def big(*shape, dtype=torch.bfloat16):
            return torch.zeros(1, *shape, device="cuda", dtype=dtype).expand(B, *shape)

        q, k = big(1, S, 128), big(1, S, 128)
        stat = big(1, S, dtype=torch.float32)
        ext = _ext()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        with pytest.raises(RuntimeError,
                           match=rf"{call}: q has batch \* heads = 65536, above the 65535"):
            if call == "fa_fwd":
                ext.fa_fwd(q, k, k, S0, True)
            else:
                ext.fa_bwd(q, k, k, q, stat, stat, S0, True)
        assert torch.cuda.max_memory_allocated() == before
