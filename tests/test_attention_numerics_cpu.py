"""The attention checker checked: the fp32 emulation of the kernels' rounding
chain stays under two thirds of every hard bound on every input family, the
ramp family really drives the forward's defer-max branch the way it claims,
and each injected error is reported by the criterion that is meant to see it.
This is the evidence that tests/test_flash_attn_numerics_gpu.py would fail on
a subtly wrong kernel. No GPU."""

import functools
import math

import pytest
import torch

import attention_check as ac
from torchft_amd.ops.attention_ref import (
    U_BF16, attention_emulated, attention_ref64, visible)

B, HQ, HKV = 1, 4, 2
SCALES = [ac.SCALE0, 0.25]
SIDS = ["s128", "s025"]


@functools.lru_cache(maxsize=None)
def _case(family, S, causal, scale):
    q, k, v, dout = ac.make_inputs(family, B, HQ, HKV, S, scale)
    ref = attention_ref64(q, k, v, dout, scale, causal)
    emu = attention_emulated(q, k, v, dout, scale, causal)
    return (q, k, v, dout), ref, emu


def _got(emu, **over):
    got = {n: getattr(emu, n) for n in ("out", "lse", "dq", "dk", "dv")}
    got.update(over)
    return got


def _second_chain(q, k, v, dout, scale, tile=64, stale_nats=3.3):
    """Causal attention by another correct bf16 chain: sums taken over 64-key
    (64-row) tiles from the last tile to the first, a softmax maximum that is
    3.3 nats stale (P up to e^3.3 before it is rounded), natural exp in place
    of exp2, `scale` applied after dS is rounded, the GQA group summed in
    reverse. Same roundings in kind, none of them in the same place."""
    B, Hq, S, Dh = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    bf = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
    qf, dof = q.float(), dout.float()
    kr = k.float().repeat_interleave(G, 1)
    vr = v.float().repeat_interleave(G, 1)
    vis = visible(S, True, None, q.device)
    tiles = [slice(t, t + tile) for t in range(S - tile, -1, -tile)]

    def tiled(a, b):  # a @ b with the inner dimension summed tile by tile
        acc = torch.zeros(*a.shape[:-1], b.shape[-1])
        for t in tiles:
            acc = acc + a[..., t] @ b[..., t, :]
        return acc

    s = ((qf @ kr.transpose(-1, -2)) * scale).masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True) - stale_nats
    e = torch.exp(s - m)
    l = sum(e[..., t].sum(-1, keepdim=True) for t in tiles)
    out = (tiled(bf(e), vr) / l).to(torch.bfloat16)
    lse = (m + torch.log(l)).squeeze(-1)
    delta = (dof * out.float()).flip(-1).sum(-1)

    p = torch.exp(s - lse[..., None])
    dS = bf(p * (dof @ vr.transpose(-1, -2) - delta[..., None]))
    dq = (tiled(dS, kr) * scale).to(torch.bfloat16)

    def group(t):
        return t.reshape(B, Hkv, G, S, Dh).flip(2).sum(2).to(torch.bfloat16)

    dk = group(tiled(dS.transpose(-1, -2), qf) * scale)
    dv = group(tiled(bf(p).transpose(-1, -2), dof))
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv)


def _verdict(what, got, ref, emu):
    """(hard failures, sharp failures) of one set of results."""
    hard, sharp = ac.Report(what), ac.Report(what)
    ac.check_hard(hard, got, ref)
    ac.check_sharp(sharp, got, emu, ref)
    return hard.failures(), sharp.failures()


class TestEmulationUnderTheBounds:
    @pytest.mark.parametrize("scale", SCALES, ids=SIDS)
    @pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
    @pytest.mark.parametrize("S", [256, 512])
    @pytest.mark.parametrize("family", ac.FAMILIES)
    def test_two_thirds(self, family, S, causal, scale):
        (q, k, v, dout), ref, emu = _case(family, S, causal, scale)
        rep = ac.Report(f"{family} S={S} causal={causal} scale={scale:.4f}")
        ac.check_hard(rep, _got(emu), ref)
        rep.add("hard delta", ac.delta_ratio(emu.delta, dout, emu.out), 1.0)
        bad = [r for r in rep.rows if not r[1] <= 2.0 / 3.0]
        assert not bad, bad

    def test_ref_fed_backward_under_factor_three(self):
        """Fed the reference's lse / delta, dq / dk lose delta's inherited
        error: 3 u A with the P.E term out of W (A_dq_ref / A_dk_ref)."""
        for family in ac.FAMILIES:
            (q, k, v, dout), ref, _ = _case(family, 512, True, ac.SCALE0)
            emu = attention_emulated(q, k, v, dout, ac.SCALE0, True,
                                     lse=ref.lse.float(), delta=ref.delta.float())
            rep = ac.Report(f"{family} ref-fed")
            ac.check_hard(rep, dict(dq=emu.dq, dk=emu.dk, dv=emu.dv), ref,
                          ac.HARD_REF_FED)
            assert all(r[1] <= 2.0 / 3.0 for r in rep.rows), rep.rows

    def test_one_unit_is_not_enough(self):
        """out / dv: with one unit of u A in place of three the correct chain
        itself is refused (it reaches 1.4-1.7 units: P's rounding and the
        store). dq / dk reach 0.2-0.45 of one unit here; their five units are
        a worst case over delta's inherited error that these inputs do not
        attain, which is why the sharp criterion exists. Any factor lowered
        to under 1.5x what the emulation reaches fails test_two_thirds."""
        worst = {n: 0.0 for n in ("out", "dv")}
        for family in ("randn", "offset"):
            _, ref, emu = _case(family, 512, True, ac.SCALE0)
            for n in worst:
                worst[n] = max(worst[n], ac.hard_ratio(
                    getattr(emu, n), getattr(ref, n), getattr(ref, "A_" + n), 1.0))
        print(worst)
        assert all(w > 1.0 for w in worst.values()), worst


class TestRampDrivesTheBranch:
    """fp64 scores of the bf16 ramp inputs, in the forward's log2 units, per
    row and 32-key block, walked the way the kernel walks them."""

    @staticmethod
    def _block_max(family, S, causal):
        (q, k, v, dout), _, _ = _case(family, S, causal, ac.SCALE0)
        G = HQ // HKV
        s = (q.double() @ k.double().repeat_interleave(G, 1).transpose(-1, -2))
        s = s * ac.SCALE0 * math.log2(math.e)
        assert s.abs().max().item() * math.log(2.0) <= 40.0
        s = s.masked_fill(~visible(S, causal, None, s.device), float("-inf"))
        return s.reshape(B, HQ, S, S // 32, 32).amax(-1)  # [B,H,row,block]

    @pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
    @pytest.mark.parametrize("S", [256, 512])
    def test_a_rescales_at_every_rising_block(self, S, causal):
        bm = self._block_max("ramp_a", S, causal)
        run = torch.cummax(bm, dim=-1).values
        rise = bm[..., 1:8] - run[..., 0:7]
        seen = torch.isfinite(bm[..., 1:8])
        assert seen.any()
        assert (rise[seen] > ac.FWD_THR_LOG2).all(), rise[seen].min()

    @pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
    @pytest.mark.parametrize("S", [256, 512])
    def test_b_never_rescales_after_the_first_block(self, S, causal):
        bm = self._block_max("ramp_b", S, causal)
        rise = bm[..., 1:] - bm[..., :1]
        seen = torch.isfinite(rise)
        assert (rise[seen] <= ac.FWD_THR_LOG2).all(), rise[seen].max()
        # and P, taken against the stale maximum, gets large: past e^6
        assert rise[seen].max().item() > 6.0 * math.log2(math.e)

    @pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
    @pytest.mark.parametrize("S", [256, 512])
    def test_c_mixes_rows_in_every_wave(self, S, causal):
        bm = self._block_max("ramp_c", S, causal)
        run = torch.cummax(bm, dim=-1).values
        rise = bm[..., 1:8] - run[..., 0:7]
        seen = torch.isfinite(bm[..., 1:8])
        odd, even = rise[:, :, 1::2], rise[:, :, 0::2]
        assert (odd[seen[:, :, 1::2]] > ac.FWD_THR_LOG2).all()
        assert (even[seen[:, :, 0::2]] <= ac.FWD_THR_LOG2).all()


class TestInjectedErrors:
    """One error at a time on top of the emulation; each must be refused by
    the criterion named."""

    S = 512

    def test_the_emulation_itself_passes_both(self):
        for family in ac.SHARP_FAMILIES:
            _, ref, emu = _case(family, self.S, True, ac.SCALE0)
            hard, sharp = _verdict(family, _got(emu), ref, emu)
            assert not hard and not sharp

    @pytest.mark.parametrize("scale", SCALES, ids=SIDS)
    @pytest.mark.parametrize("family", ac.SHARP_FAMILIES)
    def test_second_correct_chain_passes_sharp(self, family, scale):
        """A second correct chain, different wherever a correct kernel may
        differ, stays within the sharp factors of the first."""
        (q, k, v, dout), ref, emu = _case(family, self.S, True, scale)
        alt = _second_chain(q, k, v, dout, scale)
        hard, sharp = _verdict(f"{family} second chain", alt, ref, emu)
        assert not hard and not sharp, (hard, sharp)

    @pytest.mark.parametrize("family", ["randn", "needle"])
    def test_causal_diagonal_off_by_one_hard(self, family):
        (q, k, v, dout), ref, emu = _case(family, self.S, True, ac.SCALE0)
        pos = torch.arange(self.S)
        loose = (pos[None, :] <= pos[:, None] + 1)[None, None]
        bad = attention_emulated(q, k, v, dout, ac.SCALE0, True, doc_mask=loose)
        hard, _ = _verdict("diag+1", _got(bad), ref, emu)
        # needle: the extra key's P is ~e^-45, lost in out and dq, but dk / dv
        # of that key are held to a denominator that does not contain it
        want = {"hard dk", "hard dv"} | (
            {"hard out", "hard dq"} if family == "randn" else set())
        assert {h.split(":")[0] for h in hard} >= want, hard

    @pytest.mark.parametrize("family", ["randn", "offset"])
    @pytest.mark.parametrize("rb,kb", [(9, 2), (15, 15)])
    def test_dropped_block_sharp(self, family, rb, kb):
        """Row block rb loses key block kb: in P.V (out), and in dS (dq of the
        rows, dk of the keys)."""
        (q, k, v, dout), ref, emu = _case(family, self.S, True, ac.SCALE0)
        G = HQ // HKV
        h, hk = 3, 3 // G
        rows, keys = slice(32 * rb, 32 * rb + 32), slice(32 * kb, 32 * kb + 32)
        qd, kd, vd, dod = (t.double() for t in (q, k, v, dout))
        s = (qd[0, h, rows] @ kd[0, hk, keys].T) * ac.SCALE0
        if rb == kb:
            s = s.masked_fill(torch.ones(32, 32).triu(1).bool(), float("-inf"))
        P = torch.exp(s - ref.lse[0, h, rows, None])
        dS = P * (dod[0, h, rows] @ vd[0, hk, keys].T - ref.delta[0, h, rows, None])
        dS = dS * ac.SCALE0

        def minus(t, hh, where, what):
            t = t.clone()
            t[0, hh, where] = (t[0, hh, where].double() - what).to(t.dtype)
            return t

        got = _got(emu, out=minus(emu.out, h, rows, P @ vd[0, hk, keys]),
                   dq=minus(emu.dq, h, rows, dS @ kd[0, hk, keys]),
                   dk=minus(emu.dk, hk, keys, dS.T @ qd[0, h, rows]))
        _, sharp = _verdict("dropped block", got, ref, emu)
        assert {s_.split(":")[0] for s_ in sharp} == {"sharp out", "sharp dq", "sharp dk"}, sharp

    @pytest.mark.parametrize("family", ["randn", "offset"])
    def test_wrong_group_both(self, family):
        """dk / dv from the first query head of each group, doubled."""
        (q, k, v, dout), ref, emu = _case(family, self.S, True, ac.SCALE0)
        G = HQ // HKV
        per_head = attention_emulated(q, k.repeat_interleave(G, 1),
                                      v.repeat_interleave(G, 1), dout, ac.SCALE0, True)
        got = _got(emu, dk=2 * per_head.dk[:, ::G], dv=2 * per_head.dv[:, ::G])
        hard, sharp = _verdict("wrong group", got, ref, emu)
        assert {h.split(":")[0] for h in hard} == {"hard dk", "hard dv"}, hard
        assert {s_.split(":")[0] for s_ in sharp} == {"sharp dk", "sharp dv"}, sharp

    @pytest.mark.parametrize("family", ["randn", "offset"])
    def test_default_scale_in_dq_sharp(self, family):
        (q, k, v, dout), ref, emu = _case(family, self.S, True, 0.25)
        wrong = (emu.dq.float() * (ac.SCALE0 / 0.25)).to(torch.bfloat16)
        _, sharp = _verdict("scale in dq", _got(emu, dq=wrong), ref, emu)
        assert [s_.split(":")[0] for s_ in sharp] == ["sharp dq"], sharp

    @pytest.mark.parametrize("family", ["randn", "offset"])
    def test_lse_off_by_a_hundredth_sharp(self, family):
        """The backward fed lse + 1e-2: dv everywhere, dq / dk on randn (with
        offset v the delta cancellation already costs the emulation as much)."""
        (q, k, v, dout), ref, emu = _case(family, self.S, True, ac.SCALE0)
        bad = attention_emulated(q, k, v, dout, ac.SCALE0, True, lse=emu.lse + 1e-2)
        got = dict(dq=bad.dq, dk=bad.dk, dv=bad.dv)
        _, sharp = _verdict("lse + 1e-2", got, ref, emu)
        names = {s_.split(":")[0] for s_ in sharp}
        want = {"sharp dv"} | ({"sharp dq", "sharp dk"} if family == "randn" else set())
        assert names >= want, sharp
        # the lse itself, as the forward's output
        _, sharp = _verdict("lse + 1e-2 out", dict(lse=emu.lse + 1e-2), ref, emu)
        assert sharp


def test_needle_map_reaches_every_block():
    for S in (256, 768):
        for h in range(8):
            pi = ac.needle_map(S, h)
            for r in range(S // 32):
                assert set((pi[32 * r:32 * r + 32] // 32).tolist()) == set(range(r + 1))


def test_unit_round_off():
    assert U_BF16 == torch.finfo(torch.bfloat16).eps / 2
