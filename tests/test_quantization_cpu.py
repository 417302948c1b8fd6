"""CPU tests of the fp8 pack format via the pure-torch reference
implementation (ground truth for the GPU kernel tests)."""

import pytest
import torch

import fp8_check
from torchft_amd.quantization import (
    QBLOCK,
    dequantize_pack_ref,
    e4m3_codes,
    pack_geometry,
    quantize_pack_ref,
    split_slices,
)


class TestPackFormat:
    def test_geometry(self):
        t = [torch.zeros(5000), torch.zeros(2048)]
        total, padded, bpr, slice_bytes = pack_geometry(t, world=2)
        assert total == 3 + 1  # ceil(5000/2048)=3, 1
        assert padded == 4 and bpr == 2
        assert slice_bytes == 2 * (4 + QBLOCK)

    def test_roundtrip_ref(self):
        torch.manual_seed(0)
        tensors = [torch.randn(3000), torch.randn(2048)]
        pack = quantize_pack_ref(tensors, world=2)
        out = dequantize_pack_ref([3000, 2048], pack, world=2)
        for t, o in zip(tensors, out):
            torch.testing.assert_close(o, t, rtol=0.1, atol=0.1)

    def test_zero_block(self):
        tensors = [torch.zeros(2048)]
        pack = quantize_pack_ref(tensors, world=1)
        out = dequantize_pack_ref([2048], pack, world=1)
        assert (out[0] == 0).all()


class TestPackFormatProperties:
    """Property tests: the wire format must hold its error bound and
    geometry invariants for arbitrary tensor sizes and world sizes."""

    def test_roundtrip_residual_bound_random_shapes(self):
        from hypothesis import given, settings
        from hypothesis import strategies as st

        @settings(max_examples=30, deadline=None)
        @given(
            sizes=st.lists(st.integers(1, 5000), min_size=1, max_size=4),
            world=st.sampled_from([1, 2, 4]),
            scale_pow=st.integers(-8, 8),
            seed=st.integers(0, 2**31 - 1),
        )
        def run(sizes, world, scale_pow, seed):
            gen = torch.Generator().manual_seed(seed)
            tensors = [
                torch.randn(n, generator=gen) * (2.0 ** scale_pow) for n in sizes
            ]
            pack = quantize_pack_ref(tensors, world=world)
            out = dequantize_pack_ref(sizes, pack, world=world)
            for t, o in zip(tensors, out):
                assert o.shape == t.shape
                denom = t.norm().item() or 1.0
                # e4m3 block format: top-of-block ulp = amax/14; residual
                # norm on gaussian data stays well under 8% of tensor norm
                assert (o - t).norm().item() / denom < 0.08

        run()

    def test_geometry_invariants(self):
        from hypothesis import given, settings
        from hypothesis import strategies as st

        @settings(max_examples=50, deadline=None)
        @given(
            sizes=st.lists(st.integers(1, 10000), min_size=1, max_size=5),
            world=st.sampled_from([1, 2, 4, 8]),
        )
        def run(sizes, world):
            tensors = [torch.zeros(n) for n in sizes]
            total, padded, bpr, slice_bytes = pack_geometry(tensors, world=world)
            assert total == sum((n + QBLOCK - 1) // QBLOCK for n in sizes)
            assert padded >= total and padded % world == 0
            assert bpr == padded // world
            assert slice_bytes == bpr * (4 + QBLOCK)

        run()

    def test_outlier_block_keeps_other_blocks_precise(self):
        # block scaling is local: a huge outlier in block 0 must not
        # destroy precision in block 1 (per-tensor scaling would)
        t = torch.cat([torch.full((QBLOCK,), 1e4), torch.randn(QBLOCK)])
        pack = quantize_pack_ref([t], world=1)
        (out,) = dequantize_pack_ref([2 * QBLOCK], pack, world=1)
        tail, tail_ref = out[QBLOCK:], t[QBLOCK:]
        assert (tail - tail_ref).norm().item() / tail_ref.norm().item() < 0.08


class TestReferenceStatesTheKernel:
    """quantize_pack_ref is what the GPU tests hold the kernels to byte for
    byte; here it is held to codes that follow from the format alone."""

    @pytest.mark.parametrize("dtype", fp8_check.DTYPES)
    def test_enumeration_block_codes_by_construction(self, dtype):
        block, want = fp8_check.enumeration_block(dtype)
        # every finite code and both roundings of every midpoint are in it
        assert set(want.tolist()) == set(range(0x7F)) | set(range(0x80, 0xFF))
        for world in (1, 2):
            pack = quantize_pack_ref([block], world)
            scales, codes = split_slices(pack, world)
            assert scales.reshape(-1)[0].item() == 1.0
            assert torch.equal(codes.reshape(-1, QBLOCK)[0], want)
            if world == 2:  # the padding slot
                assert scales.reshape(-1)[1].item() == 0.0
                assert (codes.reshape(-1, QBLOCK)[1] == 0).all()
        (out,) = dequantize_pack_ref([QBLOCK], quantize_pack_ref([block], 1), 1)
        decoded = torch.tensor([fp8_check.e4m3_value(c) for c in want.tolist()])
        assert torch.equal(out, decoded)

    def test_e4m3_codes_saturate_and_propagate(self):
        x = torch.tensor([448.0, 449.0, 463.9, 1e30, -1e30, float("inf"),
                          -float("inf"), float("nan"), 2.0 ** -10, 3 * 2.0 ** -10, -0.0])
        got = e4m3_codes(x).tolist()
        assert got == [0x7E, 0x7E, 0x7E, 0x7E, 0xFE, 0x7F, 0x7F, 0x7F, 0x00, 0x02, 0x80]

    def test_nan_stays_nan_and_leaves_the_scale_alone(self):
        torch.manual_seed(1)
        clean = torch.randn(3 * QBLOCK)
        clean[QBLOCK : 2 * QBLOCK] = 0  # the NaN's block is otherwise zero
        dirty = clean.clone()
        dirty[5] = float("nan")
        dirty[QBLOCK + 9] = float("nan")
        pc, pd = quantize_pack_ref([clean], 1), quantize_pack_ref([dirty], 1)
        diff = (pc != pd).nonzero().flatten().tolist()
        assert diff == [3 * 4 + 5, 3 * 4 + QBLOCK + 9]  # two payload bytes, no scale
        (out,) = dequantize_pack_ref([3 * QBLOCK], pd, 1)
        (ref,) = dequantize_pack_ref([3 * QBLOCK], pc, 1)
        nan = torch.isnan(out)
        assert nan.nonzero().flatten().tolist() == [5, QBLOCK + 9]
        assert torch.equal(out[~nan], ref[~nan])

    def test_inf_block_decodes_to_nan(self):
        t = torch.randn(2 * QBLOCK)
        t[7] = -float("inf")
        (out,) = dequantize_pack_ref([2 * QBLOCK], quantize_pack_ref([t], 1), 1)
        assert torch.isnan(out[:QBLOCK]).all()
        assert torch.isfinite(out[QBLOCK:]).all()

    def test_block_below_the_scale_overflow_is_flushed(self):
        # 448/amax = inf for amax < 448/FLT_MAX: without the flush the block's
        # zeros would become inf * 0 = NaN on the wire
        t = torch.zeros(2 * QBLOCK)
        t[:4] = torch.tensor([1e-37, -2.0 ** -140, 1.0e-36, 0.0])
        t[QBLOCK] = 2.0 ** -119  # just above: live
        pack = quantize_pack_ref([t], 1)
        scales, codes = split_slices(pack, 1)
        assert scales[0, 0].item() == 0.0 and (codes[0, 0] & 0x7F == 0).all()  # +-0
        assert scales[0, 1].item() > 0 and codes[0, 1, 0].item() == 0x7E
        (out,) = dequantize_pack_ref([2 * QBLOCK], pack, 1)
        assert (out[:QBLOCK] == 0).all()
        # the dequant scale 2^-119 / 448 is itself subnormal (21 bits left)
        assert abs(out[QBLOCK].item() / 2.0 ** -119 - 1) < 2.0 ** -20

    def test_reduce_ref_exact_integers_and_avg_scale(self):
        from torchft_amd.quantization import reduce_slices_ref

        # two ranks, one block each: 448*2^k pins the scale to 2^k
        a = torch.zeros(QBLOCK); a[:3] = torch.tensor([448.0, 3.0, -16.0])
        b = torch.zeros(QBLOCK); b[:3] = torch.tensor([896.0, 30.0, 16.0])
        recv = torch.cat([quantize_pack_ref([a], 1), quantize_pack_ref([b], 1)])
        for fused in (False, True):
            s = reduce_slices_ref(recv, 2, avg=False, fused=fused)
            v = reduce_slices_ref(recv, 2, avg=True, fused=fused)
            assert torch.equal(s[4:], v[4:])
            ss, cs = split_slices(s, 1)
            sv, _ = split_slices(v, 1)
            assert ss.item() == 3.0 and sv.item() == 1.5  # amax 1344 / 448
            assert cs[0, 0, :3].tolist() == [0x7E, 0x53, 0x00]  # 448, 11 = 1.375 * 2^3, 0

    def test_block_scales_are_correctly_rounded_quotients(self):
        # torch's scalar / tensor is scalar * reciprocal(tensor), up to 1.5 ulp
        # off; the device divides. With amax = 960 every multiple of 15 sits on
        # or next to an e4m3 tie, so one ulp of 448/amax changes codes.
        from torchft_amd.quantization import block_scales_ref

        amax = torch.tensor([960.0, 3744.0, 832.0, 3.0, 1e-3])
        blocks = torch.zeros(amax.numel(), QBLOCK)
        blocks[:, 7] = -amax
        got_amax, q, dq = block_scales_ref(blocks)
        assert torch.equal(got_amax, amax)
        assert torch.equal(q, (448.0 / amax.double()).float())
        assert torch.equal(dq, (amax.double() / 448.0).float())
        assert q[0].item() != (448.0 / amax)[0].item()  # what the old reference used
