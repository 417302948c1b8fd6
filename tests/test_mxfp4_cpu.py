"""The MXFP4 reference of torchft_amd/quantization.py against the format's
definition (docs/KERNELS.md, "mxfp4_quant.hip"), and the public route's
refusals. Inputs: tests/mxfp4_check.py."""

from unittest.mock import MagicMock

import pytest
import torch

import mxfp4_check as mc
from torchft_amd import quantization as Q
from torchft_amd.collectives import _wire
from torchft_amd.local_sgd import DiLoCo
from torchft_amd.manager import quantize_wire

G = Q.MX_GROUP


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=str)
def test_enumeration_groups_get_the_codes_of_their_construction(dtype):
    vals, want = mc.enumeration_groups(dtype)
    scales, codes = Q.mx_split_slices(Q.mx_quantize_pack_ref([vals], 1), 1)
    assert (scales[0, 0, :2] == 127).all(), "amax 6 is X = 0"
    got = torch.stack([codes & 0xF, codes >> 4], dim=-1).reshape(-1)[: vals.numel()]
    assert torch.equal(got, want)


def test_saturation_idempotence_and_decode_bound():
    """|decode - v| <= 2^X wherever |v| * 2^-X <= 6 (the widest gap of the
    grid is 2, between 4 and 6) and <= 2^(X+1) in the saturation range (6, 8)."""
    g = torch.rand(Q.QBLOCK, generator=torch.Generator().manual_seed(5)) * 4 - 2
    g[0::G] = torch.linspace(6.001, 7.999, Q.MX_GROUPS)  # amax in (6, 8): X = 0
    g[1::G] = -g[0::G]
    scales, codes = Q.mx_split_slices(Q.mx_quantize_pack_ref([g], 1), 1)
    assert (scales == 127).all() and (codes[0, 0, 0::16] == 0xF7).all()  # +6 low, -6 high
    for ts in mc.family_list("randn", torch.float32), [g]:
        for world in (1, 3):
            pack = Q.mx_quantize_pack_ref(ts, world)
            dec = Q.mx_dequantize_pack_ref([t.numel() for t in ts], pack, world)
            assert torch.equal(Q.mx_quantize_pack_ref(dec, world), pack)
        X = Q.mx_split_slices(pack, world)[0].reshape(-1).int() - 127
        step = torch.ldexp(torch.ones(()), X).repeat_interleave(G)
        b = 0
        for t, d in zip(ts, dec):
            v, s = t.reshape(-1), step[b * Q.QBLOCK : b * Q.QBLOCK + t.numel()]
            err, inside = (d - v).abs(), v.abs() <= 6 * s
            assert (err <= 2 * s).all() and (err[inside] <= s[inside]).all()
            b += -(-t.numel() // Q.QBLOCK)


def test_scale_bytes_of_zero_tiny_and_nonfinite_groups_and_of_padding():
    g = torch.zeros(4 * G)
    g[G] = 2.0 ** -124  # floor(log2) - 2 = -126: the clamp holds X at -125
    g[2 * G + 3] = float("nan")
    g[3 * G + 5], g[3 * G + 6] = -float("inf"), 1.0
    pack = Q.mx_quantize_pack_ref([g], 3)  # one block and two padding blocks
    assert pack.numel() == 3 * Q.MX_BLOCK_BYTES == 3 * 1088
    scales, codes = Q.mx_split_slices(pack, 3)
    assert scales[0, 0, :4].tolist() == [2, 2, 255, 255] and (scales.reshape(-1)[4:] == 2).all()
    want = torch.zeros(3 * Q.QBLOCK // 2, dtype=torch.uint8)
    want[G // 2] = 4  # 2^-124 * 2^125 = 2, whose code is 4, in a low nibble
    assert torch.equal(codes.reshape(-1), want)
    (dec,) = Q.mx_dequantize_pack_ref([g.numel()], pack, 3)
    assert torch.isnan(dec[2 * G :]).all() and dec[G] == 2.0 ** -124


def test_should_quantize_values_and_wire_names():
    assert [quantize_wire(v) for v in (False, None, True, "mxfp4")] == [None, None, "fp8", "mxfp4"]
    for bad in ("fp8", "mxfp8", ""):
        with pytest.raises(ValueError, match="should_quantize"):
            quantize_wire(bad)
    with pytest.raises(ValueError, match="unknown wire format 'fp4'"):
        _wire("fp4")
    manager = MagicMock()
    manager._use_async_quorum = False
    model = torch.nn.Linear(4, 4)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    with pytest.raises(ValueError, match="should_quantize"):
        DiLoCo(manager, [model], opt, opt, sync_every=2, should_quantize="int4")
    with pytest.raises(ValueError, match="fused_fp8_pack keeps"):
        DiLoCo(manager, [model], opt, opt, sync_every=2, should_quantize="mxfp4",
               fused_sync=True, fused_fp8_pack=True)
    d = DiLoCo(manager, [model], opt, opt, sync_every=2, should_quantize="mxfp4")
    assert d._fragments[0].should_quantize == "mxfp4"
