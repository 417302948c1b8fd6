"""The MXFP4 trio of csrc/kernels/mxfp4_quant.hip bit for bit against the CPU
reference of torchft_amd/quantization.py (docs/KERNELS.md, "mxfp4_quant.hip"):
every byte of the quantizer's pack, every bit of the dequantizer's output and
nothing outside it, every byte of the reducer's slice, the bindings' refusals
and the collective's route. Inputs: tests/mxfp4_check.py."""

import functools

import pytest
import torch
from torch.distributed import ReduceOp

import mxfp4_check as mc
from torchft_amd import ops
from torchft_amd import quantization as Q
from torchft_amd.collectives import allreduce_quantized
from torchft_amd.process_group import ProcessGroupDummy

pytestmark = pytest.mark.gpu

QBLOCK = Q.QBLOCK
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked test without a HIP device"
    assert ops.have_hip_ext(), "HIP kernel extension must be loadable on a GPU box"
    return torch.device("cuda:0")


def _bits(t: torch.Tensor) -> torch.Tensor:
    """Bit patterns, every NaN as one pattern: the format says NaN, not which."""
    t = torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t)
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


@functools.lru_cache(maxsize=None)
def _case(family, dtype, world):
    """(CPU tensors, reference pack), built once and never modified."""
    ts = mc.family_list(family, dtype)
    return ts, Q.mx_quantize_pack_ref(ts, world)


@pytest.mark.parametrize("world", mc.WORLDS)
@pytest.mark.parametrize("dtype", mc.DTYPES, ids=str)
@pytest.mark.parametrize("family", mc.FAMILIES)
def test_quantize_every_byte_dequantize_every_bit_and_nothing_else(dev, family, dtype, world):
    ts, want = _case(family, dtype, world)
    total, padded, bpr, slice_bytes = Q.mx_pack_geometry(ts, world)
    assert (total, padded, slice_bytes) == (8, {1: 8, 2: 8, 3: 9, 4: 8}[world], bpr * 1088)
    assert ops.hip_ext().mxfp4_slice_bytes(ts, world) == slice_bytes
    d = [t.to(dev) for t in ts]
    pack = torch.full((world * slice_bytes,), 0xA5, dtype=torch.uint8, device=dev)
    Q.mx_quantize_pack(d, pack, world)
    torch.cuda.synchronize()
    got = pack.cpu()
    assert torch.equal(got, want), f"first differing bytes {(got != want).nonzero()[:6, 0].tolist()}"
    for x, t in zip(d, ts):
        assert torch.equal(_bits(x.cpu()), _bits(t)), "input modified"

    pack_ref = want  # dequantize: from the reference's pack
    numels = [t.numel() for t in ts]
    want = [v.to(dtype) for v in Q.mx_dequantize_pack_ref(numels, pack_ref, world)]
    # destinations: 16 B-aligned views into one sentinel-filled buffer, a gap
    # before every one
    per = 16 // ts[0].element_size()
    offsets, used = [], 0
    for n in numels:
        used = -(-used // per) * per + per
        offsets.append(used)
        used += n
    flat = torch.full((used + per,), SENTINEL, dtype=dtype, device=dev)
    outs = [flat[o : o + n].view(t.shape) for o, n, t in zip(offsets, numels, ts)]
    pack = pack_ref.to(dev)
    Q.mx_dequantize_pack(outs, pack, world)
    torch.cuda.synchronize()
    assert torch.equal(pack.cpu(), pack_ref), "pack modified"
    host = flat.cpu()
    covered = torch.zeros(flat.numel(), dtype=torch.bool)
    for o, n, w in zip(offsets, numels, want):
        assert torch.equal(_bits(host[o : o + n]), _bits(w))
        covered[o : o + n] = True
    assert (host[~covered] == SENTINEL).all(), "wrote outside the output views"


BPR = 5  # blocks per slice in the reduce tests: odd, more than one workgroup


def _recv(world, nan):
    """`world` reference slices of randn at different sizes; with `nan`, rank
    world - 1 holds a NaN in block 1 and an Inf in block 4."""
    gen = torch.Generator().manual_seed(900 + world)
    xs = [(1 + 0.5 * r) * torch.randn(BPR * QBLOCK, generator=gen) for r in range(world)]
    if nan:
        xs[-1][QBLOCK + 77] = float("nan")
        xs[-1][4 * QBLOCK + 2047] = float("inf")
    return torch.cat([Q.mx_quantize_pack_ref([x], 1) for x in xs])


@pytest.mark.parametrize("nan", [False, True], ids=["randn", "nan"])
@pytest.mark.parametrize("avg", [False, True], ids=["sum", "avg"])
@pytest.mark.parametrize("world", mc.WORLDS)
def test_reduce_every_byte(dev, world, avg, nan):
    recv = _recv(world, nan)
    want = Q.mx_reduce_slices_ref(recv, world, avg)
    assert (Q.mx_split_slices(want, 1)[0] == Q.MX_NAN_SCALE).sum().item() == 2 * nan
    out = torch.full((recv.numel() // world,), 0xA5, dtype=torch.uint8, device=dev)
    d = recv.to(dev)
    Q.mx_reduce_slices(d, out, world, avg)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)
    assert torch.equal(d.cpu(), recv), "recv modified"


def test_bindings_refuse_before_any_launch(dev):
    ext = ops.hip_ext()
    x = torch.ones(5000, device=dev, dtype=torch.bfloat16)
    world = 2
    nbytes = world * ext.mxfp4_slice_bytes([x], world)
    room = torch.full((2 * nbytes,), 7, dtype=torch.uint8, device=dev)  # for [x, off16] too
    good = room[:nbytes]
    off16 = torch.ones(5008, device=dev, dtype=torch.bfloat16)[1:5001]
    for fn in (ext.mxfp4_quantize, ext.mxfp4_dequantize):
        for why, args in {"pack holds": ([x], good[:-1], world),
                          "pack does not start on a 4-byte": ([x[:2048]], good[1:], 1),
                          "world must be >= 1": ([x], good, 0),
                          "tensor 1 does not start on a 16-byte": ([x, off16], room, world),
                          }.items():
            with pytest.raises(RuntimeError, match=f"{fn.__name__}: {why}"):
                fn(*args)
    out = torch.full((nbytes // world,), 7, dtype=torch.uint8, device=dev)
    for why, args in {"world must be >= 1": (good, out, 0),
                      "recv must hold world slices": (good[:-1], out, world)}.items():
        with pytest.raises(RuntimeError, match=f"mxfp4_reduce: {why}"):
            ext.mxfp4_reduce(*args, False)
    torch.cuda.synchronize()
    assert (room == 7).all() and (out == 7).all() and (x == 1).all()
    # nothing but empty tensors: no launch
    empty = [torch.empty(0, device=dev, dtype=torch.bfloat16)]
    none = torch.empty(0, dtype=torch.uint8, device=dev)
    ext.mxfp4_quantize(empty, none, 3)
    ext.mxfp4_reduce(none, none.clone(), 3, True)
    ext.mxfp4_dequantize(empty, none, 3)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=str)
def test_allreduce_quantized_routes_by_wire(dev, dtype):
    t = mc.family_list("randn", dtype)[5]  # 17 x 129
    pg = ProcessGroupDummy(0, 1)
    pack = Q.mx_reduce_slices_ref(Q.mx_quantize_pack_ref([t], 1), 1, False)
    want = Q.mx_dequantize_pack_ref([t.numel()], pack, 1)[0].to(dtype).view(t.shape)
    got = {}
    for name, kw in (("mxfp4", {"wire": "mxfp4"}), ("fp8", {"wire": "fp8"}), ("default", {})):
        got[name] = t.to(dev)
        allreduce_quantized([got[name]], ReduceOp.SUM, pg, **kw).wait()
    torch.cuda.synchronize()
    assert torch.equal(_bits(got["mxfp4"].cpu()), _bits(want))
    assert torch.equal(_bits(got["fp8"].cpu()), _bits(got["default"].cpu()))
    assert not torch.equal(got["fp8"].cpu(), got["mxfp4"].cpu())
    with pytest.raises(ValueError, match="unknown wire format"):
        allreduce_quantized([got["fp8"]], ReduceOp.SUM, pg, wire="fp4")
