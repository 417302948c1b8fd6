"""The fp8 trio of csrc/kernels/fp8_quant.hip bit for bit against the CPU
reference of torchft_amd/quantization.py (docs/KERNELS.md, "Numerics" of
fp8_quant.hip): every byte of the quantizer's pack, every bit of the
dequantizer's output and nothing outside it, the reducer on inputs whose sums
are exact, under a derived bound on randn, non-finite input, and the bindings'
refusals. Inputs: tests/fp8_check.py."""

import pytest
import torch

import fp8_check as fc
from torchft_amd import ops
from torchft_amd import quantization as Q

pytestmark = pytest.mark.gpu

QBLOCK = Q.QBLOCK
SENTINEL = 7.0
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked test without a HIP device"
    assert ops.have_hip_ext(), "HIP kernel extension must be loadable on a GPU box"
    return torch.device("cuda:0")


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


_CASES = {}


def _case(family, dtype, world):
    """(CPU tensors, reference pack), built once and never modified."""
    key = (family, dtype, world)
    if key not in _CASES:
        if (family, dtype) not in _CASES:
            _CASES[(family, dtype)] = fc.family_list(family, dtype)
        ts = _CASES[(family, dtype)]
        _CASES[key] = (ts, Q.quantize_pack_ref(ts, world))
    return _CASES[key]


def _describe_mismatch(ts, got, want, world) -> str:
    """The first differing (value, scale, code) triples, for the report."""
    gs, gc = Q.split_slices(got, world)
    ws, wc = Q.split_slices(want, world)
    lines = []
    bad_scale = (_bits(gs) != _bits(ws)).reshape(-1).nonzero().flatten().tolist()
    for b in bad_scale[:5]:
        lines.append(f"block {b}: scale {gs.reshape(-1)[b].item()!r} want "
                     f"{ws.reshape(-1)[b].item()!r}")
    vals = torch.zeros(gc.numel(), dtype=torch.float64)
    off = 0
    for t in ts:
        vals[off : off + t.numel()] = t.double().reshape(-1)
        off += -(-t.numel() // QBLOCK) * QBLOCK
    bad = (gc != wc).reshape(-1).nonzero().flatten().tolist()
    for i in bad[:10]:
        lines.append(f"element {i}: value {vals[i].item()!r} scale "
                     f"{ws.reshape(-1)[i // QBLOCK].item()!r} code "
                     f"{gc.reshape(-1)[i].item():#04x} want {wc.reshape(-1)[i].item():#04x}")
    return f"{len(bad_scale)} scales and {len(bad)} codes differ; " + "; ".join(lines)


# ---------------------------------------------------------------------------
# quantize
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("world", fc.WORLDS)
@pytest.mark.parametrize("dtype", fc.DTYPES, ids=str)
@pytest.mark.parametrize("family", fc.FAMILIES)
def test_quantize_every_byte(dev, family, dtype, world):
    ts, want = _case(family, dtype, world)
    total, padded, bpr, slice_bytes = Q.pack_geometry(ts, world)
    assert (total, padded, bpr) == (8, {1: 8, 2: 8, 3: 9, 4: 8}[world], {1: 8, 2: 4, 3: 3, 4: 2}[world])
    d = [t.to(dev) for t in ts]
    pack = torch.full((world * slice_bytes,), 0xA5, dtype=torch.uint8, device=dev)
    ops.hip_ext().fp8_quantize(d, pack, world)
    torch.cuda.synchronize()
    got = pack.cpu()
    assert torch.equal(got, want), _describe_mismatch(ts, got, want, world)
    for x, t in zip(d, ts):
        assert torch.equal(_bits(x.cpu()), _bits(t)), "input modified"
    if family == "enumeration":
        # the block's codes by construction, independent of the reference
        scales, codes = Q.split_slices(got, world)
        assert scales.reshape(-1)[fc.SPECIAL].item() == 1.0
        assert torch.equal(codes.reshape(-1, QBLOCK)[fc.SPECIAL],
                           fc.enumeration_block(dtype)[1])


# ---------------------------------------------------------------------------
# dequantize
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("world", fc.WORLDS)
@pytest.mark.parametrize("dtype", fc.DTYPES, ids=str)
@pytest.mark.parametrize("family", ["randn", "enumeration", "subnormal", "wide"])
def test_dequantize_every_bit_and_nothing_else(dev, family, dtype, world):
    ts, pack_ref = _case(family, dtype, world)  # the pack is the reference's
    numels = [t.numel() for t in ts]
    want = [v.to(dtype) for v in Q.dequantize_pack_ref(numels, pack_ref, world)]
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
    assert all(o.data_ptr() % 16 == 0 for o in outs)
    pack = pack_ref.to(dev)
    ops.hip_ext().fp8_dequantize(outs, pack, world)
    torch.cuda.synchronize()
    assert torch.equal(pack.cpu(), pack_ref), "pack modified"
    host = flat.cpu()
    covered = torch.zeros(flat.numel(), dtype=torch.bool)
    for o, n, w in zip(offsets, numels, want):
        got = host[o : o + n]
        differ = (_bits(got) != _bits(w.reshape(-1))).nonzero().flatten().tolist()
        assert not differ, (
            f"{len(differ)} outputs differ, first at {differ[0]}: "
            f"{got[differ[0]].item()!r} want {w.reshape(-1)[differ[0]].item()!r}")
        covered[o : o + n] = True
    assert (host[~covered] == SENTINEL).all(), "wrote outside the output views"


# ---------------------------------------------------------------------------
# reduce
# ---------------------------------------------------------------------------

BPR = 3  # blocks per slice in the reduce tests: odd, more than one


def _reduce(dev, recv, world, avg):
    out = torch.full((recv.numel() // world,), 0xA5, dtype=torch.uint8, device=dev)
    ops.hip_ext().fp8_reduce(recv.to(dev), out, world, avg)
    torch.cuda.synchronize()
    return out.cpu()


def _exact_recv(world):
    """Slices whose blocks hold integers +-(0..15) * 2^j, j <= 4, times 2^k, and
    one element 448 * 2^k that pins the block's scale to exactly 2^k, k
    different per rank and block. Every term code * scale and every partial
    sum is an integer below 2^24: exact in fp32 with or without fma."""
    gen = torch.Generator().manual_seed(500 + world)
    slices, ints = [], torch.zeros(BPR, QBLOCK, dtype=torch.int64)
    for r in range(world):
        k = torch.tensor([(r + 2 * b) % 4 for b in range(BPR)])
        n = torch.randint(-15, 16, (BPR, QBLOCK), generator=gen)
        j = torch.randint(0, 5, (BPR, QBLOCK), generator=gen)
        v = n * 2 ** j
        v[:, r] = 448  # a different position per rank: the sums stay varied
        v = v * (2 ** k)[:, None]
        ints += v
        sl = Q.quantize_pack_ref([v.float().reshape(-1)], 1)
        scales, _ = Q.split_slices(sl, 1)
        assert scales[0].tolist() == (2.0 ** k).tolist()
        assert torch.equal(Q.dequantize_pack_ref([BPR * QBLOCK], sl, 1)[0],
                           v.float().reshape(-1)), "inputs not exact in e4m3"
        slices.append(sl)
    return torch.cat(slices), ints


@pytest.mark.parametrize("world", fc.WORLDS)
def test_reduce_exact_family_every_byte(dev, world):
    recv, ints = _exact_recv(world)
    assert ints.abs().max() < 2 ** 24
    # the expected bytes from the integer sums, not from an accumulation
    acc = ints.float()
    _, q, dq = Q.block_scales_ref(acc)
    want_codes = Q.e4m3_codes(acc * q[:, None])
    got_sum = _reduce(dev, recv, world, False)
    got_avg = _reduce(dev, recv, world, True)
    for fused in (False, True):
        assert torch.equal(Q.reduce_slices_ref(recv, world, False, fused=fused)[BPR * 4:],
                           want_codes.reshape(-1))
    s_sum, c_sum = Q.split_slices(got_sum, 1)
    s_avg, c_avg = Q.split_slices(got_avg, 1)
    assert torch.equal(c_sum[0], want_codes), "SUM payload"
    assert torch.equal(c_avg[0], want_codes), "AVG payload differs from SUM's"
    assert torch.equal(_bits(s_sum[0]), _bits(dq)), "SUM scales"
    inv = torch.tensor(1.0, dtype=torch.float32) / world
    assert torch.equal(_bits(s_avg[0]), _bits(dq * inv)), "AVG scale is not fl(fl(amax/448)*fl(1/W))"


def _randn_recv(world):
    gen = torch.Generator().manual_seed(900 + world)
    return torch.cat([
        Q.quantize_pack_ref([(1 + 0.5 * r) * torch.randn(BPR * QBLOCK, generator=gen)], 1)
        for r in range(world)])


# which fp32 evaluation of `acc += code * scale` reproduces the device's bytes:
# "fused" (one rounding per step) or "separate" (product and sum rounded)
DEVICE_ACCUMULATION = "fused"


@pytest.mark.parametrize("world", fc.WORLDS)
def test_reduce_randn_bound_and_bytes(dev, world):
    """``d = code * scale`` of the output against the fp64 sum ``x`` of the
    decoded inputs: ``|d - x| <= max(2^-4 |x|, 2^-10 dq) + c 2^-24 (sum_r
    |term_r| + amax)``. The first term is e4m3's half step (3 mantissa bits;
    2^-10 in units of the scale below the normal range). fp32: each of the W
    accumulation steps rounds a product (at most u |term_r|) and a sum (at most
    u times a partial sum, itself at most sum_r |term_r|): (W + 1) u sum_r
    |term_r|. The scale division, the product acc * q and the stored scale's
    division are relative to |acc| <= amax: 3 u amax. All of that also moves
    the value that e4m3 rounds, by at most 2^-4 of itself on top:
    c = 17/16 * max(W + 1, 3)."""
    recv = _randn_recv(world)
    scales, codes = Q.split_slices(recv, world)
    terms = Q.e4m3_values(codes).double() * scales.double()[:, :, None]
    x, s_abs = terms.sum(0), terms.abs().sum(0)
    # the fused evaluation in fp64 is exact while all operands span < 53 bits:
    # 9 bits below a scale's last place, 12 above the largest term
    e = torch.frexp(scales.reshape(-1))[1]
    assert int(e.max() - e.min()) <= 8

    got_sum = _reduce(dev, recv, world, False)
    got_avg = _reduce(dev, recv, world, True)
    s_sum, c_sum = Q.split_slices(got_sum, 1)
    s_avg, c_avg = Q.split_slices(got_avg, 1)
    assert torch.equal(c_sum, c_avg), "AVG payload differs from SUM's"
    inv = torch.tensor(1.0, dtype=torch.float32) / world
    assert torch.equal(_bits(s_avg), _bits(s_sum * inv))

    dq = s_sum[0].double()[:, None]
    d = Q.e4m3_values(c_sum[0]).double() * dq
    amax = x.abs().amax(dim=1, keepdim=True)
    c = 17 / 16 * max(world + 1, 3)
    step = torch.maximum(2.0 ** -4 * x.abs(), 2.0 ** -10 * dq)
    bound = step + c * U32 * (s_abs + amax)
    err = (d - x).abs()
    print(f"reduce randn, world {world}: worst error / bound {float((err / bound).max()):.3f} "
          f"(c = {c:.2f})")
    assert (err <= bound).all()

    match = {name: torch.equal(got_sum, Q.reduce_slices_ref(recv, world, False, fused=f))
             for name, f in (("separate", False), ("fused", True))}
    print(f"reduce randn, world {world}: bytes equal to the separate evaluation: "
          f"{match['separate']}, to the fused one: {match['fused']}")
    assert match[DEVICE_ACCUMULATION]
    assert torch.equal(got_sum, _reduce(dev, recv, world, False)), "two calls differ"


# ---------------------------------------------------------------------------
# non-finite input
# ---------------------------------------------------------------------------


def _dirty_and_clean():
    """Four blocks: 0 randn with a NaN, 1 zeros with a NaN, 2 randn with -Inf
    and +Inf, 3 randn untouched. Element 0 of the randn blocks is the amax."""
    gen = torch.Generator().manual_seed(31)
    clean = torch.randn(4 * QBLOCK, generator=gen).clamp(-4, 4)
    clean[0::QBLOCK] = 10.0
    clean[QBLOCK : 2 * QBLOCK] = 0
    dirty = clean.clone()
    nan_at = [100, QBLOCK + 200]
    dirty[nan_at] = float("nan")
    dirty[2 * QBLOCK + 5] = -float("inf")
    dirty[2 * QBLOCK + 6] = float("inf")
    return clean, dirty, nan_at


@pytest.mark.parametrize("dtype", fc.DTYPES, ids=str)
def test_nonfinite_through_quantize_and_dequantize(dev, dtype):
    clean, dirty, nan_at = _dirty_and_clean()
    clean, dirty = clean.to(dtype), dirty.to(dtype)
    packs = {}
    for name, t in (("clean", clean), ("dirty", dirty)):
        pack = torch.full((4 * (4 + QBLOCK),), 0xA5, dtype=torch.uint8, device=dev)
        ops.hip_ext().fp8_quantize([t.to(dev)], pack, 1)
        packs[name] = pack
    torch.cuda.synchronize()
    want = Q.quantize_pack_ref([dirty], 1)
    got = packs["dirty"].cpu()
    assert torch.equal(got[:16], want[:16]), "scales"
    assert Q.split_slices(got, 1)[0][0, 2].item() == float("inf")
    assert fc.same_codes(got[16:], want[16:])
    # a NaN changes its own byte and no scale; block 3 is untouched
    base = packs["clean"].cpu()
    assert torch.equal(got[:8], base[:8]) and torch.equal(got[12:16], base[12:16])
    differ = (got[16:] != base[16:]).nonzero().flatten()
    assert differ[differ < 2 * QBLOCK].tolist() == nan_at
    assert (differ < 3 * QBLOCK).all()

    outs = {}
    for name in packs:
        o = torch.full((4 * QBLOCK,), SENTINEL, dtype=dtype, device=dev)
        ops.hip_ext().fp8_dequantize([o], packs[name], 1)
        outs[name] = o
    torch.cuda.synchronize()
    d, c = outs["dirty"].cpu(), outs["clean"].cpu()
    isnan = torch.isnan(d)
    assert isnan[2 * QBLOCK : 3 * QBLOCK].all(), "a block holding Inf must decode to NaN"
    isnan[2 * QBLOCK : 3 * QBLOCK] = False
    assert isnan.nonzero().flatten().tolist() == nan_at
    keep = torch.ones(4 * QBLOCK, dtype=torch.bool)
    keep[nan_at] = False
    keep[2 * QBLOCK : 3 * QBLOCK] = False
    assert torch.equal(_bits(d[keep]), _bits(c[keep]))


@pytest.mark.parametrize("world", [2, 3])
def test_nan_through_reduce(dev, world):
    clean, dirty, nan_at = _dirty_and_clean()
    clean, dirty = clean[: 2 * QBLOCK], dirty[: 2 * QBLOCK]  # the two NaN blocks
    gen = torch.Generator().manual_seed(32)
    others = [Q.quantize_pack_ref([torch.randn(2 * QBLOCK, generator=gen)], 1)
              for _ in range(world - 1)]
    recv = {name: torch.cat(others[:1] + [Q.quantize_pack_ref([t], 1)] + others[1:])
            for name, t in (("clean", clean), ("dirty", dirty))}  # the NaN rank is rank 1
    got = {name: _reduce(dev, r, world, False) for name, r in recv.items()}
    differ = (got["dirty"] != got["clean"]).nonzero().flatten().tolist()
    assert differ == [8 + i for i in nan_at], "a NaN must change its own byte only"
    assert ((got["dirty"][differ] & 0x7F) == 0x7F).all()
    (dec,) = Q.dequantize_pack_ref([2 * QBLOCK], got["dirty"], 1)
    assert torch.isnan(dec).nonzero().flatten().tolist() == nan_at


# ---------------------------------------------------------------------------
# bindings
# ---------------------------------------------------------------------------


def test_bindings_refuse_a_bad_pack_or_world_before_any_launch(dev):
    ext = ops.hip_ext()
    torch.manual_seed(3)
    x = torch.randn(5000, device=dev, dtype=torch.bfloat16)
    x0 = x.clone()
    world = 2
    nbytes = ext.fp8_pack_bytes([x], world)
    good = torch.full((nbytes,), 7, dtype=torch.uint8, device=dev)
    bad_packs = {
        "pack must be on the tensors' device": torch.full((nbytes,), 7, dtype=torch.uint8),
        "pack holds": good[:-1],
        "pack must be contiguous": torch.full((2 * nbytes,), 7, dtype=torch.uint8,
                                              device=dev)[::2],
        "pack must be uint8": torch.full((nbytes,), 7, dtype=torch.int8, device=dev),
    }
    for fn in ("fp8_quantize", "fp8_dequantize"):
        for why, pack in bad_packs.items():
            with pytest.raises(RuntimeError, match=f"{fn}: {why}"):
                getattr(ext, fn)([x], pack, world)
            torch.cuda.synchronize()
            assert (pack == 7).all(), "pack written by a refused call"
        for w in (0, -1):
            with pytest.raises(RuntimeError, match=f"{fn}: world must be >= 1"):
                getattr(ext, fn)([x], good, w)
    for w in (0, -2):
        with pytest.raises(RuntimeError, match="fp8_pack_bytes: world must be >= 1"):
            ext.fp8_pack_bytes([x], w)
        with pytest.raises(RuntimeError, match="fp8_slice_bytes: world must be >= 1"):
            ext.fp8_slice_bytes([x], w)
    torch.cuda.synchronize()
    assert (good == 7).all() and torch.equal(_bits(x), _bits(x0))

    out = torch.full((nbytes // world,), 7, dtype=torch.uint8, device=dev)
    for w in (0, -1):
        with pytest.raises(RuntimeError, match="fp8_reduce: world must be >= 1"):
            ext.fp8_reduce(good, out, w, False)
    with pytest.raises(RuntimeError, match="fp8_reduce: recv must hold world slices"):
        ext.fp8_reduce(good[:-1], out, world, False)
    torch.cuda.synchronize()
    assert (out == 7).all() and (good == 7).all()

    # the same arguments, all in order, go through
    ext.fp8_quantize([x], good, world)
    ext.fp8_reduce(good, out, world, True)
    y = torch.zeros_like(x)
    ext.fp8_dequantize([y], good, world)
    torch.cuda.synchronize()
    assert y.abs().max() > 0 and torch.equal(_bits(x), _bits(x0))


@pytest.mark.parametrize("world", [1, 3])
def test_only_empty_tensors_launch_nothing(dev, world):
    ext = ops.hip_ext()
    ts = [torch.empty(0, device=dev, dtype=torch.bfloat16),
          torch.empty(0, 5, device=dev, dtype=torch.bfloat16)]
    assert ext.fp8_pack_bytes(ts, world) == 0 and ext.fp8_slice_bytes(ts, world) == 0
    pack = torch.empty(0, dtype=torch.uint8, device=dev)
    out = torch.empty(0, dtype=torch.uint8, device=dev)
    ext.fp8_quantize(ts, pack, world)
    ext.fp8_reduce(pack, out, world, True)
    ext.fp8_dequantize(ts, pack, world)
    torch.cuda.synchronize()  # a zero-sized grid would surface here as a launch error
