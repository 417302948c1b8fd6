"""pseudograd_fp8_kernel / outer_sgd_fp8_kernel (csrc/kernels/diloco_sync.hip)
on the device, their bindings' refusals and the pack collective at world 1;
the outer step against fp64 is in tests/test_diloco_fp8_pack.py. Pack bytes are
exact (one fp32 subtraction, an fmaxf tree, two correctly rounded quotients, one
product, one conversion; nothing to contract): ``quantize_pack_ref``'s bytes."""

import pytest
import torch
from torch.distributed import ReduceOp, TCPStore

import diloco_fp8_check as dc
import fp8_check as fc
from torchft_amd import ops
from torchft_amd import quantization as Q
from torchft_amd.collectives import allreduce_pack
from torchft_amd.process_group import ProcessGroupRCCL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _pair(family, dtype):
    """(a, b): a family and zeros, two randn lists (their fp32 difference is not
    representable in T), or those with an Inf and a NaN in two blocks."""
    if family in fc.FAMILIES:
        a = fc.family_list(family, dtype)
        return a, [torch.zeros_like(t) for t in a]
    gen = torch.Generator().manual_seed(31)
    a = [torch.randn(s, generator=gen).to(dtype) for s in fc.SHAPES]
    b = [torch.randn(s, generator=gen).to(dtype) for s in fc.SHAPES]
    if family == "nonfinite":
        a[4][5], a[5][3, 7] = float("inf"), float("nan")
    return a, b


@pytest.mark.parametrize("dtype", fc.DTYPES)
@pytest.mark.parametrize("world", fc.WORLDS)
@pytest.mark.parametrize("family", fc.FAMILIES + ["pair", "nonfinite"])
def test_pack_bytes_are_the_reference(dtype, world, family):
    a, b = _pair(family, dtype)
    want = Q.quantize_pack_ref([x.float() - y.float() for x, y in zip(a, b)], world)
    pack = torch.full((want.numel(),), 0xA5, dtype=torch.uint8, device=DEV)
    ops.pseudograd_fp8_(pack, [t.to(DEV) for t in a], [t.to(DEV) for t in b], world)
    got_s, got_c = Q.split_slices(pack.cpu(), world)
    want_s, want_c = Q.split_slices(want, world)
    assert torch.equal(got_s.view(torch.int32), want_s.view(torch.int32)), "scales"
    assert fc.same_codes(got_c, want_c), "payload"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_outer_step_element_path_and_determinism(dtype):
    """A second identical call, and one with ``l`` as ``buf[1:]`` views (the
    element path), give the bits of the first."""
    runs = [dc.run_outer(DEV, dtype, 3, 0.9, True, 0.25, misalign_l=mis)
            for mis in (False, False, True)]
    assert all(t.data_ptr() % 16 for t in runs[2][1] if t.numel())
    for other in runs[1:]:
        for xs, ys in zip(runs[0], other):
            assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8))
                       for x, y in zip(xs, ys))


def _good():
    a = [torch.ones(4096, device=DEV), torch.ones(100, device=DEV)]
    return dict(a=a, b=[torch.ones_like(t) for t in a], m=[torch.ones_like(t) for t in a],
                pack=torch.full((3 * 2052,), 0xA5, dtype=torch.uint8, device=DEV),
                world=1, first=[0, 2], total=3, momentum=0.9)

REFUSALS = {  # what the message must say -> the one argument made wrong
    "mixed dtypes": lambda c: c["b"].__setitem__(1, c["b"][1].bfloat16()),
    "one device": lambda c: c["b"].__setitem__(1, c["b"][1].cpu()),
    "size mismatch": lambda c: c["b"].__setitem__(1, torch.ones(99, device=DEV)),
    "tensors must be contiguous": lambda c: c["b"].__setitem__(
        0, torch.ones(4096, 2, device=DEV)[:, 0]),
    "pack must be uint8": lambda c: c.update(pack=c["pack"].view(torch.int8)),
    "pack must be on": lambda c: c.update(pack=c["pack"].cpu()),
    "pack must be contiguous": lambda c: c.update(pack=c["pack"].repeat(2)[::2]),
    "pack holds": lambda c: c.update(pack=c["pack"][:-1]),
    "world must be >= 1": lambda c: c.update(world=0),
    r"first_blocks\[0\] = -1": lambda c: c.update(first=[-1, 2]),
    r"first_blocks\[0\] = 2": lambda c: c.update(first=[2, 0]),
    "momentum_bufs are needed": lambda c: c.update(momentum=0.0),
    "momentum_bufs are needed exactly": lambda c: c.update(m=[]),
}


@pytest.mark.parametrize("match", REFUSALS)
def test_bindings_refuse_before_any_launch(match):
    c = _good()
    REFUSALS[match](c)
    ext, before = ops.hip_ext(), c["pack"].clone()
    calls = [lambda: ext.diloco_outer_step_fp8(c["a"], c["b"], c["pack"], c["first"],
                                               c["total"], c["world"], c["m"], 0.1,
                                               c["momentum"], False, 0.5, 1.0)]
    if "first_blocks" not in match and "momentum" not in match:
        calls.append(lambda: ext.diloco_pseudograd_fp8(c["a"], c["b"], c["pack"], c["world"]))
    for call in calls:
        with pytest.raises(RuntimeError, match=match):
            call()
    torch.cuda.synchronize()
    assert torch.equal(c["pack"], before)
    assert all((t == 1).all() for ts in (c["a"], c["b"], c["m"]) for t in ts)


def test_allreduce_pack_world1_is_the_requantizing_reduce():
    store = TCPStore("127.0.0.1", 0, is_master=True, wait_for_workers=False)
    pg = ProcessGroupRCCL()
    pg.configure(f"127.0.0.1:{store.port}/p", "r0", 0, 1)
    pack0 = dc.outer_inputs(torch.float32, 1)[3]
    pack = pack0.to(DEV)
    allreduce_pack(pack, 1, ReduceOp.SUM, pg).wait()
    torch.cuda.synchronize()
    assert torch.equal(pack.cpu(), Q.reduce_slices_ref(pack0, 1, False))
    pg.shutdown()
