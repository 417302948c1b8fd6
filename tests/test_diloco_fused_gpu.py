"""The fused DiLoCo outer sync on the device: csrc/kernels/diloco_sync.hip
through ``ops.pseudograd_`` / ``ops.diloco_outer_step_``, and
``DiLoCo(fused_sync=True)`` end to end with a device-resident model.

Error bounds of ``diloco_outer_step_`` in fp32
----------------------------------------------
The reference is the definition evaluated in fp64 with the same three
roundings to the storage dtype (``ops.diloco.diloco_outer_step_ref``). Every
fp32 rounding on a chain contributes at most ``2^-24`` times the magnitude of
the value it rounds, and that magnitude never exceeds ``S``, the sum of the
absolute values of the terms entering the output. So an output is held to
``k * 2^-24 * S`` with ``k`` the number of roundings on its chain:

``m' = mu*m + d``, ``S_m = mu|m| + |d|``
    ``float(mu)``, the product, the sum, and the reference's own rounding of
    ``m'`` to fp32: ``k = 4``.

``g' = g - lr*u``, ``S_g = |g| + lr*S_u`` with ``S_u = S_m`` (momentum),
``|d| + mu*S_m`` (Nesterov) or ``|d|`` (no momentum)
    the three roundings of ``m'`` that ``u`` inherits (the stored, rounded
    ``m'`` is not on this chain), Nesterov's product and sum, ``float(lr)``,
    the product ``lr*u`` and the subtraction: ``k = 8``. The reference's final
    rounding would make nine; the bound stays at eight, the tighter figure.

``p`` from ``l`` and ``gs = g'``, ``S_p = |l| + |g'|``
    ``float(alpha)``, ``l - gs``, ``1 - alpha``, the product, the final sum and
    the reference's rounding: ``k = 6`` on ``S_p``, plus the budget of ``g'``
    itself, because the kernel's ``g'`` (which it lerps from) may differ from
    the reference's by that much.

The same formulas evaluated in fp32 on the CPU, at 400k elements and every
combination below, stay within 2.0 (``m'``) and 3.7 (``g'``) times
``2^-24 * S``, and ``p`` within 1.8 times ``2^-24 * (S_p + S_g)``, a quarter
of its bound. fma contraction on the device removes roundings, it adds none.
The worst ratios seen are printed by the test (``p`` against
``2^-24 * (S_p + S_g)``).

In bf16 the fp32 math is far below the bf16 rounding step, so every output
must be within one bf16 ulp of the rounded fp64 value and at most 0.1 % of
the elements may differ at all (a rounding tie broken the other way); only
arithmetic carried out in bf16 would exceed that.
"""

from concurrent.futures import ThreadPoolExecutor
from datetime import timedelta
from typing import Dict, Optional

import pytest
import torch
import torch.nn as nn
from torch.distributed import TCPStore

from torchft_amd import ops
from torchft_amd._ftcore import LighthouseServer
from torchft_amd.local_sgd import DiLoCo
from torchft_amd.manager import Manager
from torchft_amd.ops.diloco import diloco_outer_step_ref
from torchft_amd.process_group import ProcessGroupGloo

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (7,), (8,), (2047,), (2048,), (2049,), (5000,), (100, 33)]
DTYPES = [torch.bfloat16, torch.float32]
U32 = 2.0 ** -24
LR = 0.7
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked test without a HIP device"
    assert ops.have_hip_ext(), "HIP kernel extension must be loadable on a GPU box"
    return torch.device("cuda:0")


_INPUTS: Dict = {}


def _inputs(dtype):
    """CPU inputs at the scales of a DiLoCo sync, generated once per dtype and
    never modified: g ~ N(0,1), l - g ~ 0.01, d ~ 0.01, m ~ 0.02."""
    if dtype not in _INPUTS:
        gen = torch.Generator().manual_seed(1234)
        g = [torch.randn(s, generator=gen).to(dtype) for s in SHAPES]
        l = [(x.float() + 0.01 * torch.randn(x.shape, generator=gen)).to(dtype)
             for x in g]
        d = [(0.01 * torch.randn(s, generator=gen)).to(dtype) for s in SHAPES]
        m = [(0.02 * torch.randn(s, generator=gen)).to(dtype) for s in SHAPES]
        _INPUTS[dtype] = (g, l, d, m)
    return _INPUTS[dtype]


def _to(ts, dev):
    return [t.to(dev) for t in ts]


def _misaligned(ts, dev):
    """Copies of ``ts`` that start one element into their buffers."""
    out = []
    for t in ts:
        buf = torch.full((t.numel() + 1,), SENTINEL, dtype=t.dtype, device=dev)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        out.append(v)
    return out


def _ordered(t: torch.Tensor) -> torch.Tensor:
    """bf16 bit patterns as integers ordered like the values (+0 == -0)."""
    i = t.view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


# ---------------------------------------------------------------------------
# pseudograd_
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
def test_pseudograd_matches_torch_and_stays_in_its_views(dev, dtype):
    g, l, _, _ = _inputs(dtype)
    a, b = _to(g, dev), _to(l, dev)
    # the outputs are views into one flat buffer, 16 B aligned, with gaps
    per = 16 // a[0].element_size()
    offsets, used = [], 0
    for t in a:
        used = -(-used // per) * per + per  # a gap before every slot
        offsets.append(used)
        used += t.numel()
    flat = torch.full((used + per,), SENTINEL, dtype=dtype, device=dev)
    outs = [flat[o : o + t.numel()].view(t.shape) for o, t in zip(offsets, a)]
    assert all(o.data_ptr() % 16 == 0 for o in outs)
    ops.pseudograd_(outs, a, b)
    torch.cuda.synchronize()
    covered = torch.zeros(flat.numel(), dtype=torch.bool, device=dev)
    for o, off, x, y in zip(outs, offsets, a, b):
        assert torch.equal(o, x - y)
        covered[off : off + o.numel()] = True
    assert (flat[~covered] == SENTINEL).all(), "wrote outside the output views"
    for x, y, x0, y0 in zip(a, b, g, l):  # inputs untouched
        assert torch.equal(x.cpu(), x0) and torch.equal(y.cpu(), y0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("only_out", [False, True])
def test_pseudograd_misaligned(dev, dtype, only_out):
    n = 4097
    gen = torch.Generator().manual_seed(5)
    a_cpu = torch.randn(n + 1, generator=gen).to(dtype)
    b_cpu = torch.randn(n + 1, generator=gen).to(dtype)
    a_buf, b_buf = a_cpu.to(dev), b_cpu.to(dev)
    out_buf = torch.full((n + 2,), SENTINEL, dtype=dtype, device=dev)
    out = out_buf[1 : n + 1]
    a = a_buf[:n] if only_out else a_buf[1 : n + 1]
    b = b_buf[:n] if only_out else b_buf[1 : n + 1]
    assert out.data_ptr() % 16 != 0
    assert (a.data_ptr() % 16 != 0) == (not only_out)
    assert (b.data_ptr() % 16 != 0) == (not only_out)
    ops.pseudograd_([out], [a], [b])
    torch.cuda.synchronize()
    assert torch.equal(out, a - b)
    assert out_buf[0] == SENTINEL and out_buf[-1] == SENTINEL


def test_pseudograd_skips_empty_tensors_and_rejects_mixed_dtypes(dev):
    a = [torch.ones(5, device=dev), torch.empty(0, device=dev), torch.ones(3, device=dev)]
    b = [torch.full_like(t, 0.25) for t in a]
    outs = [torch.full_like(t, SENTINEL) for t in a]
    ops.pseudograd_(outs, a, b)
    assert torch.equal(outs[0], a[0] - b[0]) and torch.equal(outs[2], a[2] - b[2])
    ops.pseudograd_([outs[1]], [a[1]], [b[1]])  # nothing but empties: no launch
    with pytest.raises(TypeError, match="mixed dtypes"):
        ops.pseudograd_([outs[0].bfloat16()], [a[0]], [b[0]])


# ---------------------------------------------------------------------------
# diloco_outer_step_
# ---------------------------------------------------------------------------


def _check_outer_step(dev, dtype, momentum, nesterov, alpha, place, label):
    g0, l0, d0, m0 = _inputs(dtype)
    g, l, d, m = (place(t, dev) for t in (g0, l0, d0, m0))
    bufs = m if momentum else None
    ops.diloco_outer_step_(g, l, d, bufs, lr=LR, momentum=momentum,
                           nesterov=nesterov, alpha=alpha)
    torch.cuda.synchronize()
    worst = [0.0, 0.0, 0.0]
    differing = total = 0
    for i in range(len(SHAPES)):
        m_ref, g_ref, p_ref = diloco_outer_step_ref(
            g0[i], d0[i], m0[i] if momentum else None, l0[i], lr=LR,
            momentum=momentum, nesterov=nesterov, alpha=alpha,
            compute_dtype=torch.float64,
        )
        got_m, got_g, got_p = m[i].cpu(), g[i].cpu(), l[i].cpu()
        assert torch.equal(d[i].cpu(), d0[i]), "pseudo-gradient modified"
        if not momentum:
            assert torch.equal(got_m, m0[i]), "momentum buffer touched without momentum"
        if alpha == 0.0:
            assert torch.equal(got_p, got_g)
        if alpha == 1.0:
            assert torch.equal(got_p, l0[i])
        pairs = [(got_g, g_ref), (got_p, p_ref)]
        if momentum:
            pairs.append((got_m, m_ref))
        if dtype == torch.bfloat16:
            for got, ref in pairs:
                assert ((_ordered(got) - _ordered(ref)).abs() <= 1).all(), (
                    f"{label}: more than one bf16 ulp from the rounded fp64 value"
                )
                differing += int((got != ref).sum())
                total += got.numel()
            continue
        dd, mm, gg, ll = (x.double().abs() for x in (d0[i], m0[i], g0[i], l0[i]))
        s_u = dd
        if momentum:
            s_m = momentum * mm + dd
            err = (got_m.double() - m_ref.double()).abs()
            worst[0] = max(worst[0], float((err / (U32 * s_m)).max()))
            assert (err <= 4 * U32 * s_m).all(), f"{label}: m'"
            s_u = dd + momentum * s_m if nesterov else s_m
        s_g = gg + LR * s_u
        err = (got_g.double() - g_ref.double()).abs()
        worst[1] = max(worst[1], float((err / (U32 * s_g)).max()))
        assert (err <= 8 * U32 * s_g).all(), f"{label}: g'"
        s_p = ll + g_ref.double().abs()
        err = (got_p.double() - p_ref.double()).abs()
        worst[2] = max(worst[2], float((err / (U32 * (s_p + s_g))).max()))
        assert (err <= 6 * U32 * s_p + 8 * U32 * s_g).all(), f"{label}: p"
    if dtype == torch.bfloat16:
        print(f"{label}: {differing} of {total} bf16 outputs differ from the "
              "rounded fp64 value")
        assert differing <= 1e-3 * total
    else:
        print(f"{label}: worst error / (2^-24 * S): m' {worst[0]:.2f}, "
              f"g' {worst[1]:.2f}, p {worst[2]:.2f}")
    return g, l, m


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("alpha", [0.0, 0.25, 0.75, 1.0])
def test_outer_step_against_fp64(dev, dtype, momentum, nesterov, alpha):
    label = f"{dtype} mu={momentum} nesterov={nesterov} alpha={alpha}"
    _check_outer_step(dev, dtype, momentum, nesterov, alpha, _to, label)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("alpha", [0.0, 0.25, 0.75, 1.0])
def test_outer_step_misaligned(dev, dtype, alpha):
    """Every operand one element off a 16 B boundary: the element-wise path."""
    label = f"misaligned {dtype} alpha={alpha}"
    _check_outer_step(dev, dtype, 0.9, True, alpha, _misaligned, label)


@pytest.mark.parametrize("dtype", DTYPES)
def test_outer_step_only_parameter_misaligned(dev, dtype):
    """One misaligned pointer is enough to send a tensor down the element-wise
    path; the sentinels around the parameter must survive."""
    g0, l0, d0, m0 = _inputs(dtype)
    g, d, m = _to(g0, dev), _to(d0, dev), _to(m0, dev)
    bufs = [torch.full((t.numel() + 2,), SENTINEL, dtype=dtype, device=dev) for t in l0]
    l = [b[1:-1].view(t.shape) for b, t in zip(bufs, l0)]
    for v, t in zip(l, l0):
        v.copy_(t)
        assert v.data_ptr() % 16 != 0
    ops.diloco_outer_step_(g, l, d, m, lr=LR, momentum=0.9, nesterov=True, alpha=0.25)
    # the aligned run of the same inputs is the expectation, bit for bit
    g2, l2, d2, m2 = (_to(t, dev) for t in (g0, l0, d0, m0))
    ops.diloco_outer_step_(g2, l2, d2, m2, lr=LR, momentum=0.9, nesterov=True,
                           alpha=0.25)
    torch.cuda.synchronize()
    for i in range(len(SHAPES)):
        assert torch.equal(g[i], g2[i]) and torch.equal(m[i], m2[i])
        assert torch.equal(l[i], l2[i])
        assert bufs[i][0] == SENTINEL and bufs[i][-1] == SENTINEL


@pytest.mark.parametrize("dtype", DTYPES)
def test_outer_step_is_deterministic(dev, dtype):
    g0, l0, d0, m0 = _inputs(dtype)
    runs = []
    for _ in range(2):
        g, l, d, m = (_to(t, dev) for t in (g0, l0, d0, m0))
        ops.diloco_outer_step_(g, l, d, m, lr=LR, momentum=0.9, nesterov=True,
                               alpha=0.25)
        runs.append((g, l, m))
    torch.cuda.synchronize()
    for xs, ys in zip(runs[0], runs[1]):
        for x, y in zip(xs, ys):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_outer_step_fp16(dev):
    """The third dtype_code, at one configuration."""
    g0, l0, d0, m0 = _inputs(torch.float16)
    g, l, d, m = (_to(t, dev) for t in (g0, l0, d0, m0))
    ops.diloco_outer_step_(g, l, d, m, lr=LR, momentum=0.9, nesterov=True, alpha=0.25)
    torch.cuda.synchronize()
    differing = total = 0
    for i in range(len(SHAPES)):
        refs = diloco_outer_step_ref(
            g0[i], d0[i], m0[i], l0[i], lr=LR, momentum=0.9, nesterov=True,
            alpha=0.25, compute_dtype=torch.float64,
        )
        for got, ref in zip((m[i], g[i], l[i]), refs):
            got = got.cpu()
            # one fp16 ulp of the larger magnitude
            ulp = torch.maximum(got.abs(), ref.abs()).float().clamp(min=2.0 ** -14)
            ulp = 2.0 ** (torch.floor(torch.log2(ulp)) - 10)
            assert ((got.float() - ref.float()).abs() <= ulp).all()
            differing += int((got != ref).sum())
            total += got.numel()
    assert differing <= 1e-3 * total


def test_outer_step_rejects_bad_arguments(dev):
    g = [torch.zeros(8, device=dev)]
    with pytest.raises(ValueError, match="momentum_bufs"):
        ops.diloco_outer_step_(g, g, g, None, lr=0.1, momentum=0.9, nesterov=False,
                               alpha=0.0)
    with pytest.raises(TypeError, match="mixed dtypes"):
        ops.diloco_outer_step_(g, [g[0].bfloat16()], g, None, lr=0.1, momentum=0.0,
                               nesterov=False, alpha=0.0)
    with pytest.raises(ValueError, match="contiguous"):
        t = torch.zeros(4, 4, device=dev)
        ops.diloco_outer_step_([t.t()], [t.t()], [t.t()], None, lr=0.1, momentum=0.0,
                               nesterov=False, alpha=0.0)


# ---------------------------------------------------------------------------
# DiLoCo(fused_sync=True) end to end on the device
# (harness of tests/test_gpu_integration.py::TestDiLoCoOnGPU)
# ---------------------------------------------------------------------------


def _model(dev) -> nn.Module:
    m = nn.Sequential(nn.Linear(32, 64, bias=False), nn.Linear(64, 32, bias=False))
    with torch.no_grad():
        for i, p in enumerate(m.parameters()):
            vals = torch.arange(p.numel(), dtype=torch.float32).reshape(p.shape)
            p.copy_(vals * 1e-3 - 0.01 * (i + 1))
    return m.to(dev)


def _diloco_replica_gpu(
    replica_id: int,
    lighthouse_addr: str,
    tag: str,
    fused: bool,
    one_fragment: bool,
    bucket_cap_mb: Optional[float],
) -> Dict[str, torch.Tensor]:
    dev = torch.device("cuda:0")
    store = TCPStore("127.0.0.1", 0, is_master=True, wait_for_workers=False)
    model = _model(dev)
    fragments = [model] if one_fragment else [model[0], model[1]]
    inner_opt = torch.optim.SGD(model.parameters(), lr=0.05)
    outer_opts = [
        torch.optim.SGD(f.parameters(), lr=0.5, momentum=0.9, nesterov=True)
        for f in fragments
    ]
    manager = Manager(
        pg=ProcessGroupGloo(timeout=timedelta(seconds=30)),
        load_state_dict=model.load_state_dict,
        state_dict=model.state_dict,
        min_replica_size=2,
        use_async_quorum=False,
        init_sync=False,
        rank=0,
        world_size=1,
        store_addr="127.0.0.1",
        store_port=store.port,
        lighthouse_addr=lighthouse_addr,
        replica_id=f"{tag}_{replica_id}",
        hostname="127.0.0.1",
        timeout=timedelta(seconds=30),
    )
    try:
        diloco = DiLoCo(
            manager, fragments, inner_opt, outer_opts, sync_every=2,
            pin_memory=not fused, fragment_update_alpha=0.25,
            bucket_cap_mb=bucket_cap_mb, fused_sync=fused,
        )
        allreduces = 0
        real_allreduce = manager.allreduce

        def counting_allreduce(*args, **kwargs):
            nonlocal allreduces
            allreduces += 1
            return real_allreduce(*args, **kwargs)

        manager.allreduce = counting_allreduce
        with diloco:
            step = 0
            while manager.current_step() < 2:
                x = (
                    torch.arange(4 * 32, device=dev, dtype=torch.float32).reshape(4, 32)
                    * 1e-3
                    * (replica_id + 1 + step)
                )
                inner_opt.zero_grad()
                model(x).square().mean().backward()
                inner_opt.step()
                step += 1
        torch.cuda.synchronize()
        out = {
            f"snapshot_{i}_{k}": v.detach().cpu().clone()
            for i, frag in enumerate(diloco._fragments)
            for k, v in frag.original_parameters.items()
        }
        if fused:
            for frag in diloco._fragments:
                for v in frag.original_parameters.values():
                    assert v.device == dev, "fused snapshot must live on the device"
        out.update(
            {f"live_{k}": p.detach().cpu().clone() for k, p in model.named_parameters()}
        )
        out["allreduces"] = torch.tensor(allreduces)
        return out
    finally:
        manager.shutdown(wait=False)


def _run_pair_gpu(tag, fused, one_fragment=False, bucket_cap_mb=None):
    lh = LighthouseServer(bind="127.0.0.1:0", min_replicas=2, join_timeout_ms=100)
    try:
        with ThreadPoolExecutor(max_workers=2) as ex:
            futs = [
                ex.submit(_diloco_replica_gpu, i, lh.address(), tag, fused,
                          one_fragment, bucket_cap_mb)
                for i in range(2)
            ]
            return [f.result(timeout=120) for f in futs]
    finally:
        lh.shutdown()


def _assert_fused_matches_unfused(fused, unfused):
    a, b = fused
    for k in a:
        if k.startswith("snapshot_"):
            assert torch.equal(a[k], b[k]), f"fused replicas differ at {k}"
    for k in a:
        if k != "allreduces":
            torch.testing.assert_close(
                a[k], unfused[0][k], rtol=1e-5, atol=1e-6, msg=f"fused vs unfused at {k}"
            )


class TestFusedDiLoCoOnGPU:
    def test_two_fragments_match_unfused(self, dev):
        fused = _run_pair_gpu("fg2", True)
        unfused = _run_pair_gpu("ug2", False)
        _assert_fused_matches_unfused(fused, unfused)
        # two outer steps, one fragment each, one bucket per fragment
        assert int(fused[0]["allreduces"]) == 2

    def test_cap_splits_one_fragment_into_two_buckets(self, dev):
        # both layers hold 2048 fp32 = 8 KiB; a 12 KiB cap cannot take both
        cap_mb = 12 / 1024
        fused = _run_pair_gpu("fg1", True, one_fragment=True, bucket_cap_mb=cap_mb)
        unfused = _run_pair_gpu("ug1", False, one_fragment=True)
        _assert_fused_matches_unfused(fused, unfused)
        # sync_every=2 with one fragment: two outer steps of two buckets each
        assert int(fused[0]["allreduces"]) == 4
