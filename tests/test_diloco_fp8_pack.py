"""``ops.diloco_outer_step_fp8_`` against fp64 and ``DiLoCo(fused_fp8_pack=True)``
behind a stand-in manager, one body each for the CPU (where the ops are the
fp32 reference itself) and the device. Criteria: tests/diloco_fp8_check.py."""

from unittest.mock import MagicMock

import pytest
import torch
import torch.nn as nn

import diloco_fp8_check as dc
from torchft_amd import quantization as Q
from torchft_amd.local_sgd import DiLoCo
from torchft_amd.manager import Manager
from torchft_amd.work import _DummyWork

DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("alpha", [0.0, 0.25, 0.75, 1.0])
def test_outer_step_from_pack_against_fp64(dev, dtype, world, momentum, nesterov, alpha):
    """The ``cpu`` run shows that the fp32 evaluation leaves the bf16 0.1 % cap
    room on these inputs before the kernel is held to it."""
    g0, l0, m0, pack0 = dc.outer_inputs(dtype, world)
    g, l, m = dc.run_outer(dev, dtype, world, momentum, nesterov, alpha)
    d64 = dc.decode64(pack0, world, 3)
    counts = []
    for i, b in zip(dc.GROUP, dc.FIRST):
        n = g0[i].numel()
        d = d64[b : b + -(-n // Q.QBLOCK)].reshape(-1)[:n]
        counts.append(dc.check_outer(
            (m[i], g[i], l[i]), g0[i], d, m0[i], l0[i], lr=dc.LR, momentum=momentum,
            nesterov=nesterov, alpha=alpha, label=f"{dev} tensor {i}"))
    differing, total = (sum(c) for c in zip(*counts))
    print(f"{dev} {dtype}: {differing} of {total} differ from the rounded fp64 value")
    assert differing <= 1e-3 * total


def _run_sync(dev, commit=True, **kw):
    """Two inner steps and one sync behind a stand-in manager (world 1, one
    participant, the pack allreduce the identity)."""
    torch.manual_seed(3)
    # two layers of 2048 fp32 = 8 KiB each; a 12 KiB cap cannot take both
    model = nn.Sequential(nn.Linear(32, 64, bias=False), nn.Linear(64, 32, bias=False)).to(dev)
    inner = torch.optim.SGD(model.parameters(), lr=0.1)
    outer = torch.optim.SGD(model.parameters(), lr=dc.LR, momentum=0.9, nesterov=True)
    # the parameters before the window and, taken at pack_world(), as the sync finds them
    start, local = [p.detach().cpu().clone() for p in model.parameters()], []
    mgr = MagicMock(spec=Manager)
    mgr._use_async_quorum = False
    mgr.current_step.return_value = 0
    mgr.should_commit.return_value = commit
    mgr.num_participants.return_value = 1
    mgr.allreduce_pack.side_effect = lambda pack, world: _DummyWork(pack)
    mgr.pack_world.side_effect = lambda: local.extend(
        p.detach().cpu().clone() for p in model.parameters()) or 1
    kw = dict(dict(fused_sync=True, should_quantize=True, fused_fp8_pack=True), **kw)
    d = DiLoCo(mgr, [model], inner, outer, sync_every=2, fragment_update_alpha=0.25,
               bucket_cap_mb=12 / 1024, **kw)
    gen = torch.Generator().manual_seed(8)
    with d:
        for _ in range(2):
            for p in model.parameters():
                p.grad = torch.randn(p.shape, generator=gen).to(dev)
            inner.step()
    assert d._fragments[0]._fused_packs == [], "packs kept after the sync"
    return start, local, model, outer, mgr, d._fragments[0].original_parameters.values()


@pytest.mark.parametrize("dev", DEVICES)
def test_committed_sync_matches_the_reference_pipeline(dev):
    start, local, model, outer, mgr, snaps = _run_sync(dev)
    assert mgr.allreduce.call_count == 0 and mgr.allreduce_pack.call_count == 2
    for p, snap, g0, l0 in zip(model.parameters(), snaps, start, local):
        assert not torch.equal(g0, l0)
        d64 = dc.decode64(Q.quantize_pack_ref([g0 - l0], 1), 1, 1).reshape(-1)
        dc.check_outer((outer.state[p]["momentum_buffer"], snap, p), g0, d64,
                       torch.zeros_like(g0), l0, lr=dc.LR, momentum=0.9, nesterov=True,
                       alpha=0.25, label=f"{dev} {tuple(p.shape)}")


@pytest.mark.parametrize("dev", DEVICES)
def test_failed_commit_restores_the_parameters(dev):
    start, _, model, outer, _, snaps = _run_sync(dev, commit=False)
    for p, snap, s in zip(model.parameters(), snaps, start):
        assert torch.equal(p.detach().cpu(), s) and torch.equal(snap.cpu(), s)
    assert not outer.state_dict()["state"]


@pytest.mark.parametrize("missing", ["fused_sync", "should_quantize"])
def test_constructor_needs_both_flags(missing):
    with pytest.raises(ValueError, match="fused_fp8_pack needs"):
        _run_sync("cpu", **{missing: False})
