"""Long-context CP attention bench on one MI355X (world 1): merged-flash
CP attention (prefix+diagonal LSE merge) vs plain flash at 32k-128k.

The world-1 path is plain flash; the world>1 merge path is exercised by
pinning prefix_len explicitly. Measures fwd+bwd ms and peak memory —
the point of the flash merge is that 128k contexts run at flash memory
(the round-1 fp32-scores version OOMed by construction).

--rect: what one rank computes after the all-gather (cp_rank_attention), the
merge path against the rectangular kernels (TORCHFT_AMD_CP_RECT), both in one
process and alternated inside every round, forward + backward between device
events, ms as median [min-max] over the rounds. Default shape: the last rank
of a world-4 split of the bench shape (B=1, Hq=32, Hkv=8, s=2048, Sk=8192).
The two paths' outputs and gradients are compared first. Run on a GPU host.

    python scripts/bench_cp.py --rect [--shape B,Hq,Hkv,s] [--world W] [--rank R]

--ring: what one ring-attention rank computes from the blocks it meets
(ring_rank_attention, no process group), aten's flash + LSE merge per block
against the hand-written kernels with the carried state (TORCHFT_AMD_RING_FA),
measured the same way at the same default shape: rank + 1 blocks of s keys.

    python scripts/bench_cp.py --ring [--shape B,Hq,Hkv,s] [--world W] [--rank R]
"""
import argparse
import os, sys, time
import statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from torchft_amd.parallel.cp import _MergedFlashAttn, cp_rank_attention, ring_rank_attention

def bench(S_local, prefix, iters=5):
    B, Hq, Hkv, D = 1, 32, 8, 128
    dev = "cuda"
    q = torch.randn(B, Hq, S_local, D, device=dev, dtype=torch.bfloat16,
                    requires_grad=True)
    k = torch.randn(B, Hkv, prefix + S_local, D, device=dev, dtype=torch.bfloat16,
                    requires_grad=True)
    v = torch.randn_like(k, requires_grad=True)
    g = torch.randn(B, Hq, S_local, D, device=dev, dtype=torch.bfloat16)
    def step():
        out = _MergedFlashAttn.apply(q, k, v, prefix)
        out.backward(g)
        q.grad = k.grad = v.grad = None
    for _ in range(2): step()
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(iters): step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1000
    peak = torch.cuda.max_memory_allocated() / 2**30
    print(f"S_local={S_local} prefix={prefix} (ctx={prefix+S_local}): "
          f"{ms:8.2f} ms fwd+bwd, peak {peak:.1f} GiB", flush=True)


def bench_rect(B, Hq, Hkv, s, world, rank, rounds, iters):
    """merge (rect=False) against rect (rect=True) on the shards a model
    hands cp_attention: [B, s, H, D], K / V gathered to [B, world*s, Hkv, D]."""
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    gen = torch.Generator(device="cuda").manual_seed(0)

    def mk(S, H, grad=True):
        t = torch.randn(B, S, H, 128, device="cuda", dtype=torch.bfloat16, generator=gen)
        return t.requires_grad_(grad)

    q, k, v, g = mk(s, Hq), mk(world * s, Hkv), mk(world * s, Hkv), mk(s, Hq, False)

    def step(rect, keep=False):
        out = cp_rank_attention(q, k, v, rank, world, True, rect)
        out.backward(g)
        res = (out.detach(), q.grad, k.grad, v.grad) if keep else None
        q.grad = k.grad = v.grad = None
        return res

    alternate(step, {"merge": False, "rect": True}, rounds, iters,
              f"B={B} Hq={Hq} Hkv={Hkv} s={s} Sk={(rank + 1) * s} (rank {rank} of {world})")


def bench_ring(B, Hq, Hkv, s, world, rank, rounds, iters):
    """merge (fused=False) against fused (fused=True) on what _RingAttention
    holds: q [B, Hq, s, D] and rank + 1 contiguous KV blocks [B, Hkv, s, D] in
    hop order, the rank's own (causal) first."""
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    gen = torch.Generator(device="cuda").manual_seed(0)

    def mk(H, grad=True):
        t = torch.randn(B, H, s, 128, device="cuda", dtype=torch.bfloat16, generator=gen)
        return t.requires_grad_(grad)

    n = rank + 1
    q, g = mk(Hq), mk(Hq, False)
    ks, vs = [mk(Hkv) for _ in range(n)], [mk(Hkv) for _ in range(n)]
    leaves = [q, *ks, *vs]

    def step(fused, keep=False):
        out = ring_rank_attention(q, ks, vs, 0, fused)
        out.backward(g)
        res = (out.detach(), q.grad, torch.stack([t.grad for t in ks]),
               torch.stack([t.grad for t in vs])) if keep else None
        for t in leaves:
            t.grad = None
        return res

    alternate(step, {"merge": False, "fused": True}, rounds, iters,
              f"B={B} Hq={Hq} Hkv={Hkv} s={s}, {n} blocks (rank {rank} of {world})")


def alternate(step, paths, rounds, iters, what):
    """step(flag, keep) under each of the two paths: their results compared
    once, then timed alternately inside every round between device events."""
    (na, fa), (nb, fb) = paths.items()
    a, b = step(fa, keep=True), step(fb, keep=True)
    for name, x, y in zip(("out", "dq", "dk", "dv"), a, b):
        print(f"{name}: max |{na} - {nb}| = {(x.float() - y.float()).abs().max().item():.3e}"
              f" (max |{na}| {x.float().abs().max().item():.3e})", flush=True)
    for flag in paths.values():  # warm up
        for _ in range(3):
            step(flag)
    torch.cuda.synchronize()
    times = {n: [] for n in paths}
    for rnd in range(rounds):
        for n, flag in paths.items():
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            for _ in range(iters):
                step(flag)
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) / iters)
        print(f"round {rnd}: " + "  ".join(f"{n} {t[-1]:.3f}" for n, t in times.items()),
              flush=True)
    for n, t in times.items():
        print(f"{n}: fwd+bwd {statistics.median(t):.3f} ms [{min(t):.3f}-{max(t):.3f}] over "
              f"{rounds} rounds x {iters}, {what}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rect", action="store_true",
                    help="merge path against the rectangular kernels at one rank's shape")
    ap.add_argument("--ring", action="store_true",
                    help="one ring rank's blocks: flash + merge against the carried state")
    ap.add_argument("--shape", default="1,32,8,2048", help="B,Hq,Hkv,s (with --rect / --ring)")
    ap.add_argument("--world", type=int, default=4)
    ap.add_argument("--rank", type=int, default=-1, help="default: the last rank")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if a.rect or a.ring:
        (bench_ring if a.ring else bench_rect)(*(int(x) for x in a.shape.split(",")), a.world,
                                               a.rank % a.world, a.rounds, a.iters)
        sys.exit(0)
    for S_local, prefix in [(16384, 16384), (32768, 32768), (65536, 65536)]:
        bench(S_local, prefix)
