"""A/B: fused linear + cross-entropy head vs the unfused chunked loop, the
lm-head alone at the Llama-8B bench shape (rows = 4 x 8192, dim 4096,
vocab 128256, chunk 4096), plus the fused kernel's achieved bandwidth at the
real vocab. Run on a GPU box."""
import sys, os, time, json, argparse
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from torchft_amd.ops import linear_cross_entropy
from torchft_amd.ops.cross_entropy import fused_cross_entropy_

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=32768)
ap.add_argument("--dim", type=int, default=4096)
ap.add_argument("--vocab", type=int, default=128256)
ap.add_argument("--chunk", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--kernel-iters", type=int, default=10)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_ce.py measures on a HIP device only"
dev = "cuda"
N, D, V, CH = args.rows, args.dim, args.vocab, args.chunk
torch.manual_seed(0)
h = (torch.randn(N, D, device=dev) * 1.0).to(torch.bfloat16).requires_grad_(True)
w = (torch.randn(V, D, device=dev) * 0.02).to(torch.bfloat16).requires_grad_(True)
t = torch.randint(0, V, (N,), device=dev)


def unfused_head():
    # the loop Llama.forward_loss runs with TORCHFT_AMD_FUSED_CE=0
    losses = []
    for i in range(0, N, CH):
        logits = F.linear(h[i : i + CH], w)
        losses.append(F.cross_entropy(logits, t[i : i + CH], reduction="sum").float())
    return torch.stack(losses).sum() / N


def fused_head():
    return linear_cross_entropy(h, w, t, chunk_rows=CH)


def run(head, iters):
    """(ms per fwd+bwd, peak bytes over the resident inputs, loss)"""
    def step():
        loss = head()
        loss.backward()
        h.grad = w.grad = None
        return loss.detach()
    step()  # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    for _ in range(iters):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1000
    return ms, torch.cuda.max_memory_allocated() - base, loss.item()


# interleaved A/B, as in bench_fa.py
for rnd in range(args.rounds):
    u_ms, u_peak, u_loss = run(unfused_head, args.iters)
    f_ms, f_peak, f_loss = run(fused_head, args.iters)
    print(json.dumps({
        "bench": "lm_head_fwd_bwd", "round": rnd, "rows": N, "dim": D, "vocab": V,
        "chunk": CH, "unfused_ms": round(u_ms, 2), "fused_ms": round(f_ms, 2),
        "unfused_peak_gb": round(u_peak / 1e9, 3), "fused_peak_gb": round(f_peak / 1e9, 3),
        "unfused_loss": u_loss, "fused_loss": f_loss,
    }), flush=True)

# the kernel alone on one chunk of logits; needed bytes from the shapes:
# loss only reads the chunk once, loss+grad reads it once and writes it once
# (the second read of each 256 KB row is meant to hit cache)
del h, w
torch.cuda.empty_cache()
R = min(CH, N)
src = (torch.randn(R, V, device=dev) * 4.0).to(torch.bfloat16)
buf = torch.empty_like(src)
tk = t[:R].contiguous()
gs = torch.full((1,), 1.0 / R, dtype=torch.float32, device=dev)
for write_grad in (True, False):
    times = []
    for it in range(args.kernel_iters + 2):
        buf.copy_(src)  # fresh logits each time: the kernel overwrites them
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fused_cross_entropy_(buf, tk, ignore_index=-100, z_loss=0.0, grad_scale=gs,
                             write_grad=write_grad)
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:
            times.append(e0.elapsed_time(e1))
    times.sort()
    med = times[len(times) // 2]
    need = R * V * 2 * (2 if write_grad else 1)
    print(json.dumps({
        "bench": "cross_entropy_kernel", "rows": R, "vocab": V, "write_grad": write_grad,
        "median_ms": round(med, 4), "min_ms": round(times[0], 4),
        "needed_gb": round(need / 1e9, 3), "gb_per_s": round(need / med / 1e6, 1),
        "hbm_roofline_gb_per_s": 6300,
    }), flush=True)
