"""A/B: the fused QKV split + rotary kernels (ops.qkv_rope,
csrc/kernels/qkv_rope.hip) against the three views + two rope calls they
replace, at the bench shape. Run on a GPU box.

  kernels    qkv_rope_fwd and qkv_rope_bwd alone, with the bytes each moves and
             the share of HBM bandwidth that is
  split      (a) split + rotary, forward and backward through autograd
  attention  (b) split + rotary + flash_attention, forward and backward: what
             the attention layout copies cost on the unfused path

Device events, the two paths interleaved within every round; median
[min - max] over the rounds. Outputs and the gradient of qkv are compared bit
for bit before anything is timed."""
import sys, os, json, argparse
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torchft_amd import ops
from torchft_amd.ops import hip_ext, rope_tables

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--seq", type=int, default=8192)
ap.add_argument("--heads", type=int, default=32)
ap.add_argument("--kv-heads", type=int, default=8)
ap.add_argument("--head-dim", type=int, default=128)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_qkv_rope.py measures on a HIP device only"
dev = "cuda"
B, S, Hq, Hkv, D = args.batch, args.seq, args.heads, args.kv_heads, args.head_dim
W = (Hq + 2 * Hkv) * D
HBM_PEAK_TB_S, HBM_COPY_TB_S = 8.0, 6.29  # spec; a float4 copy kernel

torch.manual_seed(0)
qkv = torch.randn(B, S, W, device=dev, dtype=torch.bfloat16, requires_grad=True)
douts = [torch.randn(B, S, h, D, device=dev, dtype=torch.bfloat16) for h in (Hq, Hkv, Hkv)]
dattn = torch.randn(B, S, Hq, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)
cos, sin = rope_tables(S, D, device=dev)
ext = hip_ext()


def fused(t):
    return ops.qkv_rope(t, cos, sin, Hq, Hkv)


def unfused(t):
    nq, nkv = Hq * D, Hkv * D
    q = t[..., :nq].view(B, S, Hq, D)
    k = t[..., nq:nq + nkv].view(B, S, Hkv, D)
    v = t[..., nq + nkv:].view(B, S, Hkv, D)
    return ops.rope(q, cos, sin), ops.rope(k, cos, sin), v


def split_step(fn):
    qkv.grad = None
    torch.autograd.backward(fn(qkv), douts)


def attention_step(fn):
    qkv.grad = None
    q, k, v = (t.transpose(1, 2) for t in fn(qkv))
    ops.flash_attention(q, k, v, causal=True).backward(dattn)


def results(step, fn):
    step(fn)
    return qkv.grad.clone()


same = {}
for name, step in (("split", split_step), ("attention", attention_step)):
    same[name] = bool(torch.equal(results(step, fused), results(step, unfused)))
same["outputs"] = all(torch.equal(a, b) for a, b in zip(fused(qkv), unfused(qkv)))

with torch.no_grad():
    q0, k0, v0 = ext.qkv_rope_fwd(qkv, cos, sin, Hq, Hkv)
VARIANTS = [
    ("kernel_fwd", lambda: ext.qkv_rope_fwd(qkv.detach(), cos, sin, Hq, Hkv)),
    ("kernel_bwd", lambda: ext.qkv_rope_bwd(q0, k0, v0, cos, sin)),
    ("split_fused", lambda: split_step(fused)),
    ("split_unfused", lambda: split_step(unfused)),
    ("attention_fused", lambda: attention_step(fused)),
    ("attention_unfused", lambda: attention_step(unfused)),
]


def timed(fn, iters):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


for _, fn in VARIANTS:  # warm-up: code objects, the allocator
    fn()
    fn()
torch.cuda.synchronize()
ms = {name: [] for name, _ in VARIANTS}
for _ in range(args.rounds):
    for name, fn in VARIANTS:
        ms[name].append(timed(fn, args.iters))


def stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4),
            "max_ms": round(v[-1], 4)}


# each kernel reads the 2 * W bytes of a token once and writes them once; the
# fp32 tables (S * D / 2 * 4 bytes each) stay in cache
moved = 2 * B * S * W * 2
out = {"bench": "qkv_rope", "shape": [B, S, Hq, Hkv, D], "rounds": args.rounds,
       "iters": args.iters, "bitwise_equal": same,
       "kernel_bytes_moved_gb": round(moved / 1e9, 4)}
for name, _ in VARIANTS:
    out[name] = stats(ms[name])
for name in ("kernel_fwd", "kernel_bwd"):
    tb_s = moved / out[name]["median_ms"] / 1e9
    out[name].update({"tb_per_s": round(tb_s, 3),
                      "share_of_hbm_peak": round(tb_s / HBM_PEAK_TB_S, 3),
                      "share_of_copy_rate": round(tb_s / HBM_COPY_TB_S, 3)})
for what in ("split", "attention"):
    f, u = out[what + "_fused"], out[what + "_unfused"]
    out[what + "_saved_ms"] = round(u["median_ms"] - f["median_ms"], 4)
    out[what + "_spread_ms"] = round(max(f["max_ms"] - f["min_ms"],
                                         u["max_ms"] - u["min_ms"]), 4)
print(json.dumps(out), flush=True)
