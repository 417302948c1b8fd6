"""A/B/C: gradient clipping around the fused AdamW step on a Llama-shaped
parameter zoo (bf16 params and grads, fp32 moments), plus the norm pass alone
and its achieved bandwidth. Run on a GPU box.

  A  torch.nn.utils.clip_grad_norm_ followed by today's FusedAdamW.step()
  B  FusedAdamW(max_grad_norm=1.0).step()  (norm kernels + clip folded in)
  C  today's FusedAdamW.step(), no clipping

Device events, variants interleaved within every round; the spread over the
rounds is printed with the medians. The zoo is the 8B one unless --size 1b is
given or the device has too little free memory for it; the output says which."""
import sys, os, json, argparse
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torchft_amd import ops
from torchft_amd.models.llama import LLAMA3_8B, Llama, LlamaConfig
from torchft_amd.ops import FusedAdamW

ap = argparse.ArgumentParser()
ap.add_argument("--size", choices=["8b", "1b"], default="8b")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--max-blocks", type=int, default=2048)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_clip.py measures on a HIP device only"
dev = "cuda"
CONFIGS = {
    "8b": LLAMA3_8B,
    "1b": LlamaConfig(dim=2048, n_layers=16, n_heads=32, n_kv_heads=8, ffn_hidden=8192),
}


def zoo_shapes(cfg):
    with torch.device("meta"):
        m = Llama(cfg, dtype=torch.bfloat16)
    return [tuple(p.shape) for p in m.parameters()]


size = args.size
shapes = zoo_shapes(CONFIGS[size])
numel = sum(torch.Size(s).numel() for s in shapes)
# params + grads (2 B each) and two optimizers' fp32 moments (8 B each)
need = numel * (2 + 2 + 8 + 8)
free, _ = torch.cuda.mem_get_info()
if size == "8b" and need * 1.1 > free:
    size = "1b"
    shapes = zoo_shapes(CONFIGS[size])
    numel = sum(torch.Size(s).numel() for s in shapes)

torch.manual_seed(0)
params = [(torch.randn(*s, device=dev) * 0.02).to(torch.bfloat16).requires_grad_(True)
          for s in shapes]
grads = [(torch.randn(*s, device=dev) * 0.01).to(torch.bfloat16) for s in shapes]
for p, g in zip(params, grads):
    p.grad = g
plain = FusedAdamW(params, lr=1e-5)
clip = FusedAdamW(params, lr=1e-5, max_grad_norm=1.0)


def variant_a():
    torch.nn.utils.clip_grad_norm_(params, 1.0)
    plain.step()


def variant_b():
    clip.step()


def variant_c():
    plain.step()


def norm_only():
    ops.grad_norm(grads, max_blocks=args.max_blocks)


def timed(fn, iters):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


VARIANTS = [("A_torch_clip_then_step", variant_a), ("B_fused_clip_step", variant_b),
            ("C_step_no_clip", variant_c), ("norm_pass", norm_only)]
for _, fn in VARIANTS:  # warm-up: state allocation, code objects
    fn()
torch.cuda.synchronize()

ms = {name: [] for name, _ in VARIANTS}
for rnd in range(args.rounds):
    for name, fn in VARIANTS:
        ms[name].append(timed(fn, args.iters))


def stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 3), "min_ms": round(v[0], 3),
            "max_ms": round(v[-1], 3)}


out = {"bench": "grad_clip", "zoo": size, "tensors": len(shapes), "numel": numel,
       "rounds": args.rounds, "iters": args.iters, "max_blocks": args.max_blocks}
for name, _ in VARIANTS:
    out[name] = stats(ms[name])
a, b, c = (out[k]["median_ms"] for k in
           ("A_torch_clip_then_step", "B_fused_clip_step", "C_step_no_clip"))
spread = max(out[k]["max_ms"] - out[k]["min_ms"] for k in
             ("A_torch_clip_then_step", "B_fused_clip_step"))
norm_ms = out["norm_pass"]["median_ms"]
out.update({
    "B_minus_A_ms": round(b - a, 3), "B_minus_C_ms": round(b - c, 3),
    "spread_ms": round(spread, 3), "B_not_slower_than_A": b <= a + spread,
    "norm_read_gb": round(numel * 2 / 1e9, 3),
    "norm_tb_per_s": round(numel * 2 / norm_ms / 1e9, 3),
    "hbm_roofline_tb_per_s": 6.3,
    "skipped_steps": int(clip.skipped_steps),
    "last_grad_norm": float(clip.last_grad_norm),
})
print(json.dumps(out), flush=True)
