"""FusedAdamW's rounding modes on a Llama-shaped parameter zoo (bf16 params and
grads, fp32 moments, an fp32 master copy for "master"): ms per plain step for
"nearest", "stochastic" and "master", and, with --parent-so, for the nearest
step of another build of the extension (the parent commit's) in the same
process. Run on a GPU box.

Device events, variants interleaved within every round, median [min-max] over
the rounds. Traffic per element: nearest and stochastic 22 B, master 30 B. The
zoo is the 8B one unless --size 1b is given or the device has too little free
memory for it; the output says which."""
import sys, os, json, argparse, importlib.util
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torchft_amd.models.llama import LLAMA3_8B, Llama, LlamaConfig
from torchft_amd.ops import FusedAdamW

ap = argparse.ArgumentParser()
ap.add_argument("--size", choices=["8b", "1b"], default="8b")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--parent-so", default=None,
                help="_hip_kernels.so of the build to compare the nearest step with")
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_adamw_rounding.py measures on a HIP device only"
dev = "cuda"
CONFIGS = {
    "8b": LLAMA3_8B,
    "1b": LlamaConfig(dim=2048, n_layers=16, n_heads=32, n_kv_heads=8, ffn_hidden=8192),
}
BYTES = {"nearest": 22, "stochastic": 22, "master": 30, "parent_nearest": 22}


def zoo_shapes(cfg):
    with torch.device("meta"):
        m = Llama(cfg, dtype=torch.bfloat16)
    return [tuple(p.shape) for p in m.parameters()]


size = args.size
shapes = zoo_shapes(CONFIGS[size])
numel = sum(torch.Size(s).numel() for s in shapes)
# params + grads (2 B each), one set of fp32 moments shared by all variants
# (8 B; the timing does not care whose they are) and the master copy (4 B)
free, _ = torch.cuda.mem_get_info()
if size == "8b" and numel * (2 + 2 + 8 + 4) * 1.1 > free:
    size = "1b"
    shapes = zoo_shapes(CONFIGS[size])
    numel = sum(torch.Size(s).numel() for s in shapes)

torch.manual_seed(0)
params = [(torch.randn(*s, device=dev) * 0.02).to(torch.bfloat16).requires_grad_(True)
          for s in shapes]
for p in params:
    p.grad = (torch.randn(*p.shape, device=dev) * 0.01).to(torch.bfloat16)
opts = {r: FusedAdamW(params, lr=1e-5, rounding=r)
        for r in ("nearest", "stochastic", "master")}
opts["nearest"].step()
for r in ("stochastic", "master"):  # share the moments
    for p in params:
        opts[r].state[p].update(opts["nearest"].state[p])
variants = [(r, o.step) for r, o in opts.items()]

if args.parent_so:
    spec = importlib.util.spec_from_file_location("_hip_kernels", args.parent_so)
    parent = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(parent)
    st = opts["nearest"].state
    lists = ([p.detach() for p in params], [p.grad for p in params],
             [st[p]["exp_avg"] for p in params], [st[p]["exp_avg_sq"] for p in params])
    variants.append(("parent_nearest",
                     lambda: parent.adamw_step(*lists, 1e-5, 0.9, 0.95, 1e-8, 0.01, 2)))


def timed(fn, iters):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


for _, fn in variants:  # warm-up: state allocation, code objects
    fn()
torch.cuda.synchronize()
ms = {name: [] for name, _ in variants}
for rnd in range(args.rounds):
    for name, fn in variants:
        ms[name].append(timed(fn, args.iters))

out = {"bench": "adamw_rounding", "zoo": size, "tensors": len(shapes), "numel": numel,
       "rounds": args.rounds, "iters": args.iters, "hbm_roofline_tb_per_s": 6.3}
for name, _ in variants:
    v = sorted(ms[name])
    med = v[len(v) // 2]
    out[name] = {"median_ms": round(med, 3), "min_ms": round(v[0], 3),
                 "max_ms": round(v[-1], 3),
                 "tb_per_s": round(numel * BYTES[name] / med / 1e9, 3)}
print(json.dumps(out), flush=True)
