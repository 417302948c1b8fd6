"""A/B: the DiLoCo outer sync of one fragment holding a whole Llama-shaped
parameter zoo (bf16), unfused op sequence against the fused kernels, plus each
kernel alone with its achieved bandwidth. Run on a GPU box. No manager is
involved: the allreduce is a no-op, so this times the device work around it.

  A  today's sequence from prepare_sync / perform_sync / _outer_step with a
     device-resident snapshot: per-parameter subtract, clone of the local
     parameters, restore copy, grad install,
     torch.optim.SGD(momentum=0.9, nesterov=True).step(), save copy, lerp_
  B  fused_sync=True: zeroed flat buckets, ops.pseudograd_ into their views,
     ops.diloco_outer_step_

Device events, variants interleaved within every round; the spread over the
rounds is printed with the medians. Bytes are counted off the shapes: 3N
elements for the pseudo-gradient kernel, 7N for the outer step. The zoo is the
8B one unless --size 1b is given or the device has too little free memory for
it; the output says which."""
import sys, os, json, argparse
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torchft_amd import ops
from torchft_amd.local_sgd import _BucketPlan
from torchft_amd.models.llama import LLAMA3_8B, Llama, LlamaConfig

ap = argparse.ArgumentParser()
ap.add_argument("--size", choices=["8b", "1b"], default="8b")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--alpha", type=float, default=0.25)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_diloco_sync.py measures on a HIP device only"
dev = "cuda"
CONFIGS = {
    "8b": LLAMA3_8B,
    "1b": LlamaConfig(dim=2048, n_layers=16, n_heads=32, n_kv_heads=8, ffn_hidden=8192),
}
LR, MU, ALPHA = 0.7, 0.9, args.alpha
CAP_BYTES = 1 << 30  # DiLoCo's default bucket cap


def zoo_shapes(cfg):
    with torch.device("meta"):
        m = Llama(cfg, dtype=torch.bfloat16)
    return [tuple(p.shape) for p in m.parameters()]


size = args.size
shapes = zoo_shapes(CONFIGS[size])
numel = sum(torch.Size(s).numel() for s in shapes)
# bf16: params, two snapshots, two momentum sets, A's pseudo-gradients and
# clone of the local parameters, B's buckets, and A's transient clone in save
need = numel * 2 * 9
free, _ = torch.cuda.mem_get_info()
if size == "8b" and need * 1.1 > free:
    size = "1b"
    shapes = zoo_shapes(CONFIGS[size])
    numel = sum(torch.Size(s).numel() for s in shapes)

torch.manual_seed(0)
params = [(torch.randn(*s, device=dev) * 0.02).to(torch.bfloat16).requires_grad_(True)
          for s in shapes]
snap_a = [p.detach().clone() for p in params]
snap_b = [p.detach().clone() for p in params]
with torch.no_grad():
    for p in params:  # local progress since the snapshot
        p.add_(torch.randn_like(p) * 1e-3)
outer = torch.optim.SGD(params, lr=LR, momentum=MU, nesterov=True)
mom_b = [torch.zeros_like(p) for p in params]
plan = _BucketPlan([p.data for p in params], CAP_BYTES, align_bytes=16)


def variant_a():
    with torch.no_grad():
        pseudo = [o - p for o, p in zip(snap_a, params)]  # prepare_sync
        local = [p.data.clone() for p in params]  # perform_sync
        for p, o in zip(params, snap_a):  # restore_parameters
            p.data.copy_(o)
        for p, g in zip(params, pseudo):  # _outer_step
            p.grad = g
    outer.step()
    with torch.no_grad():
        for p, o in zip(params, snap_a):  # save_parameters
            o.copy_(p.data.clone(), non_blocking=True)
        for p, l in zip(params, local):
            p.data.lerp_(l, ALPHA)
    outer.zero_grad()


def fused_prepare():
    buckets = [plan.allocate(slots) for slots in plan.buckets]
    views = [v for _, vs in buckets for v in vs]
    ops.pseudograd_(views, snap_b, [p.data for p in params])
    return views


def fused_step(views):
    ops.diloco_outer_step_(snap_b, [p.data for p in params], views, mom_b,
                           lr=LR, momentum=MU, nesterov=True, alpha=ALPHA)


def variant_b():
    fused_step(fused_prepare())


kernel_views = fused_prepare()


def pseudograd_only():
    ops.pseudograd_(kernel_views, snap_b, [p.data for p in params])


def outer_step_only():
    fused_step(kernel_views)


def timed(fn, iters):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


VARIANTS = [("A_unfused_sequence", variant_a), ("B_fused_sync", variant_b),
            ("pseudograd_kernel", pseudograd_only), ("outer_step_kernel", outer_step_only)]
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


out = {"bench": "diloco_sync", "zoo": size, "tensors": len(shapes), "numel": numel,
       "buckets": len(plan.buckets), "rounds": args.rounds, "iters": args.iters,
       "alpha": ALPHA}
for name, _ in VARIANTS:
    out[name] = stats(ms[name])
a, b = out["A_unfused_sequence"]["median_ms"], out["B_fused_sync"]["median_ms"]
pg_ms = out["pseudograd_kernel"]["median_ms"]
os_ms = out["outer_step_kernel"]["median_ms"]
out.update({
    "B_over_A": round(b / a, 3),
    "pseudograd_gb": round(3 * numel * 2 / 1e9, 3),
    "pseudograd_tb_per_s": round(3 * numel * 2 / pg_ms / 1e9, 3),
    "outer_step_gb": round(7 * numel * 2 / 1e9, 3),
    "outer_step_tb_per_s": round(7 * numel * 2 / os_ms / 1e9, 3),
    "hbm_roofline_tb_per_s": 6.3,
})
print(json.dumps(out), flush=True)
