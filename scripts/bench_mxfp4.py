"""A/B: the MXFP4 wire-pack kernels against the fp8 ones on the same tensors,
a Llama-shaped bf16 parameter zoo: quantize, reduce at world 4 (the pack's
four slices standing in for four ranks' copies of one slice) and dequantize.
Run on a GPU box.

Device events, the two formats alternated within every round; medians with
the spread over the rounds. Bytes are counted off the shapes: quantize reads
2N and writes the pack, dequantize the reverse, reduce reads the pack and
writes a quarter of it."""
import sys, os, json, argparse
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torchft_amd import quantization as Q
from torchft_amd.models.llama import LLAMA3_8B, Llama, LlamaConfig

ap = argparse.ArgumentParser()
ap.add_argument("--size", choices=["8b", "1b"], default="8b")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=5)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_mxfp4.py measures on a HIP device only"
dev = "cuda"
WORLD = 4
cfg = {"8b": LLAMA3_8B,
       "1b": LlamaConfig(dim=2048, n_layers=16, n_heads=32, n_kv_heads=8, ffn_hidden=8192)}[args.size]
with torch.device("meta"):
    shapes = [tuple(p.shape) for p in Llama(cfg, dtype=torch.bfloat16).parameters()]
torch.manual_seed(0)
tensors = [(torch.randn(*s, device=dev) * 0.02).to(torch.bfloat16) for s in shapes]
outs = [torch.empty_like(t) for t in tensors]
numel = sum(t.numel() for t in tensors)

FORMATS = {
    "fp8": (Q.pack_geometry, Q.quantize_pack, Q.reduce_slices, Q.dequantize_pack),
    "mxfp4": (Q.mx_pack_geometry, Q.mx_quantize_pack, Q.mx_reduce_slices, Q.mx_dequantize_pack),
}
steps, nbytes = {}, {}
for name, (geometry, quantize, reduce, dequantize) in FORMATS.items():
    slice_bytes = geometry(tensors, WORLD)[3]
    pack = torch.empty(WORLD * slice_bytes, dtype=torch.uint8, device=dev)
    red = torch.empty(slice_bytes, dtype=torch.uint8, device=dev)
    steps[name] = {
        "quantize": lambda q=quantize, p=pack: q(tensors, p, WORLD),
        "reduce": lambda r=reduce, p=pack, o=red: r(p, o, WORLD, True),
        "dequantize": lambda d=dequantize, p=pack: d(outs, p, WORLD),
    }
    nbytes[name] = {"quantize": 2 * numel + pack.numel(), "reduce": pack.numel() + slice_bytes,
                    "dequantize": 2 * numel + pack.numel(), "pack": pack.numel()}


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / args.iters


for name in FORMATS:  # warm-up, in pipeline order: reduce and dequantize read a written pack
    for step in ("quantize", "reduce", "dequantize"):
        steps[name][step]()
torch.cuda.synchronize()
ms = {name: {step: [] for step in steps[name]} for name in FORMATS}
for _ in range(args.rounds):
    for step in ("quantize", "reduce", "dequantize"):
        for name in FORMATS:
            ms[name][step].append(timed(steps[name][step]))

out = {"bench": "mxfp4", "zoo": args.size, "tensors": len(shapes), "numel": numel,
       "world": WORLD, "rounds": args.rounds, "iters": args.iters}
for name in FORMATS:
    out[name + "_pack_bytes"] = nbytes[name]["pack"]
    for step, xs in ms[name].items():
        xs = sorted(xs)
        med = xs[len(xs) // 2]
        out[f"{name}_{step}_ms"] = [round(med, 4), round(xs[0], 4), round(xs[-1], 4)]
        out[f"{name}_{step}_GBps"] = round(nbytes[name][step] / med / 1e6, 1)
print(json.dumps(out))
