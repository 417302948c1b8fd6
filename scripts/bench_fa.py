"""A/B: custom flash-attention backward vs stock SDPA backward at the
Llama-8B bench shape. Run on a GPU box.

--docs N (off by default) times the document-masked kernels instead: every row
packed with N equal documents, against the same kernels without a mask, at
B=4, Hq=32, Hkv=8, S=8192. Forward and dkdv + dq are timed apart between
device events, the two variants interleaved in one process, --rounds rounds of
--iters calls, reported as median [min-max] ms."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from torchft_amd.ops.flash_attention import DocMask, _FlashAttentionFn

D = 128
dev = "cuda"


def stock_ab():
    B, Hq, Hkv, S = 2, 32, 8, 8192
    torch.manual_seed(0)
    q0 = torch.randn(B, Hq, S, D, device=dev, dtype=torch.bfloat16)
    k0 = torch.randn(B, Hkv, S, D, device=dev, dtype=torch.bfloat16)
    v0 = torch.randn(B, Hkv, S, D, device=dev, dtype=torch.bfloat16)
    dout = torch.randn(B, Hq, S, D, device=dev, dtype=torch.bfloat16)

    def run(custom: bool, iters=10, custom_fwd=False):
        q = q0.clone().requires_grad_(True)
        k = k0.clone().requires_grad_(True)
        v = v0.clone().requires_grad_(True)
        os.environ["TORCHFT_AMD_CUSTOM_FA_FWD"] = "1" if custom_fwd else "0"
        def step():
            if custom:
                out = _FlashAttentionFn.apply(q, k, v, True, D ** -0.5)
            else:
                out = F.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=True)
            out.backward(dout)
            q.grad = k.grad = v.grad = None
        for _ in range(3): step()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(iters): step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1000

    # interleaved A/B (guide rule 24)
    ROUNDS = int(os.environ.get("FA_ROUNDS", "3"))
    for rnd in range(ROUNDS):
        a = run(False); b = run(True); c = run(True, custom_fwd=True)
        fl_fwd = 2*2*B*Hq*S*S*D/2
        fl_bwd = fl_fwd * 2.5
        print(f"round {rnd}: custom-fwd+bwd {c:.2f} ms", flush=True)
        print(f"round {rnd}: stock {a:.2f} ms | custom {b:.2f} ms "
              f"(fwd+bwd {B*Hq=}, eff stock {(fl_fwd+fl_bwd)/a/1e9:.0f} TF/s, "
              f"custom {(fl_fwd+fl_bwd)/b/1e9:.0f} TF/s)", flush=True)


def docs_ab(n_docs, shape, rounds, iters):
    from torchft_amd.ops import hip_ext

    ext = hip_ext()
    B, Hq, Hkv, S = shape
    assert S % n_docs == 0, "--docs must divide S"
    scale = D ** -0.5
    g = torch.Generator(device=dev).manual_seed(0)

    def mk(H):
        return torch.randn(B, H, S, D, device=dev, dtype=torch.bfloat16, generator=g)

    q, k, v, dout = mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)
    m = DocMask.from_lengths([[S // n_docs] * n_docs] * B, S, device=dev)
    variants = {"causal": (), f"docs{n_docs}": (m.doc_start, m.doc_end)}
    # every variant's backward runs on its own forward's out / lse
    state = {}
    for name, doc in variants.items():
        out, lse = ext.fa_fwd(q, k, v, scale, True, *doc)
        state[name] = (lse, ext.fa_delta(dout, out))
    torch.cuda.synchronize()

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    times = {(n, p): [] for n in variants for p in ("fwd", "bwd")}
    for rnd in range(rounds):
        for name, doc in variants.items():
            lse, delta = state[name]
            times[name, "fwd"].append(
                timed(lambda: ext.fa_fwd(q, k, v, scale, True, *doc)))
            times[name, "bwd"].append(
                timed(lambda: ext.fa_bwd(q, k, v, dout, lse, delta, scale, True, *doc)))
        print(f"round {rnd}: " + "  ".join(
            f"{n} {p} {t[-1]:.3f}" for (n, p), t in times.items()), flush=True)

    def fmt(t):
        return f"{statistics.median(t):.3f} [{min(t):.3f}-{max(t):.3f}]"

    base = None
    for name in variants:
        f, b = times[name, "fwd"], times[name, "bwd"]
        tot = [x + y for x, y in zip(f, b)]
        line = (f"{name}: fwd {fmt(f)} ms, dkdv+dq {fmt(b)} ms, sum {fmt(tot)} ms "
                f"over {rounds} rounds x {iters} calls, shape {shape}")
        if base is None:
            base = (f, b, tot)
        else:
            line += " | vs causal: " + ", ".join(
                f"{lbl} x{statistics.median(t) / statistics.median(t0):.3f}"
                for lbl, t, t0 in zip(("fwd", "dkdv+dq", "sum"), (f, b, tot), base))
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=0,
                    help="N equal documents per row: time the document-masked "
                         "kernels against the unmasked ones (0: the stock A/B)")
    ap.add_argument("--shape", default="4,32,8,8192", help="B,Hq,Hkv,S for --docs")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if a.docs <= 0:
        return stock_ab()
    docs_ab(a.docs, tuple(int(x) for x in a.shape.split(",")), a.rounds, a.iters)


if __name__ == "__main__":
    main()
