"""A/B builds of the flash-attention backward kernels in one process.

Each build is a stand-alone shared library of csrc/kernels/flash_attn_bwd.hip.
The file includes fa_tile.h / fa_layout.h / kernels.h from its own directory,
so a copy compiled elsewhere needs -I csrc/kernels (a revision from before the
shared headers needs nothing but the HIP headers; the -I does no harm), e.g.
for the parent commit:

    git show HEAD~1:csrc/kernels/flash_attn_bwd.hip > /tmp/parent.hip
    hipcc -O3 --offload-arch=gfx950 -shared -fPIC -I csrc/kernels \
        /tmp/parent.hip -o parent.so
    hipcc -O3 --offload-arch=gfx950 -shared -fPIC \
        csrc/kernels/flash_attn_bwd.hip -o new.so

    python scripts/fa_bwd_ab.py parent=parent.so new=new.so

The first library is the baseline. Timing: dkdv + dq launches between device
events, builds interleaved inside every round (median [min-max] over rounds).
--check compares every build's dq/dk/dv bit for bit against the baseline at
(B=1, Hq=8, Hkv=2, S=1024), causal and full, packed and [B,S,H,D] layouts,
and at the timed shape. --drive N only launches build 0 N times (a profiler
target). --full times or drives the non-causal launch, whose workgroups are
all equal: causal / full against the tile ratio says how well the causal
launch is balanced (docs/KERNELS.md, "Workgroup order"). Run on a GPU host."""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from torchft_amd.ops import hip_ext

# launch_fa_bwd as it is now (two document-mask arrays before the stream,
# passed as null here) and as it was before the document mask
_SYM = ("_ZN11torchft_amd13launch_fa_bwdEPKvS1_S1_S1_PKfS3_PvS4_S4_"
        "iiiifbbPKiS6_P12ihipStream_t")
_SYM_NO_DOC = ("_ZN11torchft_amd13launch_fa_bwdEPKvS1_S1_S1_PKfS3_PvS4_S4_"
               "iiiifbbP12ihipStream_t")
D = 128


class Build:
    def __init__(self, spec):
        self.name, path = spec.split("=", 1)
        lib = ctypes.CDLL(os.path.abspath(path))
        self.doc_args = hasattr(lib, _SYM)
        self.fn = getattr(lib, _SYM if self.doc_args else _SYM_NO_DOC)
        self.fn.restype = None
        self.fn.argtypes = [ctypes.c_void_p] * 9 + [ctypes.c_int] * 4 + [
            ctypes.c_float, ctypes.c_bool, ctypes.c_bool] + [
            ctypes.c_void_p] * (3 if self.doc_args else 1)

    def __call__(self, p, out):
        B, Hq, S = p["q"].shape[0], p["q"].shape[1], p["q"].shape[2]
        self.fn(p["q"].data_ptr(), p["k"].data_ptr(), p["v"].data_ptr(),
                p["dout"].data_ptr(), p["lse"].data_ptr(), p["delta"].data_ptr(),
                out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                B, Hq, p["k"].shape[1], S, D ** -0.5, p["causal"], p["bshd"],
                *((None, None) if self.doc_args else ()),
                torch.cuda.current_stream().cuda_stream)


def problem(B, Hq, Hkv, S, causal, bshd, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def mk(H):
        shape = (B, S, H, D) if bshd else (B, H, S, D)
        t = torch.randn(shape, device="cuda", dtype=torch.bfloat16, generator=g)
        return t.transpose(1, 2) if bshd else t

    q, k, v, dout = mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)
    out, lse, *_ = torch.ops.aten._scaled_dot_product_flash_attention(
        q, k, v, 0.0, causal, False, scale=D ** -0.5)
    delta = hip_ext().fa_delta(dout, out)
    return dict(q=q, k=k, v=v, dout=dout, lse=lse.contiguous().float(),
                delta=delta.contiguous().float(), causal=causal, bshd=bshd)


def grads(p):
    # same storage layout as the inputs; poisoned so a missed store shows
    return [torch.full_like(p[n], float("nan")) for n in ("q", "k", "v")]


def check(builds, shapes):
    ok = True
    for (B, Hq, Hkv, S) in shapes:
        for causal in (True, False):
            for bshd in (False, True):
                p = problem(B, Hq, Hkv, S, causal, bshd)
                ref = grads(p)
                builds[0](p, ref)
                for b in builds[1:]:
                    got = grads(p)
                    b(p, got)
                    torch.cuda.synchronize()
                    same = all(torch.equal(r, g_) for r, g_ in zip(ref, got))
                    ok &= same
                    print(f"bitwise {b.name} vs {builds[0].name} B={B} Hq={Hq} "
                          f"Hkv={Hkv} S={S} causal={causal} bshd={bshd}: "
                          f"{'EQUAL' if same else 'DIFFERENT'}", flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("builds", nargs="+", help="name=path/to/lib.so")
    ap.add_argument("--shape", default="4,32,8,8192", help="B,Hq,Hkv,S")
    ap.add_argument("--full", action="store_true", help="non-causal (default: causal)")
    ap.add_argument("--bshd", action="store_true",
                    help="[B,S,H,D] storage, the model's layout (default: packed)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--drive", type=int, default=0)
    a = ap.parse_args()
    builds = [Build(s) for s in a.builds]
    shape = tuple(int(x) for x in a.shape.split(","))

    p = problem(*shape, not a.full, a.bshd)
    out = grads(p)
    if a.drive:
        for _ in range(a.drive):
            builds[0](p, out)
        torch.cuda.synchronize()
        print("done")
        return 0

    ok = True
    if a.check:
        ok = check(builds, [(1, 8, 2, 1024), shape])

    times = {b.name: [] for b in builds}
    for b in builds:  # warm up: code-object load
        b(p, out)
    torch.cuda.synchronize()
    for rnd in range(a.rounds):
        for b in builds:
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                b(p, out)
            e1.record()
            torch.cuda.synchronize()
            times[b.name].append(e0.elapsed_time(e1) / a.iters)
        print(f"round {rnd}: " + "  ".join(
            f"{n} {t[-1]:.3f}" for n, t in times.items()), flush=True)
    for n, t in times.items():
        print(f"{n}: dkdv+dq {statistics.median(t):.3f} ms "
              f"[{min(t):.3f}-{max(t):.3f}] over {len(t)} rounds, shape {shape} "
              f"{'full' if a.full else 'causal'} {'bshd' if a.bshd else 'packed'}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
