"""List-scheduling model of the attention launches: what a workgroup order
costs in makespan before anyone goes to the GPU.

Every workgroup of fa_bwd_dkdv_kernel, fa_bwd_dq_kernel and fa_fwd_kernel
streams a number of tiles that depends on its block x (and, with a document
mask, on the documents). One workgroup fits a CU, so a launch is a list of
jobs dealt in block order n = blockIdx.x + gridDim.x * blockIdx.y onto 256
machines. Cost is taken as proportional to tiles. Two dealing models bracket
what is observed of the dispatcher:

  A  any free CU takes the next block;
  B  block n is bound to XCD n % 8, 32 CUs each, each XCD a list of its own.

Printed: makespan / ideal (ideal = all tiles / 256) per launch, for the linear
order the kernels had before fa_wg_order (fa_layout.h) and for the order it
gives. The tile counts are restated from the kernels:

  dkdv  G * (i_hi - i_min) 32-row Q/dO tiles, i_min = 8 x, i_hi = S / 32, with
        documents the tile past doc_end of the block's last key
        (flash_attn_bwd.hip, `nI` / `T`; doc_last_qtile in fa_layout.h)
  dq    T - j0 64-key K/V tiles, T = 4 (x + 1), j0 = doc_start(first row) / 64
        (flash_attn_bwd.hip, `T` / `j0`; doc_first_tile in fa_layout.h)
  fwd   as dq (flash_attn_fwd.hip, `nT` / `j0`)

A model, not a measurement: docs/KERNELS.md, "Workgroup order", has both.

    python scripts/fa_wg_order_model.py [--shape B,Hq,Hkv,S] [--docs N]
"""
import argparse
import heapq

CUS, XCDS = 256, 8


def tiles(kernel, x, G, S, doc_len):
    """Tiles block x streams; doc_len = None is plain causal, otherwise the
    row is packed with equal documents of doc_len tokens (a multiple of 256)."""
    if kernel == "dkdv":
        last_key = min((x + 1) * 256, S) - 1
        end = S if doc_len is None else (last_key // doc_len + 1) * doc_len
        return G * ((end + 31) // 32 - 8 * x)
    first_row = x * 256
    start = 0 if doc_len is None else first_row // doc_len * doc_len
    return (min((x + 1) * 256, S) + 63) // 64 - start // 64


def present_order(kernel, n, nx, ny):
    """(x, y) of launch block n before fa_wg_order: linear, dq reversed in x."""
    x, y = n % nx, n // nx
    return (nx - 1 - x if kernel == "dq" else x), y


def rank_major_order(kernel, n, nx, ny):
    """fa_wg_order (fa_layout.h): all y of the heaviest x first."""
    rank, y = n // ny, n % ny
    return (rank if kernel == "dkdv" else nx - 1 - rank), y


def makespan(costs, model):
    """costs in dispatch order -> finish time of the last workgroup."""
    if model == "A":
        pools = [costs]
    else:
        pools = [costs[i::XCDS] for i in range(XCDS)]
    worst = 0
    for pool in pools:
        free = [0] * (CUS // len(pools))
        heapq.heapify(free)
        for c in pool:
            t = heapq.heappop(free) + c
            worst = max(worst, t)
            heapq.heappush(free, t)
    return worst


def ratio(kernel, order, model, B, Hq, Hkv, S, doc_len):
    nx = (S + 255) // 256
    ny = B * (Hkv if kernel == "dkdv" else Hq)
    G = Hq // Hkv if kernel == "dkdv" else 1
    costs, seen = [], set()
    for n in range(nx * ny):
        x, y = order(kernel, n, nx, ny)
        seen.add((x, y))
        costs.append(tiles(kernel, x, G, S, doc_len))
    assert len(seen) == nx * ny, "the order is not a bijection of the grid"
    return makespan(costs, model) / (sum(costs) / CUS), sum(costs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="4,32,8,8192", help="B,Hq,Hkv,S")
    ap.add_argument("--docs", type=int, default=8,
                    help="equal documents per row of the document-mask lines")
    a = ap.parse_args()
    B, Hq, Hkv, S = (int(v) for v in a.shape.split(","))
    assert S % (256 * a.docs) == 0, "documents of a multiple of 256 tokens"
    print(f"B={B} Hq={Hq} Hkv={Hkv} S={S}: makespan / ideal on {CUS} CUs")
    print(f"{'launch':<22}{'tiles':>9}  {'present A':>9} {'present B':>9}"
          f"  {'ranked A':>9} {'ranked B':>9}")
    for doc_len, tag in ((None, "causal"), (S // a.docs, f"{a.docs} documents")):
        for kernel in ("dkdv", "dq", "fwd"):
            r = [ratio(kernel, o, m, B, Hq, Hkv, S, doc_len)
                 for o in (present_order, rank_major_order) for m in "AB"]
            print(f"{kernel + ' ' + tag:<22}{r[0][1]:>9}  {r[0][0]:>9.2f} {r[1][0]:>9.2f}"
                  f"  {r[2][0]:>9.2f} {r[3][0]:>9.2f}")


if __name__ == "__main__":
    main()
