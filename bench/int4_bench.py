"""Int4 W4A16 projections vs the bf16 engine GEMMs, per Llama projection shape and M (ops/int4.py).

Cold weights (enough rotating copies that every call streams its weight from HBM, as each layer does once per
step), every implementation captured in one HIP graph of back-to-back calls, the graphs replayed interleaved
(launch overhead out, clocks shared), the best of three rounds of medians.  Columns, in microseconds per call:
  w4      gemm_w4a16 (+ w4_reduce on split grids; + silu_mul on gate|up)
  dequant dequant_w4 into the scratch tensor + the bf16 route (+ silu_mul where that route does not fuse it)
  bf16    the bf16 route of the same shape on plain bf16 weights (ops.linear / ops.linear_swiglu)
    python bench/int4_bench.py [--m 1 16 64 ...] [--shapes qkv_8b ...] [--out profiles/int4_table.md]
``--zeros``: the zero-point variant (imported AWQ / GPTQ weights: u32 scale | zero per group) against the symmetric
kernel on the same codes, measured the same way, and ``w4_repack`` of one Llama-3-70B gate|up per format.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from distributed_llms_amd import ops
from distributed_llms_amd.ops import int4

SHAPES = {  # name: (N, K, swiglu)
    "qkv_8b": (6144, 4096, False), "o_8b": (4096, 4096, False), "gate_up_8b": (28672, 4096, True),
    "down_8b": (4096, 14336, False),
    "qkv_70b": (10240, 8192, False), "o_70b": (8192, 8192, False), "gate_up_70b": (57344, 8192, True),
    "down_70b": (8192, 28672, False),
}
MALL_X3 = 768 << 20          # rotate over three times the 256 MiB MALL


def timeit(fn, iters):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts)


def weight_bytes_70b():
    """Bytes of the 80 layers' projections of Llama-3-70B: bf16, and as Int4Weight.nbytes() of the same shapes."""
    bf, q4 = 0, 0
    for name in ("qkv_70b", "o_70b", "gate_up_70b", "down_70b"):
        n, k, _ = SHAPES[name]
        w = int4.Int4Weight(torch.empty(n // 16, k // 128, 1024, dtype=torch.uint8, device="meta"),
                            torch.empty(n // 16, k // 128, 16, dtype=torch.bfloat16, device="meta"))
        bf, q4 = bf + 80 * 2 * n * k, q4 + 80 * w.nbytes()
    return bf, q4


def race(impls, streams, reps, iters):
    """{key: microseconds per call}: one graph of ``reps`` calls per implementation, replayed interleaved."""
    graphs = {}
    for key, f in impls.items():
        st = streams[key]
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            for i in range(2):
                f(i)
        torch.cuda.current_stream().wait_stream(st)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            for i in range(reps):
                f(i)
        graphs[key] = g
    for g in graphs.values():
        g.replay()
    res = {key: [] for key in graphs}
    for _ in range(3):
        for key, g in graphs.items():
            res[key].append(timeit(g.replay, iters) / reps)
    return {key: min(v) * 1e6 for key, v in res.items()}


def zeros_arm(a):
    lines = ["| shape | M | symmetric us | zero-point us | zero-point / symmetric |", "|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    streams = {key: torch.cuda.Stream() for key in ("sym", "zp")}
    for name in a.shapes:
        n, k, sw = SHAPES[name]
        first = int4.quantize_weight((torch.randn(n, k, device="cuda") * 0.02).to(torch.bfloat16))
        zeros = torch.randint(0, 16, first.scale.shape, dtype=torch.uint8, device="cuda")
        copies = max(2, -(-MALL_X3 // (n * k // 2)))
        sym = [int4.Int4Weight(first.packed.clone(), first.scale.clone()) for _ in range(copies)]
        zp = [int4.Int4Weight(first.packed.clone(), first.scale.to(torch.float16), zeros) for _ in range(copies)]
        act = ops.silu_mul if sw else (lambda y: y)
        for m in a.m:
            x = torch.randn(m, k, device="cuda").to(torch.bfloat16)
            t = race({"sym": lambda i: act(int4.linear_int4(x, sym[i % copies], dequant_min_m=1 << 30)),
                      "zp": lambda i: act(int4.linear_int4(x, zp[i % copies], dequant_min_m=1 << 30))},
                     streams, max(copies, 8), a.iters)
            lines.append(f"| {name} | {m} | {t['sym']:.1f} | {t['zp']:.1f} | {t['zp'] / t['sym']:.3f} |")
            print(lines[-1], flush=True)
        del sym, zp
        torch.cuda.empty_cache()
    n, k, _ = SHAPES["gate_up_70b"]
    lines += ["", f"w4_repack of one Llama-3-70B gate|up ({n} x {k}, two projections, {n * k / 2e6:.0f} MB of codes):", "",
              "| format | ms | GB/s read + written |", "|---|---|---|"]
    for fmt in int4.FORMATS:
        kk, nn = (k, n // 2 // 8) if fmt == "awq" else (k // 8, n // 2)
        part = (torch.randint(-2 ** 31, 2 ** 31, (kk, nn), dtype=torch.int32, device="cuda"),
                torch.randint(-2 ** 31, 2 ** 31, (k // 128, n // 16), dtype=torch.int32, device="cuda"),
                torch.rand(k // 128, n // 2, device="cuda").to(torch.float16))
        f = lambda: int4.from_checkpoint([part, part], fmt)
        f()
        ms = min(timeit(f, a.iters) for _ in range(3)) * 1e3
        lines.append(f"| {fmt} | {ms:.2f} | {n * k / ms / 1e6:.0f} |")
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", default=[1, 16, 64, 128, 192, 256, 384, 512])
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--zeros", action="store_true")
    a = ap.parse_args()
    if a.zeros:
        lines = zeros_arm(a)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    bf, q4 = weight_bytes_70b()
    lines = [f"Llama-3-70B projection weights: bf16 {bf / 1e9:.1f} GB, int4 (Int4Weight.nbytes()) {q4 / 1e9:.1f} GB", "",
             "| shape | M | w4 us | dequant us | bf16 us | bf16 / w4 | bf16 / dequant |", "|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    streams = {key: torch.cuda.Stream() for key in ("w4", "dequant", "bf16")}
    for name in a.shapes:
        n, k, sw = SHAPES[name]
        wb = [(torch.randn(n, k, device="cuda") * 0.02).to(torch.bfloat16)
              for _ in range(min(24, max(2, -(-MALL_X3 // (2 * n * k)))))]
        w4 = [int4.quantize_weight(wb[0])]
        while len(w4) < max(2, -(-MALL_X3 // (n * k // 2))):
            w4.append(int4.Int4Weight(w4[0].packed.clone(), w4[0].scale.clone()))
        act = ops.silu_mul if sw else (lambda y: y)
        for m in a.m:
            x = torch.randn(m, k, device="cuda").to(torch.bfloat16)
            impls = {
                "w4": lambda i: act(int4.linear_int4(x, w4[i % len(w4)], dequant_min_m=1 << 30)),
                "dequant": lambda i: act(int4.linear_int4(x, w4[i % len(w4)], dequant_min_m=1)),
                "bf16": (lambda i: ops.linear_swiglu(x, wb[i % len(wb)])) if sw else
                        (lambda i: ops.linear(x, wb[i % len(wb)])),
            }
            t = race(impls, streams, max(len(w4), 8), a.iters)
            lines.append(f"| {name} | {m} | {t['w4']:.1f} | {t['dequant']:.1f} | {t['bf16']:.1f} | "
                         f"{t['bf16'] / t['w4']:.2f} | {t['bf16'] / t['dequant']:.2f} |")
            print(lines[-1], flush=True)
        del wb, w4
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
