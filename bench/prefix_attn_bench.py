"""Tail-prefill attention microbenchmark: the split-context kernel (version 5) against v4, the kernel
the default dispatch runs at these shapes, for a few query rows over a long cached context -- the
shape a prefix-cache hit produces.

    python bench/prefix_attn_bench.py [--out FILE.json]

Shapes: Llama-3-8B heads (Hq 32, Hkv 8, D 128); q_len 1..64 new rows per sequence over a context of
1k..32k tokens already in the paged cache; B in {1, 8, 64} sequences.  Both kernels read a rotated q
[T, Hq, D]; version 5's time includes its split-reduce launch.  Not in either number: the rotated-q write
of rope_cache_append that version 5 needs and v4's in-kernel RoPE saves (T x Hq x D bf16, 8 KB per row, at most 4 MB here).

Method: the K/V of a call come from one of several cache copies taken in rotation (a layer of the engine
never finds its K/V warm from the previous call either): enough copies for ``--cold-bytes`` (512 MB), but 16
at the most, so at B = 1 the rotation covers only 64 / 128 / 256 MB at 1k / 2k / 4k of context and does not
exceed the 256 MiB Infinity Cache there -- those cells are cache-warm for both kernels.  The two versions
alternate, window by window; a window is ``iters`` calls (about ``--window-us`` = 20 ms of device time,
short: cells of two 12 us launches show spreads of tens of per cent) between two device events; per cell
the median over ``reps`` windows and the spread (max - min) / median of each version.
The outputs of the two kernels are compared at every timed shape.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from distributed_llms_amd import ops

HQ, HKV, D, BS = 32, 8, 128, 32


def window(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        f(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters        # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qlens", nargs="+", type=int, default=[1, 4, 16, 32, 64])
    ap.add_argument("--ctxs", nargs="+", type=int, default=[1024, 2048, 4096, 8192, 16384, 32768])
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 8, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-us", type=float, default=20000.0, help="device time a window aims for")
    ap.add_argument("--cold-bytes", type=float, default=512e6, help="K/V bytes the rotation covers at least")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prefix_attn_bench needs the GPU")
    scale = D ** -0.5
    rows = []
    print(f"{'B':>3s} {'ctx':>6s} {'q':>3s} {'nsplit':>6s} {'v4 us':>9s} {'+-%':>5s} {'v5 us':>9s} {'+-%':>5s} "
          f"{'v4/v5':>6s} {'maxdiff':>8s}", flush=True)
    for b in a.batches:
        for ctx in a.ctxs:
            nblk = -(-ctx // BS)
            kv_bytes = 2 * b * nblk * HKV * BS * D * 2
            copies = int(max(1, min(16, -(-a.cold_bytes // kv_bytes))))
            ks = [(torch.randn(b * nblk + 1, HKV, BS, D, device="cuda") * 0.5).to(torch.bfloat16) for _ in range(copies)]
            vs = [(torch.randn(b * nblk + 1, HKV, D, BS, device="cuda") * 0.5).to(torch.bfloat16) for _ in range(copies)]
            bt = (torch.randperm(b * nblk, device="cuda").to(torch.int32) + 1).view(b, nblk)
            sl = torch.full((b,), ctx, dtype=torch.int32, device="cuda")
            for ql in a.qlens:
                cu = torch.arange(0, (b + 1) * ql, ql, dtype=torch.int32, device="cuda")
                q = torch.randn(b * ql, HQ, D, device="cuda").to(torch.bfloat16)
                nsplit = ops.prefill_split_plan(b, HKV, ql, ctx, HQ // HKV)[0]
                out4, out5 = torch.empty_like(q), torch.empty_like(q)
                ws = (torch.empty(b * ql * HQ * nsplit * D, dtype=torch.float32, device="cuda"),
                      torch.empty(b * ql * HQ * nsplit * 2, dtype=torch.float32, device="cuda"))

                def f4(i):
                    ops.paged_attention_prefill(q, ks[i % copies], vs[i % copies], bt, cu, sl, scale, max_q_len=ql,
                                                version=4, out=out4)

                def f5(i):
                    ops.paged_attention_prefill(q, ks[i % copies], vs[i % copies], bt, cu, sl, scale, max_q_len=ql,
                                                version=ops.PREFILL_SPLIT, out=out5, max_ctx=ctx, workspace=ws)

                f4(0), f5(0)
                diff = float((out4.float() - out5.float()).abs().max())
                t4 = window(f4, 3)
                iters = int(max(3, min(200, a.window_us / max(t4, 1.0))))
                w4, w5 = [], []
                for _ in range(a.reps):
                    w4.append(window(f4, iters))
                    w5.append(window(f5, iters))
                m4, m5 = statistics.median(w4), statistics.median(w5)
                s4, s5 = (max(w4) - min(w4)) / m4, (max(w5) - min(w5)) / m5
                rows.append({"batch": b, "ctx": ctx, "q_len": ql, "nsplit": nsplit, "v4_us": round(m4, 2),
                             "v4_spread": round(s4, 4), "v5_us": round(m5, 2), "v5_spread": round(s5, 4),
                             "speedup": round(m4 / m5, 3), "max_abs_diff": diff, "iters": iters, "kv_copies": copies})
                print(f"{b:3d} {ctx:6d} {ql:3d} {nsplit:6d} {m4:9.1f} {100 * s4:5.1f} {m5:9.1f} {100 * s5:5.1f} "
                      f"{m4 / m5:6.2f} {diff:8.4f}", flush=True)
            del ks, vs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
