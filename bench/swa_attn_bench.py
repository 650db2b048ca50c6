"""Sliding-window attention microbenchmark: the windowed decode and prefill kernels (attention_swa.hip) against
the causal kernels on the same shapes, Mistral-7B heads (Hq 32, Hkv 8, D 128), W = 4096.

    python bench/swa_attn_bench.py [--out FILE.json]

Decode: B in {64, 256} sequences of ctx in {4k, 8k, 32k} keys, windowed against the causal split-KV kernel (which
reads all ctx keys; past W the two compute different functions -- the comparison is of time only).  Prefill: fresh
prompts 1 x 16k and 8 x 4k, windowed against version 4 over the same rotated q.  Both sides read a rotated q.

Method: all sequences draw their blocks from one shuffled pool, each call's bytes far beyond the 256 MiB Infinity
Cache.  The two kernels alternate window by window; a window is ``iters`` calls (about ``--window-us`` of device
time) between two device events; per cell the median over ``--reps`` windows and the spread (max - min) / median.
At ctx <= W the two outputs are compared (same function, other split order).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from distributed_llms_amd import ops

HQ, HKV, D, BS, W = 32, 8, 128, 32, 4096


def window(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters        # us per call


def measure(fa, fb, reps, window_us):
    """Median us and spread of two callables, alternating windows."""
    for f in (fa, fb):
        f()
    torch.cuda.synchronize()
    iters = [max(2, int(window_us / max(window(f, 2), 1.0))) for f in (fa, fb)]
    ts = ([], [])
    for _ in range(reps):
        for i, f in enumerate((fa, fb)):
            ts[i].append(window(f, iters[i]))
    return [(statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[64, 256])
    ap.add_argument("--ctxs", nargs="+", type=int, default=[4096, 8192, 32768])
    ap.add_argument("--prefill", nargs="+", default=["1x16384", "8x4096"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-us", type=float, default=30000.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("swa_attn_bench needs the GPU")
    scale = D ** -0.5
    pf = [tuple(int(x) for x in s.split("x")) for s in a.prefill]
    nb = max([b * c // BS for b in a.batches for c in a.ctxs] + [b * t // BS for b, t in pf])
    k = torch.empty(nb, HKV, BS, D, dtype=torch.bfloat16, device="cuda").normal_()
    v = torch.empty(nb, HKV, D, BS, dtype=torch.bfloat16, device="cuda").normal_()
    rows = []
    print(f"{'kind':>7s} {'B':>4s} {'ctx':>6s} {'causal us':>10s} {'+-%':>5s} {'window us':>10s} {'+-%':>5s} {'ratio':>6s}")
    for b in a.batches:
        for ctx in a.ctxs:
            bt = torch.randperm(nb, device="cuda")[:b * ctx // BS].to(torch.int32).view(b, ctx // BS)
            sl = torch.full((b,), ctx, dtype=torch.int32, device="cuda")
            q = torch.randn(b, HQ, D, device="cuda").bfloat16()
            ws = ops.decode_workspace(b, HQ, D, "cuda")
            full = lambda: ops.paged_attention_decode(q, k, v, bt, sl, scale, max_ctx=ctx, workspace=ws)
            win = lambda: ops.paged_attention_decode(q, k, v, bt, sl, scale, workspace=ws, window=W)
            if ctx <= W:
                torch.testing.assert_close(full().float(), win().float(), atol=2e-2, rtol=2e-2)
            (tf_, sf), (tw, sw) = measure(full, win, a.reps, a.window_us)
            rows.append(dict(kind="decode", batch=b, ctx=ctx, causal_us=tf_, causal_spread=sf, window_us=tw,
                             window_spread=sw, plan=ops.decode_window_plan(b, HKV, W)))
            print(f"{'decode':>7s} {b:4d} {ctx:6d} {tf_:10.1f} {100 * sf:5.1f} {tw:10.1f} {100 * sw:5.1f} {tw / tf_:6.2f}")
    for b, t in pf:
        bt = torch.randperm(nb, device="cuda")[:b * t // BS].to(torch.int32).view(b, t // BS)
        sl = torch.full((b,), t, dtype=torch.int32, device="cuda")
        cu = torch.arange(b + 1, dtype=torch.int32, device="cuda") * t
        q = torch.randn(b * t, HQ, D, device="cuda").bfloat16()
        out = torch.empty_like(q)
        full = lambda: ops.paged_attention_prefill(q, k, v, bt, cu, sl, scale, max_q_len=t, version=4, out=out, max_ctx=t)
        win = lambda: ops.paged_attention_prefill(q, k, v, bt, cu, sl, scale, max_q_len=t, out=out, max_ctx=t, window=W)
        if t <= W:
            torch.testing.assert_close(full().float().clone(), win().float(), atol=2e-2, rtol=2e-2)
        (tf_, sf), (tw, sw) = measure(full, win, a.reps, a.window_us)
        rows.append(dict(kind="prefill", batch=b, ctx=t, causal_us=tf_, causal_spread=sf, window_us=tw, window_spread=sw))
        print(f"{'prefill':>7s} {b:4d} {t:6d} {tf_:10.1f} {100 * sf:5.1f} {tw:10.1f} {100 * sw:5.1f} {tw / tf_:6.2f}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
