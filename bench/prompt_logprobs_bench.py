"""Prompt scoring at Llama-3-8B's LM head (K = 4096, V = 128256), us per call: the fused linear + log-softmax +
gather kernel (ops.lm_head_logprobs, csrc/kernels/lm_head_logprobs.hip) next to the materialised pair -- ops.linear
writes the [T, V] bf16 logits, ops.token_logprobs (want = 0) reads them back for one float per row -- at T = 256,
2048 and 8192; T = 32768 on the fused path only (the pair would first allocate T x V x 2 bytes of logits: 8.4 GB).
The two paths alternate inside every round; device events around ``iters`` calls after a warm-up of each shape,
``iters`` sized from a first timed call so that every window lasts at least --min-ms (500 ms); median of five rounds.
Run it twice and compare before trusting a difference.  FLOP/s counts the GEMM's 2 T V K only.  Both paths' results are compared at every timed T.

    python bench/prompt_logprobs_bench.py [--json-out FILE] [--t 256,2048,8192] [--fused-only-t 32768]
                                          [--min-ms 500]
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from distributed_llms_amd import _ext, ops

K, V = 4096, 128256


def window(fn, iters):
    """us per call of ``iters`` back-to-back calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def rounds(fns, min_ms):
    """(median us per call, spread, iters) of each fn: five rounds, the fns alternating inside a round; a fn's window
    is as many calls as fill ``min_ms``, by a first timed pair of calls after the warm-up."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    iters = [max(2, math.ceil(min_ms * 1e3 / window(fn, 2))) for fn in fns]
    res = [[] for _ in fns]
    for _ in range(5):
        for i, fn in enumerate(fns):
            res[i].append(window(fn, iters[i]))
    return [statistics.median(r) for r in res], [max(r) - min(r) for r in res], iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--json-out")
    ap.add_argument("--t", default="256,2048,8192")
    ap.add_argument("--fused-only-t", default="32768")
    ap.add_argument("--min-ms", type=float, default=500.0)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("prompt_logprobs_bench: needs the GPU (no CPU timing)")
    g = torch.Generator(device="cuda").manual_seed(0)
    w = (torch.randn(V, K, device="cuda", generator=g) * 0.02).to(torch.bfloat16)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {"device": torch.cuda.get_device_name(0), "cus": cus, "k": K, "v": V, "rows": []}
    both = [int(t) for t in a.t.split(",") if t]
    for t in both + [int(t) for t in a.fused_only_t.split(",") if t]:
        x = torch.randn(t, K, device="cuda", generator=g).to(torch.bfloat16)
        tg = torch.randint(0, V, (t,), device="cuda", generator=g).to(torch.int32)
        want = torch.zeros(t, dtype=torch.int32, device="cuda")
        s = ops.lm_head_ranges(t, V, cus)
        fns = [lambda: ops.lm_head_logprobs(x, w, tg)]
        if t in both:
            fns.append(lambda: ops.token_logprobs(ops.linear(x, w), tg, want, 0)[0])
        us, spread, iters = rounds(fns, a.min_ms)
        row = {"t": t, "ranges": s, "grid": -(-t // 256) * s, "iters": iters, "fused_us": us[0],
               "fused_spread_us": spread[0], "fused_tflops": 2.0 * t * V * K / us[0] * 1e-6,
               "workspace_bytes": t * _ext.kernels().LM_HEAD_WAVES * s * 3 * 4, "logits_bytes": t * V * 2}
        if t in both:
            row.update(pair_us=us[1], pair_spread_us=spread[1], pair_tflops=2.0 * t * V * K / us[1] * 1e-6,
                       max_abs_diff=(fns[0]() - fns[1]()).abs().max().item())
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
        del x, fns
        torch.cuda.empty_cache()
    if a.json_out:
        with open(a.json_out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"device": out["device"], "cus": cus}))


if __name__ == "__main__":
    main()
