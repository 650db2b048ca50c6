"""Seeded sampling over the LM head's logits (B x 128256 bf16), us per call, next to ops.argmax and
the torch chain of engine/sampler.py called without seeds.  Eight rotating inputs (each round of
them is larger than the L2; at 64 rows the 131 MB still fit the 256 MiB Infinity Cache), event
timing, median of five rounds.

    python bench/sampler_bench.py [--json-out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from distributed_llms_amd import knobs, ops
from distributed_llms_amd.engine.sampler import sample

VOCAB = 128256


def timed(fn, iters):
    fn(0)
    torch.cuda.synchronize()
    res = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i)
        e1.record()
        e1.synchronize()
        res.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    out = []
    for rows in (64, 256):
        xs = [(torch.randn(rows, VOCAB, device="cuda") * 3.0).to(torch.bfloat16) for _ in range(8)]
        seeds = torch.arange(rows, dtype=torch.int64, device="cuda") * 7919 + 1
        pos = torch.arange(rows, dtype=torch.int32, device="cuda") + 17

        def par(temp_e4, k, p_e4, half_greedy=False):
            t = torch.tensor([[temp_e4, k, p_e4]] * rows, dtype=torch.int32)
            if half_greedy:
                t[::2, 0] = 0
            return t.cuda()

        cases = [("argmax", lambda i: ops.argmax(xs[i % 8]), 40)]
        for name, p in (("fused T=1 k=0 p=1", par(10000, 0, 10000)), ("fused T=1 k=50 p=1", par(10000, 50, 10000)),
                        ("fused T=1 k=0 p=0.9", par(10000, 0, 9000)),
                        ("fused half greedy, k=50 p=0.9", par(10000, 50, 9000, True))):
            cases.append((name, lambda i, p=p: ops.sample_rows(xs[i % 8], p, seeds, pos), 40))
        temps, ks, ps = [1.0] * rows, [50] * rows, [0.9] * rows
        cases.append(("torch unseeded T=1 k=50 p=0.9", lambda i: sample(xs[i % 8], temps, ks, ps), 8))
        cases.append(("torch unseeded T=1 k=0 p=1", lambda i: sample(xs[i % 8], temps, [0] * rows, [1.0] * rows), 8))
        if rows == 64:
            # knobs.fused_sampler off: the host reference behind a device-to-host copy of the logits
            p_off = par(10000, 50, 9000)

            def off(i):
                with knobs.override(fused_sampler=False):
                    return ops.sample_rows(xs[i % 8], p_off, seeds, pos)
            cases.append(("reference on the host (knob off) k=50 p=0.9", off, 1))
        for name, fn, iters in cases:
            t = timed(fn, iters)
            out.append({"rows": rows, "case": name, "us": round(t, 1)})
            print(f"rows={rows:4d} vocab={VOCAB}  {name:44s} {t:9.1f} us", flush=True)
    if a.json_out:
        with open(a.json_out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
