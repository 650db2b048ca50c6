"""Per-token log-probabilities over the LM head's logits (256 x 128256 bf16), us per call:
ops.token_logprobs (csrc/kernels/sampler.hip token_logprobs_kernel) at n = 0, 5 and 20 with every
row asking and with 1 row of 256 asking, next to the torch chain it replaces
(float().log_softmax, topk, gather) and to ops.argmax as a reminder of scale.  Eight rotating
inputs (each round of them is larger than the L2 and the Infinity Cache), event timing, median of
five rounds.

    python bench/logprobs_bench.py [--json-out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from distributed_llms_amd import ops

VOCAB = 128256
ROWS = 256


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


def torch_chain(x, ids, n):
    """What the kernel replaces: a [B, V] fp32 copy, log_softmax, top-k and a gather."""
    lp = x.float().log_softmax(-1)
    chosen = lp.gather(1, ids.long().unsqueeze(1)).squeeze(1)
    if n == 0:
        return chosen, None, None
    top_lp, top_ids = lp.topk(n, dim=-1)
    return chosen, top_ids, top_lp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logprobs_bench needs a GPU")
    xs = [(torch.randn(ROWS, VOCAB, device="cuda") * 3.0).to(torch.bfloat16) for _ in range(8)]
    ids = (torch.arange(ROWS, dtype=torch.int32, device="cuda") * 487) % VOCAB
    out = []
    cases = [("argmax", lambda i: ops.argmax(xs[i % 8]), 40)]
    for n in (0, 5, 20):
        every = torch.full((ROWS,), n, dtype=torch.int32, device="cuda")
        one = torch.full((ROWS,), -1, dtype=torch.int32, device="cuda")
        one[ROWS // 2] = n
        cases.append((f"kernel n={n} all rows", lambda i, w=every, n=n: ops.token_logprobs(xs[i % 8], ids, w, n), 40))
        cases.append((f"kernel n={n} 1 row of {ROWS}", lambda i, w=one, n=n: ops.token_logprobs(xs[i % 8], ids, w, n), 40))
        cases.append((f"torch chain n={n}", lambda i, n=n: torch_chain(xs[i % 8], ids, n), 8))
    for name, fn, iters in cases:
        t = timed(fn, iters)
        out.append({"rows": ROWS, "vocab": VOCAB, "case": name, "us": round(t, 1)})
        print(f"rows={ROWS:4d} vocab={VOCAB}  {name:32s} {t:9.1f} us", flush=True)
    if a.json_out:
        with open(a.json_out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
