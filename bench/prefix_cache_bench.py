"""Serving with a shared prompt header, prefix cache on against off.

    python bench/prefix_cache_bench.py [--model llama3-8b] [--headers 1024 4096] [--out FILE.json]

Workload: 64 requests, each a shared header (1k or 4k tokens) plus a 32-token tail of its own, submitted
together, 32 generated tokens each; a fresh header per round so that no round finds the previous round's
blocks.  Per (header, cache) after one warm-up round: TTFT p50 / p99, output tok/s, prompt tokens
computed, hit tokens, and the KV blocks the running requests hold at their peak (a shared header is held
once).  Rounds of the two settings alternate; the figures are medians over ``--rounds`` rounds and the
spread is (max - min) / median of the round times.  One JSON line per configuration.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from distributed_llms_amd.config import EngineConfig
from distributed_llms_amd.engine.llm_engine import LLMEngine
from distributed_llms_amd.engine.sequence import SamplingParams
from distributed_llms_amd.utils.metrics import percentile


def make_round(vocab, header, tail, n, seed):
    rng = np.random.default_rng(seed)
    h = rng.integers(3, vocab - 1, size=header).tolist()
    return [h + rng.integers(3, vocab - 1, size=tail).tolist() for _ in range(n)]


def run_round(eng, prompts, gen):
    p = SamplingParams(max_new_tokens=gen, ignore_eos=True)
    used0 = eng.bm.num_blocks - eng.bm.num_free()        # evictable blocks count as free: held by nobody
    pre0 = eng.num_prefill_tokens
    hit0 = eng.scheduler.prefix_stats()["hit_tokens"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seqs = [eng.add_request(q, p) for q in prompts]
    held = 0
    while eng.has_work():
        eng.step()
        held = max(held, eng.bm.num_blocks - eng.bm.num_free() - used0)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    assert all(len(s.output) == gen for s in seqs)
    tt = [s.ttft() for s in seqs]
    return {"elapsed_s": el, "ttft_p50_ms": 1e3 * percentile(tt, 50), "ttft_p99_ms": 1e3 * percentile(tt, 99),
            "tok_per_s": len(seqs) * gen / el, "prefill_tokens": eng.num_prefill_tokens - pre0,
            "hit_tokens": eng.scheduler.prefix_stats()["hit_tokens"] - hit0, "blocks_held_peak": held}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--headers", nargs="+", type=int, default=[1024, 4096])
    ap.add_argument("--tail", type=int, default=32)
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--gen", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prefix_cache_bench needs the GPU")
    max_len = max(a.headers) + a.tail + a.gen + 32
    # two engines side by side (their rounds alternate), each with its own weights and KV pool
    engines = {cache: LLMEngine(EngineConfig(model=f"synthetic:{a.model}", max_batch=a.requests, max_seq_len=max_len,
                                             max_prefill_tokens=16384, kv_cache_fraction=0.35,
                                             enable_prefix_caching=cache))
               for cache in (False, True)}
    vocab = engines[False].mcfg.vocab_size
    lines = []
    for header in a.headers:
        rounds = {False: [], True: []}
        for r in range(a.rounds + 1):
            for cache in (False, True):
                res = run_round(engines[cache], make_round(vocab, header, a.tail, a.requests, 1000 * header + r), a.gen)
                if r:                   # round 0 warms up graphs and the allocator
                    rounds[cache].append(res)
        for cache in (False, True):
            rs = rounds[cache]
            med = {k: statistics.median(x[k] for x in rs) for k in rs[0]}
            el = [x["elapsed_s"] for x in rs]
            line = {"bench": "prefix_cache", "model": a.model, "header": header, "tail": a.tail, "requests": a.requests,
                    "gen": a.gen, "cache": cache, "rounds": len(rs), **{k: round(v, 3) for k, v in med.items()},
                    "spread": round((max(el) - min(el)) / med["elapsed_s"], 4)}
            lines.append(line)
            print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
