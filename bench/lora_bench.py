"""Multi-LoRA cost on the GPU: the shrink / expand kernels of csrc/kernels/lora.hip at Llama-3-8B
projection shapes, and an engine A/B.

Kernel part: shrink + expand, us per call, for the four projections (qkv 4096 -> 4096|1024|1024, o
4096 -> 4096, gate|up 4096 -> 14336|14336, down 14336 -> 4096) at M in {16, 64, 256, 4096} rows and
rank in {16, 64}, with every row on one adapter and with the rows spread over 8 adapters.  Eight
rotating input / output buffers, event timing, median of five rounds.

Engine part (--engine): bench.py's single-GPU workload (llama3-8b, 256 x 128 + 128) on one engine
with 8 rank-16 adapters configured, rounds interleaved: no request with an adapter, every request
on one adapter, the requests spread over the 8 adapters.  ``--base`` adds rounds of an engine
without ``lora_modules`` (what the parent commit runs) to the interleave.

    python bench/lora_bench.py [--json-out FILE] [--engine] [--base] [--rounds N]
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

from distributed_llms_amd.ops import lora as lo
from distributed_llms_amd.ops import reference as ref

H, I, Q, KV = 4096, 14336, 4096, 1024
PROJ = {"qkv": (H, (Q, KV, KV)), "o": (Q, (H,)), "gate_up": (H, (I, I)), "down": (I, (H,))}
NBUF = 8


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


def kernels(out):
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, (k, widths) in PROJ.items():
        n = sum(widths)
        starts = tuple(sum(widths[:i]) for i in range(len(widths)))
        for rank in (16, 64):
            rp = ref.lora_rank_pad(rank)
            for nslots in (1, 8):
                a = torch.zeros(nslots, len(widths) * rp, k, device="cuda", dtype=torch.bfloat16)
                b = torch.zeros(nslots, n, rp, device="cuda", dtype=torch.bfloat16)
                for i in range(len(widths)):
                    a[:, i * rp:i * rp + rank] = (torch.randn(nslots, rank, k, device="cuda", generator=g) * 0.02
                                                  ).to(torch.bfloat16)
                b[:, :, :rank] = (torch.randn(nslots, n, rank, device="cuda", generator=g) * 0.02).to(torch.bfloat16)
                w = lo.LoraWeight(a, b, torch.ones(nslots, device="cuda"), starts)
                for m in (16, 64, 256, 4096):
                    nb = NBUF if m * n * 2 * NBUF < (2 << 30) else 2
                    xs = [torch.randn(m, k, device="cuda", generator=g).to(torch.bfloat16) for _ in range(nb)]
                    ys = [torch.randn(m, n, device="cuda", generator=g).to(torch.bfloat16) for _ in range(nb)]
                    plan = lo.make_plan((np.arange(m) % nslots).astype(np.int32), "cuda")
                    ws = torch.empty(lo.workspace_floats(k, plan.nt, a.shape[1]), dtype=torch.float32, device="cuda")
                    iters = 40 if m <= 256 else 10
                    t_s = timed(lambda i: lo.shrink(xs[i % nb], w, plan, ws), iters)
                    t_e = timed(lambda i: lo.expand(ys[i % nb], ws, k, w, plan), iters)
                    t_b = timed(lambda i: lo.apply(ys[i % nb], xs[i % nb], w, plan), iters)
                    row = {"proj": name, "K": k, "N": n, "M": m, "rank": rank, "adapters": nslots, "tiles": plan.nt,
                           "shrink_us": round(t_s, 1), "expand_us": round(t_e, 1), "both_us": round(t_b, 1)}
                    out.append(row)
                    print(json.dumps(row), flush=True)
                    del xs, ys


def engine_rounds(out, rounds, with_base):
    from distributed_llms_amd.config import EngineConfig
    from distributed_llms_amd.engine.llm_engine import LLMEngine
    from distributed_llms_amd.engine.sequence import SamplingParams
    batch, plen, glen = 256, 128, 128
    names = [f"a{i}" for i in range(8)]
    args = dict(model="synthetic:llama3-8b", max_batch=batch, max_prefill_tokens=batch * plen,
                max_seq_len=plen + glen + 32, kv_cache_fraction=0.35)
    eng = LLMEngine(EngineConfig(lora_modules={n: f"synthetic:16:{i + 1}" for i, n in enumerate(names)}, **args))
    base = LLMEngine(EngineConfig(**args)) if with_base else None
    vocab = eng.mcfg.vocab_size

    def round_(e, who, seed):
        rng = np.random.default_rng(seed)
        prompts = rng.integers(3, vocab, size=(batch, plen)).tolist()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, p in enumerate(prompts):
            e.add_request(p, SamplingParams(max_new_tokens=glen, ignore_eos=True, adapter=who(i)))
        e.run_until_done()
        torch.cuda.synchronize()
        return batch * glen / (time.perf_counter() - t0)

    kinds = {"no_adapter": (eng, lambda i: None), "one_adapter": (eng, lambda i: names[0]),
             "eight_adapters": (eng, lambda i: names[i % 8])}
    if base is not None:
        kinds = dict({"without_lora_modules": (base, lambda i: None)}, **kinds)
    for j, (e, who) in enumerate(kinds.values()):
        round_(e, who, 100 + j)                          # warm-up: graph capture, allocator
    res = {k: [] for k in kinds}
    for r in range(rounds):                              # interleaved
        for k, (e, who) in kinds.items():
            res[k].append(round(round_(e, who, r), 1))
    row = {"engine_round": f"llama3-8b {batch} x {plen}+{glen}, 8 adapters of rank 16 configured"}
    for k, v in res.items():
        row[k + "_tok_s"] = v
        row[k + "_median"] = statistics.median(v)
    ref_rate = row[("without_lora_modules" if base is not None else "no_adapter") + "_median"]
    for k in res:
        row[k + "_ratio"] = round(row[k + "_median"] / ref_rate, 4)
    out.append(row)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json-out", default=None)
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--base", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_bench needs a GPU")
    out = []
    if not a.no_kernels:
        kernels(out)
    if a.engine:
        engine_rounds(out, a.rounds, a.base)
    if a.json_out:
        with open(a.json_out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
