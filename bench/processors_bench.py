"""Logit processors over the LM head's logits (256 x 128256 bf16), us per call: the three kernels of
csrc/kernels/logit_processors.hip (ops.logit_state_update / apply_logit_processors /
logit_state_count) with 1, 32 and 256 of the 256 rows asking and token histories of 128 and 4096
tokens (half prompt, half output; 16 bias entries per row), next to the torch formulation of the
same contract -- a scatter_add count over [B, V], a where chain, an indexed bias add, on the asking
rows only -- and to a device copy of the bytes the apply kernel must move (one logits row and one
state row per asking row).  Eight rotating logits buffers, event timing, median of five rounds.

    python bench/processors_bench.py [--json-out FILE] [--engine]

--engine adds one engine round (bench.py's single-GPU workload: llama3-8b, 256 x 128 + 128) with
every request asking, next to the same round plain.
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

from distributed_llms_amd import ops
from distributed_llms_amd.engine.logit_state import LogitState
from distributed_llms_amd.ops import reference as ref

VOCAB = 128256
ROWS = 256
N_BIAS = 16
REP, PRES, FREQ = 1.3, 0.5, 0.25


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


def proc_rows(asking, hist, flags):
    p = np.zeros((ROWS, ref.PROC_WORDS), dtype=np.int32)
    p[:, ref.PROC_ROW] = -1
    p[:asking, ref.PROC_ROW] = np.arange(asking)
    p[:asking, ref.PROC_PROMPT_LEN] = hist // 2
    p[:asking, ref.PROC_FLAGS] = flags
    p[:asking, ref.PROC_REP:ref.PROC_FREQ + 1] = np.array([REP, PRES, FREQ], dtype=np.float32).view(np.int32)
    return torch.from_numpy(p).cuda()


def torch_chain(x, hist, plen, bias_ids, bias_vals):
    """The same contract in torch ops on the asking rows x [A, V]; hist [A, H] int64 tokens, the
    first ``plen`` of each the prompt."""
    a, v = x.shape
    out = hist[:, plen:]
    cnt = torch.zeros(a, v, dtype=torch.int32, device=x.device).scatter_add_(
        1, out, torch.ones_like(out, dtype=torch.int32))
    seen = torch.zeros(a, v, dtype=torch.bool, device=x.device).scatter_(1, hist, True)
    xf = x.float()
    xf = torch.where(seen, torch.where(xf > 0, xf / REP, xf * REP), xf)
    xf = xf - FREQ * cnt - PRES * (cnt > 0)
    xf.scatter_add_(1, bias_ids, bias_vals)
    x.copy_(xf)


def kernels(out):
    g = torch.Generator(device="cuda").manual_seed(0)
    xs = [(torch.randn(ROWS, VOCAB, device="cuda", generator=g) * 3.0).to(torch.bfloat16) for _ in range(8)]
    ls = LogitState().ensure(ROWS, VOCAB, "cuda")
    seq_lens = torch.full((ROWS,), 1 << 20, dtype=torch.int32, device="cuda")
    drawn = (torch.arange(ROWS, dtype=torch.int32, device="cuda") * 487) % VOCAB
    for hist in (128, 4096):
        for asking in (1, 32, 256):
            toks = torch.randint(0, VOCAB, (ROWS, hist), device="cuda", generator=g, dtype=torch.int32)
            ids = toks[:asking].reshape(-1).contiguous()
            cu = torch.zeros(ROWS + 1, dtype=torch.int32, device="cuda")
            cu[1:asking + 1] = torch.arange(1, asking + 1, dtype=torch.int32, device="cuda") * hist
            cu[asking + 1:] = asking * hist
            bcu = torch.zeros(ROWS + 1, dtype=torch.int32, device="cuda")
            bcu[1:asking + 1] = torch.arange(1, asking + 1, dtype=torch.int32, device="cuda") * N_BIAS
            bcu[asking + 1:] = asking * N_BIAS
            bids = torch.randint(0, VOCAB, (asking, N_BIAS), device="cuda", generator=g, dtype=torch.int32)
            bvals = torch.rand(asking, N_BIAS, device="cuda", generator=g) * 10 - 5
            p_up = proc_rows(asking, hist, ref.PROC_UPDATE | ref.PROC_SAMPLE)
            p_dec = proc_rows(asking, hist, ref.PROC_SAMPLE)

            def update(i):
                ops.logit_state_update(ls, ids, cu, p_up, bcu, bids.reshape(-1), bvals.reshape(-1))

            t_up = timed(update, 20)
            t_apply = timed(lambda i: ops.apply_logit_processors(xs[i % 8], ls, p_dec, seq_lens, -1), 40)
            t_count = timed(lambda i: ops.logit_state_count(ls, drawn, p_dec), 40)
            update(0)                                   # the counts the timing loop added are gone again
            h64, b64 = toks[:asking].long(), bids.long()
            t_torch = timed(lambda i: torch_chain(xs[i % 8][:asking], h64, hist // 2, b64, bvals), 8)
            nbytes = asking * (VOCAB * 2 + ls.state.shape[1] * 4)
            src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            dsts = [torch.empty_like(src) for _ in range(4)]
            t_copy = timed(lambda i: dsts[i % 4].copy_(src), 40)
            row = {"rows": ROWS, "vocab": VOCAB, "asking": asking, "history": hist, "update_us": round(t_up, 1),
                   "apply_us": round(t_apply, 1), "count_us": round(t_count, 1), "torch_us": round(t_torch, 1),
                   "torch_over_apply_count": round(t_torch / (t_apply + t_count), 1),
                   "torch_over_all_three": round(t_torch / (t_up + t_apply + t_count), 1),
                   "apply_bytes": nbytes, "apply_gbps": round(nbytes / t_apply * 1e-3, 1),
                   "copy_same_bytes_us": round(t_copy, 1)}
            out.append(row)
            print(json.dumps(row), flush=True)


def engine_round(out):
    from distributed_llms_amd.config import EngineConfig
    from distributed_llms_amd.engine.llm_engine import LLMEngine
    from distributed_llms_amd.engine.sequence import SamplingParams
    batch, plen, glen = 256, 128, 128
    eng = LLMEngine(EngineConfig(model="synthetic:llama3-8b", max_batch=batch, max_prefill_tokens=batch * plen,
                                 max_seq_len=plen + glen + 32))
    vocab = eng.mcfg.vocab_size
    plain = SamplingParams(max_new_tokens=glen, ignore_eos=True)
    asking = SamplingParams(max_new_tokens=glen, ignore_eos=True, repetition_penalty=REP, presence_penalty=PRES,
                            frequency_penalty=FREQ, min_tokens=8, logit_bias={i * 97: 1.0 for i in range(N_BIAS)})

    def round_(params, seed):
        rng = np.random.default_rng(seed)
        prompts = rng.integers(3, vocab, size=(batch, plen)).tolist()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for p in prompts:
            eng.add_request(p, params)
        eng.run_until_done()
        torch.cuda.synchronize()
        return batch * glen / (time.perf_counter() - t0)

    round_(plain, 100)
    round_(asking, 101)
    res = {"plain": [], "asking": []}
    for r in range(3):                                   # interleaved
        res["plain"].append(round(round_(plain, r), 1))
        res["asking"].append(round(round_(asking, r), 1))
    row = {"engine_round": f"llama3-8b {batch} x {plen}+{glen}", "plain_tok_s": res["plain"], "asking_tok_s": res["asking"],
           "asking_over_plain": round(statistics.median(res["asking"]) / statistics.median(res["plain"]), 4)}
    out.append(row)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json-out", default=None)
    ap.add_argument("--engine", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("processors_bench needs a GPU")
    out = []
    kernels(out)
    if a.engine:
        engine_round(out)
    if a.json_out:
        with open(a.json_out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
