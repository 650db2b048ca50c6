"""SHA-256 of the logits of one prefill step and three decode steps through LLMEngine, per model config and quant, eager
and with decode graphs: the bit-for-bit comparison of two trees' model stage host path (profiles/stage_forward.md).

    python bench/debug/stage_digest.py [--out digests.json]

Batch 3, prompts of 5 / 33 / 70 tokens, the synthetic weights of the engine tests (seed 5).  Run it twice in one tree
first: a config whose digests differ between two runs of the same tree (atomics in the MoE combine) says nothing."""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from distributed_llms_amd.config import EngineConfig, get_model_config      # noqa: E402
from distributed_llms_amd.engine.llm_engine import LLMEngine                # noqa: E402
from distributed_llms_amd.engine.sequence import SamplingParams             # noqa: E402
from distributed_llms_amd.models import weights as W                        # noqa: E402
from distributed_llms_amd.models.stage import ModelStage                    # noqa: E402

CONFIGS = [("tiny-llama", "none", False), ("tiny-llama", "fp8", False), ("tiny-llama", "int4", False),
           ("tiny-llama-d128", "none", False), ("tiny-qwen2-g7", "none", False), ("tiny-qwen3-d128", "none", False),
           ("tiny-mixtral", "none", False), ("tiny-mixtral", "fp8", False), ("tiny-llama", "none", True)]
PROMPT_LENS = (5, 33, 70)
DECODE_STEPS = 3


def digests(name: str, quant: str, lora: bool, graphs: bool, device: str = "cuda"):
    cfg = get_model_config(name)
    dtype = "bfloat16" if device == "cuda" else "float32"
    ecfg = EngineConfig(model=name, dtype=dtype, device=device, quant=quant, max_batch=4, max_seq_len=256,
                        num_kv_blocks=64, graph_batch_sizes=(1, 2, 4), use_graphs=graphs,
                        lora_modules={"a": "synthetic:8:11"} if lora else {})
    sd = W.synth_hf_state_dict(cfg, seed=5, dtype=torch.float32)
    stage = ModelStage(cfg, 0, cfg.num_layers, device, getattr(torch, dtype)).load_hf_state(sd)
    stage.quantize(quant).load_lora(ecfg)
    eng = LLMEngine(ecfg, stage)
    for i, n in enumerate(PROMPT_LENS):
        prompt = [(7 * i + 3 * j + 1) % cfg.vocab_size for j in range(n)]
        eng.add_request(prompt, SamplingParams(max_new_tokens=DECODE_STEPS + 2, ignore_eos=True,
                                               adapter="a" if lora and i != 1 else None))
    out = []
    for _ in range(1 + DECODE_STEPS):
        step = eng.scheduler.schedule(0)
        logits = eng.runner.execute(eng._host_batch(step))
        assert logits.shape == (len(PROMPT_LENS), cfg.vocab_size) and logits.dtype == stage.dtype
        out.append(hashlib.sha256(logits.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16])
        eng.scheduler.complete(step, logits.argmax(-1).to(torch.int32).cpu().numpy(), 0.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--device", default="cuda", help="cpu: a dry run of the script itself (float32)")
    args = ap.parse_args()
    table = {}
    for name, quant, lora in CONFIGS:
        for graphs in (False, True):
            key = f"{name}|{quant}{'|lora' if lora else ''}|{'graphs' if graphs else 'eager'}"
            table[key] = digests(name, quant, lora, graphs, args.device)
            print(key, *table[key], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(table, f, indent=1)


if __name__ == "__main__":
    main()
