"""What does not combine -- model x quant x tensor parallelism x LoRA x sub-layer cuts x prefix caching -- at every
entry point that refuses it, against a table recorded before the refusals were gathered into config.check_features.

ROWS holds the inputs; tests/golden/refusals.json holds, per row and entry point, the exception type and the full
message, or null where the call passes ("-": the stage could not be built, so its methods were not called).
``python tests/test_refusals.py --record`` rewrites it from whatever tree it runs in.  MESSAGES lists every refusal
that existed when the table was recorded: each must win somewhere in it, so the table cannot lose a message silently.
The rows with two violations pin which message wins."""
import json
import os
import sys

import pytest
import torch

from distributed_llms_amd.config import EngineConfig, get_model_config
from distributed_llms_amd.models import lora
from distributed_llms_amd.models.stage import ModelStage
from distributed_llms_amd.parallel.tensor_parallel import TPGroup

TABLE = os.path.join(os.path.dirname(__file__), "golden", "refusals.json")
ENTRY_POINTS = ["validate", "check_tensor_parallel", "check_engine", "ModelStage", "quantize", "load_lora",
                "build_stage_lora"]
DEFAULTS = dict(preset="tiny-llama", quant="none", tp=1, lora=False, fine=False, prefix=False, units=None, pad=None,
                rank=64)
# units: [u0, u1) in sub-layer atoms (five per layer); (0, 6) ends after a qkv projection, (1, 2) holds no weight
ROWS = [dict(DEFAULTS, **r) for r in [
    {},
    {"quant": "fp8"}, {"quant": "int4"}, {"lora": True}, {"tp": 2}, {"prefix": True}, {"fine": True},
    {"units": (0, 6)}, {"preset": "tiny-mixtral", "quant": "fp8", "tp": 2},
    # one violation
    {"quant": "int8"},
    {"preset": "tiny-qwen2", "quant": "fp8"}, {"preset": "tiny-qwen3", "quant": "fp8"},
    {"preset": "tiny-qwen2", "tp": 2}, {"preset": "tiny-qwen3", "tp": 2},
    {"preset": "tiny-mixtral", "quant": "int4"}, {"preset": "tiny-gpt2", "quant": "int4"},
    {"preset": "tiny-qwen2", "quant": "int4"}, {"quant": "int4", "tp": 2}, {"quant": "int4", "fine": True},
    {"quant": "int4", "units": (1, 2)}, {"quant": "fp8", "units": (1, 2)},
    {"tp": 2, "prefix": True}, {"tp": 2, "lora": True},
    {"preset": "tiny-gpt2", "lora": True}, {"quant": "fp8", "lora": True}, {"quant": "int4", "lora": True},
    {"lora": True, "fine": True}, {"lora": True, "rank": 0}, {"lora": True, "rank": 65},
    {"preset": "tiny-qwen2-g7", "pad": True}, {"preset": "tiny-qwen2-g7", "pad": True, "lora": True},
    {"preset": "tiny-gpt2", "units": (0, 6)}, {"preset": "tiny-mixtral", "units": (0, 6)},
    {"tp": 2, "units": (0, 6)}, {"preset": "tiny-qwen2-g7", "pad": True, "units": (0, 6)},
    {"lora": True, "units": (0, 6)}, {"units": (0, 99)}, {"tp": 3}, {"preset": "tiny-gpt2", "tp": 2},
    # two violations: which message wins
    {"preset": "tiny-qwen3", "quant": "fp8", "tp": 2}, {"preset": "tiny-qwen2", "quant": "int4", "tp": 2},
    {"quant": "int4", "tp": 2, "fine": True}, {"preset": "tiny-mixtral", "quant": "int4", "tp": 2},
    {"tp": 2, "prefix": True, "lora": True}, {"quant": "int4", "tp": 2, "lora": True},
    {"quant": "int4", "tp": 2, "prefix": True},
    {"preset": "tiny-qwen2", "quant": "fp8", "lora": True}, {"preset": "tiny-gpt2", "quant": "int4", "lora": True},
    {"quant": "int4", "lora": True, "fine": True}, {"quant": "fp8", "lora": True, "fine": True},
    {"preset": "tiny-gpt2", "lora": True, "rank": 0}, {"preset": "tiny-gpt2", "lora": True, "fine": True},
    {"preset": "tiny-qwen2-g7", "pad": True, "lora": True, "fine": True},
    {"preset": "tiny-qwen2-g7", "pad": True, "lora": True, "quant": "fp8"},
    {"preset": "tiny-qwen2-g7", "pad": True, "lora": True, "rank": 0},
    {"preset": "tiny-mixtral", "tp": 2, "units": (0, 6)}, {"preset": "tiny-qwen2", "tp": 2, "units": (0, 6)},
    {"tp": 3, "units": (0, 6)}, {"preset": "tiny-qwen2", "tp": 3}, {"lora": True, "fine": True, "units": (0, 6)},
    {"lora": True, "tp": 2, "units": (0, 6)}, {"lora": True, "tp": 2, "prefix": True, "fine": True},
]]

MESSAGES = [
    "tensor parallelism (tp > 1) is not supported for models with a qkv bias or a q/k norm (Qwen2 / Qwen3): the bias "
    "shard is not built",
    'quant="fp8" is not supported for models with a qkv bias or a q/k norm (Qwen2 / Qwen3)',
    'quant="int4" serves dense Llama-architecture models only (arch \'mixtral\', 4 experts)',
    'quant="int4" serves dense Llama-architecture models only (arch \'gpt2\', 0 experts)',
    'quant="int4" is not supported for models with a qkv bias or a q/k norm (Qwen2 / Qwen3)',
    'quant="int4" is not supported with tensor parallelism (tp > 1)',
    'quant="int4" is not supported with sub-layer pipeline cuts (DLLM_PP_FINE=1)',
    'quant="int4" converted no weight of this stage (N and K multiples of 128)',
    "quant 'int8' (none, fp8, int4)",
    "unknown quantization 'int8' (none, fp8, int4)",
    "prefix caching is not supported with tensor parallelism (tp > 1)",
    "LoRA adapters are not supported with tensor parallelism (tp > 1)",
    "max_lora_rank must be in [1, 64], got 0",
    "LoRA adapters are not supported on GPT-2 models",
    "LoRA adapters are not supported with quant='fp8'",
    "LoRA adapters are not supported with quant='int4'",
    "LoRA adapters are not supported with sub-layer pipeline cuts (DLLM_PP_FINE=1)",
    "LoRA adapters are not supported with sub-layer pipeline cuts",
    "LoRA adapters are not supported on a stage that pads its GQA group (7 -> 8 q heads per kv head)",
    "sub-layer cuts need a dense SwiGLU model",
    "sub-layer cuts are not combined with tensor parallelism",
    "sub-layer cuts are not combined with a padded GQA group (7 -> 8 q heads per kv head)",
]


def row_id(r):
    return ",".join(f"{k}={v}" for k, v in r.items() if v != DEFAULTS[k]) or "defaults"


def outcome(f):
    try:
        f()
    except Exception as e:          # noqa: BLE001 -- the type is part of the table
        return [type(e).__name__, str(e)]
    return None


def run_row(r):
    """{entry point: outcome} of the row."""
    saved = os.environ.get("DLLM_PP_FINE")
    os.environ["DLLM_PP_FINE"] = "1" if r["fine"] else "0"
    try:
        ecfg = EngineConfig(model=r["preset"], quant=r["quant"], device="cpu", dtype="float32",
                            enable_prefix_caching=r["prefix"], max_lora_rank=r["rank"],
                            lora_modules={"a": "synthetic:4:1"} if r["lora"] else {})
        cfg = get_model_config(r["preset"])
        out = {"validate": outcome(ecfg.validate),
               "check_tensor_parallel": outcome(lambda: ecfg.check_tensor_parallel(r["tp"])),
               "check_engine": outcome(lambda: lora.check_engine(ecfg, cfg))}
        built = []
        out["ModelStage"] = outcome(lambda: built.append(
            ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32, units=r["units"], unit_group=5 if r["units"] else 2,
                       tp=TPGroup(0, r["tp"]), pad_heads=r["pad"]).init_synthetic(0)))
        for name in ("quantize", "load_lora", "build_stage_lora"):
            out[name] = "-"
        if built:
            st = built[0]
            out["quantize"] = outcome(lambda: st.quantize(r["quant"]))
            out["load_lora"] = outcome(lambda: st.load_lora(ecfg))
            out["build_stage_lora"] = outcome(lambda: lora.build_stage_lora(st, ecfg))
        return out
    finally:
        if saved is None:
            del os.environ["DLLM_PP_FINE"]
        else:
            os.environ["DLLM_PP_FINE"] = saved


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


def test_table_covers_rows_and_messages(table):
    assert list(table) == [row_id(r) for r in ROWS] and len(set(table)) == len(ROWS)
    assert all(list(v) == ENTRY_POINTS for v in table.values())
    raised = [o for v in table.values() for o in v.values() if isinstance(o, list)]
    assert {t for t, _ in raised} == {"ValueError"}
    won = {m for _, m in raised}
    assert not [m for m in MESSAGES if m not in won]
    for name in ENTRY_POINTS:        # every entry point both passes and refuses somewhere
        col = [v[name] for v in table.values()]
        assert None in col and any(isinstance(o, list) for o in col), name


@pytest.mark.parametrize("r", ROWS, ids=row_id)
def test_entry_points_refuse_as_recorded(r, table):
    assert run_row(r) == table[row_id(r)]


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    with open(TABLE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(row_id(r))}: {json.dumps(run_row(r))}" for r in ROWS) + "\n}\n")
    print(len(ROWS), "rows,", os.path.getsize(TABLE), "bytes")
