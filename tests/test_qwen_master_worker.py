"""Master + two ``run_worker.py`` processes on CPU serve a Qwen3 synthetic model and a Qwen2 HF checkpoint
directory: the shard manager splits the directory, every worker loads its shard (bias and norm tensors
included), and the pipeline decodes what the single engine decodes."""
import pytest
import torch

from distributed_llms_amd.checkpoint.shard_manager import iter_checkpoint, write_synthetic_checkpoint
from distributed_llms_amd.config import get_model_config
from distributed_llms_amd.engine.llm_engine import LLMEngine
from distributed_llms_amd.engine.sequence import SamplingParams
from distributed_llms_amd.models.stage import ModelStage
from test_master_worker import PROMPTS, _cfg, cluster  # noqa: F401  (the fixture)

pytestmark = pytest.mark.slow


def test_synthetic_qwen3_two_workers(cluster):  # noqa: F811
    make, _ = cluster
    model = "synthetic:tiny-qwen3"
    m = make(model, 2)
    m.assign_shards()
    m.distribute_shards(timeout=300)
    res = m.generate(PROMPTS, max_new_tokens=6, ignore_eos=True, timeout=120)
    ref = LLMEngine(_cfg(model)).generate(PROMPTS, SamplingParams(max_new_tokens=6, ignore_eos=True))
    assert [r["tokens"] for r in res] == ref


def test_qwen2_checkpoint_directory_two_workers(cluster, tmp_path):  # noqa: F811
    d = write_synthetic_checkpoint("tiny-qwen2", str(tmp_path / "ckpt"), seed=7)
    make, _ = cluster
    m = make(d, 2)
    m.assign_shards()
    m.distribute_shards(timeout=300)
    res = m.generate(PROMPTS, max_new_tokens=5, ignore_eos=True, timeout=120)
    cfg = get_model_config(d)
    assert cfg.attn_bias and not cfg.qk_norm
    st = ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32).load_hf_state(dict(iter_checkpoint(d)))
    ref = LLMEngine(_cfg(d), st).generate(PROMPTS, SamplingParams(max_new_tokens=5, ignore_eos=True))
    assert [r["tokens"] for r in res] == ref
