"""Every logits row the GPU engine computes -- prefill, chunk, mixed, decode, lookahead, recompute -- against
the cacheless fp32 forward of tests/model_reference.py, through the harness of tests/teacher_forced.py
(gfx950 only).

All engines: bf16, KV block 32, max_seq_len 512, weights sharpened by teacher_forced.SHARPEN.  The bounds
are teacher_forced.GPU_BOUNDS, 1.3 x what an MI355X measured (profiles/teacher_forced_errors.md); every
scenario also asserts that the path it is named for ran.

What runs what
  buckets       decode graphs of the batch buckets 8 / 4 / 2 / 1 (6 and 5 rows padded into 8, 3 into 4: padded
                rows write scratch slot 0) and of the context buckets 256 and 512 (max_ctx of the split plan);
                graphs off: the same steps eager; lookahead on: the on-device id gather
  families      Mixtral MoE, a padded GQA group of 7, Qwen3 q/k norm + biases at head_dim 128
  chunked       a 300-token prompt in 64-token chunks (prefill over cached context), then decode
  mixed         prefill chunks riding along with decode rows
  preemption    recompute of prompt + drawn tokens after the KV pool ran out
  prefix cache  tail prefill over shared blocks, decode on them
  two slots     two microbatch slots with a graph set each"""
import pytest

import teacher_forced as tf

pytestmark = pytest.mark.gpu

_SD = {}


def _sd(name):
    if name not in _SD:
        _SD[name] = tf.state_dict(name, tf.SHARPEN[name])
    return _SD[name]


def _judge(name, seqs, rec, what, repeats=False):
    cfg, sd = _sd(name)
    return tf.judge(cfg, sd, seqs, rec, tf.GPU_BOUNDS[name], f"{name} {what}", bf16=True, repeats=repeats)


def _buckets(name, graphs, lookahead, streams=1):
    cfg, sd = _sd(name)
    eng, seqs, rec = tf.run_buckets(name, sd, "cuda", use_graphs=graphs, lookahead=lookahead, streams=streams)
    assert [len(s.output) for s in seqs] == tf.BUCKET_NEW
    kinds = rec.kinds()
    if lookahead:
        assert eng.num_lookahead > 0 and "lookahead" in kinds, "lookahead path never taken"
    else:
        assert eng.num_lookahead == 0 and "lookahead" not in kinds
    return eng, seqs, rec


@pytest.mark.parametrize("lookahead", [False, True], ids=["sync", "lookahead"])
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("name", ["tiny-llama", "tiny-llama-d128"])
def test_buckets(cuda, name, graphs, lookahead):
    eng, seqs, rec = _buckets(name, graphs, lookahead)
    if graphs:
        keys = set(eng.runner.graphs.num_replays)
        assert {k[0] for k in keys} >= {8, 4, 2, 1}, keys
        assert len({k[1] for k in keys}) >= 2, keys
    else:
        assert eng.runner.graphs is None
    _judge(name, seqs, rec, f"buckets graphs={graphs} lookahead={lookahead}")


@pytest.mark.parametrize("name", ["tiny-mixtral", "tiny-qwen2-g7", "tiny-qwen3-d128"])
def test_families(cuda, name):
    eng, seqs, rec = _buckets(name, True, True)
    assert eng.runner.graphs.num_replays
    if name == "tiny-qwen2-g7":
        assert eng.stage.group == 8 and eng.stage.group_real == 7, "the GQA group was not padded"
    _judge(name, seqs, rec, "families")


def test_chunked_prefill_then_decode(cuda):
    name = "tiny-llama"
    eng, seqs, rec = tf.run_chunked(name, _sd(name)[1], "cuda")
    assert rec.num_chunk_rows > 1, "the long prompt was not prefilled in chunks"
    assert all(len(s.output) == 40 for s in seqs)
    _judge(name, seqs, rec, "chunked")


def test_mixed_steps(cuda):
    name = "tiny-llama-d128"
    eng, seqs, rec = tf.run_mixed(name, _sd(name)[1], "cuda")
    assert eng.scheduler.num_mixed > 0 and "mixed" in rec.kinds()
    assert len(seqs) == 14 and all(len(s.output) == 12 for s in seqs)
    _judge(name, seqs, rec, "mixed")


def test_preemption_recompute(cuda):
    name = "tiny-llama"
    eng, seqs, rec = tf.run_preemption(name, _sd(name)[1], "cuda")
    assert eng.scheduler.num_preemptions >= 1
    assert all(len(s.output) == 30 for s in seqs)
    _judge(name, seqs, rec, "preemption", repeats=True)


def test_prefix_cache(cuda):
    name = "tiny-llama"
    eng, seqs, rec = tf.run_prefix(name, _sd(name)[1], "cuda")
    stats = eng.scheduler.prefix_stats()
    assert stats["hit_tokens"] >= 96, stats
    assert all(len(s.output) == 20 for s in seqs)
    _judge(name, seqs, rec, "prefix cache")


def test_two_microbatch_slots(cuda):
    name = "tiny-llama"
    eng, seqs, rec = _buckets(name, True, True, streams=2)
    assert eng.num_slots == 2 and len(eng.runner.graph_sets) == 2
    assert all(g.num_replays for g in eng.runner.graph_sets), "a slot never replayed a graph"
    _judge(name, seqs, rec, "two slots")
