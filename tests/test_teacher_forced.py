"""The teacher-forced harness (tests/teacher_forced.py) and its reference (tests/model_reference.py), on the CPU.

* The cacheless reference agrees with the CPU float32 engine -- itself pinned token for token to
  ``transformers`` -- to 1e-4 on every row of the bucket workload, for each sharpened tiny model the GPU
  scenarios use; the harness passes that engine, and the other scenarios' CPU runs, at a tight bound.
* The comparator rejects wiring mutants AT THE GPU BOUNDS (teacher_forced.GPU_BOUNDS, what
  tests/test_teacher_forced_gpu.py asserts): each mutant, applied to the HostBatch of a CPU float32 engine,
  exceeds 1.5 x the model's bound on at least one row (for the MoE model: a row with a clear routing margin,
  which no exception covers), and ``compare`` refuses the run.
* The MoE model's rnd=_bf reference alone stays inside the MoE exception at the GPU bound.

Measured mutant errors per model: profiles/teacher_forced_errors.md."""
import pytest
import torch

import model_reference as mr
import teacher_forced as tf

MODELS = list(tf.SHARPEN)
TIGHT = tf.Bound(max=1e-3, mean=1e-4)        # float32 against float32: measured 5e-6 / 1e-6 x spread
MUT_LENS = [1, 3, 31, 32, 250]               # the mutants' workload: 16 decode steps of five rows
MUT_NEW = 16
# (mutant, the row it strikes by prompt length, the row it borrows from): each on the row where its class shows
# most -- a context of 1 - 3 for the lost key and the position, a row that has just crossed a block edge (32 ->
# 33 tokens) reading the second block of the 250-token row
CASES = [("position", 3, None), ("lost_key", 1, None), ("wrong_block", 32, 250), ("stale_id", 3, None),
         ("shared_slot", 3, 31), ("slot_zero", 3, None)]
_CACHE = {}


def _sd(name):
    if ("sd", name) not in _CACHE:
        _CACHE["sd", name] = tf.state_dict(name, tf.SHARPEN[name])
    return _CACHE["sd", name]


def _clean(name):
    """The bucket workload on the CPU float32 engine, once per model."""
    if ("run", name) not in _CACHE:
        cfg, sd = _sd(name)
        _, seqs, rec = tf.run_buckets(name, sd, "cpu")
        _CACHE["run", name] = (seqs, rec, tf.reference(cfg, sd, seqs))
    return _CACHE["run", name]


@pytest.mark.parametrize("name", MODELS)
def test_reference_matches_the_cpu_float32_engine(name):
    seqs, rec, ref = _clean(name)
    assert [len(s.output) for s in seqs] == tf.BUCKET_NEW
    got = torch.stack([r.logits for r in rec.records])
    want, _ = tf.gather(rec.records, ref)
    assert len(rec.records) == sum(tf.BUCKET_NEW)
    err = (got - want).abs().max().item()
    print(f"{name}: {len(rec.records)} rows, max |logit error| {err:.2e}")
    assert err <= 1e-4, err


@pytest.mark.parametrize("name", MODELS)
def test_harness_passes_the_cpu_engine(name):
    cfg, sd = _sd(name)
    seqs, rec, ref = _clean(name)
    st = tf.compare(rec.records, ref, TIGHT, seqs, moe=False, what=f"{name} buckets (cpu float32)")
    assert st["decided"] > 0.9 * st["rows"]          # the token check is not vacuous


@pytest.mark.parametrize("scenario", ["chunked", "mixed", "preemption", "prefix"])
def test_harness_passes_the_cpu_engine_on_every_scenario(scenario):
    """What the GPU scenarios run, on the CPU engine: chunk rows are left out, mixed steps file their decode and
    prefill rows, a recompute after preemption lands on its position, a prefix hit prefills the tail only."""
    name = "tiny-llama-d128" if scenario == "mixed" else "tiny-llama"
    cfg, sd = _sd(name)
    eng, seqs, rec = getattr(tf, "run_" + scenario)(name, sd, "cpu")
    if scenario == "chunked":
        assert rec.num_chunk_rows > 1
    if scenario == "mixed":
        assert eng.scheduler.num_mixed > 0 and "mixed" in rec.kinds()
    if scenario == "preemption":
        assert eng.scheduler.num_preemptions >= 1
    if scenario == "prefix":
        assert eng.scheduler.prefix_stats()["hit_tokens"] >= 96
    tf.judge(cfg, sd, seqs, rec, TIGHT, f"{name} {scenario} (cpu float32)", bf16=False, repeats=scenario == "preemption")


def _mutant_run(name, kind, row, other):
    cfg, sd = _sd(name)
    m = tf.mutant(kind, row, other)
    _, seqs, rec = tf.run_buckets(name, sd, "cpu", mutate=m, lens=MUT_LENS, new=[MUT_NEW] * len(MUT_LENS))
    ref = tf.reference(cfg, sd, seqs)
    want, margin = tf.gather(rec.records, ref)
    row_max, _, _ = tf.row_errors(torch.stack([r.logits for r in rec.records]), want)
    return m, seqs, rec, ref, row_max, margin


@pytest.mark.parametrize("kind,row,other", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("name", MODELS)
def test_comparator_rejects_mutant_at_the_gpu_bound(name, kind, row, other):
    cfg, _ = _sd(name)
    bound = tf.GPU_BOUNDS[name]
    m, seqs, rec, ref, row_max, margin = _mutant_run(name, kind, row, other)
    assert m.state["hits"] > 0, "the mutant never struck"
    counts = row_max[margin >= tf.MOE_MARGIN] if cfg.is_moe else row_max      # rows no MoE exception covers
    print(f"{name} {kind}: max row error {row_max.max().item():.4f} x spread, on rows that count "
          f"{counts.max().item():.4f}; GPU bound {bound.max} (x 1.5 = {1.5 * bound.max:.4f})")
    assert counts.max().item() >= 1.5 * bound.max, (kind, counts.max().item(), bound.max)
    with pytest.raises(AssertionError):
        tf.compare(rec.records, ref, bound, seqs, moe=cfg.is_moe, what=f"{name} {kind}")


@pytest.mark.parametrize("name", MODELS)
def test_lost_key_at_a_long_context_is_reported(name):
    """seq_lens - 1 on the 250-token row: one key of 250.  Printed for the table only -- it sits near the bf16
    floor for most models, and the kernel needle tests own it."""
    m, _, _, _, row_max, _ = _mutant_run(name, "lost_key", 250, None)
    assert m.state["hits"] == MUT_NEW - 1
    print(f"{name} lost_key at 250 tokens: max row error {row_max.max().item():.4f} x spread; GPU bound "
          f"{tf.GPU_BOUNDS[name].max}")


def test_moe_bf16_reference_alone_stays_inside_the_moe_exception():
    """rnd=_bf against fp32 at the GPU bound: the rows over it all have a routing margin below MOE_MARGIN and
    are at most MOE_ROWS of the rows -- the seed (teacher_forced.WEIGHT_SEED) is chosen for that."""
    name = "tiny-mixtral"
    cfg, sd = _sd(name)
    seqs, rec, _ = _clean(name)
    ref = tf.reference(cfg, sd, seqs, rnd_weights=mr._bf)
    floor = tf.reference(cfg, sd, seqs, rnd_weights=mr._bf, rnd=mr._bf)
    want, margin = tf.gather(rec.records, ref)
    row_max, _, _ = tf.row_errors(tf.gather(rec.records, floor)[0], want)
    bad = row_max > tf.GPU_BOUNDS[name].max
    print(f"{name}: rnd=_bf rows over {tf.GPU_BOUNDS[name].max}: {int(bad.sum())} of {len(bad)}, margins "
          f"{[round(float(x), 4) for x in margin[bad].tolist()]}")
    assert bool((margin[bad] < tf.MOE_MARGIN).all())
    assert int(bad.sum()) <= tf.MOE_ROWS * len(bad)


def test_sharpen_changes_what_it_says():
    for name in ("tiny-llama", "tiny-qwen2-g7", "tiny-qwen3-d128"):
        cfg = tf.get_model_config(name)
        base = tf.W.synth_hf_state_dict(cfg, seed=5, dtype=torch.float32)
        sd = tf.sharpen(base, cfg, 4.0)
        a = "model.layers.1.self_attn."
        changed = {k for k in sd if not torch.equal(sd[k], base[k])}
        if cfg.qk_norm:
            assert torch.equal(sd[a + "q_norm.weight"], base[a + "q_norm.weight"] * 4)
            assert torch.equal(sd[a + "q_proj.weight"], base[a + "q_proj.weight"])
        else:
            assert torch.equal(sd[a + "k_proj.weight"], base[a + "k_proj.weight"] * 4)
        if cfg.attn_bias:
            assert all(float(sd[a + f"{n}_proj.bias"].abs().max()) > 0.05 for n in "qkv")
        assert all(".self_attn." in k and "v_proj.weight" not in k and "o_proj.weight" not in k for k in changed)


@pytest.mark.parametrize("name", ["tiny-llama", "llama3-8b", "mixtral-8x7b"])
def test_rope_table_of_the_reference(name):
    """The reference's own table (Llama-3 rescaling from the published formula) against the engine's."""
    from distributed_llms_amd.ops import reference as ref
    cfg = tf.get_model_config(name)
    mine = mr.rope_table(cfg)
    torch.testing.assert_close(mine, ref.rope_cos_sin(cfg.head_dim, cfg.max_position, cfg.rope_theta, cfg.rope_scaling),
                               atol=1e-6, rtol=0)
    if cfg.rope_scaling:       # the rescaling does something: the unscaled table differs
        plain = mr.rope_table(tf.dataclasses.replace(cfg, rope_scaling=None))
        assert (mine - plain).abs().max() > 0.1
