"""Teacher-forced engine checks: every logits row an engine computes, prefill and decode, against the
cacheless forward of tests/model_reference.py.

The engine runs its own loop (greedy, ignore_eos) and nothing is forced into it.  ``record`` wraps the two
test-side seams -- ``scheduler.schedule`` / ``schedule_lookahead`` and ``runner.execute`` -- pairs every
executed HostBatch with its Step and files each logits row under (sequence, position of the row's last
input token).  Afterwards the reference is fed each sequence's ``prompt + output`` once and yields the
logits of all of its positions: the two sides see the same tokens by construction, so a bf16 near-tie can
not make them drift apart, and each row is judged on its own.

``compare`` then checks attribution (exact), coverage, the logit error against a bound and the tokens of
the rows that the reference decides clearly.  ``sharpen`` makes the synthetic models able to see attention
wiring errors at all: with N(0, 0.02) weights the q.k scores have a standard deviation of ~0.1, softmax is
almost uniform, and a wrong position or a lost key moves the logits no more than bf16 rounding does."""
import dataclasses
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

import model_reference as mr
from distributed_llms_amd.config import EngineConfig, get_model_config
from distributed_llms_amd.engine.llm_engine import LLMEngine
from distributed_llms_amd.engine.sequence import SamplingParams
from distributed_llms_amd.models import weights as W
from distributed_llms_amd.models.stage import ModelStage

# Sharpening factor per model, from a CPU sweep over 1, 1.5, 2, 3, 4 (profiles/teacher_forced_errors.md): the
# one at which the weakest mutant of tests/test_teacher_forced.py stands furthest above the model's rnd=_bf
# floor.  head_dim 128 and the q/k-normed heads saturate softmax (and lift the floor) sooner than head_dim 64
SHARPEN = {"tiny-llama": 4.0, "tiny-llama-d128": 3.0, "tiny-mixtral": 3.0, "tiny-qwen2-g7": 4.0,
           "tiny-qwen3-d128": 1.5}

MOE_MARGIN = 0.02        # a row may miss the error bound only with a routing margin below this ...
MOE_ROWS = 0.05          # ... and only this share of the rows (the rule of test_production_shapes_gpu.py)


@dataclasses.dataclass(frozen=True)
class Bound:
    max: float                              # per-row max |logit error| / reference spread
    mean: float                             # mean |logit error| / reference spread, over the rows within ``max``
    floor_ratio: Optional[float] = None     # dense models: mean error <= this x the rnd=_bf floor


# Bounds of the GPU (bf16) engines per model: 1.3 x the largest max / mean row error any scenario of
# tests/test_teacher_forced_gpu.py measured on an MI355X, table in profiles/teacher_forced_errors.md; the floor
# ratio of the dense models is the 1.35 of test_production_shapes_gpu.py (measured: the third figure).
# tiny-mixtral's max is taken over the rows with a routing margin >= MOE_MARGIN (the others may route
# differently from bf16 activations).  tests/test_teacher_forced.py rejects its mutants at these bounds.
GPU_BOUNDS: Dict[str, Bound] = {
    "tiny-llama": Bound(max=0.0639, mean=0.00969, floor_ratio=1.35),         # measured 0.0491 / 0.00746 / 1.12
    "tiny-llama-d128": Bound(max=0.1006, mean=0.01323, floor_ratio=1.35),    # measured 0.0774 / 0.01018 / 1.08
    "tiny-mixtral": Bound(max=0.0329, mean=0.00708),                         # measured 0.0253 / 0.00544
    "tiny-qwen2-g7": Bound(max=0.0526, mean=0.00786, floor_ratio=1.35),      # measured 0.0404 / 0.00605 / 1.11
    "tiny-qwen3-d128": Bound(max=0.0509, mean=0.00795, floor_ratio=1.35),    # measured 0.0391 / 0.00612 / 1.07
}


# ------------------------------------------------------------------ weights
def sharpen(sd: Dict[str, torch.Tensor], cfg, s: float, seed: int = 17) -> Dict[str, torch.Tensor]:
    """A copy of the HF-named ``sd`` whose attention is sharp: q and k each grow by ``s`` (scores by s^2).
    Models without a q/k norm: q_proj and k_proj (and their biases) are scaled.  ``qk_norm`` models
    normalise the heads, which undoes any scale of the projections, so there the q/k norm weights are scaled.
    ``attn_bias`` models also get qkv biases (and o_proj bias, where the model has one) of N(0, 0.1):
    comparable to the projections' outputs (std ~0.3), not the 0.01 / zero of the synthetic init."""
    out = dict(sd)
    g = torch.Generator().manual_seed(seed)
    for l in range(cfg.num_layers):
        a = f"model.layers.{l}.self_attn."
        if cfg.attn_bias:
            for n in ("q", "k", "v") + (("o",) if cfg.qk_norm else ()):
                k = a + f"{n}_proj.bias"
                out[k] = (0.1 * torch.randn(sd[k].shape, generator=g)).to(sd[k].dtype)
        if cfg.qk_norm:
            for n in ("q_norm", "k_norm"):
                out[a + n + ".weight"] = sd[a + n + ".weight"] * s
        else:
            for n in ("q_proj", "k_proj"):
                out[a + n + ".weight"] = sd[a + n + ".weight"] * s
                if cfg.attn_bias:
                    out[a + n + ".bias"] = out[a + n + ".bias"] * s
    return out


# Seed of the synthetic weights.  tiny-mixtral: of the seeds 5 .. 8, the one whose rnd=_bf reference alone has
# the fewest rows over the model's bound (2 of 213 on the buckets workload; seed 5 has 13, more than MOE_ROWS)
WEIGHT_SEED = {"tiny-mixtral": 8}


def state_dict(name: str, s: float, seed: Optional[int] = None):
    cfg = get_model_config(name)
    seed = WEIGHT_SEED.get(name, 5) if seed is None else seed
    return cfg, sharpen(W.synth_hf_state_dict(cfg, seed=seed, dtype=torch.float32), cfg, s)


def make_engine(name: str, sd, device: str, dtype: str = None, **kw) -> LLMEngine:
    """An engine over the state dict ``sd``: KV block 32, max_seq_len 512, batch 8 unless ``kw`` says otherwise."""
    cfg = get_model_config(name)
    dtype = dtype or ("bfloat16" if device == "cuda" else "float32")
    ec = dict(model=name, dtype=dtype, device=device, max_batch=8, max_seq_len=512, kv_block_size=32,
              num_kv_blocks=256, graph_batch_sizes=(1, 2, 4, 8), use_graphs=device == "cuda")
    lookahead = kw.pop("lookahead", None)
    ec.update(kw)
    tdt = {"bfloat16": torch.bfloat16, "float32": torch.float32}[dtype]
    eng = LLMEngine(EngineConfig(**ec), ModelStage(cfg, 0, cfg.num_layers, device, tdt).load_hf_state(sd))
    if lookahead is not None:
        eng.lookahead = bool(lookahead) and device == "cuda"
    return eng


def prompts_of(lens, vocab: int, seed: int = 3) -> List[List[int]]:
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(3, vocab, (n,), generator=g).tolist() for n in lens]


def greedy(n: int) -> SamplingParams:
    return SamplingParams(max_new_tokens=n, ignore_eos=True)


# ------------------------------------------------------------------ recording
@dataclasses.dataclass
class Record:
    seq: object          # the engine's Sequence
    pos: int             # position of the row's last input token
    logits: torch.Tensor  # [V] float32, CPU (after Recorder.finish)
    step: int            # index of the executed step
    kind: str            # "prefill", "decode", "lookahead", "mixed-decode", "mixed-prefill"


class Recorder:
    """See ``record``.  ``mutate(recorder, step, hb)`` (tests of the comparator) may edit the HostBatch
    before it runs."""

    def __init__(self, engine: LLMEngine, mutate: Optional[Callable] = None):
        self.engine = engine
        self.mutate = mutate
        self.pending = None
        self.steps = []                  # (kind, decode rows, seqs, positions, rows that count, logits clone)
        self.step_kinds: List[str] = []
        self.num_chunk_rows = 0          # rows of non-final prefill chunks (their logits mean nothing)
        self.last_rows: Dict[int, np.ndarray] = {}
        self.records: List[Record] = []
        sch, run = engine.scheduler, engine.runner
        self._schedule, self._lookahead, self._execute = sch.schedule, sch.schedule_lookahead, run.execute

        def schedule(*a, **kw):
            st = self._schedule(*a, **kw)
            if st is not None:
                self.pending = st
            return st

        def schedule_lookahead(*a, **kw):
            st = self._lookahead(*a, **kw)
            if st is not None:
                self.pending = st
            return st

        def execute(hb, *a, **kw):
            st, self.pending = self.pending, None
            assert st is not None, "a HostBatch was executed that no scheduled step stands behind"
            assert hb.slot == st.slot and hb.num_seqs == st.size, (hb.slot, st.slot, hb.num_seqs, st.size)
            seqs = list(st.decode_seqs) + list(st.seqs) if st.mixed else list(st.seqs)
            nd = st.num_decode if st.mixed else (0 if st.is_prefill else len(seqs))
            pos = np.array(hb.positions[hb.logits_idx] if hb.is_prefill else hb.positions, dtype=np.int64)
            if self.mutate is not None:
                self.mutate(self, st, hb)
            keep = np.array([i < nd or not s.chunk for i, s in enumerate(seqs)])
            if st.mixed:
                kind = "mixed"
            else:
                kind = "prefill" if st.is_prefill else ("lookahead" if st.keep is not None or kw.get("ids_dev") is not None
                                                        else "decode")
            if not st.is_prefill:
                rows = np.array(st.rows)
                if kw.get("ids_dev") is not None:
                    # lookahead: row i takes its input id from row keep[i] of the slot's step in flight
                    prev = self.last_rows[st.slot]
                    src = prev if st.keep is None else prev[np.asarray(st.keep)]
                    assert np.array_equal(src, rows), ("lookahead gather rows", src, rows)
                self.last_rows[st.slot] = rows
            else:
                self.last_rows.pop(st.slot, None)
            out = self._execute(hb, *a, **kw)
            assert out.shape[0] == len(seqs), (out.shape, len(seqs))
            # graph output is a static buffer: clone on the executing stream, before the next replay
            self.steps.append((kind, nd, seqs, pos, keep, out.detach().clone()))
            self.step_kinds.append(kind)
            return out

        sch.schedule, sch.schedule_lookahead, run.execute = schedule, schedule_lookahead, execute

    def kinds(self) -> List[str]:
        """The kind of every executed step, in order: "prefill", "decode", "lookahead" or "mixed"."""
        return list(self.step_kinds)

    def finish(self) -> List[Record]:
        sch, run = self.engine.scheduler, self.engine.runner
        sch.schedule, sch.schedule_lookahead, run.execute = self._schedule, self._lookahead, self._execute
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        for n, (kind, nd, seqs, pos, keep, logits) in enumerate(self.steps):
            lg = logits.float().cpu()
            for i, s in enumerate(seqs):
                if not keep[i]:
                    self.num_chunk_rows += 1
                    continue
                k = kind if kind != "mixed" else ("mixed-decode" if i < nd else "mixed-prefill")
                self.records.append(Record(s, int(pos[i]), lg[i], n, k))
        self.steps = []
        return self.records


def record(engine: LLMEngine, mutate: Optional[Callable] = None) -> Recorder:
    """Wrap ``engine.runner.execute`` and ``scheduler.schedule`` / ``schedule_lookahead`` (instance
    attributes; ``finish`` takes them off again).  Run the engine, then ``finish()`` -> the records."""
    return Recorder(engine, mutate)


# ------------------------------------------------------------------ reference
def reference(cfg, sd, seqs, rnd_weights=None, rnd=None, dtype=torch.float32):
    """{seq_id: (logits [T, V], routing margin [T])} of each sequence's ``prompt + output``, one forward
    each.  ``rnd_weights=_bf``: the weights a bf16 engine holds; ``rnd=_bf``: bf16 activations too."""
    w = mr.weights_from_hf(cfg, sd, dtype, rnd=rnd_weights)
    cs = mr.rope_table(cfg, dtype)
    out = {}
    for s in seqs:
        toks = torch.tensor([list(s.prompt) + list(s.output)], dtype=torch.long)
        lg, mg = mr.forward_all(cfg, w, toks, cs, rnd=rnd)
        out[s.seq_id] = (lg[0].float(), mg[0].float())
    return out


def _first_argmax(x: torch.Tensor) -> torch.Tensor:
    """arg-max per row, the first index on ties."""
    return (x == x.max(dim=-1, keepdim=True).values).float().argmax(dim=-1)


def gather(records: List[Record], ref):
    want = torch.stack([ref[r.seq.seq_id][0][r.pos] for r in records])
    margin = torch.stack([ref[r.seq.seq_id][1][r.pos] for r in records])
    return want, margin


def row_errors(got: torch.Tensor, want: torch.Tensor):
    """(per-row max |error| / spread, per-row mean |error| / spread, spread): the spread is the standard
    deviation of all reference logits compared."""
    spread = want.std().item()
    err = (got - want).abs()
    return err.max(dim=-1).values / spread, err.mean(dim=-1) / spread, spread


def check_attribution_and_coverage(records: List[Record], seqs, repeats: bool = False):
    """Exact: every row's arg-max (first index on ties) is the token its sequence received at the next
    position; every sequence has one record for its last prompt position and one per generated token
    (``repeats``: a position recomputed after a preemption may have two)."""
    by_seq: Dict[int, List[Record]] = {s.seq_id: [] for s in seqs}
    for r in records:
        assert r.seq.seq_id in by_seq, ("a row of a sequence nobody asked about", r.seq.seq_id)
        by_seq[r.seq.seq_id].append(r)
    for s in seqs:
        toks = list(s.prompt) + list(s.output)
        lo, hi = len(s.prompt) - 1, len(toks) - 2
        count = {p: 0 for p in range(lo, hi + 1)}
        for r in by_seq[s.seq_id]:
            assert r.pos in count, ("row outside the sequence's generated range", s.seq_id, r.pos, lo, hi, r.kind)
            count[r.pos] += 1
            tok = int(_first_argmax(r.logits[None])[0])
            assert tok == toks[r.pos + 1], ("row's arg-max is not the token the sequence received", s.seq_id, r.pos,
                                            r.kind, r.step, tok, toks[r.pos + 1])
        allowed = (1, 2) if repeats else (1,)
        bad = {p: c for p, c in count.items() if c not in allowed}
        assert not bad, ("positions without exactly one record", s.seq_id, len(s.prompt), bad)


def compare(records: List[Record], ref, bound: Bound, seqs=None, moe: bool = False, repeats: bool = False,
            floor=None, what: str = "") -> dict:
    """The four checks of the module docstring; returns the achieved figures (printed before any assertion
    on them).  ``floor``: the rnd=_bf reference of the same sequences, for ``bound.floor_ratio``."""
    seqs = seqs if seqs is not None else list({r.seq.seq_id: r.seq for r in records}.values())
    check_attribution_and_coverage(records, seqs, repeats)
    got = torch.stack([r.logits for r in records])
    want, margin = gather(records, ref)
    row_max, row_mean, spread = row_errors(got, want)
    bad = row_max > bound.max
    ok_mean = row_mean[~bad].mean().item() if bool((~bad).any()) else 0.0
    stats = {"what": what, "rows": len(records), "spread": spread, "max": row_max.max().item(),
             "mean": row_mean.mean().item(), "mean_within": ok_mean, "over": int(bad.sum())}
    if moe:       # what the bound is derived from: the rows that must meet it whatever their number
        stats["max_clear"] = row_max[margin >= MOE_MARGIN].max().item()
        stats["clear_rows"] = int((margin >= MOE_MARGIN).sum())
        # rows a bound of 1.3 x max_clear (how GPU_BOUNDS is derived) would have to excuse
        stats["over_1.3x_max_clear"] = int((row_max > 1.3 * stats["max_clear"]).sum())
    if floor is not None:
        fl = gather(records, floor)[0]
        f_max, f_mean, _ = row_errors(fl, want)
        f_bad = f_max > bound.max
        if moe:
            stats["floor_over_1.3x_max_clear"] = int((f_max > 1.3 * stats["max_clear"]).sum())
        stats.update(floor_max=f_max.max().item(), floor_mean=f_mean.mean().item(), floor_over=int(f_bad.sum()),
                     ratio=row_mean.mean().item() / f_mean.mean().item())
    worst = int(row_max.argmax())
    print(f"{what}: {stats}; worst row: seq prompt {len(records[worst].seq.prompt)} pos {records[worst].pos} "
          f"{records[worst].kind}", flush=True)
    if moe:
        assert bool((margin[bad] < MOE_MARGIN).all()), (what, "rows off with a clear routing decision",
                                                        row_max[bad].tolist(), margin[bad].tolist())
        assert int(bad.sum()) <= MOE_ROWS * len(records), (what, int(bad.sum()), len(records))
    else:
        assert not bool(bad.any()), (what, "rows over the bound", bound.max,
                                     [(len(records[i].seq.prompt), records[i].pos, records[i].kind,
                                       round(row_max[i].item(), 4)) for i in bad.nonzero().flatten().tolist()][:8])
    assert ok_mean <= bound.mean, (what, "mean error", ok_mean, bound.mean)
    if bound.floor_ratio is not None and floor is not None and not moe:
        assert stats["ratio"] <= bound.floor_ratio, (what, "mean error over the bf16 floor", stats["ratio"])
    top2 = want.topk(2, dim=-1).values
    decided = ((top2[:, 0] - top2[:, 1]) > 2 * row_max * spread) & ~bad
    agree = _first_argmax(got) == want.argmax(-1)
    stats["decided"] = int(decided.sum())
    assert bool(agree[decided].all()), (what, "clearly decided rows with another token", int((~agree[decided]).sum()))
    return stats


# ------------------------------------------------------------------ mutants (tests of the comparator)
MUTANTS = ("position", "lost_key", "wrong_block", "stale_id", "shared_slot", "slot_zero")


def mutant(kind: str, row_len: int, other_len: Optional[int] = None, at: int = 1) -> Callable:
    """A ``mutate`` callback for ``record``: the wiring error ``kind`` on the decode row of the sequence
    whose prompt has ``row_len`` tokens (``other_len``: the row it borrows a block or a slot from).
      position     RoPE / cache position + 1, every decode step
      lost_key     seq_lens - 1 (the newest key is not attended to), every decode step
      wrong_block  the row's second block-table entry is the other row's, every decode step
      stale_id     the previous step's input id once more, at the row's ``at``-th decode step only
      shared_slot  the row appends its K/V to the other row's slot, at that step only
      slot_zero    the row appends its K/V to the scratch slot 0, at that step only"""
    assert kind in MUTANTS, kind
    state = {"n": 0, "prev": None, "hits": 0}

    def find(seqs, n):
        return next((i for i, s in enumerate(seqs) if len(s.prompt) == n), None)

    def mutate(rec, st, hb):
        if st.is_prefill:
            return
        i = find(st.seqs, row_len)
        if i is None:
            return
        j = find(st.seqs, other_len) if other_len is not None else None
        n, prev = state["n"], state["prev"]
        state["n"], state["prev"] = n + 1, int(hb.ids[i])
        if kind == "position":
            hb.positions = hb.positions.copy()
            hb.positions[i] += 1
        elif kind == "lost_key":
            hb.seq_lens = hb.seq_lens.copy()
            hb.seq_lens[i] -= 1
        elif kind == "wrong_block" and j is not None:
            hb.block_tables = hb.block_tables.copy()
            hb.block_tables[i, 1] = hb.block_tables[j, 1]
        elif kind == "stale_id" and n >= at and state["hits"] == 0 and prev is not None and prev != int(hb.ids[i]):
            hb.ids = hb.ids.copy()
            hb.ids[i] = prev
        elif kind in ("shared_slot", "slot_zero") and n == at and (j is not None or kind == "slot_zero"):
            hb.slots = hb.slots.copy()
            hb.slots[i] = 0 if kind == "slot_zero" else hb.slots[j]
        else:
            return
        state["hits"] += 1

    mutate.state = state
    return mutate


# ------------------------------------------------------------------ scenarios (CPU fp32 and GPU bf16 run the same ones)
BUCKET_LENS = [1, 3, 31, 32, 33, 250]
BUCKET_NEW = [40, 70, 5, 66, 2, 30]


def _drive(eng, mutate, waves):
    """``waves``: [(engine step at which they arrive, [(prompt, max_new_tokens), ...])].  Runs the engine's
    own loop under ``record``; -> (sequences in arrival order, the finished Recorder)."""
    rec = record(eng, mutate)
    waves = sorted(waves, key=lambda w: w[0])
    seqs, step = [], 0
    while waves or eng.has_work():
        while waves and waves[0][0] <= step:
            seqs += [eng.add_request(p, greedy(n)) for p, n in waves.pop(0)[1]]
        eng.step()
        step += 1
    rec.finish()
    return seqs, rec


def run_buckets(name, sd, device, mutate=None, lens=BUCKET_LENS, new=BUCKET_NEW, **kw):
    """Six prompts of 1 .. 250 tokens: the decode batch shrinks 6 -> 1 through the padded graph buckets
    (6 and 5 rows in 8, 3 in 4), contexts cross the 32 / 64 / 96 block edges and the 256 context bucket."""
    eng = make_engine(name, sd, device, **kw)
    seqs, rec = _drive(eng, mutate, [(0, list(zip(prompts_of(lens, eng.mcfg.vocab_size), new)))])
    return eng, seqs, rec


def run_chunked(name, sd, device, **kw):
    """A 300-token prompt prefilled in chunks of at most 64 tokens next to two short ones, then decode."""
    eng = make_engine(name, sd, device, max_prefill_tokens=64, **kw)
    seqs, rec = _drive(eng, None, [(0, [(p, 40) for p in prompts_of([300, 7, 40], eng.mcfg.vocab_size, seed=4)])])
    return eng, seqs, rec


def run_mixed(name, sd, device, **kw):
    """The arrival waves of test_mixed_prefill_decode_steps_gpu: 14 prompts of 8 .. 60 tokens in four
    waves, the later ones riding along with the running decode rows."""
    eng = make_engine(name, sd, device, max_batch=16, mixed_prefill_tokens=64, graph_batch_sizes=(4, 8, 16), **kw)
    rng = np.random.default_rng(5)
    prompts = [rng.integers(3, 500, size=int(rng.integers(8, 60))).tolist() for _ in range(14)]
    waves, i = [], 0
    for at, n in [(0, 4), (3, 4), (6, 3), (10, 3)]:
        waves.append((at, [(p, 12) for p in prompts[i:i + n]]))
        i += n
    seqs, rec = _drive(eng, None, waves)
    return eng, seqs, rec


def run_preemption(name, sd, device, **kw):
    """The sizing of tests/test_sampler_seeded.py with blocks of 32: three usable blocks, two sequences that
    need two each once they pass 32 tokens -- the younger is preempted in decode and recomputed."""
    eng = make_engine(name, sd, device, num_kv_blocks=4, **kw)
    seqs, rec = _drive(eng, None, [(0, [(p, 30) for p in prompts_of([20, 25], eng.mcfg.vocab_size, seed=6)])])
    return eng, seqs, rec


def run_prefix(name, sd, device, **kw):
    """Four requests sharing a 96-token header (three full blocks), tails of 5 .. 40 tokens, in two waves:
    the second arrives during decode and prefills only its tail."""
    eng = make_engine(name, sd, device, enable_prefix_caching=True, **kw)
    v = eng.mcfg.vocab_size
    head = prompts_of([96], v, seed=7)[0]
    tails = prompts_of([5, 17, 40, 23], v, seed=8)
    seqs, rec = _drive(eng, None, [(0, [(head + t, 20) for t in tails[:2]]), (6, [(head + t, 20) for t in tails[2:]])])
    return eng, seqs, rec


def judge(cfg, sd, seqs, rec, bound: Bound, what: str, bf16: bool, repeats: bool = False) -> dict:
    """``compare`` against the reference of the weights the engine holds (``bf16``: rounded to bf16, with
    the rnd=_bf floor next to it)."""
    rw = mr._bf if bf16 else None
    ref = reference(cfg, sd, seqs, rnd_weights=rw)
    floor = reference(cfg, sd, seqs, rnd_weights=rw, rnd=mr._bf) if bf16 else None
    return compare(rec.records, ref, bound, seqs, moe=cfg.is_moe, repeats=repeats, floor=floor, what=what)
