"""Per-token log-probabilities on the CPU: the reference contract, the HostBatch wire section, the
ids message, the engine's bookkeeping and the public interfaces."""
import math

import numpy as np
import pytest
import torch

import logprobs_cases as lc
from distributed_llms_amd import ops
from distributed_llms_amd.ops import reference as ref

NINF = float("-inf")


# ------------------------------------------------------------------ the reference contract
def test_reference_matches_torch_log_softmax():
    g = torch.Generator().manual_seed(11)
    for spread in (3.0, 10.0):
        logits = (torch.randn(6, 1531, generator=g) * spread).to(torch.bfloat16)
        ids = torch.randint(0, 1531, (6,), generator=g, dtype=torch.int32)
        want = torch.full((6,), 7, dtype=torch.int32)
        c, ti, tl = ref.token_logprobs_detail(logits.double().numpy(), ids.numpy(), want.numpy(), 7)
        lsm = torch.log_softmax(logits.double(), -1)
        assert np.allclose(c, lsm[torch.arange(6), ids.long()].numpy(), rtol=0, atol=1e-12)
        vals, idx = torch.sort(logits.double(), dim=-1, descending=True, stable=True)
        assert np.array_equal(ti, idx[:, :7].to(torch.int32).numpy())
        assert np.allclose(tl, lsm.gather(1, idx[:, :7]).numpy(), rtol=0, atol=1e-12)


def test_reference_order_ties_and_filler():
    x = torch.tensor([[1.0, 3.0, 3.0, -0.0, 0.0, 3.0, 2.0, NINF]])
    c, ti, tl = ref.token_logprobs(x, torch.tensor([6], dtype=torch.int32), torch.tensor([5], dtype=torch.int32), 8)
    assert ti[0].tolist() == [1, 2, 5, 6, 0, -1, -1, -1]
    assert tl[0, 5:].tolist() == [0.0, 0.0, 0.0]
    assert tl[0, 0] == tl[0, 1] == tl[0, 2] and c[0] == tl[0, 3]
    # -0 equals +0: the smaller index first
    c, ti, tl = ref.token_logprobs(x, torch.tensor([3], dtype=torch.int32), torch.tensor([8], dtype=torch.int32), 8)
    assert ti[0].tolist() == [1, 2, 5, 6, 0, 3, 4, 7]
    assert tl[0, 7].item() == NINF and tl[0, 5] == tl[0, 6] == c[0]
    # more entries wanted than the row has
    c, ti, tl = ref.token_logprobs(x[:, :3], torch.tensor([0], dtype=torch.int32),
                                   torch.tensor([8], dtype=torch.int32), 8)
    assert ti[0].tolist() == [1, 2, 0, -1, -1, -1, -1, -1]


def test_reference_edge_rows():
    v = 777
    h = lc.hand_rows(v, torch.Generator().manual_seed(0))
    ids = torch.tensor([0, v - 1, 3, 0, 9, v - 1], dtype=torch.int32)
    want = torch.full((lc.NUM_HAND,), 4, dtype=torch.int32)
    c, ti, tl = ref.token_logprobs(h, ids, want, 4)
    # all -inf: every lp is -inf, the order is the index order
    assert c[0].item() == NINF and ti[0].tolist() == [0, 1, 2, 3] and (tl[0] == NINF).all()
    # one finite entry: probability 1
    assert c[1].item() == 0.0 and ti[1].tolist() == [v - 1, 0, 1, 2] and tl[1].tolist() == [0.0, NINF, NINF, NINF]
    # two +inf maxima: -ln 2 each, everything else -inf
    assert ti[2, :2].tolist() == [3, v // 2 + 1]
    assert tl[2, :2].tolist() == pytest.approx([-math.log(2)] * 2) and (tl[2, 2:] == NINF).all()
    assert c[2].item() == pytest.approx(-math.log(2))
    # NaN counts as -inf; -0 and +0 tie at the top, smaller index first
    assert c[3].item() == NINF and ti[3, :2].tolist() == [2, 5] and tl[3, 0] == tl[3, 1]
    # all equal: -ln V
    assert c[4].item() == pytest.approx(-math.log(v), rel=1e-6) and ti[4].tolist() == [0, 1, 2, 3]
    # out-of-range ids are not read; skipped rows hold the filler
    c, ti, tl = ref.token_logprobs(h[4:], torch.tensor([v, -1], dtype=torch.int32),
                                   torch.tensor([0, -1], dtype=torch.int32), 2)
    assert c.tolist() == [NINF, 0.0] and (ti == -1).all() and (tl == 0).all()


def test_ops_checks_and_cpu_route():
    case = lc.make_case(3, 777)
    got = ops.token_logprobs(case["logits"], case["ids"], case["want"], lc.N_MAX)
    for a, b in zip(got, lc.reference(case)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(ValueError):
        ops.token_logprobs(case["logits"], case["ids"], case["want"], 21)
    with pytest.raises(TypeError):
        ops.token_logprobs(case["logits"], case["ids"].long(), case["want"], 5)
    with pytest.raises(ValueError):
        ops.token_logprobs(case["logits"], case["ids"][:2], case["want"], 5)


# ------------------------------------------------------------------ HostBatch wire section
from distributed_llms_amd.config import EngineConfig  # noqa: E402
from distributed_llms_amd.engine.batch import HostBatch, build_host_batch, merge_mixed  # noqa: E402
from distributed_llms_amd.engine.llm_engine import LLMEngine, make_block_manager  # noqa: E402
from distributed_llms_amd.engine.sampler import (MAX_LOGPROBS, ids_message_len, pack_ids_message,  # noqa: E402
                                                 sample_step, unpack_ids_message)
from distributed_llms_amd.engine.scheduler import Scheduler, Step  # noqa: E402
from distributed_llms_amd.engine.sequence import SamplingParams, Sequence, validate_logprobs  # noqa: E402


def _hb(logprobs=None, b=3, mb=2, seeded=True):
    t = b
    samp = np.arange(3 * b, dtype=np.int32).reshape(b, 3) + 100 if seeded else None
    seeds = np.arange(2 * b, dtype=np.int32).reshape(b, 2) - 7 if seeded else None
    return HostBatch(False, np.arange(t, dtype=np.int32) + 1, np.arange(t, dtype=np.int32) + 10,
                     np.arange(t, dtype=np.int32) + 20, np.arange(b, dtype=np.int32) + 30,
                     np.arange(b + 1, dtype=np.int32), np.arange(b * mb, dtype=np.int32).reshape(b, mb) + 40,
                     np.arange(b, dtype=np.int32), 1, 33, slot=2, step_id=9, sampling=samp, sample_seeds=seeds,
                     logprobs=logprobs)


def _parent_format(hb):
    """The packed array as the format was before the logprobs section, built from the documented
    layout: [header(16) | ids | positions | slots | seq_lens | cu_seqlens | block_tables |
    logits_idx | sampling 3B (header word 8) | sample_seeds 2B (header word 10)]."""
    b, t = hb.seq_lens.shape[0], hb.ids.shape[0]
    hdr = [int(hb.is_prefill), t, b, hb.block_tables.shape[1], hb.max_q_len, hb.max_ctx, hb.slot, hb.step_id,
           int(hb.sampling is not None), hb.num_decode, int(hb.sample_seeds is not None), 0, 0, 0, 0, 0]
    parts = [hdr, hb.ids, hb.positions, hb.slots, hb.seq_lens, hb.cu_seqlens, hb.block_tables.reshape(-1),
             hb.logits_idx]
    if hb.sampling is not None:
        parts.append(hb.sampling.reshape(-1))
    if hb.sample_seeds is not None:
        parts.append(hb.sample_seeds.reshape(-1))
    return np.concatenate([np.asarray(p, dtype=np.int32) for p in parts])


@pytest.mark.parametrize("seeded", [True, False])
def test_host_batch_round_trip_with_and_without_the_section(seeded):
    plain = _hb(None, seeded=seeded)
    packed = plain.pack()
    assert packed.dtype == np.int32 and np.array_equal(packed, _parent_format(plain))
    assert HostBatch.unpack(packed).logprobs is None
    want = np.array([-1, 0, 5], dtype=np.int32)
    asking = _hb(want, seeded=seeded)
    p2 = asking.pack()
    assert p2[11] == 1 and p2.shape[0] == packed.shape[0] + 3
    assert np.array_equal(p2[-3:], want)
    rest = p2[:-3].copy()
    rest[11] = 0
    assert np.array_equal(rest, packed)                    # everything before the section is unchanged
    back = HostBatch.unpack(p2)
    assert back.logprobs.tolist() == [-1, 0, 5]
    assert (back.sample_seeds is None) == (not seeded)
    if seeded:
        assert np.array_equal(back.sample_seeds, asking.sample_seeds)
    assert np.array_equal(back.pack(), p2)


def test_build_host_batch_merge_mixed_and_native_decode_fill_the_field():
    bm = make_block_manager(64, 4)
    sch = Scheduler(bm, num_slots=1, max_batch=8, max_prefill_tokens=64, max_seq_len=64, mixed_prefill_tokens=16)
    plain = Sequence([1, 2, 3, 4, 5], SamplingParams(max_new_tokens=8, ignore_eos=True))
    sch.add(plain)
    st = sch.schedule(0)
    assert build_host_batch(st, bm, 4).logprobs is None
    sch.complete(st, [7])
    # a decode step of a slot in which nobody asked: no section, the parent's packed format
    st = sch.schedule(0)
    hb = build_host_batch(st, bm, 4)
    assert hb.logprobs is None and st.packed[11] == 0 and np.array_equal(st.packed, _parent_format(hb))
    sch.complete(st, [8])
    asking = Sequence([9, 8, 7], SamplingParams(max_new_tokens=8, ignore_eos=True, logprobs=4))
    zero = Sequence([6, 5], SamplingParams(max_new_tokens=8, ignore_eos=True, logprobs=0))
    sch.add(asking)
    sch.add(zero)
    st = sch.schedule(0)
    assert st.mixed
    hb = build_host_batch(st, bm, 4)                        # decode row did not ask: padded with -1
    assert hb.num_decode == 1 and hb.logprobs.tolist() == [-1, 4, 0]
    assert HostBatch.unpack(hb.pack()).logprobs.tolist() == [-1, 4, 0]
    lps = (np.array([0.0, -1.5, -2.5], np.float32), np.full((3, 4), 3, np.int32), np.full((3, 4), -4.0, np.float32))
    sch.complete(st, np.array([9, 10, 11], np.int32), 0.0, lps)
    assert plain.logprobs == [] and asking.logprobs == [(-1.5, [3] * 4, [-4.0] * 4)] and zero.logprobs == [(-2.5, [], [])]
    # now the native batcher's decode step carries the section (SlotBatcher.admit's num_logprobs)
    st = sch.schedule(0)
    hb = build_host_batch(st, bm, 4)
    assert not st.is_prefill and hb.logprobs.tolist() == [-1, 4, 0] and hb.sampling is None
    # the other way round: decode rows asked, the prefill rows did not
    pre = build_host_batch(Step(True, [Sequence([1, 2], SamplingParams())], 0), _bm_with(2), 4)
    assert merge_mixed(hb, pre, 0, 0).logprobs.tolist() == [-1, 4, 0, -1]


def _bm_with(n):
    class _Any:
        """A block manager stand-in for a one-off prefill batch: slot i, one block table row."""
        def fill_slots(self, seq_ids, starts, qlens, slots):
            slots[:] = np.arange(slots.shape[0])
            return slots.shape[0]

        def fill_block_tables(self, seq_ids, bt, pad):
            bt[:] = 0
    return _Any()


def test_sampling_params_field_and_validation():
    assert SamplingParams().logprobs is None
    p = SamplingParams.from_dict({"logprobs": 3, "temperature": 0.5, "junk": 1})
    assert p.logprobs == 3 and SamplingParams.from_dict(p.to_dict()) == p
    for ok in (None, 0, 1, 20):
        assert validate_logprobs(ok) == ok
    for bad in (21, -1, True, False, 2.0, "3"):
        with pytest.raises(ValueError):
            validate_logprobs(bad)
    assert MAX_LOGPROBS == ops.MAX_LOGPROBS == ref.MAX_LOGPROBS == 20


# ------------------------------------------------------------------ the ids message
@pytest.mark.parametrize("want", [None, [0, 0, 0], [-1, 0, -1], [-1, 5, 2], [20, -1, 1]])
def test_ids_message_len_and_round_trip(want):
    b, v = 3, 97
    hb = _hb(None if want is None else np.array(want, np.int32), seeded=False)
    n = 0 if want is None else max(0, max(want))
    assert ids_message_len(hb) == (b if want is None else b * (2 + 2 * n))
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(b, v, generator=g)
    ids, msg = sample_step(logits, hb)
    assert ids.tolist() == logits.argmax(-1).tolist()
    if want is None:
        assert msg is None
        got, lps = unpack_ids_message(ids.numpy(), hb)
        assert lps is None and got.tolist() == ids.tolist()
        return
    assert msg.dtype == torch.int32 and msg.shape[0] == ids_message_len(hb)
    got, (chosen, top_ids, top_lp) = unpack_ids_message(msg.numpy(), hb)
    ec, ei, el = ref.token_logprobs(logits, ids, torch.tensor(want, dtype=torch.int32), n)
    assert got.tolist() == ids.tolist() and top_ids.shape == top_lp.shape == (b, n)
    assert np.array_equal(chosen.view(np.int32), ec.numpy().view(np.int32))
    assert np.array_equal(top_ids, ei.numpy()) and np.array_equal(top_lp.view(np.int32), el.numpy().view(np.int32))
    for r, w in enumerate(want):                          # rows that did not ask hold the filler
        if w < 0:
            assert chosen[r] == 0 and (top_ids[r] == -1).all() and (top_lp[r] == 0).all()
    again = pack_ids_message(torch.from_numpy(got.copy()), torch.from_numpy(chosen.copy()),
                             torch.from_numpy(top_ids.copy()), torch.from_numpy(top_lp.copy()))
    assert torch.equal(again, msg)
    with pytest.raises(ValueError):
        unpack_ids_message(msg.numpy()[:-1], hb)


# ------------------------------------------------------------------ CPU engine
PROMPTS = [[1, 5, 9, 200], [3, 4, 7], list(range(10, 40)), [8] * 13]
LOGIT_TOL = dict(rtol=2e-4, atol=2e-4)      # test_pipeline.py's bound on fp32 logits of this model


def _engine(**kw):
    cfg = dict(model="synthetic:tiny-llama", device="cpu", dtype="float32", max_batch=8, max_seq_len=128,
               use_graphs=False, num_kv_blocks=128)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg))


def _params(logprobs, n=8, eos=False):
    """Greedy, seeded, greedy, seeded; ``logprobs``: one value per request."""
    kinds = [dict(), dict(temperature=0.9, top_k=50, top_p=0.95, seed=101), dict(),
             dict(temperature=1.3, seed=202)]
    return [SamplingParams(max_new_tokens=n, ignore_eos=not eos, logprobs=lp, **k) for k, lp in zip(kinds, logprobs)]


def _run(eng, prompts, params, eos_tokens=None):
    seqs = [eng.add_request(p, q) for p, q in zip(prompts, params)]
    for s, e in zip(seqs, eos_tokens or []):
        s.eos_token_id = e
    eng.run_until_done()
    return seqs


def _rerun_logits(tokens):
    """Logits at the last position of a plain prefill of ``tokens`` in a fresh engine."""
    eng = _engine()
    eng.add_request(tokens, SamplingParams(max_new_tokens=1))
    st = eng.scheduler.schedule(0)
    return eng.runner.execute(build_host_batch(st, eng.bm, eng.ecfg.kv_block_size)).float()


def _check_against_rerun(seq):
    n = seq.params.logprobs
    assert len(seq.logprobs) == len(seq.output)
    for t, (chosen, top_ids, top_lps) in enumerate(seq.logprobs):
        logits = _rerun_logits(seq.prompt + seq.output[:t])
        exp = ref.token_logprobs(logits, torch.tensor([seq.output[t]], dtype=torch.int32),
                                 torch.tensor([0], dtype=torch.int32), 0)[0]
        torch.testing.assert_close(torch.tensor([chosen]), exp, **LOGIT_TOL)
        assert len(top_ids) == len(top_lps) == n
        assert all(a >= b for a, b in zip(top_lps, top_lps[1:])) and len(set(top_ids)) == n
        if seq.output[t] in top_ids:
            assert top_lps[top_ids.index(seq.output[t])] == chosen
        elif n:
            assert chosen <= top_lps[-1]
        if seq.params.temperature <= 0 and n:
            assert top_ids[0] == seq.output[t]            # greedy: the chosen token is the most likely


@pytest.fixture(scope="module")
def plain_run():
    return [s.output for s in _run(_engine(), PROMPTS, _params([None] * 4))]


def test_engine_values_invariant_and_unchanged_ids(plain_run):
    seqs = _run(_engine(), PROMPTS, _params([5, 2, None, 0]))
    assert [s.output for s in seqs] == plain_run            # asking leaves the generated ids unchanged
    assert seqs[2].logprobs == [] and all(len(s.logprobs) == len(s.output) == 8 for i, s in enumerate(seqs) if i != 2)
    assert all(e[1] == [] and e[2] == [] for e in seqs[3].logprobs)
    for i in (0, 1, 3):
        _check_against_rerun(seqs[i])


def test_engine_eos_finish_and_preemption_keep_the_invariant(plain_run):
    # EOS: each request stops at the token its plain run produced fourth
    eos = [o[3] for o in plain_run]
    seqs = _run(_engine(), PROMPTS, _params([3, 3, 3, 3], eos=True), eos)
    for s, o, e in zip(seqs, plain_run, eos):
        assert s.finish_reason == "eos" and s.output == o[:o.index(e) + 1]
        assert len(s.logprobs) == len(s.output)
    # preemption: a pool too small for both sequences' full length
    prompts = [[1, 5, 9, 200, 7, 3, 2], [3, 4, 7, 11, 12, 13, 14]]
    params = _params([4, 4], n=24)
    calm = _run(_engine(num_kv_blocks=128, kv_block_size=16), prompts, params)
    tight_eng = _engine(num_kv_blocks=4, kv_block_size=16)
    tight = _run(tight_eng, prompts, params)
    assert tight_eng.scheduler.num_preemptions >= 1
    for a, b in zip(calm, tight):
        assert a.output == b.output and len(b.logprobs) == len(b.output) == 24
        for (ca, ia, la), (cb, ib, lb) in zip(a.logprobs, b.logprobs):
            # the preempted run recomputes its context in a prefill: fp32 logits a few ulp apart
            assert ia == ib and ca == pytest.approx(cb, rel=0, abs=PP_TOL) and la == pytest.approx(lb, rel=0, abs=PP_TOL)


def test_no_asking_request_never_calls_the_op(monkeypatch, plain_run):
    calls = []
    real = ops.token_logprobs
    monkeypatch.setattr(ops, "token_logprobs", lambda *a, **k: calls.append(1) or real(*a, **k))
    seqs = _run(_engine(), PROMPTS, _params([None] * 4))
    assert [s.output for s in seqs] == plain_run and not calls and all(s.logprobs == [] for s in seqs)
    _run(_engine(), PROMPTS[:1], _params([1]))
    assert calls


def test_lookahead_throw_away_row_is_skipped():
    """The ordering hazard of a lookahead step: a sequence that EOS finished one step earlier still
    has a row in the step issued before that was known; its row is discarded like its token."""
    bm = make_block_manager(64, 4)
    sch = Scheduler(bm, num_slots=1, max_batch=8, max_prefill_tokens=64, max_seq_len=64)
    a = Sequence([1, 2, 3], SamplingParams(max_new_tokens=8, logprobs=1), eos_token_id=42)
    b = Sequence([4, 5], SamplingParams(max_new_tokens=8, logprobs=1), eos_token_id=42)
    for s in (a, b):
        sch.add(s)

    def lps(vals):
        n = len(vals)
        return (np.array(vals, np.float32), np.zeros((n, 1), np.int32), np.array(vals, np.float32).reshape(n, 1))

    st = sch.schedule(0)
    sch.complete(st, [7, 8], 0.0, lps([-1.0, -2.0]))
    st1 = sch.schedule(0)
    st2 = sch.schedule_lookahead(0)
    assert st2 is not None and len(st2.rows) == 2
    done = sch.complete(st1, np.array([42, 9], np.int32), 0.0, lps([-3.0, -4.0]))     # a: EOS
    assert done == [a] and a.output == [7, 42] and [e[0] for e in a.logprobs] == [-1.0, -3.0]
    sch.complete(st2, np.array([5, 10], np.int32), 0.0, lps([-99.0, -5.0]))           # a's row: thrown away
    assert [e[0] for e in a.logprobs] == [-1.0, -3.0]
    assert [e[0] for e in b.logprobs] == [-2.0, -4.0, -5.0] and sch.sync_output(b) == [8, 9, 10]


def test_tensor_parallel_lanes_refuse_logprobs():
    eng = _engine()
    with pytest.raises(ValueError):
        eng.add_request([1, 2], SamplingParams(logprobs=21))
    with pytest.raises(ValueError):
        eng.add_request([1, 2], SamplingParams(logprobs=True))
    eng.tp = object()                                       # what a tensor-parallel leader holds
    with pytest.raises(ValueError, match="tensor parallel"):
        eng.add_request([1, 2], SamplingParams(logprobs=2))
    assert eng.add_request([1, 2], SamplingParams()).params.logprobs is None


# ------------------------------------------------------------------ pipeline
# A pipeline runs the single engine's fp32 math, but its scheduler batches other rows together, and
# the CPU GEMMs round differently with the batch: logits of magnitude <= 16 differ by a few ulp
# (2^-20 each), and a log-probability is a difference of two such numbers: 8 ulp = 7.6e-6 < 1e-5.
PP_TOL = 1e-5
PP_PROMPTS = [[i + 1, i + 5, 7, 9, 3 * i + 2] for i in range(6)]
PP_PARAMS = [SamplingParams(max_new_tokens=6, ignore_eos=True, logprobs=lp, **k)
             for lp, k in zip((5, None, 0, 2, None, 20),
                              (dict(), dict(), dict(temperature=0.8, seed=5), dict(temperature=1.1, top_k=40, seed=6),
                               dict(temperature=0.7, seed=7), dict()))]


def _pp_ecfg(**kw):
    d = dict(model="tiny-llama", dtype="float32", device="cpu", max_batch=4, max_seq_len=128, use_graphs=False,
             num_kv_blocks=256)
    d.update(kw)
    return EngineConfig(**d)


@pytest.fixture(scope="module")
def pp_expected():
    eng = LLMEngine(_pp_ecfg())
    seqs = [eng.add_request(p, q) for p, q in zip(PP_PROMPTS, PP_PARAMS)]
    eng.run_until_done()
    return [(s.output, s.logprobs) for s in seqs]


def _same_as_single(got, expected):
    """Generated ids and top ids equal; log-probabilities within PP_TOL (see there)."""
    worst = 0.0
    for (out, lps), (eout, elps) in zip(got, expected):
        assert out == eout and len(lps) == len(elps)
        for (c, ti, tl), (ec, eti, etl) in zip(lps, elps):
            assert ti == eti
            assert c == pytest.approx(ec, rel=0, abs=PP_TOL) and tl == pytest.approx(etl, rel=0, abs=PP_TOL)
            worst = max([worst, abs(c - ec)] + [abs(a - b) for a, b in zip(tl, etl)])
    print(f"largest |logprob difference| to the single engine: {worst:.3e}")


def _recorded(monkeypatch):
    """The sequences a PipelineDriver admits from here on (run_loopback_pipeline returns ids only)."""
    from distributed_llms_amd.parallel.pipeline import PipelineDriver
    seqs, real = [], PipelineDriver.add_request

    def add_request(self, *a, **k):
        seqs.append(real(self, *a, **k))
        return seqs[-1]
    monkeypatch.setattr(PipelineDriver, "add_request", add_request)
    return seqs


def test_loopback_pipeline_matches_single(pp_expected, monkeypatch):
    from distributed_llms_amd.parallel.pipeline import run_loopback_pipeline
    seqs = _recorded(monkeypatch)
    run_loopback_pipeline(_pp_ecfg(), 2, PP_PROMPTS, PP_PARAMS)
    _same_as_single([(s.output, s.logprobs) for s in seqs], pp_expected)
    assert [len(s.logprobs) for s in seqs] == [6, 0, 6, 6, 0, 6]


def _rank_main(rank, world, pp, port, env, cfg, out_q):
    import os
    import traceback
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), **env)
    torch.set_num_threads(1)
    import torch.distributed as dist
    from distributed_llms_amd.parallel.dist_engine import RankRole, init_distributed
    try:
        ctx = init_distributed(pp=pp, backend="gloo")
        role = RankRole(ctx, _pp_ecfg(num_workers=pp, **cfg))
        seqs = [role.add_request(p, q) for p, q in zip(PP_PROMPTS, PP_PARAMS)] if role.is_driver else []
        role.run_round()
        role.shutdown()
        dist.barrier()
        out_q.put((rank, role.transport.kind, [(s.output, s.logprobs) for s in seqs] if role.is_driver else None, None))
        dist.destroy_process_group()
    except Exception:      # noqa: BLE001 - reported to the test
        out_q.put((rank, None, None, traceback.format_exc()))
        raise


# the RCCL transport's multi-rank branch over its stand-in communicators, with a prefill budget far
# below the longest ids message (4 rows x 42 words = 168 > 16): the ids ring must be sized for the
# message, not for the hop's rows
STANDIN = (dict(DLLM_TRANSPORT="rccl", DLLM_RCCL_STANDIN="1"), dict(max_prefill_tokens=16, comm_timeout_s=20.0))


@pytest.mark.slow
@pytest.mark.parametrize("env,cfg,kind", [({}, {}, "torch"), (*STANDIN, "rccl")], ids=["gloo", "rccl-standin"])
def test_two_stage_process_pipeline_matches_single(pp_expected, env, cfg, kind):
    import socket

    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, 2, port, env, cfg, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(2):
            r, got_kind, res, err = q.get(timeout=240)
            assert err is None, f"rank {r} failed:\n{err}"
            assert got_kind == kind
            results[r] = res
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    _same_as_single(results[0], pp_expected)


# ------------------------------------------------------------------ worker, master, HTTP
def test_result_payload_round_trip():
    from distributed_llms_amd.network.protocol import pack_ids, pack_result, unpack_result
    ids = [5, 6, 7]
    assert pack_result(ids) == pack_ids(ids) and unpack_result(pack_ids(ids)) == (ids, None)
    entries = [(-0.5, [5, 9], [-0.5, -1.25]), (NINF, [1, 2], [-0.25, NINF]), (-2.0, [7, 3], [-2.0, -3.0])]
    payload = pack_result(ids, entries, 2)
    assert len(payload) == 4 * 3 * (2 + 2 * 2)
    got, lp = unpack_result(payload, 3, 2)
    assert got == ids and lp == {"token_logprobs": [-0.5, NINF, -2.0], "top_ids": [[5, 9], [1, 2], [7, 3]],
                                 "top_logprobs": [[-0.5, -1.25], [-0.25, NINF], [-2.0, -3.0]]}
    got, lp = unpack_result(pack_result(ids, [(-1.0, [], [])] * 3, 0), 3, 0)
    assert lp == {"token_logprobs": [-1.0] * 3, "top_ids": [[], [], []], "top_logprobs": [[], [], []]}
    with pytest.raises(ValueError):
        unpack_result(payload, 3, 1)


def test_http_objects_serialise_minus_inf_as_null():
    import json

    from distributed_llms_amd.master import http_api

    class Tok:
        def decode(self, ids):
            return "".join("ab"[i % 2] for i in ids)       # ids 1 and 3 decode to the same text

    lp = {"token_logprobs": [-0.5, NINF], "top_ids": [[1, 3], [2, 4]], "top_logprobs": [[-0.5, -1.0], [-0.25, NINF]]}
    o = json.loads(json.dumps(http_api._openai_logprobs(Tok(), [1, 2], lp), allow_nan=False))
    assert o == {"tokens": ["b", "a"], "token_logprobs": [-0.5, None], "text_offset": [0, 1],
                 "top_logprobs": [{"b": -0.5}, {"a": -0.25}], "token_ids": [1, 2], "top_token_ids": [[1, 3], [2, 4]]}
    g = json.loads(json.dumps(http_api._generate_logprobs(lp), allow_nan=False))
    assert g == {"token_logprobs": [-0.5, None], "top_ids": [[1, 3], [2, 4]], "top_logprobs": [[-0.5, -1.0], [-0.25, None]]}
    assert http_api._sampling({"logprobs": 20})["logprobs"] == 20 and "logprobs" not in http_api._sampling({})
    for bad in (21, True, -1, "2", 1.5):
        with pytest.raises(ValueError):
            http_api._sampling({"logprobs": bad})
    with pytest.raises(ValueError):
        http_api._sampling({"logprobs": 1, "stream": True})


from test_master_worker import PROMPTS as MW_PROMPTS, _cfg as _mw_cfg, _spawn_worker, cluster  # noqa: E402,F401


@pytest.mark.slow
def test_worker_pipeline_sizes_the_ids_ring_for_the_message(monkeypatch):
    """Master + two worker processes on the RCCL transport (stand-in communicators) with a prefill
    budget of 16 tokens: a step of 4 rows with logprobs = 20 answers with 168 words, which must fit
    the transport's ids ring (sized by max_ids_message_len, not by the hop's rows)."""
    import dataclasses
    import subprocess

    from distributed_llms_amd.master.node import MasterNode
    monkeypatch.setenv("DLLM_TRANSPORT", "rccl")
    monkeypatch.setenv("DLLM_RCCL_STANDIN", "1")
    model = "synthetic:tiny-llama"
    cfg = dataclasses.replace(_mw_cfg(model), max_batch=4, max_prefill_tokens=16, comm_timeout_s=20.0)
    prompts = [[i + 1, i + 5, 7, 9, 3 * i + 2] for i in range(4)]
    eng = LLMEngine(cfg)
    seqs = [eng.add_request(p, SamplingParams(max_new_tokens=4, ignore_eos=True, logprobs=20)) for p in prompts]
    eng.run_until_done()
    m = MasterNode("127.0.0.1", 0, cfg).start()
    procs = []
    try:
        m.initialize_model(model, num_shards=2)
        procs = [_spawn_worker(m.port) for _ in range(2)]
        m.wait_for_workers(2, timeout=120)
        m.assign_shards()
        m.distribute_shards(timeout=300)
        res = m.generate(prompts, max_new_tokens=4, ignore_eos=True, logprobs=20, timeout=60)
        transports = {w["remote"].get("transport") for w in m.status()["workers"].values()}
    finally:
        m.stop()
        for p in procs:
            try:
                p.wait(timeout=15)
            except subprocess.TimeoutExpired:
                p.kill()
    for r, s in zip(res, seqs):
        assert r["tokens"] == s.output and r["logprobs"]["top_ids"] == [e[1] for e in s.logprobs]
        assert r["logprobs"]["token_logprobs"] == pytest.approx([e[0] for e in s.logprobs], rel=0, abs=PP_TOL)
    assert transports == {"rccl"}, transports


@pytest.mark.slow
def test_http_logprobs_against_master_and_cpu_workers(cluster):  # noqa: F811
    import json
    import urllib.error
    import urllib.request

    from distributed_llms_amd.master.http_api import serve_http
    make, _ = cluster
    model = "synthetic:tiny-llama"
    m = make(model, 2)
    m.assign_shards()
    m.distribute_shards(timeout=300)
    srv, _ = serve_http(m, "127.0.0.1", 0)
    base = f"http://127.0.0.1:{srv.server_address[1]}"

    def post(path, body):
        req = urllib.request.Request(base + path, data=json.dumps(body).encode(),
                                     headers={"Content-Type": "application/json"})
        with urllib.request.urlopen(req, timeout=120) as r:
            return json.loads(r.read())

    try:
        eng = LLMEngine(_mw_cfg(model))
        seqs = [eng.add_request(p, SamplingParams(max_new_tokens=5, ignore_eos=True, logprobs=3)) for p in MW_PROMPTS[:2]]
        eng.run_until_done()
        # the Python API: the result dict carries the values; None for a request that did not ask
        res = m.generate([MW_PROMPTS[0]], max_new_tokens=5, ignore_eos=True, logprobs=3, timeout=120)[0]
        assert res["tokens"] == seqs[0].output
        assert res["logprobs"]["top_ids"] == [e[1] for e in seqs[0].logprobs]
        assert res["logprobs"]["token_logprobs"] == pytest.approx([e[0] for e in seqs[0].logprobs], rel=2e-4, abs=2e-4)
        assert m.generate([MW_PROMPTS[0]], max_new_tokens=2, ignore_eos=True, timeout=120)[0]["logprobs"] is None
        g = post("/generate", {"prompt_ids": MW_PROMPTS[0], "max_new_tokens": 5, "ignore_eos": True, "logprobs": 3})
        assert g["tokens"] == seqs[0].output and sorted(g["logprobs"]) == ["token_logprobs", "top_ids", "top_logprobs"]
        assert g["logprobs"]["top_ids"] == res["logprobs"]["top_ids"]
        assert "logprobs" not in post("/generate", {"prompt_ids": MW_PROMPTS[0], "max_new_tokens": 2})
        c = post("/v1/completions", {"prompt": [MW_PROMPTS[0], MW_PROMPTS[1]], "max_tokens": 5, "ignore_eos": True,
                                     "logprobs": 3})
        for ch, s in zip(c["choices"], seqs):
            lp = ch["logprobs"]
            assert sorted(lp) == ["text_offset", "token_ids", "token_logprobs", "tokens", "top_logprobs", "top_token_ids"]
            assert lp["token_ids"] == ch["tokens"] == s.output and len(lp["tokens"]) == len(lp["text_offset"]) == 5
            assert lp["top_token_ids"] == [e[1] for e in s.logprobs] and lp["text_offset"][0] == 0
            assert lp["token_logprobs"] == pytest.approx([e[0] for e in s.logprobs], rel=2e-4, abs=2e-4)
            assert all(isinstance(d, dict) and 1 <= len(d) <= 3 for d in lp["top_logprobs"])
            assert [d[t] for d, t in zip(lp["top_logprobs"], lp["tokens"])] == lp["token_logprobs"]    # greedy
        z = post("/v1/completions", {"prompt": MW_PROMPTS[0], "max_tokens": 3, "ignore_eos": True, "logprobs": 0})
        assert z["choices"][0]["logprobs"]["top_logprobs"] == [{}, {}, {}]
        assert "logprobs" not in post("/v1/completions", {"prompt": MW_PROMPTS[0], "max_tokens": 2})["choices"][0]
        for body in ({"logprobs": 21}, {"logprobs": True}, {"logprobs": 2, "stream": True}):
            for path in ("/v1/completions", "/generate"):
                req = urllib.request.Request(base + path, data=json.dumps(dict(body, prompt=MW_PROMPTS[0],
                                                                              prompt_ids=MW_PROMPTS[0])).encode())
                with pytest.raises(urllib.error.HTTPError) as ei:
                    urllib.request.urlopen(req, timeout=30)
                assert ei.value.code == 400, (path, body)
    finally:
        srv.shutdown()
