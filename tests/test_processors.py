"""Logit processors on the CPU: the reference contract, validation, the HostBatch wire section, the
scheduler's state rows, the engine against a stateless oracle, pipelines and the HTTP front end."""
import collections
import json

import numpy as np
import pytest
import torch

import processors_cases as pc
from distributed_llms_amd import ops
from distributed_llms_amd.config import EngineConfig
from distributed_llms_amd.engine.batch import HostBatch, build_host_batch, merge_mixed
from distributed_llms_amd.engine.llm_engine import LLMEngine, make_block_manager
from distributed_llms_amd.engine.scheduler import Scheduler, Step
from distributed_llms_amd.engine.sequence import SamplingParams, Sequence, validate_processors
from distributed_llms_amd.ops import reference as ref

INF, NINF, NAN = float("inf"), float("-inf"), float("nan")
f32 = np.float32


def _bits(x):
    return torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _bf16(x):
    """The bf16 value nearest to x, as float32."""
    return torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).float().numpy()


# ------------------------------------------------------------------ the reference contract
def _apply_row(logits, in_prompt=(), outputs=(), bias=None, min_tokens=0, eos=1, **pen):
    """One bf16 row through ref.apply_logit_processors with a state built by ref.logit_state_update
    from a prompt and outputs (token lists) -> the new row's bf16 bits."""
    v = len(logits)
    ls = pc.empty_state(3, v)
    ls.state[:] = 0x55                                    # row 1 is reset by the chunk; 0 and 2 must stay
    prompt, outputs = list(in_prompt), list(outputs)
    toks = prompt + outputs
    bias = bias or {}
    procs = torch.from_numpy(pc.proc_row(1, len(prompt), ref.PROC_SAMPLE | ref.PROC_UPDATE, min_tokens=min_tokens,
                                         **pen)[None])
    ref.logit_state_update(ls.state, v, torch.tensor(toks, dtype=torch.int32), torch.tensor([0, len(toks)], dtype=torch.int32),
                           procs, ls.bias_n, ls.bias_ids, ls.bias_vals, torch.tensor([0, len(bias)], dtype=torch.int32),
                           torch.tensor(list(bias), dtype=torch.int32), torch.tensor(list(bias.values()), dtype=torch.float32))
    assert (ls.state[0] == 0x55).all() and (ls.state[2] == 0x55).all()
    row = torch.tensor([logits], dtype=torch.float32).to(torch.bfloat16)
    ref.apply_logit_processors(row, ls.state, procs, torch.tensor([len(toks)], dtype=torch.int32), eos, ls.bias_n,
                               ls.bias_ids, ls.bias_vals)
    return row.view(torch.int16).numpy().view(np.uint16)[0]


BASE = [2.0, -3.0, 0.5, -0.0, INF, NINF, NAN, 1.25]


def test_reference_each_rule_alone():
    base = _bits(BASE)
    # repetition: prompt and output tokens, positive divided, the rest multiplied; -0 stays -0
    got = _apply_row(BASE, in_prompt=[0, 3], outputs=[1, 4, 5], rep=1.5)
    exp = base.copy()
    exp[[0, 1]] = _bits([f32(2.0) / f32(1.5), f32(-3.0) * f32(1.5)])
    assert got.tolist() == exp.tolist()                    # -0 * 1.5 = -0, inf / 1.5 = inf, -inf * 1.5 = -inf
    # presence: output tokens only, whatever their count
    got = _apply_row(BASE, in_prompt=[0], outputs=[1, 1, 2], pres=0.75)
    exp = base.copy()
    exp[[1, 2]] = _bits([-3.75, -0.25])
    assert got.tolist() == exp.tolist()
    # frequency: times the output count; the prompt's occurrences do not count
    got = _apply_row(BASE, in_prompt=[2, 2, 2], outputs=[2, 7, 7, 7], freq=0.25)
    exp = base.copy()
    exp[[2, 7]] = _bits([0.25, 0.5])
    assert got.tolist() == exp.tolist()
    # bias: also on a token nothing else touches; inf + bias = inf, NaN stays NaN
    got = _apply_row(BASE, bias={0: -100.0, 4: -100.0, 6: 5.0, 3: 0.0})
    exp = base.copy()
    exp[0] = _bits([-98.0])[0]
    exp[3] = 0x0000                                        # -0 + 0 = +0: a touched token is recomputed
    assert got[[0, 3, 4]].tolist() == exp[[0, 3, 4]].tolist() and (got[6] & 0x7FFF) > 0x7F80
    assert got[[1, 2, 5, 7]].tolist() == base[[1, 2, 5, 7]].tolist()
    # min_tokens: EOS is -inf while the output index is below it, and only then
    assert _apply_row(BASE, outputs=[2], min_tokens=2, eos=0).tolist() == [0xFF80] + base[1:].tolist()
    assert _apply_row(BASE, in_prompt=[7], outputs=[7, 7, 7], min_tokens=3, eos=0)[0] == base[0]
    assert _apply_row(BASE, outputs=[2], min_tokens=2, eos=6)[6] == 0xFF80        # NaN at EOS: banned all the same


def test_reference_all_rules_round_once():
    # chosen so that rounding to bf16 between the steps would give another result: the chain in
    # float32 from the bf16 logit, one rounding at the end
    x, rep, freq, pres, b, n = f32(_bf16(1.25)), f32(1.3), f32(0.013), f32(0.003), f32(0.0171), 3
    y = x / rep
    y = y - freq * f32(n)
    y = y - pres
    y = y + b
    once = _bits([float(y)])[0]
    stepwise = x
    for op in (lambda t: t / rep, lambda t: t - freq * f32(n), lambda t: t - pres, lambda t: t + b):
        stepwise = f32(_bf16(float(op(stepwise))))
    assert _bits([float(stepwise)])[0] != once            # the case tells the two apart
    row = [0.0, float(x), -1.0, 4.0]
    got = _apply_row(row, in_prompt=[1, 2], outputs=[1] * n, bias={1: float(b), 3: 1.0}, min_tokens=n + 1, eos=3, rep=float(rep),
                     pres=float(pres), freq=float(freq))
    neg = _bits([float(f32(-1.0) * rep)])[0]
    assert got.tolist() == [0x0000, once, neg, 0xFF80]    # untouched, the chain, prompt-only, biased then banned


def test_reference_untouched_bits_and_edge_entries():
    """Every shape's case: tokens no rule touches keep -0, NaN payloads and subnormals; rows that did
    not ask keep everything; touched +-inf / NaN / -0 follow IEEE arithmetic."""
    case = pc.make_apply_case(5, 5003)
    before = case["logits"].clone()
    out = pc.reference(case)
    changed = pc.check_bits(out, out, before, case["touched"], "reference")
    assert changed > 500
    b, o = (t.view(torch.int16).numpy().view(np.uint16) for t in (before, out))
    assert (o[1] == b[1]).all() and (o[4] == b[4]).all()                  # "none" and "flagless"
    for r in (0, 2, 3):
        t = case["touched"][r]
        for pat in pc.SPECIAL:
            assert ((b[r] == pat) & ~t).any(), (r, hex(pat))             # planted under untouched tokens too
        nan_in = (b[r] & 0x7FFF) > 0x7F80
        banned = np.zeros_like(t)
        if case["seq_lens"][r] - 4 < 6 and r != 3:
            banned[case["eos"]] = True
        assert (((o[r] & 0x7FFF) > 0x7F80) == (nan_in & ~banned)).all()   # NaN in stays NaN, none appears


def test_bf16_rne_bits_matches_torch():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(20000, generator=g) * 50
    x[:6] = torch.tensor([INF, NINF, 0.0, -0.0, 1.00390625, 1.01171875])   # two ties: to even
    got = ref.bf16_rne_bits(x.numpy())
    assert got.tolist() == x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).tolist()
    assert (ref.bf16_rne_bits(np.array([NAN], f32)) & 0x7FFF) > 0x7F80


def test_state_update_and_count_reference():
    v = 21
    ls = pc.empty_state(4, v)
    ls.state[:] = 9
    procs = np.stack([pc.proc_row(2, 3, ref.PROC_UPDATE, start=0), pc.proc_row(-1, 0, ref.PROC_UPDATE),
                      pc.proc_row(1, 2, ref.PROC_UPDATE | ref.PROC_SAMPLE, start=4), pc.proc_row(3, 0, ref.PROC_SAMPLE)])
    ids = torch.tensor([5, 5, 6, 5, 7, 7, 99, -1,   1, 2,   4, 20, 21, 4,   8], dtype=torch.int32)
    cu = torch.tensor([0, 8, 10, 14, 15], dtype=torch.int32)
    bcu = torch.tensor([0, 2, 2, 3, 3], dtype=torch.int32)
    ops.logit_state_update(ls, ids, cu, torch.from_numpy(procs), bcu, torch.tensor([7, 0, 3], dtype=torch.int32),
                           torch.tensor([1.5, -2.0, 9.0]))
    st = ls.state.numpy().view(np.uint32)
    P, B = ref.STATE_PROMPT_BIT, ref.STATE_BIAS_BIT
    exp2 = np.zeros(24, np.uint32)
    exp2[[5, 6]] = P
    exp2[5] += 1
    exp2[7] = 2 | B
    exp2[0] = B
    assert st[2].tolist() == exp2.tolist()                 # reset, bias installed, 99 and -1 ignored
    assert ls.bias_n.tolist() == [0, 0, 2, 0] and ls.bias_ids[2, :2].tolist() == [7, 0] and ls.bias_vals[2, :2].tolist() == [1.5, -2.0]
    exp1 = np.full(24, 9, np.uint32)
    exp1[4] += 2
    exp1[20] += 1
    assert st[1].tolist() == exp1.tolist()                 # start 4 > 0: no reset, no bias list, 21 = vocab ignored
    assert (st[0] == 9).all() and (st[3] == 9).all()       # no UPDATE flag / other rows: untouched
    ops.logit_state_count(ls, torch.tensor([5, 5, 4, 30], dtype=torch.int32), torch.from_numpy(procs))
    exp1[4] += 1
    assert st[1].tolist() == exp1.tolist() and st[2].tolist() == exp2.tolist() and (st[3] == 9).all()


# ------------------------------------------------------------------ validation
def test_sampling_params_fields_and_validation():
    p = SamplingParams()
    assert (p.repetition_penalty, p.presence_penalty, p.frequency_penalty, p.logit_bias, p.min_tokens) == (1.0, 0.0, 0.0, None, 0)
    assert not p.has_processors and validate_processors(p, 100) is False
    q = SamplingParams(max_new_tokens=8, repetition_penalty=2, logit_bias={"7": 1, 9: -100.0}, min_tokens=8)
    assert validate_processors(q, 100) is True and q.logit_bias == {7: 1.0, 9: -100.0} and q.has_processors
    assert SamplingParams.from_dict(json.loads(json.dumps(q.to_dict()))).logit_bias == {"7": 1.0, "9": -100.0}
    d = {"logit_bias": {"3": 0.5}, "max_new_tokens": 4}
    assert validate_processors(d, 10) is True and d == {"logit_bias": {3: 0.5}, "max_new_tokens": 4}
    assert validate_processors({"logit_bias": {}}, 10) is False
    for k in ("presence_penalty", "frequency_penalty"):
        assert validate_processors({k: -2.0}, 10) and validate_processors({k: 2}, 10)
    bad = [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=INF),
           dict(repetition_penalty=NAN), dict(repetition_penalty="1.2"), dict(repetition_penalty=True),
           dict(presence_penalty=2.01), dict(presence_penalty=-2.5), dict(presence_penalty=NAN),
           dict(frequency_penalty=3), dict(frequency_penalty=None), dict(logit_bias=[1, 2]),
           dict(logit_bias={i: 0.0 for i in range(301)}), dict(logit_bias={100: 1.0}), dict(logit_bias={-1: 1.0}),
           dict(logit_bias={"x": 1.0}), dict(logit_bias={1.5: 1.0}), dict(logit_bias={1: 100.5}),
           dict(logit_bias={1: -101}), dict(logit_bias={1: NAN}), dict(logit_bias={1: "3"}),
           dict(logit_bias={"1": 1.0, 1: 2.0}), dict(min_tokens=-1), dict(min_tokens=65), dict(min_tokens=1.0),
           dict(min_tokens=True), dict(min_tokens=3, max_new_tokens=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            validate_processors(SamplingParams(**kw), 100)
        with pytest.raises(ValueError):
            validate_processors(dict(kw), 100)
    assert validate_processors(SamplingParams(logit_bias={i: 0.0 for i in range(300)}), 300)
    eng = _engine()
    with pytest.raises(ValueError):
        eng.add_request([1, 2], SamplingParams(logit_bias={512: 1.0}))            # tiny-llama's vocabulary is 512
    with pytest.raises(ValueError):
        eng.add_request([1, 2], SamplingParams(presence_penalty=5.0))
    assert eng.add_request([1, 2], SamplingParams(logit_bias={"511": 1.0})).params.logit_bias == {511: 1.0}
    eng.tp = object()                                       # what a tensor-parallel leader holds
    with pytest.raises(ValueError, match="tensor parallel"):
        eng.add_request([1, 2], SamplingParams(frequency_penalty=0.5))
    assert eng.add_request([1, 2], SamplingParams()).state_row == -1
    with pytest.raises(ValueError):
        EngineConfig(model="synthetic:tiny-llama", max_seq_len=1 << 24).validate()


# ------------------------------------------------------------------ HostBatch
def _hb(b=3, mb=2):
    t = b
    return HostBatch(False, np.arange(t, dtype=np.int32) + 1, np.arange(t, dtype=np.int32) + 10,
                     np.arange(t, dtype=np.int32) + 20, np.arange(b, dtype=np.int32) + 30,
                     np.arange(b + 1, dtype=np.int32), np.arange(b * mb, dtype=np.int32).reshape(b, mb) + 40,
                     np.arange(b, dtype=np.int32), 1, 33, slot=2, step_id=9,
                     sampling=np.arange(3 * b, dtype=np.int32).reshape(b, 3) + 100,
                     sample_seeds=np.arange(2 * b, dtype=np.int32).reshape(b, 2) - 7,
                     logprobs=np.array([-1, 2, 0], np.int32))


def _parent_format(hb):
    """The packed array as the format was before the processors section, from the documented layout:
    [header(16) | ids | positions | slots | seq_lens | cu_seqlens | block_tables | logits_idx |
    sampling 3B (header word 8) | sample_seeds 2B (word 10) | logprobs B (word 11)]."""
    b, t = hb.seq_lens.shape[0], hb.ids.shape[0]
    hdr = [int(hb.is_prefill), t, b, hb.block_tables.shape[1], hb.max_q_len, hb.max_ctx, hb.slot, hb.step_id,
           int(hb.sampling is not None), hb.num_decode, int(hb.sample_seeds is not None), int(hb.logprobs is not None),
           0, 0, 0, 0]
    parts = [hdr, hb.ids, hb.positions, hb.slots, hb.seq_lens, hb.cu_seqlens, hb.block_tables.reshape(-1), hb.logits_idx]
    for opt in (hb.sampling, hb.sample_seeds, hb.logprobs):
        if opt is not None:
            parts.append(opt.reshape(-1))
    return np.concatenate([np.asarray(p, dtype=np.int32) for p in parts])


def test_host_batch_round_trip_with_and_without_the_section():
    plain = _hb()
    packed = plain.pack()
    assert packed.dtype == np.int32 and np.array_equal(packed, _parent_format(plain)) and packed[12] == 0
    assert HostBatch.unpack(packed).procs is None
    hb = _hb()
    hb.procs = np.stack([pc.proc_row(), pc.proc_row(4, 7, 3, 1.5, -0.5, 0.25, 2, 0), pc.proc_row(1, 2, 1, 0.5)])
    hb.bias_cu = np.array([0, 0, 2, 2], np.int32)
    hb.bias_ids = np.array([17, 3], np.int32)
    hb.bias_vals = pc.f32_bits([2.5, -100.0])
    hb.state_rows = 11
    p2 = hb.pack()
    extra = 1 + 3 * ref.PROC_WORDS + 4 + 2 + 2
    assert p2[12] == 1 and p2.shape[0] == packed.shape[0] + extra
    rest = p2[:-extra].copy()
    rest[12] = 0
    assert np.array_equal(rest, packed)                    # everything before the section is unchanged
    back = HostBatch.unpack(p2)
    assert back.state_rows == 11 and np.array_equal(back.procs, hb.procs) and back.bias_cu.tolist() == [0, 0, 2, 2]
    assert back.bias_ids.tolist() == [17, 3] and back.bias_vals.view(np.float32).tolist() == [2.5, -100.0]
    assert back.logprobs.tolist() == [-1, 2, 0] and np.array_equal(back.pack(), p2)
    assert back.procs[1, [ref.PROC_REP, ref.PROC_PRES, ref.PROC_FREQ]].view(np.float32).tolist() == [1.5, -0.5, 0.25]


def test_build_host_batch_merge_mixed_and_native_decode_carry_the_section():
    bm = make_block_manager(64, 4)
    sch = Scheduler(bm, num_slots=1, max_batch=8, max_prefill_tokens=64, max_seq_len=64, mixed_prefill_tokens=16,
                    state_rows=5)
    plain = Sequence([1, 2, 3, 4, 5], SamplingParams(max_new_tokens=8, ignore_eos=True))
    sch.add(plain)
    st = sch.schedule(0)
    assert st.state_rows == 0 and build_host_batch(st, bm, 4).procs is None
    sch.complete(st, [7])
    # a decode step while nobody asks: no section, the parent's packed bytes, the native array itself
    st = sch.schedule(0)
    hb = build_host_batch(st, bm, 4)
    assert hb.procs is None and st.packed[12] == 0 and hb.pack() is st.packed
    assert np.array_equal(st.packed, _parent_format(hb))
    sch.complete(st, [8])
    asking = Sequence([9, 8, 7], SamplingParams(max_new_tokens=8, ignore_eos=True, repetition_penalty=1.25,
                                                 presence_penalty=0.5, frequency_penalty=-0.25, min_tokens=2,
                                                 logit_bias={3: 1.5, 400: -2.0}))
    biased = Sequence([6, 5], SamplingParams(max_new_tokens=8, ignore_eos=True, logit_bias={9: 100.0}))
    sch.add(asking)
    sch.add(biased)
    st = sch.schedule(0)
    assert st.mixed and st.state_rows == 5 and asking.state_row >= 0 and biased.state_row >= 0 and plain.state_row == -1
    assert asking.state_row != biased.state_row
    hb = build_host_batch(st, bm, 4)                        # the decode row did not ask: state row -1
    assert hb.num_decode == 1 and hb.procs[:, ref.PROC_ROW].tolist() == [-1, asking.state_row, biased.state_row]
    both = ref.PROC_SAMPLE | ref.PROC_UPDATE
    assert hb.procs[:, ref.PROC_FLAGS].tolist() == [0, both, both] and hb.procs[:, ref.PROC_PROMPT_LEN].tolist() == [0, 3, 2]
    assert hb.procs[1, ref.PROC_REP:ref.PROC_FREQ + 1].view(np.float32).tolist() == [1.25, 0.5, -0.25]
    assert hb.procs[1, ref.PROC_MIN_TOKENS] == 2 and hb.procs[:, ref.PROC_START].tolist() == [0, 0, 0]
    assert hb.bias_cu.tolist() == [0, 0, 2, 3] and hb.bias_ids.tolist() == [3, 400, 9]
    assert hb.bias_vals.view(np.float32).tolist() == [1.5, -2.0, 100.0] and hb.state_rows == 5
    back = HostBatch.unpack(hb.pack())
    assert np.array_equal(back.procs, hb.procs) and back.bias_ids.tolist() == [3, 400, 9] and back.state_rows == 5
    sch.complete(st, np.array([9, 10, 11], np.int32), 0.0)
    # now a natively packed decode step carries the section, and pack() holds it
    st = sch.schedule(0)
    hb = build_host_batch(st, bm, 4)
    assert not st.is_prefill and st.packed[12] == 0 and hb.raw is None
    assert hb.procs[:, ref.PROC_FLAGS].tolist() == [0, ref.PROC_SAMPLE, ref.PROC_SAMPLE] and hb.bias_ids.shape == (0,)
    p = hb.pack()
    assert p[12] == 1 and np.array_equal(HostBatch.unpack(p).procs, hb.procs) and hb.bias_cu.tolist() == [0, 0, 0, 0]
    # the other way round: decode rows asked, the prefill rows did not
    pre = build_host_batch(Step(True, [Sequence([1, 2], SamplingParams())], 0), _bm_with(2), 4)
    m = merge_mixed(hb, pre, 0, 0)
    assert m.procs[:, ref.PROC_ROW].tolist() == [-1, asking.state_row, biased.state_row, -1] and m.bias_cu.tolist() == [0] * 5
    assert m.state_rows == 5 and HostBatch.unpack(m.pack()).procs.shape == (4, ref.PROC_WORDS)


def _bm_with(n):
    class _Any:
        def fill_slots(self, seq_ids, starts, qlens, slots):
            slots[:] = np.arange(slots.shape[0])
            return slots.shape[0]

        def fill_block_tables(self, seq_ids, bt, pad):
            bt[:] = 0
    return _Any()


def test_chunked_prefill_flags_and_bias_only_at_position_zero():
    bm = make_block_manager(64, 4)
    sch = Scheduler(bm, num_slots=1, max_batch=8, max_prefill_tokens=4, max_seq_len=64)
    s = Sequence(list(range(1, 11)), SamplingParams(max_new_tokens=4, ignore_eos=True, logit_bias={5: 1.0}))
    sch.add(s)
    seen = []
    for _ in range(3):
        st = sch.schedule(0)
        hb = build_host_batch(st, bm, 4)
        seen.append((int(hb.procs[0, ref.PROC_FLAGS]), int(hb.procs[0, ref.PROC_START]), hb.bias_ids.tolist()))
        sch.complete(st, [3])
    up = ref.PROC_UPDATE
    assert seen == [(up, 0, [5]), (up, 4, []), (up | ref.PROC_SAMPLE, 8, [])]


# ------------------------------------------------------------------ state rows in the scheduler
def _asking(prompt, n=8, **kw):
    return Sequence(prompt, SamplingParams(max_new_tokens=n, presence_penalty=0.5, **kw), eos_token_id=42)


def test_released_state_row_waits_for_the_steps_in_flight():
    """A lookahead step in flight still names the row of a sequence that EOS finished one step
    earlier (its throw-away row counts a token into the state row).  The row is handed to a new
    request only after every step issued before the release has completed."""
    bm = make_block_manager(64, 4)
    sch = Scheduler(bm, num_slots=2, max_batch=8, max_prefill_tokens=64, max_seq_len=64, state_rows=2)
    a, b = _asking([1, 2, 3]), _asking([4, 5])
    sch.add(a)
    sch.add(b)
    pa, pb = sch.schedule(0), sch.schedule(1)               # an even share: a on slot 0, b on slot 1
    assert pa.seqs == [a] and pb.seqs == [b] and sorted([a.state_row, b.state_row]) == [0, 1]
    row_a = a.state_row
    sch.complete(pa, [7], 0.0)
    sch.complete(pb, [8], 0.0)
    st1 = sch.schedule(0)
    st2 = sch.schedule_lookahead(0)                         # issued before st1's tokens are known
    hb2 = build_host_batch(st2, bm, 4, sch.max_blocks)
    assert hb2.procs[:, ref.PROC_ROW].tolist() == [row_a]
    assert sch.complete(st1, np.array([42], np.int32), 0.0) == [a]                   # a: EOS, its row released
    assert a.state_row == -1
    c = _asking([6, 6, 6])
    sch.add(c)
    # st2 is still in flight and names a's old row: c must not get it -- and there is no other
    assert sch.schedule(0) is None and c.state_row == -1 and c in sch.waiting
    stb = sch.schedule(1)                                   # the other slot's stream goes on meanwhile
    assert not stb.is_prefill and c.state_row == -1
    sch.complete(st2, np.array([5], np.int32), 0.0)         # the throw-away row's step completes; stb, issued
    st3 = sch.schedule(0)                                   # after the release, cannot name the row
    assert st3 is not None and st3.seqs == [c] and c.state_row == row_a
    # abort releases too, and a request that does not ask never takes a row
    plain = Sequence([1], SamplingParams(max_new_tokens=2))
    sch.add(plain)
    assert sch.abort(b.seq_id) and b.state_row == -1 and plain.state_row == -1


def test_state_rows_default_and_preemption_keeps_the_row():
    bm = make_block_manager(64, 4)
    assert Scheduler(bm, num_slots=3, max_batch=16).state_rows == 3 * 18
    with pytest.raises(ValueError):
        Scheduler(bm, max_seq_len=1 << 24)
    eng = _engine(num_kv_blocks=4, kv_block_size=16, max_batch=2)
    seqs = [eng.add_request(p, SamplingParams(max_new_tokens=24, ignore_eos=True, frequency_penalty=0.5))
            for p in ([1, 5, 9, 200, 7, 3, 2], [3, 4, 7, 11, 12, 13, 14])]
    rows = set()
    while eng.has_work():
        eng.step()
        rows |= {(s.seq_id, s.state_row) for s in seqs if s.state_row >= 0}
    assert eng.scheduler.num_preemptions >= 1 and len(rows) == 2           # one row each, kept throughout
    assert all(s.state_row == -1 for s in seqs) and eng.scheduler._rows_held == 0


# ------------------------------------------------------------------ CPU engine against a stateless oracle
PROMPTS = [[1, 5, 9, 200, 5, 5], [3, 4, 7], list(range(10, 40)), [8] * 13, [2, 2, 9, 9, 4], [30, 31, 32, 33]]
N_NEW = 12


def _engine(**kw):
    cfg = dict(model="synthetic:tiny-llama", device="cpu", dtype="float32", max_batch=8, max_seq_len=128,
               use_graphs=False, num_kv_blocks=128)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg))


def _mixed_params(eos):
    """Plain requests beside asking ones: every rule alone and all together."""
    mk = lambda **k: SamplingParams(max_new_tokens=N_NEW, **k)      # noqa: E731
    return [mk(repetition_penalty=1.8), mk(), mk(presence_penalty=1.5, frequency_penalty=0.9),
            mk(repetition_penalty=0.6, presence_penalty=-1.0, frequency_penalty=1.1, min_tokens=7,
               logit_bias={eos: 3.0, 17: 2.5, 300: -100.0}),
            mk(ignore_eos=True), mk(logit_bias={40: 4.0, 41: 3.9, 42: 3.8}, frequency_penalty=2.0)]


def _rerun_logits(eng, tokens):
    """Logits at the last position of a plain prefill of ``tokens`` (float32 [V])."""
    seq = eng.add_request(tokens, SamplingParams(max_new_tokens=1))
    st = eng.scheduler.schedule(0)
    logits = eng.runner.execute(build_host_batch(st, eng.bm, eng.ecfg.kv_block_size))[0].float().numpy().copy()
    eng.scheduler.complete(st, [0])
    assert seq.finished
    return logits


def _oracle(prompt, p: SamplingParams, eos):
    """Greedy generation, stateless: every step recomputes the counts from the full token lists and
    applies the issue's chain in numpy float32 to a fresh prefill's logits."""
    eng = _engine()
    out = []
    while len(out) < p.max_new_tokens:
        x = _rerun_logits(eng, prompt + out).astype(np.float32)
        n_out = collections.Counter(out)
        seen = set(prompt) | set(out)
        bias = p.logit_bias or {}
        for t in sorted(seen | set(bias) | {eos}):
            y = x[t]
            if t in seen and p.repetition_penalty != 1.0:
                y = y / f32(p.repetition_penalty) if y > 0 else y * f32(p.repetition_penalty)
            if n_out[t] > 0:
                y = f32(y - f32(f32(p.frequency_penalty) * f32(n_out[t])))
                y = f32(y - f32(p.presence_penalty))
            if t in bias:
                y = f32(y + f32(bias[t]))
            if t == eos and len(out) < p.min_tokens:
                y = f32(NINF)
            x[t] = y
        out.append(int(np.argmax(x)))
        if out[-1] == eos and not p.ignore_eos:
            break
    return out


@pytest.fixture(scope="module")
def oracle_run():
    eos = _engine().mcfg.eos_token_id
    params = _mixed_params(eos)
    return params, [_oracle(pr, q, eos) for pr, q in zip(PROMPTS, params)]


@pytest.mark.parametrize("cfg", [dict(), dict(max_prefill_tokens=8, mixed_prefill_tokens=0),
                                 dict(max_prefill_tokens=16, mixed_prefill_tokens=8, max_batch=3),
                                 dict(num_kv_blocks=5, kv_block_size=16, max_batch=3)],
                         ids=["plain", "chunked", "mixed", "preemption"])
def test_engine_matches_the_stateless_oracle(oracle_run, cfg):
    params, expected = oracle_run
    eng = _engine(**cfg)
    seqs = [eng.add_request(p, q) for p, q in zip(PROMPTS, params)]
    eng.run_until_done()
    assert [s.output for s in seqs] == expected
    if "num_kv_blocks" in cfg:
        assert eng.scheduler.num_preemptions >= 1
    if cfg.get("mixed_prefill_tokens"):
        assert eng.scheduler.num_mixed >= 1
    assert eng.scheduler._rows_held == 0 and eng.logit_state.allocated


def test_oracle_run_exercises_the_rules(oracle_run):
    """The expectation is not vacuous: the asking requests' tokens differ from a plain run's."""
    params, expected = oracle_run
    eng = _engine()
    plain = eng.generate(PROMPTS, [SamplingParams(max_new_tokens=N_NEW, ignore_eos=q.ignore_eos) for q in params])
    assert not eng.logit_state.allocated                    # nobody asked: no device state at all
    differ = [a != b for a, b in zip(plain, expected)]
    assert differ == [True, False, True, True, False, True], differ


def test_no_asking_request_never_calls_the_ops(monkeypatch):
    calls = []
    for name in ("logit_state_update", "apply_logit_processors", "logit_state_count"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _r=real, _n=name, **k: calls.append(_n) or _r(*a, **k))
    eng = _engine()
    eng.generate(PROMPTS[:3], SamplingParams(max_new_tokens=4))
    assert not calls and not eng.logit_state.allocated
    eng.generate(PROMPTS[:1], SamplingParams(max_new_tokens=3, presence_penalty=1.0))
    assert calls.count("logit_state_update") == 1 and calls.count("apply_logit_processors") == 3
    assert calls.count("logit_state_count") == 3


def test_crisp_end_to_end_cases():
    eng = _engine()
    eos = eng.mcfg.eos_token_id
    assert eng.generate([[1, 2, 3]], SamplingParams(max_new_tokens=9, logit_bias={77: 100}))[0] == [77] * 9
    s = eng.add_request([1, 2, 3], SamplingParams(max_new_tokens=20, logit_bias={eos: 100}, min_tokens=5))
    eng.run_until_done()
    assert len(s.output) == 6 and s.output[-1] == eos and eos not in s.output[:5] and s.finish_reason == "eos"
    plain = eng.generate([[1, 2, 3]], SamplingParams(max_new_tokens=10, ignore_eos=True))[0]
    banned = plain[0]
    out = eng.generate([[1, 2, 3]], SamplingParams(max_new_tokens=10, ignore_eos=True, logit_bias={banned: -100}))[0]
    assert banned in plain and banned not in out
    # logprobs report the processed distribution: the forced token has probability ~1
    s = eng.add_request([1, 2, 3], SamplingParams(max_new_tokens=3, logit_bias={77: 100}, logprobs=1))
    eng.run_until_done()
    assert all(ti == [77] and c == pytest.approx(0.0, abs=1e-6) for c, ti, _ in s.logprobs)


def test_sampled_requests_see_the_processed_logits():
    """A seeded request with a -100 bias on everything it would otherwise draw never draws it."""
    eng = _engine()
    base = eng.generate([[4, 5, 6]], SamplingParams(max_new_tokens=12, temperature=1.0, seed=5, ignore_eos=True))[0]
    ban = {t: -100.0 for t in set(base)}
    out = eng.generate([[4, 5, 6]], SamplingParams(max_new_tokens=12, temperature=1.0, seed=5, ignore_eos=True,
                                                   logit_bias=ban))[0]
    assert not set(out) & set(base)


# ------------------------------------------------------------------ pipelines
PP_PROMPTS = [[i + 1, i + 5, 7, 9, 3 * i + 2] for i in range(6)]
PP_PARAMS = [SamplingParams(max_new_tokens=8, ignore_eos=True, **k)
             for k in (dict(repetition_penalty=1.7), dict(), dict(presence_penalty=1.0, frequency_penalty=0.7),
                       dict(logit_bias={11: 5.0, 12: 4.5}, frequency_penalty=1.5), dict(),
                       dict(repetition_penalty=0.7, min_tokens=4, logit_bias={3: -100.0}))]


def _pp_ecfg(**kw):
    d = dict(model="tiny-llama", dtype="float32", device="cpu", max_batch=4, max_seq_len=128, use_graphs=False,
             num_kv_blocks=256)
    d.update(kw)
    return EngineConfig(**d)


@pytest.fixture(scope="module")
def pp_expected():
    eng = LLMEngine(_pp_ecfg())
    plain = eng.generate(PP_PROMPTS, SamplingParams(max_new_tokens=8, ignore_eos=True))
    got = eng.generate(PP_PROMPTS, PP_PARAMS)
    assert [a != b for a, b in zip(plain, got)] == [q.has_processors for q in PP_PARAMS]
    return got


def test_loopback_pipeline_matches_single(pp_expected):
    from distributed_llms_amd.parallel.pipeline import run_loopback_pipeline
    outs, drv, _ = run_loopback_pipeline(_pp_ecfg(), 2, PP_PROMPTS, PP_PARAMS)
    assert outs == pp_expected and drv.scheduler._rows_held == 0


def _rank_main(rank, world, pp, port, out_q):
    import os
    import traceback
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from distributed_llms_amd.parallel.dist_engine import RankRole, init_distributed
    try:
        ctx = init_distributed(pp=pp, backend="gloo")
        role = RankRole(ctx, _pp_ecfg(num_workers=pp))
        seqs = [role.add_request(p, q) for p, q in zip(PP_PROMPTS, PP_PARAMS)] if role.is_driver else []
        role.run_round()
        role.shutdown()
        dist.barrier()
        out_q.put((rank, [s.output for s in seqs] if role.is_driver else None, None))
        dist.destroy_process_group()
    except Exception:      # noqa: BLE001 - reported to the test
        out_q.put((rank, None, traceback.format_exc()))
        raise


@pytest.mark.slow
def test_two_stage_gloo_pipeline_matches_single(pp_expected):
    import socket

    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(2):
            r, res, err = q.get(timeout=240)
            assert err is None, f"rank {r} failed:\n{err}"
            results[r] = res
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    assert results[0] == pp_expected


# ------------------------------------------------------------------ HTTP and master
def test_http_sampling_parses_and_refuses():
    from distributed_llms_amd.master import http_api
    body = {"repetition_penalty": 1.2, "presence_penalty": -0.5, "frequency_penalty": 2, "min_tokens": 3,
            "logit_bias": {"50": 10, "7": -100}, "max_tokens": 9, "stream": True, "stop": "x"}
    p = http_api._sampling(body, default_max=16, max_key="max_tokens", vocab_size=512)
    assert p == {"repetition_penalty": 1.2, "presence_penalty": -0.5, "frequency_penalty": 2.0, "min_tokens": 3,
                 "logit_bias": {50: 10.0, 7: -100.0}, "max_new_tokens": 9}
    assert SamplingParams.from_dict(p).has_processors
    assert http_api._sampling({}) == {"max_new_tokens": 64}
    for bad in ({"presence_penalty": 2.5}, {"repetition_penalty": 0}, {"logit_bias": {"512": 1}}, {"logit_bias": {"a": 1}},
                {"logit_bias": {"1": 101}}, {"min_tokens": 65}, {"min_tokens": "2"}, {"frequency_penalty": "x"},
                {"logit_bias": 5}):
        with pytest.raises(ValueError):
            http_api._sampling(bad, vocab_size=512)


from test_master_worker import PROMPTS as MW_PROMPTS, _cfg as _mw_cfg, cluster  # noqa: E402,F401


@pytest.mark.slow
def test_http_processors_against_master_and_cpu_workers(cluster):  # noqa: F811
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

    def post(path, body, raw=False):
        req = urllib.request.Request(base + path, data=json.dumps(body).encode(),
                                     headers={"Content-Type": "application/json"})
        with urllib.request.urlopen(req, timeout=120) as r:
            data = r.read()
            return data.decode() if raw else json.loads(data)

    try:
        eng = LLMEngine(_mw_cfg(model))
        kw = dict(repetition_penalty=1.6, presence_penalty=0.8, frequency_penalty=0.4, min_tokens=2)
        bias = {11: 6.0, 300: -100.0}
        exp = eng.generate([MW_PROMPTS[0]], SamplingParams(max_new_tokens=6, ignore_eos=True, logit_bias=bias, **kw))[0]
        plain = eng.generate([MW_PROMPTS[0]], SamplingParams(max_new_tokens=6, ignore_eos=True))[0]
        assert exp != plain
        wire_bias = {str(k): v for k, v in bias.items()}
        res = m.generate([MW_PROMPTS[0]], max_new_tokens=6, ignore_eos=True, logit_bias=bias, timeout=120, **kw)[0]
        assert res["tokens"] == exp
        g = post("/generate", dict(kw, prompt_ids=MW_PROMPTS[0], max_new_tokens=6, ignore_eos=True, logit_bias=wire_bias))
        assert g["tokens"] == exp
        c = post("/v1/completions", dict(kw, prompt=MW_PROMPTS[0], max_tokens=6, ignore_eos=True, logit_bias=wire_bias))
        assert c["choices"][0]["tokens"] == exp
        forced = post("/v1/completions", {"prompt": MW_PROMPTS[0], "max_tokens": 4, "logit_bias": {"77": 100}})
        assert forced["choices"][0]["tokens"] == [77] * 4
        sse = post("/v1/completions", dict(kw, prompt=MW_PROMPTS[0], max_tokens=6, ignore_eos=True, logit_bias=wire_bias,
                                           stream=True), raw=True)
        events = [json.loads(l[6:]) for l in sse.splitlines() if l.startswith("data: {")]
        assert sum((e["choices"][0]["tokens"] for e in events), []) == exp and sse.rstrip().endswith("data: [DONE]")
        assert post("/generate", {"prompt_ids": MW_PROMPTS[0], "max_new_tokens": 6, "ignore_eos": True})["tokens"] == plain
        for body in ({"presence_penalty": 3}, {"repetition_penalty": -1}, {"logit_bias": {"999999": 1}},
                     {"logit_bias": {"1": 1000}}, {"min_tokens": 999}, {"frequency_penalty": 2.5, "stream": True}):
            for path in ("/v1/completions", "/generate"):
                req = urllib.request.Request(base + path, data=json.dumps(dict(body, prompt=MW_PROMPTS[0],
                                                                              prompt_ids=MW_PROMPTS[0])).encode())
                with pytest.raises(urllib.error.HTTPError) as ei:
                    urllib.request.urlopen(req, timeout=30)
                assert ei.value.code == 400, (path, body)
    finally:
        srv.shutdown()
