"""Seeded sampling on the CPU: the Philox draw, the contract of ops/reference.py sample_rows on
hand-built rows, the seeds' way through the batch wire format and the native batcher, and the
engine's reproducibility (tiny llama, fp32)."""
import numpy as np
import pytest
import torch

import sampler_cases as sc
from distributed_llms_amd import _ext
from distributed_llms_amd.config import EngineConfig
from distributed_llms_amd.engine.batch import HostBatch, build_host_batch, merge_mixed
from distributed_llms_amd.engine.llm_engine import LLMEngine, make_block_manager
from distributed_llms_amd.engine.sampler import sample
from distributed_llms_amd.engine.scheduler import Scheduler, Step
from distributed_llms_amd.engine.sequence import SamplingParams, Sequence, request_seed, split_seed
from distributed_llms_amd.ops import reference as ref


# ------------------------------------------------------------------ the draw
def _philox4x32_10(ctr, key):
    """From the specification (Salmon et al., SC'11): ten rounds, the key bumped between rounds."""
    c, k = [int(x) for x in ctr], [int(x) for x in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    assert tuple(_philox4x32_10(ctr, key)) == want
    assert tuple(int(x) for x in ref.philox4x32_10(ctr, key)) == want


def test_reference_draws_u_from_philox_of_seed_and_position():
    seeds = np.array([0, 1, -1, 0x0123456789ABCDEF, -0x7000000000000001], dtype=np.int64)
    pos = np.array([0, 7, 4095, 2 ** 31 - 1, 12], dtype=np.int32)
    u = ref.sample_uniforms(seeds, pos)
    for s, p, got in zip(seeds.tolist(), pos.tolist(), u.tolist()):
        s &= (1 << 64) - 1
        want = (_philox4x32_10((p, 0, 0, 0), (s & 0xFFFFFFFF, s >> 32))[0] >> 8) * 2.0 ** -24
        assert got == want and 0.0 <= got < 1.0


# ------------------------------------------------------------------ contract on hand-built rows
def _ref(rows, params, uniforms):
    b = len(rows)
    return ref.sample_rows(torch.tensor(rows, dtype=torch.float32), torch.tensor(params, dtype=torch.int32),
                           torch.zeros(b, dtype=torch.int64), torch.zeros(b, dtype=torch.int32),
                           torch.tensor(uniforms, dtype=torch.float32)).tolist()


def _kept(row, params):
    return np.nonzero(ref.sample_rows_detail(np.array([row]), np.array([params]), np.array([0.5]))[1][0])[0].tolist()


U_LAST = 1.0 - 2.0 ** -24
NINF, NAN = float("-inf"), float("nan")


def test_ties_across_the_top_k_threshold_are_all_kept():
    row = [1.0, 5.0, 3.0, 3.0, 0.0, 3.0, 7.0]
    assert _kept(row, (10000, 3, 10000)) == [1, 2, 3, 5, 6]        # the 3rd largest is 3.0: all three 3.0s
    assert _kept(row, (10000, 2, 10000)) == [1, 6]
    assert _kept(row, (10000, 7, 10000)) == _kept(row, (10000, 0, 10000)) == list(range(7))   # k >= V: off
    assert _ref([row] * 2, [(10000, 3, 10000)] * 2, [0.0, U_LAST]) == [1, 6]


def test_top_p_keeps_whole_value_groups():
    # masses 4 : 2 : 2 : 1 : 1 (T = 1 / ln 2 would be exact; use logs of the masses instead)
    row = np.log(np.array([1.0, 2.0, 4.0, 2.0, 1.0])).tolist()
    t = (10000, 0)
    assert _kept(row, t + (1,)) == [2]                   # a tiny p: the maximal group only
    assert _kept(row, t + (3900,)) == [2]                # mass above 2.0 is 0.4 > 0.39
    assert _kept(row, t + (4100,)) == [1, 2, 3]          # 0.4 <= 0.41: the whole 2.0 group
    assert _kept(row, t + (7900,)) == [1, 2, 3]          # mass above 1.0 is 0.8 > 0.79
    assert _kept(row, t + (8100,)) == [0, 1, 2, 3, 4]
    assert _kept(row, t + (10000,)) == [0, 1, 2, 3, 4]
    # top-p acts on the top-k survivors: with k = 1 the group of 4.0 is everything, p = 0.5 of it
    assert _kept(row, (10000, 1, 5000)) == [2]
    # k = 3 keeps {4, 2, 2} (Z_k = 8): mass above 2.0 is 4 = 0.5 * 8, kept at p = 0.5, not at 0.49
    assert _kept(row, (10000, 3, 5000)) == [1, 2, 3]
    assert _kept(row, (10000, 3, 4900)) == [2]


def test_greedy_rows_equal_argmax_and_bad_entries_are_never_drawn():
    rows = [[1.0, 9.0, 9.0, 2.0], [NINF, NINF, NINF, NINF], [NAN, NINF, 2.0, NAN], [NAN, NAN, NAN, NAN]]
    t = torch.tensor(rows)
    greedy = _ref(rows, [(0, 2, 5000)] * 4, [0.7] * 4)
    assert greedy == [1, 0, 2, 0]
    assert greedy[:2] == ref.argmax(t[:2]).tolist()
    assert _ref(rows, [(10000, 0, 10000)] * 4, [0.99] * 4) == [2, 0, 2, 0]     # all -inf / NaN rows: 0
    row = [NINF, 1.0, NAN, 2.0, NINF, 1.5, NAN]
    us = np.linspace(0.0, U_LAST, 257).tolist()
    got = set(_ref([row] * len(us), [(15000, 0, 10000)] * len(us), us))
    assert got == {1, 3, 5}
    assert _ref([row] * 2, [(15000, 0, 10000)] * 2, [0.0, U_LAST]) == [1, 5]    # first and last kept with mass


def test_u_zero_and_u_max_return_the_first_and_the_last_kept_index():
    g = torch.Generator().manual_seed(3)
    rows = torch.randn(4, 300, generator=g).mul(3).to(torch.bfloat16).float()
    params = [(7000, 5, 10000), (10000, 0, 9000), (20000, 40, 5000), (10000, 0, 10000)]
    lo = _ref(rows.tolist(), params, [0.0] * 4)
    hi = _ref(rows.tolist(), params, [U_LAST] * 4)
    for i in range(4):
        kept = _kept(rows[i].tolist(), params[i])
        assert lo[i] == kept[0] and hi[i] == kept[-1]


def test_sampler_with_seeds_takes_the_reference_on_the_cpu():
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(5, 97, generator=g) * 2
    seeds = np.array([split_seed(s) for s in (1, 2 ** 63 + 5, 3, 4, 2 ** 64 - 1)], dtype=np.int32)
    pos = np.array([3, 9, 27, 81, 243], dtype=np.int32)
    temps, ks, ps = [0.0, 0.7, 1.0, 2.0, 1.0], [0, 5, 0, 50, 1], [1.0, 0.9, 0.5, 1.0, 1.0]
    ids = sample(logits, temps, ks, ps, seeds=seeds, positions=pos)
    s64 = torch.tensor([1, 2 ** 63 + 5 - 2 ** 64, 3, 4, -1], dtype=torch.int64)
    par = torch.tensor([[0, 0, 10000], [7000, 5, 9000], [10000, 0, 5000], [20000, 50, 10000], [10000, 1, 10000]],
                       dtype=torch.int32)
    want = ref.sample_rows(logits, par, s64, torch.from_numpy(pos))
    assert ids.dtype == torch.int32 and ids.tolist() == want.tolist()
    assert ids[0].item() == logits[0].argmax().item() and ids[4].item() == logits[4].argmax().item()
    again = sample(logits, temps, ks, ps, seeds=seeds, positions=pos)
    assert again.tolist() == ids.tolist()


# ------------------------------------------------------------------ tolerance of the GPU test, measured here
def test_measured_float32_gap_and_the_widened_cap():
    """sampler_cases.MEASURED_GAP is the float32-vs-float64 mass gap of these very inputs, and the
    reference's own float32 form passes the acceptance rule the kernel is held to."""
    gap = 0.0
    for rows, vocab in sc.SHAPES:
        case = sc.make_case(rows, vocab)
        lg, pr = case["logits"].float().numpy(), case["params"].numpy()
        for i in range(lg.shape[0]):
            if pr[i, 0] > 0 and np.nanmax(lg[i]) > -np.inf:
                gap = max(gap, sc.mass_gap(lg[i], int(pr[i, 0])))
        u = ref.sample_uniforms(case["seeds"].numpy(), case["pos"].numpy())
        sc.check_ids(case, ref.sample_rows_detail(lg, pr, u, dtype=np.float32)[0])
        sc.check_ids(case, ref.sample_rows(case["logits"], case["params"], case["seeds"], case["pos"]).numpy())
    print(f"largest float32 mass gap {gap:.3e}")
    assert 0.5 * sc.MEASURED_GAP <= gap <= sc.MEASURED_GAP


def test_reference_distribution_passes_the_chi_square():
    n = sc.DIST_N
    ids = ref.sample_rows(sc.dist_row().expand(n, -1), torch.tensor([sc.DIST_PARAMS], dtype=torch.int32).expand(n, -1),
                          torch.full((n,), sc.DIST_SEED, dtype=torch.int64), torch.arange(n, dtype=torch.int32))
    chi2, dof = sc.check_distribution(ids.numpy())
    assert 3 <= dof <= 11
    # the critical value against the tabulated 99.9 % points
    for d, tab in ((3, 16.266), (4, 18.467), (7, 24.322), (10, 29.588), (11, 31.264)):
        assert abs(sc.chi2_critical_999(d) - tab) < 2e-3


# ------------------------------------------------------------------ wire format
def _hb(seeds=None, sampling=None, b=3):
    return HostBatch(False, np.arange(b, dtype=np.int32), np.arange(b, dtype=np.int32) + 4,
                     np.arange(b, dtype=np.int32) + 9, np.arange(b, dtype=np.int32) + 5,
                     np.arange(b + 1, dtype=np.int32), np.arange(b * 2, dtype=np.int32).reshape(b, 2),
                     np.arange(b, dtype=np.int32), 1, 7, 0, 11, sampling, sample_seeds=seeds)


def test_host_batch_round_trips_sample_seeds():
    samp = np.array([[7000, 40, 9000], [0, 0, 10000], [10000, 0, 10000]], dtype=np.int32)
    seeds = np.array([split_seed(s) for s in (0xDEADBEEFCAFEF00D, 0, 2 ** 64 - 1)], dtype=np.int32)
    hb = HostBatch.unpack(_hb(seeds, samp).pack())
    assert np.array_equal(hb.sample_seeds, seeds) and hb.sample_seeds.shape == (3, 2)
    assert np.array_equal(hb.sampling, samp) and hb.sampling.shape == (3, 3)
    args = hb.sampling_args()
    assert np.array_equal(args["seeds"], seeds) and np.array_equal(args["positions"], hb.seq_lens)
    assert args["top_k"] == [40, 0, 0]
    assert np.array_equal(HostBatch.unpack(hb.pack()).sample_seeds, seeds)      # the raw path


def test_a_batch_without_seeds_packs_to_the_bytes_it_always_did():
    samp = np.array([[7000, 40, 9000], [0, 0, 10000], [10000, 0, 10000]], dtype=np.int32)
    for s in (None, samp):
        hb = _hb(None, s)
        packed = hb.pack()
        hdr = [0, 3, 3, 2, 1, 7, 0, 11, 0 if s is None else 1, 0] + [0] * 6
        old = np.concatenate([np.array(hdr, np.int32), hb.ids, hb.positions, hb.slots, hb.seq_lens, hb.cu_seqlens,
                              hb.block_tables.reshape(-1), hb.logits_idx] + ([] if s is None else [s.reshape(-1)]))
        assert packed.dtype == np.int32 and packed.tobytes() == old.astype(np.int32).tobytes()
        un = HostBatch.unpack(packed)
        assert un.sample_seeds is None and "seeds" not in un.sampling_args()


def test_native_batcher_packs_the_admitted_seeds():
    bm = _ext.runtime().BlockManager(64, 4)
    sb = _ext.runtime().SlotBatcher(bm, 1, 64)
    want = {}
    for sid, (temp, seed) in enumerate([(0, 0), (7000, 0xDEADBEEFCAFEF00D), (10000, 5)], start=1):
        assert bm.ensure_capacity(sid, 6)
        lo, hi = split_seed(seed)
        sb.admit(0, sid, 6, 1, 10, -1, temp, 40, 9000, seed_lo=lo, seed_hi=hi)
        want[sid] = [lo, hi]
    packed, rows, _ = sb.build_decode(0, 16, 0, False)
    hb = HostBatch.unpack(packed)
    assert packed[10] == 1 and hb.sampling.shape == (3, 3)
    assert hb.sample_seeds.tolist() == [want[int(r)] for r in rows]
    sb.complete(0, rows, np.array([3, 4, 5], dtype=np.int32), 0.0)
    look = sb.build_decode(0, 16, 1, False)
    packed2, rows2, _ = look
    sb_l = sb.build_decode(0, 16, 2, True)                     # lookahead: the step after packed2
    assert sb_l is not None
    hl = HostBatch.unpack(sb_l[0])
    assert hl.sample_seeds.tolist() == [want[int(r)] for r in sb_l[1]]
    assert hl.seq_lens.tolist() == (HostBatch.unpack(packed2).seq_lens + 1).tolist()
    # an all-greedy slot packs no sampling block and no seeds
    bm2 = _ext.runtime().BlockManager(16, 4)
    sb2 = _ext.runtime().SlotBatcher(bm2, 1, 64)
    assert bm2.ensure_capacity(1, 6)
    sb2.admit(0, 1, 6, 1, 10)
    g = HostBatch.unpack(sb2.build_decode(0, 4, 0, False)[0])
    assert g.sampling is None and g.sample_seeds is None


def test_mixed_step_merges_the_seeds():
    bm = make_block_manager(64, 4)
    sch = Scheduler(bm, num_slots=1, max_batch=8, max_prefill_tokens=64, max_seq_len=64, mixed_prefill_tokens=16)
    sp = SamplingParams(max_new_tokens=8, ignore_eos=True, temperature=0.8, top_k=5)
    first = Sequence([1, 2, 3, 4, 5], sp)
    first.seed = 0xABCDEF0123456789
    sch.add(first)
    st = sch.schedule(0)
    hb = build_host_batch(st, bm, 4)
    assert hb.sample_seeds.tolist() == [list(split_seed(first.seed))] and hb.seq_lens.tolist() == [5]
    sch.complete(st, [7])
    late = Sequence([9, 8, 7], SamplingParams(max_new_tokens=8, ignore_eos=True))        # greedy
    late2 = Sequence([6, 5], SamplingParams(max_new_tokens=8, ignore_eos=True, temperature=1.0))
    late2.seed = 42
    sch.add(late)
    sch.add(late2)
    st = sch.schedule(0)
    assert st.mixed
    hb = build_host_batch(st, bm, 4)
    assert hb.num_decode == 1 and hb.sampling.shape == (3, 3)
    assert hb.sample_seeds.tolist() == [list(split_seed(first.seed)), [0, 0], [42, 0]]
    assert hb.sampling_args()["positions"].tolist() == [6, 3, 2]
    # decode rows greedy, prefill rows sampled: the decode side contributes zero seeds
    dec = _hb(None, None, b=2)
    lone, bm2 = Sequence([1, 2], sp), make_block_manager(16, 4)
    assert bm2.ensure_capacity(lone.seq_id, 2)
    pre = build_host_batch(Step(True, [lone], 0), bm2, 4)
    both = merge_mixed(dec, pre, 0, 0)
    assert both.sample_seeds.shape == (3, 2) and both.sample_seeds[:2].tolist() == [[0, 0], [0, 0]]


def test_step_sampling_args_agree_with_the_host_batch():
    """Whole-prompt prefill, a chunk of a long prompt, and decode rows."""
    from distributed_llms_amd.engine.sampler import step_sampling_args
    bm = make_block_manager(64, 4)
    sp = SamplingParams(max_new_tokens=8, ignore_eos=True, temperature=0.8, top_k=5, top_p=0.9)
    whole, long_, greedy = Sequence([1, 2, 3, 4, 5], sp), Sequence(list(range(1, 20)), sp), Sequence([7, 8], SamplingParams())
    whole.seed, long_.seed = 0xABCDEF0123456789, 77
    long_.num_cached, long_.chunk = 8, 6                     # computes tokens 8..13 of 19
    seqs = [whole, long_, greedy]
    for s in seqs:
        assert bm.ensure_capacity(s.seq_id, s.num_cached + s.prefill_len)

    def same(step):
        a, b = step_sampling_args(seqs), build_host_batch(step, bm, 4).sampling_args()
        assert sorted(a) == sorted(b) == ["positions", "seeds", "temperatures", "top_k", "top_p"]
        assert np.array_equal(a["seeds"], b["seeds"]) and a["positions"].tolist() == b["positions"].tolist()
        assert a["top_k"] == b["top_k"] and a["temperatures"] == pytest.approx(b["temperatures"])
        assert a["top_p"] == pytest.approx(b["top_p"])
        return a["positions"].tolist()

    assert same(Step(True, seqs, 0)) == [5, 14, 2]
    for s in seqs:                                          # now decode rows with some output
        s.num_cached, s.chunk = s.total_len, 0
        s.output += [3, 4]
        assert bm.ensure_capacity(s.seq_id, s.total_len)
    assert same(Step(False, seqs, 0)) == [7, 21, 4]
    assert step_sampling_args([greedy]) == {}


def test_request_seed_rules():
    import random
    rng = random.Random(1)
    assert request_seed(SamplingParams(temperature=0.0, seed=9), rng) == 0
    assert request_seed(SamplingParams(temperature=0.5, seed=2 ** 64 + 9), rng) == 9
    assert request_seed(SamplingParams(temperature=0.5, seed=-1), rng) == 2 ** 64 - 1
    a, b = (request_seed(SamplingParams(temperature=0.5), rng) for _ in range(2))
    assert a != b and 0 <= a < 2 ** 64
    for s in (0, 1, 2 ** 31, 2 ** 32 - 1, 2 ** 63, 2 ** 64 - 1):
        lo, hi = split_seed(s)
        assert -2 ** 31 <= lo < 2 ** 31 and -2 ** 31 <= hi < 2 ** 31
        assert (lo & 0xFFFFFFFF) | ((hi & 0xFFFFFFFF) << 32) == s


# ------------------------------------------------------------------ engine
PROMPTS = [[1, 5, 9, 200], [3, 4, 7], list(range(10, 40)), [8] * 13, [9, 9, 9], [2, 3]]


def _engine(**kw):
    cfg = dict(model="synthetic:tiny-llama", device="cpu", dtype="float32", max_batch=8, max_seq_len=128,
               use_graphs=False, num_kv_blocks=128)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg))


def _params(seeds, n=10):
    return [SamplingParams(max_new_tokens=n, ignore_eos=True, temperature=0.9, top_k=50, top_p=0.95, seed=s)
            for s in seeds]


def test_engine_same_seeds_same_outputs_other_seeds_other_outputs():
    seeds = [100 + i for i in range(len(PROMPTS))]
    a = _engine().generate(PROMPTS, _params(seeds))
    b = _engine().generate(PROMPTS, _params(seeds))
    assert a == b
    c = _engine().generate(PROMPTS, _params([s + 1000 for s in seeds]))
    assert all(x != y for x, y in zip(a, c))
    # a request's tokens do not depend on the batch it sits in
    alone = _engine().generate(PROMPTS[2:3], _params(seeds[2:3]))
    assert alone[0] == a[2]


def test_engine_unseeded_sampled_requests_differ():
    eng = _engine()
    sp = SamplingParams(max_new_tokens=10, ignore_eos=True, temperature=1.0)
    s1, s2 = eng.add_request(PROMPTS[2], sp), eng.add_request(PROMPTS[2], sp)
    eng.run_until_done()
    assert s1.seed != s2.seed and s1.output != s2.output
    g = eng.add_request(PROMPTS[2], SamplingParams(max_new_tokens=4))
    assert g.seed == 0


def test_engine_preempted_sampled_request_reproduces_its_uninterrupted_run():
    """A pool too small for both sequences' full length: the younger one is preempted in decode and
    recomputed from its prompt plus the tokens it already drew; token n is Philox(seed, n) again."""
    prompts = [[1, 5, 9, 200, 7, 3, 2], [3, 4, 7, 11, 12, 13, 14]]
    params = _params([7, 8], n=24)
    calm = _engine(num_kv_blocks=128, kv_block_size=16)
    want = calm.generate(prompts, params)
    assert calm.scheduler.num_preemptions == 0
    tight = _engine(num_kv_blocks=4, kv_block_size=16)          # 3 usable blocks; the two need 2 each from token 17 on
    got = tight.generate(prompts, params)
    assert tight.scheduler.num_preemptions >= 1
    assert got == want
