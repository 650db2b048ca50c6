"""Automatic prefix caching on the CPU: the native block manager's reference counts, content index and
LRU eviction; the scheduler's admission with a cached prefix and its pending-key rule for requests of
one burst; engines and pipelines with the cache on against the cache off (tiny-llama, float32: the
same tokens); "n" completions and the cache counters through the HTTP front end."""
import json
import os
import socket
import urllib.error
import urllib.request

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from distributed_llms_amd import _ext
from distributed_llms_amd.config import EngineConfig
from distributed_llms_amd.engine.graphs import SCRATCH_SEQ_ID
from distributed_llms_amd.engine.llm_engine import LLMEngine, make_block_manager
from distributed_llms_amd.engine.scheduler import Scheduler
from distributed_llms_amd.engine.sequence import SamplingParams, Sequence, SeqStatus


def _bm(nb=16, bs=4, on=True):
    return make_block_manager(nb, bs, on)


def _i32(x):
    return np.asarray(x, dtype=np.int32)


def _fill(bm, seq, toks, register=True):
    """A sequence as the scheduler runs it: take the cached prefix, allocate the rest, register."""
    hit = bm.acquire_prefix(seq, _i32(toks))
    assert bm.ensure_capacity(seq, len(toks))
    if register:
        bm.register_prefix(seq, _i32(toks), len(toks))
    return int(hit)


# ------------------------------------------------------------------ block manager
def test_cache_off_is_the_plain_free_list():
    off, ref = _bm(on=False), _ext.runtime().BlockManager(16, 4)
    assert ref.ensure_capacity(SCRATCH_SEQ_ID, 1)
    toks = list(range(13))
    for bm in (off, ref):
        assert not bm.prefix_caching and bm.acquire_prefix(1, _i32(toks)) == 0 and not bm.has_sequence(1)
        assert bm.ensure_capacity(1, 13) and bm.register_prefix(1, _i32(toks), 13) == 0
        assert bm.ensure_capacity(2, 5)
        bm.free_sequence(1)
        assert bm.ensure_capacity(3, 9)
    for s in (1, 2, 3):
        assert off.has_sequence(s) == ref.has_sequence(s)
    assert off.block_table(2) == ref.block_table(2) and off.block_table(3) == ref.block_table(3)   # same order
    assert off.num_free() == ref.num_free() and tuple(off.prefix_stats()) == (0, 0, 0, 0)


def test_reference_counts_and_shared_frees():
    bm = _bm()
    toks = list(range(13))                                  # 3 full blocks + 1 token
    assert _fill(bm, 1, toks) == 0
    t1 = bm.block_table(1)
    assert [bm.ref_count(b) for b in t1] == [1, 1, 1, 1]
    assert [bm.is_registered(b) for b in t1] == [True, True, True, False]      # only full blocks
    assert _fill(bm, 2, toks) == 12
    t2 = bm.block_table(2)
    assert t2[:3] == t1[:3] and t2[3] != t1[3]               # the last token's block is private
    assert [bm.ref_count(b) for b in t1] == [2, 2, 2, 1]
    free0 = bm.num_free()
    bm.free_sequence(1)
    assert [bm.ref_count(b) for b in t1[:3]] == [1, 1, 1] and bm.num_free() == free0 + 1
    assert bm.evictable_blocks() == []                       # still referenced by sequence 2
    bm.free_sequence(2)
    assert bm.evictable_blocks() == t1[2::-1]                # deepest first: leaves before the root
    assert bm.num_free() == 15 and bm.num_evictable() == 3   # evictable blocks count as free
    assert bm.can_fit(9, 15 * 4) and not bm.can_fit(9, 15 * 4 + 1)
    q, h, e, r = bm.prefix_stats()
    assert (q, h, e, r) == (26, 12, 0, 3)


def test_free_list_before_eviction_and_lru_order():
    bm = _bm(nb=8)                                           # blocks 1..7 usable
    a, b = [1] * 8 + [9], [2] * 4 + [9]                      # chains of 2 and 1 blocks
    _fill(bm, 1, a)
    _fill(bm, 2, b)
    ta, tb = bm.block_table(1), bm.block_table(2)
    bm.free_sequence(1)
    bm.free_sequence(2)
    assert bm.evictable_blocks() == [ta[1], ta[0], tb[0]]    # a's leaf, a's root, then b
    assert len(bm.free_blocks()) == 4 and bm.num_free() == 7
    assert bm.ensure_capacity(3, 16)                         # four blocks: all from the free list
    assert bm.prefix_stats()[2] == 0 and bm.num_evictable() == 3
    assert bm.match_prefix(_i32(a)) == 2
    assert bm.ensure_capacity(4, 4)                          # one more: evicts the LRU head, a's leaf
    assert bm.block_table(4) == [ta[1]] and not bm.is_registered(ta[1])
    assert bm.match_prefix(_i32(a)) == 1 and bm.match_prefix(_i32(b)) == 1
    assert bm.ensure_capacity(4, 8) and bm.block_table(4)[1] == ta[0]          # then a's root
    assert bm.match_prefix(_i32(a)) == 0 and bm.prefix_stats()[2:] == (2, 1)
    assert not bm.ensure_capacity(6, 8) and bm.num_free() == 1                 # all-or-nothing
    # a hit takes a chain off the list, and its release puts it at the tail again
    bm.free_sequence(3)
    c = [3] * 4 + [9]
    _fill(bm, 7, c)
    tc = bm.block_table(7)
    bm.free_sequence(7)
    assert bm.evictable_blocks() == [tb[0], tc[0]]
    _fill(bm, 5, b)
    assert bm.evictable_blocks()[-1] != tb[0] and tb[0] not in bm.evictable_blocks()
    bm.free_sequence(5)
    assert bm.evictable_blocks()[-1] == tb[0] and len(bm.evictable_blocks()) == 2


def test_duplicate_registration_keeps_the_older_block():
    bm = _bm()
    toks = list(range(9))
    bm.ensure_capacity(1, 9)
    bm.ensure_capacity(2, 9)                                 # computed the same prompt side by side
    assert bm.register_prefix(1, _i32(toks), 9) == 2
    assert bm.register_prefix(2, _i32(toks), 9) == 0
    t1, t2 = bm.block_table(1), bm.block_table(2)
    assert all(bm.is_registered(b) for b in t1[:2]) and not any(bm.is_registered(b) for b in t2)
    assert _fill(bm, 3, toks) == 8 and bm.block_table(3)[:2] == t1[:2]
    bm.free_sequence(2)
    assert set(t2) <= set(bm.free_blocks())                  # the newer copy was private: plain free
    assert bm.register_prefix(1, _i32(toks), 9) == 0         # registering again changes nothing
    assert bm.num_registered() == 2


def test_match_is_capped_below_the_last_token():
    bm = _bm(nb=64, bs=32)
    toks = list(range(100, 164))                             # exactly 64 tokens = 2 full blocks
    assert _fill(bm, 1, toks) == 0
    assert all(bm.is_registered(b) for b in bm.block_table(1))
    assert bm.acquire_prefix(2, _i32(toks)) == 32            # (64 - 1) // 32 = 1 block
    assert bm.acquire_prefix(3, _i32(toks + [7])) == 64
    assert bm.acquire_prefix(4, _i32(toks[:33])) == 32 and bm.acquire_prefix(5, _i32(toks[:32])) == 0
    assert bm.acquire_prefix(6, _i32([5])) == 0 and not bm.has_sequence(6)
    with pytest.raises(ValueError):
        bm.acquire_prefix(2, _i32(toks))                     # only for a sequence without a table


def test_block_zero_is_never_cached():
    bm = _bm()
    assert bm.block_table(SCRATCH_SEQ_ID) == [0]
    assert bm.register_prefix(SCRATCH_SEQ_ID, _i32([1, 2, 3, 4]), 4) == 0 and not bm.is_registered(0)
    with pytest.raises(ValueError):
        bm.acquire_prefix(SCRATCH_SEQ_ID, _i32(range(9)))
    for s in range(1, 4):
        _fill(bm, s, [s] * 9)
    for s in range(1, 4):
        bm.free_sequence(s)
    assert 0 not in bm.evictable_blocks() and 0 not in bm.free_blocks() and bm.ref_count(0) == 1
    raw = _ext.runtime().BlockManager(4, 4, True)            # no scratch sequence: block 0 goes to a sequence
    raw.ensure_capacity(1, 8)
    assert raw.block_table(1)[0] == 0 and raw.register_prefix(1, _i32(range(8)), 8) == 0


def test_forced_key_collision_does_not_match():
    """Every key masked to 0: all blocks share one bucket of the index, so only the stored parent link
    and the stored token ids tell them apart."""
    bm = _bm(nb=32)
    bm.set_hash_mask(0)
    a, b = [1, 2, 3, 4, 5, 6, 7, 8, 0], [1, 2, 3, 9, 5, 6, 7, 8, 0]
    c = [5, 6, 7, 8, 1, 2, 3, 4, 0]                          # a's blocks in the other order
    _fill(bm, 1, a)
    assert bm.match_prefix(_i32(a)) == 2
    assert bm.match_prefix(_i32(b)) == 0                     # first block differs in one token
    assert bm.match_prefix(_i32(c)) == 0                     # [5..8] is known, but not as a first block
    assert _fill(bm, 2, b) == 0 and _fill(bm, 3, c) == 0
    assert bm.num_registered() == 6                          # nothing was taken for a duplicate either
    assert bm.match_prefix(_i32(b)) == 2 and bm.match_prefix(_i32(c)) == 2
    assert _fill(bm, 4, a[:8] + [1, 2, 3, 9, 0]) == 8        # a's chain, then a new third block
    assert bm.block_table(4)[:2] == bm.block_table(1)[:2]
    assert len({tuple(bm.block_table(s)[:2]) for s in (1, 2, 3)}) == 3
    with pytest.raises(RuntimeError):
        bm.set_hash_mask(1)                                  # not once blocks are registered


class _Model:
    """The manager's contract in plain Python (cache on)."""

    def __init__(self, nb, bs):
        self.bs, self.free, self.lru = bs, list(range(nb - 1, -1, -1)), []
        self.ref, self.tables, self.reg, self.info, self.uid = [0] * nb, {}, {}, {}, 0
        self.query = self.hit = self.evictions = 0

    def num_free(self):
        return len(self.free) + len(self.lru)

    def _take(self):
        if self.free:
            b = self.free.pop()
        else:
            b = self.lru.pop(0)
            del self.reg[self.info.pop(b)[1]]
            self.evictions += 1
        self.ref[b] = 1
        return b

    def ensure(self, seq, tokens):
        need = max(0, -(-tokens // self.bs) - len(self.tables.get(seq, ())))
        if need > self.num_free():
            return False
        t = self.tables.setdefault(seq, [])
        t.extend(self._take() for _ in range(need))
        return True

    def free_seq(self, seq):
        for b in reversed(self.tables.pop(seq, [])):
            self.ref[b] -= 1
            if self.ref[b] == 0:
                (self.lru if b in self.info else self.free).append(b)

    def _blocks(self, toks, n):
        return [tuple(toks[i * self.bs:(i + 1) * self.bs]) for i in range(n)]

    def acquire(self, seq, toks):
        chain, parent = [], 0
        for tk in self._blocks(toks, (len(toks) - 1) // self.bs):
            b = self.reg.get((parent, tk))
            if b is None:
                break
            chain.append(b)
            parent = self.info[b][0]
        self.query += len(toks)
        if not chain:
            return 0
        for b in chain:
            if self.ref[b] == 0:
                self.lru.remove(b)
            self.ref[b] += 1
        self.tables[seq] = chain
        self.hit += len(chain) * self.bs
        return len(chain) * self.bs

    def register(self, seq, toks, n):
        tab, parent = self.tables[seq], 0
        for i, tk in enumerate(self._blocks(toks, min(n // self.bs, len(toks) // self.bs, len(tab)))):
            b = tab[i]
            if b == 0:
                break
            if b in self.info:
                uid, key = self.info[b]
                if key[0] != parent:
                    other = self.reg.get((parent, tk))
                    if other is not None:
                        parent = self.info[other][0]
                        continue
                    del self.reg[key]
                    self.reg[(parent, tk)] = b
                    self.info[b] = (uid, (parent, tk))
                parent = uid
                continue
            older = self.reg.get((parent, tk))
            if older is not None:
                parent = self.info[older][0]
                continue
            self.uid += 1
            self.info[b] = (self.uid, (parent, tk))
            self.reg[(parent, tk)] = b
            parent = self.uid


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_operations_against_a_python_model(seed):
    nb, bs = 24, 4
    rng = np.random.default_rng(seed)
    bm, m = _ext.runtime().BlockManager(nb, bs, True), _Model(nb, bs)
    assert bm.ensure_capacity(SCRATCH_SEQ_ID, 1) and m.ensure(SCRATCH_SEQ_ID, 1)
    headers = [rng.integers(0, 3, size=int(n)).tolist() for n in (8, 12, 9, 4)]
    seqs, next_id = {}, 1

    def check():
        assert bm.num_free() == m.num_free() and bm.free_blocks() == m.free and bm.evictable_blocks() == m.lru
        named = [0] * nb
        for s in list(seqs) + [SCRATCH_SEQ_ID]:
            assert bm.block_table(s) == m.tables[s]
            for b in bm.block_table(s):
                named[b] += 1
        free, lru = set(bm.free_blocks()), set(bm.evictable_blocks())
        assert len(free) == len(bm.free_blocks()) and len(lru) == len(bm.evictable_blocks())
        for b in range(nb):
            assert bm.ref_count(b) == named[b] == m.ref[b]            # counts = tables naming the block
            assert (b in free) + (b in lru) + (named[b] > 0) == 1      # exactly one of the three states
            assert bm.is_registered(b) == (b in m.info) and (b not in lru or bm.is_registered(b))
        assert tuple(bm.prefix_stats()) == (m.query, m.hit, m.evictions, len(m.info))

    for _ in range(600):
        op = rng.integers(0, 10)
        if op < 4 or not seqs:                                # a new sequence
            toks = headers[rng.integers(0, 4)][: int(rng.integers(1, 13))] + \
                rng.integers(0, 3, size=int(rng.integers(0, 7))).tolist()
            sid, next_id = next_id, next_id + 1
            assert bm.acquire_prefix(sid, _i32(toks)) == m.acquire(sid, toks)
            ok = bm.ensure_capacity(sid, len(toks))
            assert ok == m.ensure(sid, len(toks))
            if ok:
                seqs[sid] = toks
            else:                                             # all-or-nothing: give the prefix back
                bm.free_sequence(sid)
                m.free_seq(sid)
        elif op < 6:                                          # register a computed part of one
            sid = int(rng.choice(list(seqs)))
            n = int(rng.integers(0, len(seqs[sid]) + 1))
            bm.register_prefix(sid, _i32(seqs[sid]), n)
            m.register(sid, seqs[sid], n)
        elif op < 8:                                          # decode: grow by a few tokens
            sid = int(rng.choice(list(seqs)))
            more = rng.integers(0, 3, size=int(rng.integers(1, 6))).tolist()
            ok = bm.ensure_capacity(sid, len(seqs[sid]) + len(more))
            assert ok == m.ensure(sid, len(seqs[sid]) + len(more))
            if ok:
                seqs[sid] = seqs[sid] + more
        else:
            sid = int(rng.choice(list(seqs)))
            bm.free_sequence(sid)
            m.free_seq(sid)
            del seqs[sid]
        check()
    assert m.evictions > 0 and m.hit > 0                      # the run did reach both


# ------------------------------------------------------------------ scheduler: the pending-key rule
P1 = SamplingParams(max_new_tokens=1, ignore_eos=True)


def _sched(nb=64, bs=4, **kw):
    bm = make_block_manager(nb, bs, True)
    d = dict(num_slots=1, max_batch=16, max_prefill_tokens=1000, max_seq_len=64)
    d.update(kw)
    return bm, Scheduler(bm, **d)


def test_identical_prompts_of_one_burst_prefill_the_header_once():
    bm, sch = _sched()
    seqs = [Sequence(list(range(1, 14)), P1) for _ in range(8)]          # 13 tokens: 3 blocks + 1
    for s in seqs:
        sch.add(s)
    st = sch.schedule(0)
    assert st.seqs == [seqs[0]] and st.num_tokens == 13                  # the others wait for its blocks
    assert list(sch.waiting) == seqs[1:] and sch.num_deferrals == 7      # in their queue order
    assert sch.schedule(0) is None                                        # nothing else to run meanwhile
    sch.complete(st, [5])
    st = sch.schedule(0)
    assert st.seqs == seqs[1:] and st.num_tokens == 7                    # one token each
    assert [s.cached_tokens for s in seqs] == [0] + [12] * 7
    tabs = [bm.block_table(s.seq_id) for s in seqs[1:]]
    assert all(t[:3] == tabs[0][:3] for t in tabs) and len({t[3] for t in tabs}) == 7
    sch.complete(st, [5] * 7)
    assert not sch.has_work() and not sch._pending and not sch._pending_of
    assert sch.prefix_stats() == {"query_tokens": 8 * 13, "hit_tokens": 7 * 12, "evictions": 0, "cached_blocks": 3}
    assert bm.num_free() == 63


def test_aborting_the_producer_releases_the_deferred():
    bm, sch = _sched(max_prefill_tokens=8)
    a, b, c = (Sequence(list(range(1, 14)), P1) for _ in range(3))
    for s in (a, b, c):
        sch.add(s)
    st = sch.schedule(0)
    assert st.seqs == [a] and st.num_tokens == 8                          # a chunk of the producer
    sch.complete(st, [0])
    assert a.num_cached == 8 and list(sch.waiting) == [a, b, c] and sch._pending
    assert sch.abort(a.seq_id) and not sch._pending
    st = sch.schedule(0)                                                  # admitted on the next call
    assert st.seqs == [b] and b.cached_tokens == 8 and st.num_tokens == 5  # a's two registered blocks survive it
    sch.complete(st, [5])
    st = sch.schedule(0)
    assert st.seqs == [c] and c.cached_tokens == 12
    sch.complete(st, [5])
    assert not sch.has_work() and not sch._pending and bm.num_free() == 63


def test_no_deferral_without_a_producer():
    bm, sch = _sched()
    a = Sequence(list(range(1, 14)), P1)
    sch.add(a)
    sch.complete(sch.schedule(0), [5])
    assert sch.num_deferrals == 0 and not sch._pending
    b, c = Sequence(list(range(1, 14)), P1), Sequence(list(range(1, 10)) + [77] * 6, P1)
    sch.add(b)
    sch.add(c)
    st = sch.schedule(0)                                                  # hits, and nobody to wait for
    assert st.seqs == [b, c] and (b.cached_tokens, c.cached_tokens) == (12, 8) and sch.num_deferrals == 0
    sch.complete(st, [5, 5])
    # different prompts in one burst: nothing to gain from each other
    d, e = Sequence([9] * 13, P1), Sequence([8] * 13, P1)
    sch.add(d)
    sch.add(e)
    assert sch.schedule(0).seqs == [d, e] and sch.num_deferrals == 0


def test_a_blocked_head_is_queried_once():
    """A waiting sequence that finds nothing and cannot get KV blocks is looked up again on every
    admission pass; the queried-tokens counter takes it once."""
    bm, sch = _sched(nb=6)                                                # five usable blocks
    a = Sequence(list(range(1, 14)), SamplingParams(max_new_tokens=6, ignore_eos=True))
    sch.add(a)
    sch.complete(sch.schedule(0), [5])                                    # a runs: four blocks
    b = Sequence(list(range(50, 59)), P1)                                 # needs three
    sch.add(b)
    for _ in range(3):
        st = sch.schedule(0)
        assert not st.is_prefill and list(sch.waiting) == [b] and not bm.has_sequence(b.seq_id)
        sch.complete(st, [5])
        assert sch.prefix_stats()["query_tokens"] == 13 + 9
    while sch.has_work():
        st = sch.schedule(0)
        sch.complete(st, [5] * st.size)
    assert b.finished and sch.prefix_stats()["query_tokens"] == 13 + 9


def test_rejected_with_tensor_parallelism_on_every_rank():
    from types import SimpleNamespace
    from distributed_llms_amd.parallel.dist_engine import RankRole
    on = EngineConfig(model="synthetic:tiny-llama", device="cpu", dtype="float32", enable_prefix_caching=True)
    on.check_tensor_parallel(1)
    EngineConfig(model="synthetic:tiny-llama").check_tensor_parallel(2)
    with pytest.raises(ValueError, match="prefix caching"):
        on.check_tensor_parallel(2)
    # every rank of a tp layout refuses before it builds anything: leader, lane follower, tp follower
    for pp, stage, tp_rank in [(1, 0, 0), (1, 0, 1), (2, 0, 1), (2, 1, 0)]:
        with pytest.raises(ValueError, match="prefix caching"):
            RankRole(SimpleNamespace(tp=2, pp=pp, stage=stage, tp_rank=tp_rank), on)


def test_off_scheduler_never_defers_or_registers():
    bm = make_block_manager(64, 4)
    sch = Scheduler(bm, 1, 16, 1000, 64)
    seqs = [Sequence(list(range(1, 14)), P1) for _ in range(4)]
    for s in seqs:
        sch.add(s)
    st = sch.schedule(0)
    assert st.seqs == seqs and st.num_tokens == 52 and not sch.prefix
    sch.complete(st, [5] * 4)
    assert sch.prefix_stats() == {"query_tokens": 0, "hit_tokens": 0, "evictions": 0, "cached_blocks": 0}
    assert [s.cached_tokens for s in seqs] == [0] * 4


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_nothing_waits_forever(seed):
    """Random bursts with shared headers, chunked prompts, a pool small enough to preempt and to hit
    the KV deadlock breaker, and aborts at every stage of a request's life: every request ends, in a
    bounded number of scheduler calls, and nothing is left pending or allocated."""
    rng = np.random.default_rng(seed)
    bm, sch = _sched(nb=14, max_prefill_tokens=12, max_batch=4, max_seq_len=48, mixed_prefill_tokens=int(seed % 2) * 6)
    headers = [rng.integers(1, 50, size=9).tolist() for _ in range(2)]
    todo = [Sequence(headers[int(rng.integers(0, 2))][: int(rng.integers(4, 10))] +
                     rng.integers(1, 50, size=int(rng.integers(0, 8))).tolist(),
                     SamplingParams(max_new_tokens=int(rng.integers(1, 9)), ignore_eos=True)) for _ in range(40)]
    every = list(todo)
    calls = idle = 0
    while todo or sch.has_work():
        calls += 1
        assert calls < 4000
        for _ in range(int(rng.integers(0, 4))):
            if todo:
                sch.add(todo.pop())
        if rng.integers(0, 8) == 0:
            live = [s for s in every if s.status in (SeqStatus.WAITING, SeqStatus.RUNNING) and s not in todo]
            if live:
                sch.abort(live[int(rng.integers(0, len(live)))].seq_id)
        st = sch.schedule(0)
        if st is None:
            idle += 1
            assert idle < 50 or todo          # one slot, synchronous: work left means a step comes
            continue
        idle = 0
        sch.complete(st, [7] * st.size)
        # a pending key always has a producer that is admitted or between two chunks
        owners = {i for ids in sch._pending.values() for i in ids}
        assert owners <= {s.seq_id for s in every if s.status in (SeqStatus.WAITING, SeqStatus.RUNNING)}
    assert all(s.finished for s in every)
    assert not sch._pending and not sch._pending_of
    assert bm.num_free() == 13 and bm.num_sequences() == 1
    assert sch.prefix_stats()["hit_tokens"] > 0


# ------------------------------------------------------------------ engines on the CPU
def _workload(seed=0, n=9, header=70):
    rng = np.random.default_rng(seed)
    hdrs = [rng.integers(3, 200, size=header).tolist(), rng.integers(3, 200, size=header // 2).tolist()]
    out = [hdrs[i % 3 == 2] + rng.integers(3, 200, size=int(rng.integers(1, 30))).tolist() for i in range(n - 1)]
    return out + [rng.integers(3, 200, size=20).tolist()]


def _run_engine(cache, prompts, gen=10, waves=3, **kw):
    """Requests arrive in waves between steps -> (outputs, engine, sequences, prompt tokens computed).
    Every step's HostBatch is checked: no written slot lies in a registered or shared block."""
    d = dict(model="synthetic:tiny-llama", device="cpu", dtype="float32", max_batch=16, max_seq_len=256,
             use_graphs=False, num_kv_blocks=256, enable_prefix_caching=cache)
    d.update(kw)
    eng = LLMEngine(EngineConfig(**d))
    computed = [0]
    build = eng._host_batch

    def checked(step):
        hb = build(step)
        if hb.is_prefill:
            computed[0] += hb.num_tokens - hb.num_decode
        if cache:
            for b in set((hb.slots // eng.ecfg.kv_block_size).tolist()):
                assert not eng.bm.is_registered(b) and eng.bm.ref_count(b) == 1, (b, hb.step_id)
        return hb

    eng._host_batch = checked
    p = SamplingParams(max_new_tokens=gen, ignore_eos=True)
    seqs = []
    for i, q in enumerate(prompts):
        seqs.append(eng.add_request(q, p))
        if i % waves == waves - 1:
            eng.step()
    eng.run_until_done()
    return [s.output for s in seqs], eng, seqs, computed[0]


@pytest.mark.parametrize("kw", [dict(), dict(max_prefill_tokens=64), dict(mixed_prefill_tokens=0),
                                dict(max_prefill_tokens=64, mixed_prefill_tokens=16)],
                         ids=["whole", "chunked", "prefill-first", "chunked-mixed"])
def test_engine_outputs_equal_cache_off(kw):
    prompts = _workload()
    ref, e0, s0, n0 = _run_engine(False, prompts, **kw)
    out, e1, s1, n1 = _run_engine(True, prompts, **kw)
    assert out == ref                                                     # exactly, as test_mixed_steps compares
    hits = sum(s.cached_tokens for s in s1)
    assert hits > 0 and hits == e1.scheduler.prefix_stats()["hit_tokens"]
    assert e0.scheduler.num_preemptions == e1.scheduler.num_preemptions == 0
    assert n0 == sum(len(p) for p in prompts) and n0 - n1 == hits         # prompt tokens drop by exactly the hits
    assert e0.num_prefill_tokens - e1.num_prefill_tokens == hits + \
        (e0.num_prefill_tokens - n0) - (e1.num_prefill_tokens - n1)       # (the counter also holds mixed steps' decode rows)
    assert all(s.cached_tokens == 0 for s in s0) and e1.bm.num_free() == 255
    assert e1.scheduler.prefix_stats()["cached_blocks"] > 0


def test_engine_with_a_pool_small_enough_to_preempt():
    """Preemption frees (now: decrements) and re-admission hits the sequence's own prompt blocks where
    they survived.  How many tokens are recomputed depends on which blocks were evicted meanwhile, so
    here only the tokens and the presence of hits are asserted."""
    prompts = _workload(seed=1)
    kw = dict(num_kv_blocks=14, gen=60)
    ref, e0, _, _ = _run_engine(False, prompts, **kw)
    out, e1, s1, _ = _run_engine(True, prompts, **kw)
    assert e0.scheduler.num_preemptions > 0 and e1.scheduler.num_preemptions > 0
    assert out == ref and sum(s.cached_tokens for s in s1) > 0
    assert e1.bm.num_free() == 13 and all(len(o) == 60 for o in out)
    assert e1.scheduler.prefix_stats()["evictions"] > 0


def test_engine_burst_of_identical_prompts():
    prompts = [_workload()[0]] * 8
    ref, _, _, n0 = _run_engine(False, prompts, waves=100)
    out, e1, s1, n1 = _run_engine(True, prompts, waves=100)
    bs, n = 32, len(prompts[0])
    assert out == ref and n0 == 8 * n
    assert n1 == n + 7 * (n - (n - 1) // bs * bs)                        # the header once, seven tails
    assert e1.scheduler.num_deferrals >= 7


def test_loopback_pipeline_equals_cache_off():
    from distributed_llms_amd.parallel.pipeline import run_loopback_pipeline
    prompts = _workload(seed=2, n=7)
    p = SamplingParams(max_new_tokens=8, ignore_eos=True)
    kw = dict(model="synthetic:tiny-llama", device="cpu", dtype="float32", max_batch=8, max_seq_len=256,
              use_graphs=False, num_kv_blocks=256, max_prefill_tokens=96)
    ref = LLMEngine(EngineConfig(**kw)).generate(prompts, p)
    outs, drv, _ = run_loopback_pipeline(EngineConfig(enable_prefix_caching=True, **kw), 2, prompts, p, device="cpu")
    assert outs == ref
    assert drv.scheduler.prefix_stats()["hit_tokens"] > 0 and not drv.scheduler._pending


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_cfg(**kw):
    return EngineConfig(model="tiny-llama", dtype="float32", device="cpu", max_batch=4, max_seq_len=256,
                        use_graphs=False, num_kv_blocks=256, max_prefill_tokens=96, **kw)


def _rank_main(rank, world, port, prompts, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from distributed_llms_amd.parallel.dist_engine import RankRole, init_distributed
    ctx = init_distributed(pp=world, backend="gloo")
    role = RankRole(ctx, _gloo_cfg(num_workers=world, enable_prefix_caching=True))
    p = SamplingParams(max_new_tokens=6, ignore_eos=True)
    res = []
    for _ in range(2):          # the second round finds the first round's prompts in the cache
        seqs = [role.add_request(q, p) for q in prompts] if role.is_driver else []
        role.run_round()
        res.append(([s.output for s in seqs], sum(s.cached_tokens for s in seqs)))
    role.shutdown()
    dist.barrier()
    out_q.put((rank, res if role.is_driver else None))
    dist.destroy_process_group()


@pytest.mark.slow
def test_two_stage_gloo_pipeline_equals_cache_off():
    prompts = _workload(seed=3, n=6)
    ref = LLMEngine(_gloo_cfg()).generate(prompts, SamplingParams(max_new_tokens=6, ignore_eos=True))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, prompts, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (out1, hit1), (out2, hit2) = results[0]
    assert out1 == ref and out2 == ref
    assert 0 < hit1 < hit2 == sum((len(p) - 1) // 32 * 32 for p in prompts)


# ------------------------------------------------------------------ HTTP: "n", usage, metrics
from test_master_worker import _spawn_worker  # noqa: E402


@pytest.fixture
def cached_cluster():
    from distributed_llms_amd.master.node import MasterNode
    cfg = EngineConfig(model="synthetic:tiny-llama", dtype="float32", device="cpu", max_batch=16, max_seq_len=256,
                       use_graphs=False, num_kv_blocks=128, heartbeat_interval=0.5, heartbeat_timeout=4.0,
                       enable_prefix_caching=True)
    m = MasterNode("127.0.0.1", 0, cfg).start()
    m.initialize_model("synthetic:tiny-llama", num_shards=1)
    proc = _spawn_worker(m.port)
    try:
        m.wait_for_workers(1, timeout=120)
        m.assign_shards()
        m.distribute_shards(timeout=300)
        yield m
    finally:
        m.stop()
        try:
            proc.wait(timeout=15)
        except Exception:                   # noqa: BLE001
            proc.kill()


@pytest.mark.slow
def test_http_n_completions_usage_and_metrics(cached_cluster):
    from distributed_llms_amd.master.http_api import serve_http
    m = cached_cluster
    srv, _ = serve_http(m, "127.0.0.1", 0)
    base = f"http://127.0.0.1:{srv.server_address[1]}"

    def post(path, body):
        req = urllib.request.Request(base + path, data=json.dumps(body).encode(),
                                     headers={"Content-Type": "application/json"})
        with urllib.request.urlopen(req, timeout=120) as r:
            return json.loads(r.read())

    pa, pb = _workload(seed=4)[0], _workload(seed=5)[0]
    try:
        # greedy, two prompts x n = 3: six choices in index order, prompt-major
        c = post("/v1/completions", {"prompt": [pa, pb], "max_tokens": 5, "ignore_eos": True, "n": 3})
        assert [ch["index"] for ch in c["choices"]] == list(range(6))
        ea, eb = (m.generate([p], max_new_tokens=5, ignore_eos=True, timeout=120)[0]["tokens"] for p in (pa, pb))
        assert [ch["tokens"] for ch in c["choices"]] == [ea] * 3 + [eb] * 3
        u = c["usage"]
        assert u["prompt_tokens"] == len(pa) + len(pb) and u["completion_tokens"] == 30      # each prompt once
        cap = sum((len(p) - 1) // 32 * 32 for p in (pa, pb))
        assert u["prompt_tokens_details"]["cached_tokens"] == 2 * cap                       # children 1, 2 of each
        # seed s with n = 3 == three single requests with seeds s, s + 1, s + 2 (also across 2^64)
        for s in (1234, (1 << 64) - 2):
            body = {"prompt": pa, "max_tokens": 6, "ignore_eos": True, "temperature": 0.9, "top_k": 50}
            c = post("/v1/completions", dict(body, seed=s, n=3))
            singles = [post("/v1/completions", dict(body, seed=(s + j) % (1 << 64)))["choices"][0]["tokens"]
                       for j in range(3)]
            assert [ch["tokens"] for ch in c["choices"]] == singles
            assert len({tuple(t) for t in singles}) > 1
        assert c["usage"]["prompt_tokens_details"]["cached_tokens"] == 3 * ((len(pa) - 1) // 32 * 32)
        g = post("/generate", {"prompt_ids": pa, "max_new_tokens": 5, "ignore_eos": True, "n": 2})
        assert [r["tokens"] for r in g["results"]] == [ea, ea]
        g1 = post("/generate", {"prompt_ids": pa, "max_new_tokens": 5, "ignore_eos": True, "n": 1})
        assert g1["tokens"] == ea and g1["cached_tokens"] == (len(pa) - 1) // 32 * 32
        for path, bad in [("/v1/completions", {"prompt": pa, "n": 0}), ("/v1/completions", {"prompt": pa, "n": 17}),
                          ("/v1/completions", {"prompt": pa, "n": 2.0}), ("/generate", {"prompt_ids": pa, "n": True}),
                          ("/generate", {"prompt_ids": pa, "n": "2"}),
                          ("/v1/completions", {"prompt": pa, "n": 2, "stream": True}),
                          ("/generate", {"prompt_ids": pa, "n": 1, "stream": True})]:
            with pytest.raises(urllib.error.HTTPError) as ei:
                post(path, bad)
            assert ei.value.code == 400, bad
        with urllib.request.urlopen(base + "/metrics", timeout=30) as r:
            text = r.read().decode()
        vals = {ln.split()[0]: float(ln.split()[1]) for ln in text.splitlines() if ln.startswith("dllm_prefix_cache_")}
        assert set(vals) == {"dllm_prefix_cache_query_tokens_total", "dllm_prefix_cache_hit_tokens_total",
                             "dllm_prefix_cache_evictions_total", "dllm_prefix_cache_blocks"}
        assert vals["dllm_prefix_cache_hit_tokens_total"] > 0 and vals["dllm_prefix_cache_blocks"] > 0
        assert vals["dllm_prefix_cache_query_tokens_total"] > vals["dllm_prefix_cache_hit_tokens_total"]
        assert "# TYPE dllm_prefix_cache_hit_tokens_total counter" in text
    finally:
        srv.shutdown()
