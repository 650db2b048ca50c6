"""The fused sampling kernel (csrc/kernels/sampler.hip, ops.sample_rows) on the GPU: exactness
against ops/reference.py sample_rows, greedy parity with ops.argmax, draw boundaries, bit
reproducibility, the drawn distribution, graph capture, and the engine's seeded path."""
import numpy as np
import pytest
import torch

import sampler_cases as sc
from distributed_llms_amd import ops
from distributed_llms_amd.config import EngineConfig
from distributed_llms_amd.engine.llm_engine import LLMEngine
from distributed_llms_amd.engine.sequence import SamplingParams
from distributed_llms_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


def _run(case, dev, uniforms=None):
    return ops.sample_rows(case["logits"].to(dev), case["params"].to(dev), case["seeds"].to(dev),
                           case["pos"].to(dev), None if uniforms is None else uniforms.to(dev)).cpu().numpy()


def _args(dev, rows, temp_e4, k, p_e4, seed=1, pos=0):
    par = torch.tensor([[temp_e4, k, p_e4]] * rows, dtype=torch.int32, device=dev)
    return (par, torch.full((rows,), seed, dtype=torch.int64, device=dev),
            torch.full((rows,), pos, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("rows,vocab", sc.SHAPES)
def test_kernel_matches_the_reference(cuda, rows, vocab):
    """Every (temperature, top-k, top-p) mix on random, tie-heavy and hand-built rows; aligned and
    unaligned rows (odd vocab), rows shorter than the workgroup (777), more rows than CUs (300).
    Acceptance: sampler_cases.check_ids (exact, or within EPS * Z of a boundary for at most 2 % of
    the random rows and for no hand-built row)."""
    case = sc.make_case(rows, vocab)
    got = _run(case, cuda)
    widened = sc.check_ids(case, got)
    print(f"rows {rows} vocab {vocab}: {widened} of {got.shape[0]} rows needed the widened rule")


@pytest.mark.parametrize("rows,vocab", [(256, 128256), (3, 50257)])
def test_greedy_rows_equal_argmax(cuda, rows, vocab):
    """temp_e4 = 0 on the tie and -inf rows of test_argmax_ties_take_the_first_index: ops.argmax bit
    for bit.  T = 1e-4 on logits without ties: the argmax too."""
    g = torch.Generator().manual_seed(rows + vocab)
    logits = (torch.randn(rows, vocab, generator=g) * 3.0).round().to(torch.bfloat16).to(cuda)
    logits[0] = 1.0
    logits[-1, :] = -5.0
    logits[-1, vocab - 3:] = 7.0
    extra = torch.full((4, vocab), float("-inf"), dtype=torch.bfloat16, device=cuda)
    extra[0, vocab - 1] = -3.0
    extra[2] = logits[1]
    extra[2, vocab // 2 + 1] = float("inf")
    extra[3, vocab - 1] = -3.0
    logits = torch.cat([extra, logits])
    n = logits.shape[0]
    par, seeds, pos = _args(cuda, n, 0, 0, 10000)
    par[1::2, 1] = 40                  # greedy rows ignore top-k / top-p
    par[::3, 2] = 5000
    assert torch.equal(ops.sample_rows(logits, par, seeds, pos), ops.argmax(logits))
    # distinct values per row: a permutation of an increasing ramp (exact in bf16)
    m = min(vocab, 256)
    ramp = torch.stack([torch.randperm(m, generator=g).float() * 0.25 - 20.0 for _ in range(5)])
    distinct = torch.full((5, vocab), float("-inf"))
    distinct[:, vocab - m:] = ramp
    distinct = distinct.to(torch.bfloat16).to(cuda)
    par, seeds, pos = _args(cuda, 5, 1, 0, 10000, seed=77, pos=3)
    assert torch.equal(ops.sample_rows(distinct, par, seeds, pos), ops.argmax(distinct))


def test_uniform_boundaries(cuda):
    """u = 0 and u = 1 - 2^-24 with k = 3: the lowest and the highest index of the three kept.  Any
    u: an index of the kept set."""
    vocab = 5003
    g = torch.Generator().manual_seed(9)
    logits = (torch.randn(6, vocab, generator=g) * 3.0).to(torch.bfloat16)
    top3 = torch.stack([torch.randperm(vocab, generator=g)[:3] for _ in range(6)])
    top3[0, 0], top3[1, 1], top3[2, 2] = 0, vocab - 1, vocab - 2      # the row's ends, the ragged tail
    for i in range(6):
        logits[i, top3[i]] = torch.tensor([20.0, 19.0, 18.5], dtype=torch.bfloat16)
    par, seeds, pos = _args(cuda, 6, 20000, 3, 10000)
    lo = ops.sample_rows(logits.to(cuda), par, seeds, pos, torch.zeros(6, device=cuda)).cpu()
    hi = ops.sample_rows(logits.to(cuda), par, seeds, pos,
                         torch.full((6,), 1.0 - 2.0 ** -24, device=cuda)).cpu()
    assert lo.tolist() == top3.min(-1).values.tolist()
    assert hi.tolist() == top3.max(-1).values.tolist()
    row = logits[:1].expand(4096, -1).to(cuda)
    par, seeds, pos = _args(cuda, 4096, 20000, 3, 10000)
    u = torch.rand(4096, generator=g).to(cuda)
    ids = ops.sample_rows(row, par, seeds, pos, u).cpu()
    assert set(ids.tolist()) == set(top3[0].tolist())
    want = ref.sample_rows(logits[:1].expand(4096, -1), par.cpu(), seeds.cpu(), pos.cpu(), u.cpu())
    assert (ids != want).sum().item() <= 1       # a u within 1e-6 of a CDF step, at most


def test_bit_reproducible(cuda):
    """The same [256, 128256] inputs five times; rows moved to other row indices; rows alone in a
    batch of one; one row expanded (stride 0) over positions against single-row launches."""
    rows, vocab = 256, 128256
    g = torch.Generator(device=cuda).manual_seed(4)
    logits = (torch.randn(rows, vocab, generator=g, device=cuda) * 3.0).to(torch.bfloat16)
    rng = np.random.default_rng(5)
    ks = sc.top_ks(vocab)
    par = torch.tensor([[sc.TEMPS_E4[1 + i % 4], ks[(i // 4) % 6], sc.TOP_PS_E4[(i // 24 + i) % 4]]
                        for i in range(rows)], dtype=torch.int32, device=cuda)
    seeds = torch.from_numpy(rng.integers(-2 ** 63, 2 ** 63 - 1, size=rows, dtype=np.int64)).to(cuda)
    pos = torch.from_numpy(rng.integers(0, 8192, size=rows).astype(np.int32)).to(cuda)
    first = ops.sample_rows(logits, par, seeds, pos)
    for _ in range(4):
        assert torch.equal(ops.sample_rows(logits, par, seeds, pos), first)
    assert len(set(first.tolist())) > 32                  # not a constant
    perm = torch.from_numpy(rng.permutation(rows)).to(cuda)
    moved = ops.sample_rows(logits[perm], par[perm], seeds[perm], pos[perm])
    assert torch.equal(moved, first[perm])
    for i in (0, 17, 130, 255):
        one = ops.sample_rows(logits[i:i + 1], par[i:i + 1].contiguous(), seeds[i:i + 1].clone(),
                              pos[i:i + 1].clone())
        assert one.item() == first[i].item()
    n = 64
    par1, seeds1, _ = _args(cuda, n, 10000, 0, 9000, seed=123456789012345)
    allpos = torch.arange(n, dtype=torch.int32, device=cuda)
    expanded = ops.sample_rows(logits[3:4].expand(n, -1), par1, seeds1, allpos)
    assert len(set(expanded.tolist())) > 8
    for p in (0, 1, 31, 63):
        one = ops.sample_rows(logits[3:4], par1[:1], seeds1[:1], allpos[p:p + 1].clone())
        assert one.item() == expanded[p].item()


def test_rows_longer_than_the_kernel_holds_are_refused(cuda):
    """The kernel keeps a row of at most 131,072 entries in registers; a longer one is an error, not
    another path."""
    logits = torch.zeros(1, ops.SAMPLE_MAX_VOCAB + 1, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(ValueError, match="131072"):
        ops.sample_rows(logits, *_args(cuda, 1, 10000, 0, 10000))
    edge = torch.zeros(2, ops.SAMPLE_MAX_VOCAB, dtype=torch.bfloat16, device=cuda)
    edge[0, -1] = 30.0
    edge[1, 5] = 30.0
    assert ops.sample_rows(edge, *_args(cuda, 2, 10000, 0, 10000)).tolist() == [ops.SAMPLE_MAX_VOCAB - 1, 5]


def test_knob_off_takes_the_reference(cuda):
    from distributed_llms_amd import knobs
    case = sc.make_case(3, 777)
    want = ref.sample_rows(case["logits"], case["params"], case["seeds"], case["pos"])
    with knobs.override(fused_sampler=False):
        got = ops.sample_rows(case["logits"].to(cuda), case["params"].to(cuda), case["seeds"].to(cuda),
                              case["pos"].to(cuda))
    assert got.device.type == "cuda" and got.cpu().tolist() == want.tolist()


def test_distribution(cuda):
    """V = 37, T = 1.3, k = 12, p = 0.9, pos = 0..65535 under one seed: no draw outside the kept set
    and a chi-square against the reference's exact kept probabilities under the 99.9 % point."""
    n = sc.DIST_N
    par, seeds, _ = _args(cuda, n, *sc.DIST_PARAMS, seed=sc.DIST_SEED)
    ids = ops.sample_rows(sc.dist_row().to(cuda).expand(n, -1), par, seeds,
                          torch.arange(n, dtype=torch.int32, device=cuda)).cpu().numpy()
    chi2, dof = sc.check_distribution(ids)
    print(f"chi2 {chi2:.2f} at {dof} degrees of freedom (99.9 % point {sc.chi2_critical_999(dof):.2f})")


def test_graph_capture(cuda):
    """One launch captured on a single stream; replays follow new params / seeds / positions
    written into the captured buffers and equal eager launches."""
    case = sc.make_case(9, 50257)
    logits = case["logits"].to(cuda)
    n = logits.shape[0]
    par, seeds, pos = case["params"].to(cuda), case["seeds"].to(cuda), case["pos"].to(cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.sample_rows(logits, par, seeds, pos)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.sample_rows(logits, par, seeds, pos)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.sample_rows(logits, par, seeds, pos))
    before = out.clone()
    par.copy_(torch.tensor([[15000, 0, 9500]] * n, dtype=torch.int32))
    seeds.copy_(torch.arange(n, dtype=torch.int64) * 7919 + 11)
    pos.copy_(torch.arange(n, dtype=torch.int32) + 100)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.sample_rows(logits, par, seeds, pos))
    assert not torch.equal(out, before)


def _engine(graphs):
    eng = LLMEngine(EngineConfig(model="synthetic:tiny-llama", dtype="bfloat16", device="cuda", max_batch=8,
                                 max_seq_len=256, use_graphs=graphs, num_kv_blocks=128,
                                 graph_batch_sizes=(1, 2, 4, 8)))
    eng.lookahead = graphs
    return eng


@pytest.mark.parametrize("graphs", [True, False])
def test_engine_seeded_requests_reproduce(cuda, graphs):
    """The same seeds on two engines: identical outputs (graphs and lookahead on, then eager and
    synchronous).  The greedy rows of a mixed batch return the tokens of an all-greedy run, its
    sampled rows those of the all-sampled run."""
    prompts = [[1, 5, 9, 200], [3, 4, 7], list(range(10, 40)), [8] * 13, [9, 9, 9], [2, 3]]
    sampled = [SamplingParams(max_new_tokens=12, ignore_eos=True, temperature=0.9, top_k=40, top_p=0.95,
                              seed=1000 + i) for i in range(len(prompts))]
    greedy = SamplingParams(max_new_tokens=12, ignore_eos=True)
    e1, e2 = _engine(graphs), _engine(graphs)
    a = e1.generate(prompts, sampled)
    b = e2.generate(prompts, sampled)
    assert a == b
    assert graphs == (e1.num_lookahead > 0)
    assert len({tuple(o) for o in a}) > 1 and a != e1.generate(prompts, [greedy] * len(prompts))
    all_greedy = e1.generate(prompts, [greedy] * len(prompts))
    mixed = e2.generate(prompts, [greedy if i % 2 == 0 else sampled[i] for i in range(len(prompts))])
    assert mixed[0::2] == all_greedy[0::2]
    assert mixed[1::2] == a[1::2]
