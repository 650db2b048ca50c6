"""The logit-processor kernels (csrc/kernels/logit_processors.hip) on the GPU: bit equality with
ops/reference.py, the state kernels' bookkeeping and guards, bit reproducibility, and the engine's
token identity across its execution modes."""
import numpy as np
import pytest
import torch

import processors_cases as pc
from distributed_llms_amd import knobs, ops
from distributed_llms_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

P, B = ref.STATE_PROMPT_BIT, ref.STATE_BIAS_BIT


def _u32(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _run_apply(case, dev, logits=None):
    lg = case["logits"].to(dev) if logits is None else logits
    ops.apply_logit_processors(lg, pc.state_to(case["ls"], dev), case["procs"].to(dev), case["seq_lens"].to(dev),
                               case["eos"])
    return lg


# (7, 2048): every kind of row (processors_cases.KINDS) twice over at an aligned vocabulary
@pytest.mark.parametrize("rows,vocab", pc.SHAPES + [(7, 2048)])
def test_apply_matches_the_reference_bit_for_bit(cuda, rows, vocab):
    case = pc.make_apply_case(rows, vocab)
    exp = pc.reference(case)
    state_before = case["ls"].state.clone()
    ls_dev = pc.state_to(case["ls"], cuda)
    got = case["logits"].to(cuda)
    ops.apply_logit_processors(got, ls_dev, case["procs"].to(cuda), case["seq_lens"].to(cuda), case["eos"])
    changed = pc.check_bits(got, exp, case["logits"], case["touched"], f"{rows}x{vocab}")
    print(f"rows {rows} vocab {vocab}: {changed} elements changed")
    assert changed > 50
    assert torch.equal(ls_dev.state.cpu(), state_before)    # apply only reads the state


def test_apply_strided_rows_keep_their_guard_columns(cuda):
    """Rows taken from a wider buffer: a row stride above the vocabulary, every row unaligned; the
    columns beside the rows keep their bits."""
    case = pc.make_apply_case(5, 5003)
    exp = pc.reference(case)
    wide = torch.full((5, 5003 + 13), -7.5, dtype=torch.bfloat16, device=cuda)
    wide[:, 5:5008] = case["logits"].to(cuda)
    _run_apply(case, cuda, wide[:, 5:5008])
    pc.check_bits(wide[:, 5:5008], exp, case["logits"], case["touched"], "strided")
    assert (wide[:, :5] == -7.5).all() and (wide[:, 5008:] == -7.5).all()


def test_apply_bit_reproducible_across_row_batch_and_launch(cuda):
    """A row's result is the same as row 0 of 1 and as row 39 of 40, and across launches."""
    case = pc.make_apply_case(4, 128256)
    exp = pc.reference(case)
    ls = pc.state_to(case["ls"], cuda)
    one = case["logits"][:1].to(cuda)
    ops.apply_logit_processors(one, ls, case["procs"][:1].to(cuda), case["seq_lens"][:1].to(cuda), case["eos"])
    g = torch.Generator().manual_seed(11)
    big = (torch.randn(40, 128256, generator=g) * 3.0).to(torch.bfloat16)
    big[39] = case["logits"][0]
    procs = torch.from_numpy(np.stack([pc.proc_row() for _ in range(40)]))
    procs[39] = case["procs"][0]
    procs[7] = case["procs"][2]                             # another asking row, on other logits
    seq_lens = torch.full((40,), 9, dtype=torch.int32)
    seq_lens[39] = case["seq_lens"][0]
    runs = []
    for _ in range(2):
        lg = big.to(cuda)
        ops.apply_logit_processors(lg, ls, procs.to(cuda), seq_lens.to(cuda), case["eos"])
        runs.append(lg.view(torch.int16))
    assert torch.equal(runs[0], runs[1])
    assert torch.equal(runs[0][39], one.view(torch.int16)[0])
    pc.check_bits(one, exp[:1], case["logits"][:1], case["touched"][:1], "row 0 of 1")
    rest = [r for r in range(39) if r != 7]
    assert torch.equal(runs[0][rest].cpu(), big.view(torch.int16)[rest])        # rows that did not ask


# ------------------------------------------------------------------ update
def _update(ls, ids, cu, procs, bias=((0,), (), ())):
    dev = ls.state.device
    bcu, bids, bvals = bias
    ops.logit_state_update(ls, torch.tensor(ids, dtype=torch.int32, device=dev) if not torch.is_tensor(ids) else ids.to(dev),
                           torch.tensor(cu, dtype=torch.int32, device=dev), torch.from_numpy(np.stack(procs)).to(dev),
                           torch.tensor(bcu, dtype=torch.int32, device=dev), torch.tensor(bids, dtype=torch.int32, device=dev),
                           torch.tensor(bvals, dtype=torch.float32, device=dev))


def test_update_counts_a_long_repeated_chunk_exactly(cuda):
    """70,000 tokens of one id straddling prompt_len: one prompt bit, an exact count; a second id
    sprinkled over both parts; the neighbouring rows, pre-filled, stay."""
    v = 777
    ls = pc.empty_state(3, v, cuda)
    ls.state[:] = 0x1234567
    ids = torch.full((70000,), 5, dtype=torch.int32)
    ids[::1000] = 6                                         # 70 of them, 31 before prompt_len = 30001
    _update(ls, ids, [0, 70000], [pc.proc_row(1, 30001, ref.PROC_UPDATE, start=0)], ((0, 0), (), ()))
    st = _u32(ls.state)
    exp = np.zeros(784, np.uint32)
    exp[5] = P | (39999 - 39)
    exp[6] = P | 39
    assert st[1].tolist() == exp.tolist()
    assert (st[0] == 0x1234567).all() and (st[2] == 0x1234567).all()
    assert ls.bias_n.tolist() == [0, 0, 0]


def test_update_resets_only_at_position_zero_and_only_its_row(cuda):
    v = 2048
    ls = pc.empty_state(4, v, cuda)
    ls.state[:] = 3
    ls.bias_n[:] = 9
    procs = [pc.proc_row(2, 4, ref.PROC_UPDATE | ref.PROC_SAMPLE, start=0), pc.proc_row(1, 2, ref.PROC_UPDATE, start=6),
             pc.proc_row(3, 0, ref.PROC_SAMPLE), pc.proc_row(-1, 0, ref.PROC_UPDATE)]
    ids = [10, 11, 10, 12, 10, 2047,   20, 20, 21,   30,   40]
    _update(ls, ids, [0, 6, 9, 10, 11], procs, ((0, 3, 3, 3, 3), (11, 0, 2047), (1.0, -2.0, 3.5)))
    st = _u32(ls.state)
    exp2 = np.zeros(v, np.uint32)
    exp2[[10, 11, 12]] = P
    exp2[10] += 1
    exp2[2047] = 1 | B
    exp2[11] |= B
    exp2[0] = B
    assert st[2].tolist() == exp2.tolist()
    exp1 = np.full(v, 3, np.uint32)
    exp1[20] += 2
    exp1[21] += 1
    assert st[1].tolist() == exp1.tolist()                  # a chunk that starts at 6: no reset, all outputs
    assert (st[0] == 3).all() and (st[3] == 3).all()        # a decode row (no UPDATE) and a foreign row
    assert ls.bias_n.tolist() == [9, 9, 3, 9] and ls.bias_ids[2, :3].tolist() == [11, 0, 2047]
    assert ls.bias_vals[2, :3].tolist() == [1.0, -2.0, 3.5]


def test_update_and_count_ignore_ids_outside_the_vocabulary(cuda):
    """Ids in [vocab, pitch) and id -1 on a state row >= 1 would land inside the allocation: the
    padding words and the neighbouring row's last word stay zero."""
    v = 777                                                 # pitch 784
    ls = pc.empty_state(3, v, cuda)
    ids = [777, 783, -1, 5, 780, -1, 776]
    _update(ls, ids, [0, 7], [pc.proc_row(1, 3, ref.PROC_UPDATE, start=0)], ((0, 2), (778, -1), (1.0, 1.0)))
    ops.logit_state_count(ls, torch.tensor([779, -1, 5], dtype=torch.int32, device=cuda),
                          torch.from_numpy(np.stack([pc.proc_row(1, 0, ref.PROC_SAMPLE), pc.proc_row(2, 0, ref.PROC_SAMPLE),
                                                     pc.proc_row(1, 0, ref.PROC_SAMPLE)])).to(cuda))
    st = _u32(ls.state)
    exp = np.zeros(784, np.uint32)
    exp[5] = 2
    exp[776] = 1
    assert st[1].tolist() == exp.tolist() and not st[0].any() and not st[2].any()


def test_count_duplicates_and_rows_without_sample(cuda):
    v = 5003
    ls = pc.empty_state(4, v, cuda)
    procs = [pc.proc_row(1, 0, ref.PROC_SAMPLE), pc.proc_row(2, 0, ref.PROC_SAMPLE), pc.proc_row(3, 0, ref.PROC_UPDATE),
             pc.proc_row(-1, 0, ref.PROC_SAMPLE), pc.proc_row(1, 0, ref.PROC_SAMPLE), pc.proc_row(2, 0, 0)]
    ids = torch.tensor([42, 42, 42, 42, 42, 42], dtype=torch.int32, device=cuda)
    pr = torch.from_numpy(np.stack(procs)).to(cuda)
    for _ in range(3):
        ops.logit_state_count(ls, ids, pr)
    st = _u32(ls.state)
    assert st[1, 42] == 6 and st[2, 42] == 3 and st.sum() == 9       # the same id in two rows of one state row: both count


def test_kernels_match_the_reference_through_a_request_life(cuda):
    """update (two chunks) -> apply -> count -> apply, the state the kernels built themselves,
    against the same calls on the CPU."""
    v = 5003
    g = torch.Generator().manual_seed(2)
    toks = torch.randint(0, 200, (300,), generator=g).to(torch.int32)
    logits = (torch.randn(2, v, generator=g) * 3.0).to(torch.bfloat16)
    outs = {}
    for dev in ("cpu", cuda):
        ls = pc.empty_state(2, v, dev)
        kw = dict(rep=1.4, pres=0.3, freq=0.07, min_tokens=51)      # output index 50 banned, 51 not
        bias = ((0, 3), (7, 150, 5002), (4.0, -100.0, 9.5))
        _update(ls, toks[:128], [0, 128], [pc.proc_row(1, 250, ref.PROC_UPDATE, start=0, **kw)], bias)
        _update(ls, toks[128:], [0, 172], [pc.proc_row(1, 250, ref.PROC_UPDATE | ref.PROC_SAMPLE, start=128, **kw)],
                ((0, 0), (), ()))
        pr = torch.from_numpy(np.stack([pc.proc_row(), pc.proc_row(1, 250, ref.PROC_SAMPLE, **kw)])).to(dev)
        res = []
        for step, drawn in enumerate((17, 17)):
            lg = logits.clone().to(dev)                    # .to("cpu") alone would hand out the same tensor
            ops.apply_logit_processors(lg, ls, pr, torch.tensor([5, 300 + step], dtype=torch.int32, device=dev), 150)
            ops.logit_state_count(ls, torch.tensor([drawn, drawn], dtype=torch.int32, device=dev), pr)
            res.append(lg.cpu())
        outs[str(dev)] = (res, ls.state.cpu())
    (cres, cstate), (gres, gstate) = outs["cpu"], outs[str(cuda)]
    assert torch.equal(cstate, gstate)
    for a, b in zip(cres, gres):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert not torch.equal(cres[0].view(torch.int16), cres[1].view(torch.int16))     # the counted id moved on


# ------------------------------------------------------------------ engine and pipeline
NAME = "tiny-llama-d128"
PROMPTS = [[1, 7, 9, 11, 13, 9, 9], [2, 4, 6], [3, 5, 8, 13, 21, 34], [9, 9, 2], [4, 1], [6, 6, 6, 6]]
N_NEW = 14


def _params(asking=True):
    """Greedy requests, all processors on (``asking`` False: the same requests plain); request 2 and 4
    are plain in both."""
    from distributed_llms_amd.engine.sequence import SamplingParams
    kinds = [dict(repetition_penalty=1.6, presence_penalty=0.4, frequency_penalty=0.3, min_tokens=5,
                  logit_bias={21: 3.0, 500: -100.0}),
             # finishes by EOS at its 7th token: with lookahead its row is in one more step, thrown away
             dict(repetition_penalty=0.75, presence_penalty=-0.5, frequency_penalty=1.2, min_tokens=6, ignore_eos=False,
                  logit_bias={7: 2.0, _eos(): 100.0}),
             dict(), dict(repetition_penalty=1.3, presence_penalty=1.0, frequency_penalty=0.5, min_tokens=14,
                          logit_bias={i: 0.25 * (i % 9) for i in range(100, 400)}),
             dict(), dict(repetition_penalty=2.0, presence_penalty=2.0, frequency_penalty=2.0, min_tokens=1,
                          logit_bias={1023: 1.5})]
    return [SamplingParams(**dict(dict(max_new_tokens=N_NEW, ignore_eos=True), **(k if asking else {}))) for k in kinds]


def _eos():
    from distributed_llms_amd.config import get_model_config
    return int(get_model_config(NAME).eos_token_id)


def _state():
    from distributed_llms_amd.config import get_model_config
    from distributed_llms_amd.models import weights as W
    cfg = get_model_config(NAME)
    return cfg, W.synth_hf_state_dict(cfg, seed=9, dtype=torch.float32)


def _ecfg(**kw):
    from distributed_llms_amd.config import EngineConfig
    d = dict(model=NAME, dtype="bfloat16", device="cuda", max_batch=4, max_seq_len=256, num_kv_blocks=128,
             graph_batch_sizes=(1, 2, 4))
    d.update(kw)
    return EngineConfig(**d)


def _engine_run(params, **kw):
    from distributed_llms_amd.engine.llm_engine import LLMEngine
    from distributed_llms_amd.models.stage import ModelStage
    cfg, sd = _state()
    eng = LLMEngine(_ecfg(**kw), ModelStage(cfg, 0, cfg.num_layers, "cuda:0", torch.bfloat16).load_hf_state(sd))
    outs = eng.generate(PROMPTS, params)
    assert eng.scheduler._rows_held == 0
    return outs, eng


@pytest.fixture(scope="module")
def base_run():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    outs, eng = _engine_run(_params())
    assert eng.num_lookahead > 0 and eng.logit_state.allocated
    assert len(outs[1]) == 7 and outs[1][-1] == _eos() and _eos() not in outs[1][:6]
    return outs


def test_engine_plain_requests_beside_asking_ones_are_unchanged(cuda, base_run):
    plain, eng = _engine_run(_params(asking=False))
    assert not eng.logit_state.allocated
    differ = [a != b for a, b in zip(plain, base_run)]
    assert differ == [True, True, False, True, False, True], differ


@pytest.mark.parametrize("mode", ["no-lookahead", "eager", "streams-2", "host-reference"])
def test_engine_tokens_identical_across_modes(cuda, base_run, mode):
    # knob overrides go through the engine's config: a stage runner resets the knobs when it is built
    if mode == "no-lookahead":
        outs, eng = _engine_run(_params(), kernel_knobs={"lookahead": False})
        assert eng.num_lookahead == 0
    elif mode == "eager":
        outs, _ = _engine_run(_params(), use_graphs=False)
    elif mode == "streams-2":
        outs, eng = _engine_run(_params(), streams=2)
        assert eng.num_slots == 2
    else:
        outs, _ = _engine_run(_params(), kernel_knobs={"fused_sampler": False})
        assert not knobs.K.fused_sampler
    assert outs == base_run


def test_two_stage_thread_pipeline_matches_single(cuda, base_run):
    from distributed_llms_amd.parallel.pipeline import run_loopback_pipeline
    _, sd = _state()
    outs, drv, _ = run_loopback_pipeline(_ecfg(), 2, PROMPTS, _params(), device="cuda", hf_state=sd)
    assert outs == base_run and drv.scheduler._rows_held == 0
