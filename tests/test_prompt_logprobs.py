"""Prompt scoring on the CPU: the contract (ops/reference.py lm_head_logprobs) on hand-made rows, and
SamplingParams.prompt_logprobs through the float32 engine, the HostBatch section and the HTTP front end."""
import json
import math
import urllib.request

import numpy as np
import pytest
import torch

from distributed_llms_amd import ops
from distributed_llms_amd.config import EngineConfig
from distributed_llms_amd.engine.batch import HostBatch, build_host_batch
from distributed_llms_amd.engine.llm_engine import LLMEngine
from distributed_llms_amd.engine.sequence import SamplingParams


def _call(x, w, targets, dtype=torch.float32):
    return ops.lm_head_logprobs(torch.tensor(x, dtype=dtype), torch.tensor(w, dtype=dtype),
                                torch.tensor(targets, dtype=torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_hand_made_rows(dtype):
    """Two equal logits: ln 2; a skipped row: 0.0; a target at the last column of logits (0, 1, 3)."""
    w = [[0.0, 0.0], [0.0, 1.0], [0.0, 3.0]]
    got = _call([[1.0, 0.0], [5.0, 7.0], [0.0, 1.0]], w, [1, -1, 2], dtype)
    last = -math.log(1 + math.exp(-2) + math.exp(-3))
    assert got.dtype == torch.float32 and got.tolist() == pytest.approx([-math.log(3), 0.0, last], abs=1e-6)
    assert _call([[1.0, 0.0]], w[:2], [0]).item() == pytest.approx(-math.log(2), abs=1e-7)


# ------------------------------------------------------------------ CPU engine, HostBatch, HTTP
PROMPTS = [list(range(10, 40)), [1, 5, 9, 200], [8] * 13]
ASKS = [True, False, True]


def _engine(asks=(), n=12, **kw):
    cfg = dict(model="synthetic:tiny-llama", device="cpu", dtype="float32", max_batch=8, max_seq_len=128,
               use_graphs=False, num_kv_blocks=128)
    eng = LLMEngine(EngineConfig(**dict(cfg, **kw)))
    return eng, [eng.add_request(p, SamplingParams(max_new_tokens=n, ignore_eos=True, prompt_logprobs=a))
                 for p, a in zip(PROMPTS, asks)]


@pytest.fixture(scope="module")
def expected():
    """Per prompt: (log_softmax of the engine's own full-prompt logits, one bf16 rounding through target and sum)."""
    out = []
    for p in PROMPTS:
        eng, _ = _engine()
        eng.add_request(p, SamplingParams(max_new_tokens=1))
        hb = build_host_batch(eng.scheduler.schedule(0), eng.bm, eng.ecfg.kv_block_size)
        hb.logits_idx = np.arange(len(p), dtype=np.int32)          # every row's logits
        lg = eng.runner.execute(hb).double()
        lp = torch.log_softmax(lg, -1)[torch.arange(len(p) - 1), torch.tensor(p[1:])]
        out.append((lp.tolist(), 2 * 2.0 ** -9 * lg.abs().max().item()))
    return out


@pytest.mark.parametrize("kw,preempts,mixed", [
    (dict(), False, False),
    (dict(max_prefill_tokens=8, mixed_prefill_tokens=0), False, False),
    (dict(max_prefill_tokens=8, mixed_prefill_tokens=8), False, True),
    (dict(num_kv_blocks=6, kv_block_size=16), True, False)], ids=["whole", "chunked", "mixed", "preempting"])
def test_engine_prompt_logprobs(expected, kw, preempts, mixed):
    """Every variant is held to ONE expected list within the contract's single bf16 rounding.  Bit equality between
    variants cannot hold: chunked float32 attention changes a logit's last bits, which can move that rounding."""
    eng, seqs = _engine(ASKS, **kw)
    eng.run_until_done()
    assert (eng.scheduler.num_preemptions > 0) == preempts and (eng.scheduler.num_mixed > 0) == mixed
    for s, a, (want, bound) in zip(seqs, ASKS, expected):
        if not a:
            assert s.prompt_logprobs is None
            continue
        assert len(s.prompt_logprobs) == len(s.prompt) and s.prompt_logprobs[0] is None
        err = max(abs(g - w) for g, w in zip(s.prompt_logprobs[1:], want))
        assert err <= bound, (err, bound)


def test_host_batch_is_unchanged_when_nobody_asks():
    """The asking step's packed words are the plain step's, header word 14 set and the section appended."""
    def packed(asks):
        eng, _ = _engine(asks, n=4)
        return build_host_batch(eng.scheduler.schedule(0), eng.bm, eng.ecfg.kv_block_size, None, 7).pack()
    plain, asked = packed([False] * 3), packed(ASKS)
    a = HostBatch.unpack(asked)
    assert plain[14] == 0 and HostBatch.unpack(plain).score_idx is None and asked[14] == 1
    assert np.array_equal(np.delete(asked[:len(plain)], 14), np.delete(plain, 14)) and len(asked) == len(plain) + 83
    assert a.score_idx.tolist() == list(range(29)) + list(range(34, 46))
    assert a.score_targets.tolist() == PROMPTS[0][1:] + PROMPTS[2][1:]


def _refusing(how):
    eng = _engine()[0]
    eng.tp = object() if how == "tp" else None                               # a tensor-parallel leader
    if how == "head":
        eng.stage.head["lm_head"] = torch.zeros(2, 2, dtype=torch.int8)      # a quantised LM head
    return eng


@pytest.mark.parametrize("value,how", [(1, None), ("yes", None), (True, "head"), (True, "tp")])
def test_refusals_at_admission(value, how):
    with pytest.raises(ValueError):
        _refusing(how).add_request([1, 2], SamplingParams(prompt_logprobs=value))


def test_http_prompt_logprobs(expected):
    """The HTTP front end over a master whose stage 0 is a CPU engine in this process: what the worker would
    send (RESULT, or ERROR for a request refused at admission) goes through the master's own message handler."""
    from distributed_llms_amd.master.http_api import serve_http
    from distributed_llms_amd.master.node import MasterNode
    from distributed_llms_amd.network.protocol import pack_prompt_logprobs, pack_result

    class Master(MasterNode):
        how = None
        def _send_request(self, ids, params, fut, stream_q, hint, attempts):
            self._tasks["t"] = fut
            eng = _refusing(self.how)
            try:
                s = eng.add_request(ids, SamplingParams.from_dict(params))
            except ValueError as e:
                err = {"task_id": "t", "error": str(e), "refused": True}
                return self._handle_worker_command("w0", "ERROR", err, None)
            eng.run_until_done()
            meta, payload = {"task_id": "t", "num_tokens": len(s.output)}, pack_result(s.output)
            if s.prompt_logprobs is not None:
                s.prompt_logprobs[1] = -math.inf if len(ids) == 3 else s.prompt_logprobs[1]
                meta["prompt_logprobs"] = len(ids)
                payload += pack_prompt_logprobs(s.prompt_logprobs)
            self._handle_worker_command("w0", "RESULT", meta, payload)

    m = Master("127.0.0.1", 0, EngineConfig(model="synthetic:tiny-llama", device="cpu", dtype="float32"))
    m.initialize_model("synthetic:tiny-llama", 1)
    m.state, m.stage_workers = "ready", ["w0"]
    srv, _ = serve_http(m, "127.0.0.1", 0)

    def post(path, body):
        req = urllib.request.Request(f"http://127.0.0.1:{srv.server_address[1]}{path}", data=json.dumps(body).encode())
        with urllib.request.urlopen(req, timeout=120) as r:
            return json.loads(r.read())
    try:
        want, bound = expected[2]
        g = post("/generate", {"prompt_ids": PROMPTS[2], "max_new_tokens": 2, "prompt_logprobs": True})
        assert g["prompt_logprobs"][0] is None and g["prompt_logprobs"][1:] == pytest.approx(want, rel=0, abs=bound)
        assert "prompt_logprobs" not in post("/generate", {"prompt_ids": PROMPTS[2], "max_new_tokens": 2})
        c = post("/v1/completions", {"prompt": PROMPTS[2], "max_tokens": 2, "prompt_logprobs": True, "n": 2})
        assert [ch["prompt_logprobs"] for ch in c["choices"]] == [g["prompt_logprobs"]] * 2
        inf = post("/generate", {"prompt_ids": [1, 2, 3], "max_new_tokens": 1, "prompt_logprobs": True})
        assert inf["prompt_logprobs"][:2] == [None, None] and inf["prompt_logprobs"][2] is not None     # -inf: null
        yes = {"prompt_logprobs": True}
        for body, stages, how in (({"prompt_logprobs": 1}, 1, None), (dict(yes, stream=True), 1, None), (yes, 2, None),
                                  (yes, 1, "head"), (yes, 1, "tp")):
            m.stage_workers, m.how = ["w"] * stages, how
            for path in ("/generate", "/v1/completions"):
                with pytest.raises(urllib.request.HTTPError) as ei:
                    post(path, dict(body, prompt=[1, 2, 3], prompt_ids=[1, 2, 3]))
                assert ei.value.code == 400, (path, body, how)
    finally:
        srv.shutdown()
