"""Multi-LoRA through the distributed paths on CPU: the in-process loopback pipeline, and a master
with two real ``run_worker.py`` processes (gloo pipeline) behind the HTTP front end."""
import json
import os
import subprocess
import sys
import urllib.error
import urllib.request

import pytest

from distributed_llms_amd.config import EngineConfig
from distributed_llms_amd.engine.llm_engine import LLMEngine
from distributed_llms_amd.engine.sequence import SamplingParams
from distributed_llms_amd.master.node import MasterNode
from distributed_llms_amd.parallel.pipeline import run_loopback_pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = "synthetic:tiny-llama"
ADAPTERS = {"alpha": "synthetic:8:11", "beta": "synthetic:16:12:q_proj+v_proj+down_proj"}
PROMPTS = [[3, 5, 7, 9, 11], [20, 21, 22], [100, 4, 4, 4, 4, 4, 4, 4, 9]]
WHO = [None, "alpha", "beta"]


def _cfg(**kw):
    return EngineConfig(model=MODEL, dtype="float32", device="cpu", max_batch=8, max_seq_len=128, use_graphs=False,
                        num_kv_blocks=128, heartbeat_interval=0.5, heartbeat_timeout=4.0,
                        lora_modules=dict(ADAPTERS), **kw)


def _params(who, n=6):
    return SamplingParams(max_new_tokens=n, ignore_eos=True, adapter=who)


@pytest.fixture(scope="module")
def single():
    """Each request's tokens from the single CPU engine, and the base model's for the adapter prompts."""
    eng = LLMEngine(_cfg())
    return eng.generate(PROMPTS, [_params(w) for w in WHO]), eng.generate(PROMPTS, _params(None))


def test_loopback_pipeline_matches_single_engine(single):
    outs = run_loopback_pipeline(_cfg(), 2, PROMPTS, [_params(w) for w in WHO], device="cpu")
    outs = outs[0] if isinstance(outs, tuple) else outs
    assert outs == single[0]
    assert single[0][1] != single[1][1] and single[0][2] != single[1][2], "the adapters must change the tokens"


@pytest.mark.slow
def test_two_worker_pipeline_and_http(single):
    from distributed_llms_amd.master.http_api import serve_http
    m = MasterNode("127.0.0.1", 0, _cfg()).start()
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    procs = []
    srv = None
    try:
        m.initialize_model(MODEL, num_shards=2)
        for _ in range(2):
            procs.append(subprocess.Popen(
                [sys.executable, os.path.join(ROOT, "run_worker.py"), "--master", f"127.0.0.1:{m.port}", "--device",
                 "cpu", "--port", "0", "--heartbeat", "0.5", "--log-level", "WARNING"], env=env,
                stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL))
        m.wait_for_workers(2, timeout=120)
        m.assign_shards()
        m.distribute_shards(timeout=300)
        # the gloo pipeline, requests of three kinds in one batch
        futs = [m.submit(p, dict(max_new_tokens=6, ignore_eos=True, adapter=w)) for p, w in zip(PROMPTS, WHO)]
        assert [m._finish(f, 120)["tokens"] for f in futs] == single[0]
        with pytest.raises(ValueError, match="unknown adapter"):
            m.submit(PROMPTS[0], dict(max_new_tokens=2, adapter="gamma"))
        srv, _ = serve_http(m, "127.0.0.1", 0)
        base = f"http://127.0.0.1:{srv.server_address[1]}"

        def post(path, body):
            req = urllib.request.Request(base + path, data=json.dumps(body).encode(),
                                         headers={"Content-Type": "application/json"})
            with urllib.request.urlopen(req, timeout=120) as r:
                return json.loads(r.read())

        g = post("/generate", {"prompt_ids": PROMPTS[1], "max_new_tokens": 6, "ignore_eos": True, "adapter": "alpha"})
        assert g["tokens"] == single[0][1] and g["model"] == "alpha"
        g = post("/generate", {"prompt_ids": PROMPTS[1], "max_new_tokens": 6, "ignore_eos": True})
        assert g["tokens"] == single[1][1] and "model" not in g
        # "model" equal to an adapter name selects it; any other value stays ignored
        c = post("/v1/completions", {"prompt": PROMPTS[2], "max_tokens": 6, "ignore_eos": True, "model": "beta"})
        assert c["choices"][0]["tokens"] == single[0][2] and c["model"] == "beta"
        c = post("/v1/completions", {"prompt": PROMPTS[2], "max_tokens": 6, "ignore_eos": True, "model": "gpt-x"})
        assert c["choices"][0]["tokens"] == single[1][2] and c["model"] == m.model_spec
        for path in ("/generate", "/v1/completions"):
            with pytest.raises(urllib.error.HTTPError) as ei:
                post(path, {"prompt": PROMPTS[0], "adapter": "gamma"})
            assert ei.value.code == 400
        with urllib.request.urlopen(base + "/status", timeout=60) as r:
            assert json.loads(r.read())["adapters"] == ["alpha", "beta"]
    finally:
        if srv is not None:
            srv.shutdown()
        m.stop()
        for p in procs:
            try:
                p.wait(timeout=15)
            except subprocess.TimeoutExpired:
                p.kill()
