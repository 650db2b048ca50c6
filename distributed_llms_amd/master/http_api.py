"""HTTP front end of the master: the serving entry point for clients that are not Python.

The reference has an interactive REPL only (``run_master.py:26-42``); a ``/status`` HTTP
endpoint and Prometheus metrics appear in its docs (``implementation.md:34-41,80-83``).
Here ``run_master.py --http PORT`` serves, from a threaded stdlib HTTP server (no extra
dependency; every request thread only submits to the master's request futures):

  GET  /health                 {"state": "ready" | "degraded" | "idle", "workers": n}
  GET  /status                 the master's STATUS fan-out (workers, KV occupancy, metrics)
  GET  /metrics                Prometheus text: request metrics + per-worker gauges (HBM, KV blocks,
                               running / waiting sequences, microbatches executed)
  POST /generate               {"prompt": str | "prompt_ids": [int], "max_new_tokens", "temperature",
                                "top_k", "top_p", "ignore_eos", "logprobs", "repetition_penalty",
                                "presence_penalty", "frequency_penalty", "logit_bias", "min_tokens"} ->
                                {"tokens", "text", "latency_s", ...}; with "logprobs": n (0..20) also
                                "logprobs": {"token_logprobs", "top_ids", "top_logprobs"}
  POST /v1/completions         OpenAI-style: {"prompt": str | [int] | [str...], "max_tokens", ...}
                               -> {"object": "text_completion", "choices": [...], "usage": {...}};
                               "logprobs": n (0..20) adds to each choice the legacy object {"tokens",
                               "token_logprobs", "top_logprobs": [{text: lp}], "text_offset"} plus
                               "token_ids" / "top_token_ids" (two ids can decode to the same text);
                               -inf is serialised as null
  logit processors             (either POST, also with "stream") "repetition_penalty" (> 0, over prompt and
                               output tokens), "presence_penalty" / "frequency_penalty" ([-2, 2], over output
                               tokens), "logit_bias" ({"token id": bias in [-100, 100]}, at most 300 entries,
                               OpenAI's string keys), "min_tokens" (no EOS before that many tokens).  They
                               rewrite the logits that greedy selection, sampling and "logprobs" then see;
                               a value out of range: 400
  "n": k                       (either POST, 1..16, not with "stream") k completions per prompt, submitted as k
                               plain requests: child j of a request with "seed" s samples with seed
                               (s + j) mod 2^64, without a seed every child draws its own.  /v1/completions:
                               choices[i * k + j] is child j of prompt i, "usage.prompt_tokens" counts each
                               prompt once and "usage.prompt_tokens_details.cached_tokens" the prompt tokens
                               found in the prefix cache (EngineConfig.enable_prefix_caching); /generate with
                               k > 1: {"results": [the k replies]}.  Anything else: 400
  "adapter": name              (either POST, also with "stream" and "n") run the request with that LoRA adapter
                               of EngineConfig.lora_modules; a "model" equal to a configured adapter name
                               selects it too (any other "model" value is ignored).  An unknown "adapter":
                               400.  The reply's "model" is the adapter's name when one ran; GET /status
                               lists the configured names under "adapters"
  "stream": true               (either POST, one prompt) server-sent events: one ``data: {...}`` event
                               per pipeline step that produced tokens (TOKENS messages from stage 0),
                               then ``data: [DONE]`` (not together with "logprobs": 400)

Batches of prompts submitted together are scheduled together (continuous batching on stage 0).
"""
from __future__ import annotations

import json
import logging
import math
import threading
import time
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer
from typing import Any, Dict, List, Tuple

from ..engine.sequence import PROCESSOR_KEYS, validate_logprobs, validate_processors
from ..utils.metrics import cluster_prometheus_text

log = logging.getLogger("dllm.http")

_PARAM_KEYS = ("temperature", "top_k", "top_p", "ignore_eos", "seed", "logprobs") + PROCESSOR_KEYS


def _sampling(body: Dict[str, Any], default_max: int = 64, max_key: str = "max_new_tokens",
              vocab_size: int = 1 << 31, adapters=()) -> Dict[str, Any]:
    """``adapters``: the configured LoRA adapter names."""
    p = {k: body[k] for k in _PARAM_KEYS if k in body}
    adapter = body.get("adapter")
    if adapter is None and isinstance(body.get("model"), str) and body["model"] in adapters:
        adapter = body["model"]
    if adapter is not None:
        if not isinstance(adapter, str) or adapter not in adapters:
            raise ValueError(f"unknown adapter {adapter!r} (configured: {sorted(adapters)})")
        p["adapter"] = adapter
    p["max_new_tokens"] = int(body.get(max_key, body.get("max_new_tokens", default_max)))
    if p["max_new_tokens"] < 1:
        raise ValueError("max tokens must be >= 1")
    validate_logprobs(p.get("logprobs"))
    if p.get("logprobs") is not None and body.get("stream"):
        raise ValueError("logprobs are not available with stream")
    validate_processors(p, vocab_size)       # logit_bias arrives with string keys: {int: float} from here on
    return p


MAX_N = 16


def _num_completions(body: Dict[str, Any]) -> int:
    """The request's ``"n"``: an integer (not a bool) from 1 to MAX_N, not together with "stream"."""
    n = body.get("n")
    if n is None:
        return 1
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= MAX_N:
        raise ValueError(f"n must be an integer from 1 to {MAX_N}, got {n!r}")
    if body.get("stream"):
        raise ValueError("n is not available with stream")
    return n


def _child_params(params: Dict[str, Any], j: int) -> Dict[str, Any]:
    """Child ``j`` of an ``n``-fold request: the same parameters, the seed moved on by j."""
    if j == 0 or params.get("seed") is None:
        return params
    return dict(params, seed=(int(params["seed"]) + j) & ((1 << 64) - 1))


def _finite(x: float):
    """JSON has no -inf: a log-probability of -inf is serialised as null."""
    return x if math.isfinite(x) else None


def _generate_logprobs(lp: Dict[str, Any]) -> Dict[str, Any]:
    return {"token_logprobs": [_finite(x) for x in lp["token_logprobs"]], "top_ids": lp["top_ids"],
            "top_logprobs": [[_finite(x) for x in row] for row in lp["top_logprobs"]]}


def _openai_logprobs(tokenizer, tokens: List[int], lp: Dict[str, Any]) -> Dict[str, Any]:
    """The legacy OpenAI completions object, plus the ids (two ids can decode to the same text, and
    then share a key of a ``top_logprobs`` dict: the more likely one, listed first, keeps it)."""
    texts = [tokenizer.decode([t]) for t in tokens]
    offsets, o = [], 0
    for t in texts:
        offsets.append(o)
        o += len(t)
    tops = []
    for ids, lps in zip(lp["top_ids"], lp["top_logprobs"]):
        d: Dict[str, Any] = {}
        for i, x in zip(ids, lps):
            d.setdefault(tokenizer.decode([i]), _finite(x))
        tops.append(d)
    return {"tokens": texts, "token_logprobs": [_finite(x) for x in lp["token_logprobs"]], "top_logprobs": tops,
            "text_offset": offsets, "token_ids": list(tokens), "top_token_ids": lp["top_ids"]}


class _Handler(BaseHTTPRequestHandler):
    server_version = "dllm-master/1"
    master = None            # set by serve_http
    timeout_s = 600.0

    # -------------------------------------------------------------- plumbing
    def log_message(self, fmt, *args):      # route through logging, not stderr
        log.debug("%s " + fmt, self.address_string(), *args)

    def _send(self, code: int, obj: Any, ctype: str = "application/json"):
        data = obj.encode() if isinstance(obj, str) else json.dumps(obj, default=str).encode()
        self.send_response(code)
        self.send_header("Content-Type", ctype)
        self.send_header("Content-Length", str(len(data)))
        self.end_headers()
        self.wfile.write(data)

    def _body(self) -> Dict[str, Any]:
        n = int(self.headers.get("Content-Length") or 0)
        if n > 64 << 20:
            raise ValueError("request body too large")
        raw = self.rfile.read(n) if n else b"{}"
        body = json.loads(raw or b"{}")
        if not isinstance(body, dict):
            raise ValueError("JSON object expected")
        return body

    # -------------------------------------------------------------- routes
    def do_GET(self):
        m = self.master
        try:
            if self.path == "/health":
                self._send(200, {"state": m.state, "workers": len(m.workers)})
            elif self.path == "/status":
                self._send(200, m.status())
            elif self.path == "/metrics":
                self._send(200, cluster_prometheus_text(m.status()), "text/plain; version=0.0.4")
            else:
                self._send(404, {"error": f"no route {self.path}"})
        except Exception as e:  # noqa: BLE001 - reported to the client
            self._send(500, {"error": repr(e)})

    def do_POST(self):
        try:
            body = self._body()
            if body.get("stream") and self.path in ("/generate", "/v1/completions"):
                return self._stream(body)
            if self.path == "/generate":
                self._send(200, self._generate(body))
            elif self.path == "/v1/completions":
                self._send(200, self._completions(body))
            else:
                self._send(404, {"error": f"no route {self.path}"})
        except (ValueError, KeyError, TypeError) as e:
            self._send(400, {"error": repr(e)})
        except Exception as e:  # noqa: BLE001 - worker failures, timeouts
            self._send(503, {"error": repr(e)})

    def _stream(self, body: Dict[str, Any]):
        """Server-sent events: token chunks as stage 0 produces them, then [DONE]."""
        completions = self.path == "/v1/completions"
        _num_completions(body)
        prompt = body["prompt_ids"] if "prompt_ids" in body else body.get("prompt", "")
        ids = self._ids(prompt)
        if not ids:
            raise ValueError("empty prompt")
        params = _sampling(body, default_max=16 if completions else 64,
                           max_key="max_tokens" if completions else "max_new_tokens", vocab_size=self._vocab(),
                           adapters=self._adapters())
        model = params.get("adapter") or self.master.model_spec
        gen = self.master.stream(ids, timeout=self.timeout_s, **params)
        first = next(gen, None)                       # errors before the first byte -> HTTP status
        self.send_response(200)
        self.send_header("Content-Type", "text/event-stream")
        self.send_header("Cache-Control", "no-cache")
        self.send_header("Connection", "close")
        self.end_headers()
        tok = self.master.tokenizer

        def event(chunk):
            if completions:
                obj = {"object": "text_completion", "model": model,
                       "choices": [{"index": 0, "text": tok.decode(chunk), "tokens": chunk, "finish_reason": None}]}
            else:
                obj = {"tokens": chunk, "text": tok.decode(chunk)}
            self.wfile.write(b"data: " + json.dumps(obj).encode() + b"\n\n")
            self.wfile.flush()

        try:
            if first is not None:
                event(first)
            for chunk in gen:
                event(chunk)
            self.wfile.write(b"data: [DONE]\n\n")
        except Exception as e:  # noqa: BLE001 - mid-stream failure: report in-band
            self.wfile.write(b"data: " + json.dumps({"error": repr(e)}).encode() + b"\n\n")
        self.wfile.flush()
        self.close_connection = True

    def _vocab(self) -> int:
        cfg = getattr(self.master, "model_config", None)
        return int(cfg.vocab_size) if cfg is not None else 1 << 31

    def _adapters(self):
        cfg = getattr(self.master, "config", None)
        return tuple(getattr(cfg, "lora_modules", None) or ())

    def _ids(self, prompt) -> List[int]:
        if isinstance(prompt, str):
            return self.master.tokenizer.encode(prompt)
        if isinstance(prompt, list) and all(isinstance(t, int) for t in prompt):
            return list(prompt)
        raise ValueError("prompt must be a string or a list of token ids")

    def _run(self, prompts: List[List[int]], params: Dict[str, Any], n: int = 1) -> List[Dict[str, Any]]:
        """``n`` results per prompt, prompt-major (result i * n + j: child j of prompt i)."""
        if not prompts or any(not p for p in prompts):
            raise ValueError("empty prompt")
        m = self.master
        # submitted together -> batched together (the children of a prompt share its blocks
        # through the prefix cache when the engines run with one)
        futs = [m.submit(p, _child_params(params, j)) for p in prompts for j in range(n)]
        out = []
        for f in futs:
            r = m._finish(f, self.timeout_s)
            r["text"] = m.tokenizer.decode(r["tokens"])
            if r.get("logprobs") is None:
                r.pop("logprobs", None)                # a request that did not ask: the reply it always got
            if not r.get("cached_tokens"):
                r.pop("cached_tokens", None)           # no hit (or no cache): likewise
            out.append(r)
        return out

    def _generate(self, body: Dict[str, Any]) -> Dict[str, Any]:
        ids = body["prompt_ids"] if "prompt_ids" in body else self._ids(body.get("prompt", ""))
        n = _num_completions(body)
        params = _sampling(body, vocab_size=self._vocab(), adapters=self._adapters())
        res = self._run([self._ids(ids)], params, n)
        for r in res:
            if params.get("adapter"):
                r["model"] = params["adapter"]
            if "logprobs" in r:
                r["logprobs"] = _generate_logprobs(r["logprobs"])
        return res[0] if n == 1 else {"results": res}

    def _completions(self, body: Dict[str, Any]) -> Dict[str, Any]:
        prompt = body.get("prompt", "")
        if isinstance(prompt, list) and prompt and not all(isinstance(t, int) for t in prompt):
            prompts = [self._ids(p) for p in prompt]           # a batch of prompts
        else:
            prompts = [self._ids(prompt)]
        n = _num_completions(body)
        params = _sampling(body, default_max=16, max_key="max_tokens", vocab_size=self._vocab(),
                           adapters=self._adapters())
        res = self._run(prompts, params, n)
        choices = [{"index": i, "text": r["text"], "tokens": r["tokens"],
                    "finish_reason": "length" if r.get("finish_reason") in ("length", "max_seq_len") else "stop"}
                   for i, r in enumerate(res)]
        for c, r in zip(choices, res):
            if "logprobs" in r:
                c["logprobs"] = _openai_logprobs(self.master.tokenizer, r["tokens"], r["logprobs"])
        ptok = sum(len(p) for p in prompts)
        ctok = sum(len(r["tokens"]) for r in res)
        return {"id": res[0].get("task_id"), "object": "text_completion", "created": int(time.time()),
                "model": params.get("adapter") or self.master.model_spec, "choices": choices,
                "usage": {"prompt_tokens": ptok, "completion_tokens": ctok, "total_tokens": ptok + ctok,
                          "prompt_tokens_details": {"cached_tokens": sum(int(r.get("cached_tokens") or 0)
                                                                         for r in res)}}}


def serve_http(master, host: str = "127.0.0.1", port: int = 8000,
               timeout_s: float = 600.0) -> Tuple[ThreadingHTTPServer, threading.Thread]:
    """Start the HTTP front end on a daemon thread; returns (server, thread).  port 0 = any free port
    (``server.server_address[1]``).  ``server.shutdown()`` stops it."""
    handler = type("Handler", (_Handler,), {"master": master, "timeout_s": timeout_s})
    srv = ThreadingHTTPServer((host, port), handler)
    srv.daemon_threads = True
    th = threading.Thread(target=srv.serve_forever, name="dllm-http", daemon=True)
    th.start()
    log.info("HTTP API on http://%s:%d", host, srv.server_address[1])
    return srv, th
