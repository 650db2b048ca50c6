"""Request / sequence state.

The reference has no generation loop at all: a "request" is one fan-out of the
same text to every worker and one raw pickled result back.
Here a :class:`Sequence` carries prompt ids, generated ids, sampling params and
per-token timestamps (TTFT / inter-token latency / end-to-end latency metrics).
"""
from __future__ import annotations

import enum
import itertools
import math
import time
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional


class SeqStatus(enum.Enum):
    WAITING = 0
    RUNNING = 1
    FINISHED = 2
    ABORTED = 3


@dataclass
class SamplingParams:
    max_new_tokens: int = 64
    temperature: float = 0.0        # 0 -> greedy (argmax kernel)
    top_k: int = 0
    top_p: float = 1.0
    ignore_eos: bool = False
    seed: Optional[int] = None
    # per-token log-probabilities of the model's distribution: None = off, 0 = the chosen token's
    # only, 1..MAX_LOGPROBS = that many most likely alternatives too (validate_logprobs)
    logprobs: Optional[int] = None
    # logit processors (validate_processors; contract in ops/reference.py), applied to the logits
    # before greedy / sampled selection and before logprobs are taken.  The defaults mean "off"
    repetition_penalty: float = 1.0     # > 0; over prompt + output tokens
    presence_penalty: float = 0.0       # [-2, 2]; over output tokens
    frequency_penalty: float = 0.0      # [-2, 2]; times the output count
    logit_bias: Optional[Dict[int, float]] = None    # <= MAX_LOGIT_BIAS entries, values in [-100, 100]
    min_tokens: int = 0                 # EOS cannot be drawn before this many output tokens
    # the LoRA adapter the request runs with (a name of EngineConfig.lora_modules); None: the base model
    adapter: Optional[str] = None

    @property
    def has_processors(self) -> bool:
        """Whether the request asks for any logit processor (it then holds a LogitState row)."""
        return (self.repetition_penalty != 1.0 or self.presence_penalty != 0.0 or self.frequency_penalty != 0.0
                or bool(self.logit_bias) or self.min_tokens > 0)

    def to_dict(self):
        return dict(self.__dict__)

    @staticmethod
    def from_dict(d):
        return SamplingParams(**{k: v for k, v in (d or {}).items() if k in SamplingParams.__dataclass_fields__})


MAX_LOGPROBS = 20      # ops.MAX_LOGPROBS: the top slots of the kernel


def validate_logprobs(value) -> Optional[int]:
    """``SamplingParams.logprobs`` as the engines take it: None, or an int (not a bool) in
    [0, MAX_LOGPROBS]; anything else raises ValueError."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value <= MAX_LOGPROBS:
        raise ValueError(f"logprobs must be an integer from 0 to {MAX_LOGPROBS}, got {value!r}")
    return value


SAMPLE_MAX_VOCAB = 131072      # ops.SAMPLE_MAX_VOCAB: the row the fused sampler holds in registers


def fused_sampler_serves(device, dtype, kernel_knobs=None) -> bool:
    """Whether a stage on ``device`` with logits of ``dtype`` (a torch dtype or its EngineConfig name) draws
    sampled rows with the fused HIP sampler (ops.sample_rows) and not the host reference."""
    from .. import knobs
    on = (kernel_knobs or {}).get("fused_sampler", knobs.K.fused_sampler)
    return bool(on) and str(device).startswith("cuda") and str(dtype).replace("torch.", "") == "bfloat16"


def validate_sampling(params, vocab_size: int, fused: bool) -> None:
    """A request with temperature > 0 on a vocabulary the fused sampler cannot hold is refused when it is
    admitted (ValueError): ops.sample_rows would raise inside a running step, after the step's KV was
    written and with every other sequence of the batch in flight.  ``params``: a SamplingParams or a dict
    of its fields; ``fused``: fused_sampler_serves() of the sampling stage."""
    t = params.get("temperature", 0.0) if isinstance(params, dict) else params.temperature
    if fused and vocab_size > SAMPLE_MAX_VOCAB and isinstance(t, (int, float)) and t > 0:
        raise ValueError(f"temperature > 0 is not supported on this model: its vocabulary of {vocab_size} exceeds "
                         f"the {SAMPLE_MAX_VOCAB} entries the fused GPU sampler holds; send temperature 0 (greedy) "
                         f"or run with kernel_knobs fused_sampler=0 (host sampler)")


MAX_LOGIT_BIAS = 300   # ops.reference.MAX_LOGIT_BIAS: bias entries of one request
PROCESSOR_KEYS = ("repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias", "min_tokens")


def _number(name: str, value, lo: float, hi: float, lo_open: bool = False) -> float:
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) \
            or not (lo < value if lo_open else lo <= value) or not value <= hi:
        raise ValueError(f"{name} must be a number in {'(' if lo_open else '['}{lo:g}, {hi:g}], got {value!r}")
    return float(value)


def validate_processors(params, vocab_size: int) -> bool:
    """The logit-processor fields of ``params`` (a SamplingParams, or a dict of its fields as the
    master and the HTTP front end hold them) as the engines take them; ``logit_bias`` is normalised
    in place to {int id: float} (JSON delivers string keys).  Returns whether the request asks for
    any processor; a bad value raises ValueError."""
    is_dict = isinstance(params, dict)
    defaults = SamplingParams.__dataclass_fields__

    def get(k):
        return params.get(k, defaults[k].default) if is_dict else getattr(params, k)

    def put(k, v):
        if is_dict:
            if k in params:
                params[k] = v
        else:
            setattr(params, k, v)

    rep = _number("repetition_penalty", get("repetition_penalty"), 0.0, math.inf, lo_open=True)
    pres = _number("presence_penalty", get("presence_penalty"), -2.0, 2.0)
    freq = _number("frequency_penalty", get("frequency_penalty"), -2.0, 2.0)
    for k, x in (("repetition_penalty", rep), ("presence_penalty", pres), ("frequency_penalty", freq)):
        put(k, x)
    bias = get("logit_bias")
    if bias is not None:
        if not isinstance(bias, dict) or len(bias) > MAX_LOGIT_BIAS:
            raise ValueError(f"logit_bias must be an object of at most {MAX_LOGIT_BIAS} entries")
        norm: Dict[int, float] = {}
        for k, x in bias.items():
            try:
                if isinstance(k, (bool, float)):
                    raise ValueError
                t = int(k)
            except (TypeError, ValueError):
                raise ValueError(f"logit_bias key {k!r} is not a token id") from None
            if not 0 <= t < vocab_size:
                raise ValueError(f"logit_bias token id {t} outside [0, {vocab_size})")
            if t in norm:
                raise ValueError(f"logit_bias names token id {t} twice")
            norm[t] = _number(f"logit_bias[{t}]", x, -100.0, 100.0)
        bias = norm or None
        put("logit_bias", bias)
    mt = get("min_tokens")
    max_new = get("max_new_tokens")
    if isinstance(mt, bool) or not isinstance(mt, int) or not 0 <= mt <= max_new:
        raise ValueError(f"min_tokens must be an integer from 0 to max_new_tokens ({max_new}), got {mt!r}")
    return rep != 1.0 or pres != 0.0 or freq != 0.0 or bool(bias) or mt > 0


def resolve_adapter(adapter, slots: Dict[str, int]) -> int:
    """The slot of a request's ``adapter`` among the engine's adapters (``slots``: name -> slot,
    models/lora.py adapter_slots), -1 for None; an unknown name raises ValueError."""
    if adapter is None:
        return -1
    if not isinstance(adapter, str) or adapter not in slots:
        raise ValueError(f"unknown adapter {adapter!r} (configured: {sorted(slots)})")
    return slots[adapter]


_ids = itertools.count(1)

SEED_MASK = (1 << 64) - 1


def request_seed(params: SamplingParams, rng) -> int:
    """The seed a request samples with: the user's, masked to 64 bits, or one drawn from ``rng``
    (a ``random.Random``) once per request; greedy requests need none."""
    if params.temperature <= 0:
        return 0
    if params.seed is None:
        return rng.getrandbits(64)
    return int(params.seed) & SEED_MASK


def split_seed(seed: int):
    """A 64-bit seed as (low, high) signed 32-bit words, the wire form of ``HostBatch.sample_seeds``."""
    def i32(w):
        return (w ^ 0x80000000) - 0x80000000
    return i32(seed & 0xFFFFFFFF), i32((seed >> 32) & 0xFFFFFFFF)


@dataclass
class Sequence:
    prompt: List[int]
    params: SamplingParams = field(default_factory=SamplingParams)
    eos_token_id: Optional[int] = None
    seq_id: int = field(default_factory=lambda: next(_ids))
    request_id: Optional[str] = None
    output: List[int] = field(default_factory=list)
    status: SeqStatus = SeqStatus.WAITING
    num_cached: int = 0              # tokens whose K/V are in the paged cache
    chunk: int = 0                   # prefill tokens scheduled in the current step (0 = all the rest)
    slot: int = -1                   # pipeline microbatch slot
    arrival: float = field(default_factory=time.perf_counter)
    first_token_time: Optional[float] = None
    finish_time: Optional[float] = None
    token_times: List[float] = field(default_factory=list)
    finish_reason: Optional[str] = None
    # the 64-bit sampling seed of the request (request_seed), fixed at admission: preemption,
    # chunked prefill and recompute draw token n from Philox(seed, n) again
    seed: int = 0
    # requests with params.logprobs set: one (chosen_lp, top_ids, top_lps) per generated token
    logprobs: List[tuple] = field(default_factory=list)
    # requests with logit processors: their LogitState row, handed out by the Scheduler at admission,
    # kept through preemption, released at finish or abort (-1: none)
    state_row: int = -1
    # prefix caching: tokens this sequence did not compute because their K/V blocks were found in the
    # paged cache at admission (summed over re-admissions after preemption); prefix_hit: the hit of an
    # acquisition whose first step has not been admitted yet
    cached_tokens: int = 0
    prefix_hit: int = 0
    # prefix caching: whether this admission's query is in the cache's queried-tokens counter already
    # (a sequence that found nothing and could not be admitted is looked up again on every pass), and
    # the prompt ids as the int32 array the block manager takes (made once by the scheduler)
    prefix_queried: bool = False
    # the slot of params.adapter among the engine's adapters (resolve_adapter), -1: the base model
    lora_slot: int = -1
    prompt_i32: Optional[Any] = field(default=None, repr=False, compare=False)

    def __post_init__(self):
        if not self.prompt:
            raise ValueError("empty prompt")
        self.prompt = [int(t) for t in self.prompt]

    @property
    def num_logprobs(self) -> int:
        """The row's ``HostBatch.logprobs`` word: -1 when the request did not ask."""
        n = self.params.logprobs
        return -1 if n is None else int(n)

    @property
    def total_len(self) -> int:
        return len(self.prompt) + len(self.output)

    @property
    def prefill_len(self) -> int:
        """Tokens the current prefill step computes for this sequence (a chunk of a long prompt,
        or everything not yet in the KV cache)."""
        return self.chunk or (self.total_len - self.num_cached)

    def all_tokens(self) -> List[int]:
        return self.prompt + self.output

    def last_token(self) -> int:
        return self.output[-1] if self.output else self.prompt[-1]

    @property
    def finished(self) -> bool:
        return self.status in (SeqStatus.FINISHED, SeqStatus.ABORTED)

    def append(self, tok: int, now: Optional[float] = None) -> bool:
        """Append a generated token; returns True if the sequence just finished."""
        now = time.perf_counter() if now is None else now
        self.output.append(tok if type(tok) is int else int(tok))
        self.token_times.append(now)
        if self.first_token_time is None:
            self.first_token_time = now
        if (not self.params.ignore_eos and self.eos_token_id is not None and tok == self.eos_token_id):
            self.finish("eos", now)
        elif len(self.output) >= self.params.max_new_tokens:
            self.finish("length", now)
        return self.finished

    def finish(self, reason: str, now: Optional[float] = None):
        self.status = SeqStatus.FINISHED if reason != "abort" else SeqStatus.ABORTED
        self.finish_reason = reason
        self.finish_time = time.perf_counter() if now is None else now

    # metrics
    def ttft(self) -> Optional[float]:
        return None if self.first_token_time is None else self.first_token_time - self.arrival

    def latency(self) -> Optional[float]:
        return None if self.finish_time is None else self.finish_time - self.arrival

    def itl(self) -> List[float]:
        t = self.token_times
        return [b - a for a, b in zip(t, t[1:])]
