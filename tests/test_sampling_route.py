"""Kernel or reference, for every op of the sampling stage, against a table recorded before ops/sampling.py and
its route() existed.

tests/golden/sampling_routes.json holds, for the grid below, what the wrapper did with the input: "kernel" (it
called its native launcher), "reference" (it did not), "reference-warn" (nor did it, and the once-per-process
host-sampler warning fired) or the name of the exception it raised.

The harness drives the public wrappers on meta tensors: the module's _gpu says what the row's device column says,
_ext.kernels is a recorder, torch.cuda.current_stream is replaced and the ops/reference.py functions are wrapped so
that they record and compute nothing.  It finds the wrappers' module by getattr(ops, "sampling", ops), so run_row
and the table pass unchanged at the commit before the move, where the table was recorded (``python
tests/test_sampling_route.py --record`` rewrites it from whatever tree it runs in).  On top of that, route() must
return the recorded outcome for the row's description, or raise the recorded exception."""
import itertools
import json
import os
import sys
import types

import pytest
import torch

from distributed_llms_amd import _ext, knobs, ops
from distributed_llms_amd.ops import reference as ref

TABLE = os.path.join(os.path.dirname(__file__), "golden", "sampling_routes.json")
COLUMNS = ["op", "device", "dtype", "last_stride", "row_stride", "rows", "vocab", "fused", "outcome"]
N_IN = 8
OPS = ["argmax", "sample_rows", "token_logprobs", "apply_logit_processors", "logit_state_update", "logit_state_count",
       "lm_head_logprobs"]
STATE_OPS = ("logit_state_update", "logit_state_count")
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
K = 64                                      # lm_head_logprobs: x [rows, K], the row stride is against K
STREAM = 0x7E57                             # no real stream's handle (the GEMM workspace is cached per stream)


def grid():
    """The inputs of every row, in table order: the full cross."""
    return [list(r) for r in itertools.product(OPS, ("cpu", "cuda"), DTYPES, (1, 2), ("lt", "eq", "gt"), (1, 2),
                                               (8, 131072, 131073), (1, 0))]


def _i32(*shape):
    return torch.empty(*shape, dtype=torch.int32, device="meta")


def deciding_tensor(inputs):
    """The tensor whose description the row gives: the logits [rows, vocab], lm_head_logprobs' x [rows, K]; the
    two state ops have none (their state is what _ck_state admits: int32, contiguous)."""
    op, _, dtype, last, row, rows, vocab, _ = inputs
    if op in STATE_OPS:
        return None
    width = K if op == "lm_head_logprobs" else vocab
    return torch.empty_strided((rows, width), (width + {"lt": -1, "eq": 0, "gt": 8}[row], last), dtype=DTYPES[dtype],
                               device="meta")


def call(inputs):
    """The row's wrapper call, as a thunk."""
    op, _, dtype, _, _, rows, vocab, _ = inputs
    t = deciding_tensor(inputs)
    ls = types.SimpleNamespace(vocab=vocab, state=_i32(2, -(-vocab // 8) * 8), bias_n=_i32(2), bias_ids=_i32(2, 4),
                               bias_vals=torch.empty(2, 4, device="meta"))
    procs = _i32(rows, ref.PROC_WORDS)
    if op == "argmax":
        return lambda: ops.argmax(t)
    if op == "sample_rows":
        return lambda: ops.sample_rows(t, _i32(rows, 3), torch.empty(rows, dtype=torch.int64, device="meta"), _i32(rows))
    if op == "token_logprobs":
        return lambda: ops.token_logprobs(t, _i32(rows), _i32(rows), 5)
    if op == "apply_logit_processors":
        return lambda: ops.apply_logit_processors(t, ls, procs, _i32(rows), -1)
    if op == "logit_state_update":
        return lambda: ops.logit_state_update(ls, _i32(3), _i32(rows + 1), procs, _i32(rows + 1), _i32(2),
                                              torch.empty(2, device="meta"))
    if op == "logit_state_count":
        return lambda: ops.logit_state_count(ls, _i32(rows), procs)
    return lambda: ops.lm_head_logprobs(t, torch.empty(vocab, K, dtype=DTYPES[dtype], device="meta"), _i32(rows))


class Recorder:
    """Stands in for the extension module: records which launchers are called."""
    LM_HEAD_WAVES = 4

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a: self.calls.append(name)


def run_row(inputs):
    """One wrapper call under the row's device and knob -> the outcome."""
    op, device, fused = inputs[0], inputs[1], inputs[7]
    mod = getattr(ops, "sampling", ops)
    rec, ref_calls = Recorder(), []
    saved = (_ext.kernels, torch.cuda.current_stream, mod._gpu, mod._host_sampler_warned)
    saved_ref = {name: getattr(ref, name) for name in OPS}
    _ext.kernels = lambda: rec
    torch.cuda.current_stream = lambda *a: types.SimpleNamespace(cuda_stream=STREAM)
    mod._gpu = lambda t: device == "cuda"
    mod._host_sampler_warned = False
    for name in OPS:
        setattr(ref, name, lambda *a, _n=name: ref_calls.append(_n))
    try:
        with knobs.override(fused_sampler=bool(fused)):
            call(inputs)()
        warned = mod._host_sampler_warned
    except (TypeError, ValueError) as e:
        return type(e).__name__
    finally:
        _ext.kernels, torch.cuda.current_stream, mod._gpu, mod._host_sampler_warned = saved
        for name, f in saved_ref.items():
            setattr(ref, name, f)
    assert rec.calls in ([], [op]) and ref_calls in ([], [op]) and not (rec.calls and ref_calls), (rec.calls, ref_calls)
    # one of the two ran; only argmax's GPU fallback was, where the table was recorded, an inline torch.argmax
    assert rec.calls or ref_calls or (op, device) == ("argmax", "cuda"), inputs
    assert not (warned and rec.calls)
    return "kernel" if rec.calls else "reference-warn" if warned else "reference"


def route_row(inputs):
    """route() on the row's description, as the wrapper derives it from the deciding tensor."""
    op, device, dtype, last, _, rows, vocab, fused = inputs
    t = deciding_tensor(inputs)
    if t is None:                            # state ops: route() must not look at the logits' columns
        unit, row_stride = last == 1, vocab
    else:
        unit, row_stride = (t.is_contiguous() if op == "lm_head_logprobs" else t.stride(-1) == 1), t.stride(0)
    try:
        return ops.sampling.route(op, is_cuda=device == "cuda", dtype=DTYPES[dtype], unit_stride=unit,
                                  row_stride=row_stride, rows=rows, vocab=vocab, fused=bool(fused))
    except (TypeError, ValueError) as e:
        return type(e).__name__


@pytest.fixture(scope="module")
def shipped_knobs():
    saved = knobs.as_dict()
    knobs.update(knobs.Knobs().__dict__)     # a DLLM_KNOBS override in the environment cannot move the table
    yield
    knobs.update(saved)


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        t = json.load(f)
    assert t["columns"] == COLUMNS
    return t["rows"]


def test_table_covers_the_grid(table):
    assert [r[:N_IN] for r in table] == grid()
    assert len(table) == len(OPS) * 2 * 3 * 2 * 3 * 2 * 3 * 2
    seen = {(r[0], r[-1]) for r in table}
    for op in OPS:
        assert (op, "kernel") in seen and (op, "reference") in seen, op
        assert ((op, "reference-warn") in seen) == (op in ("sample_rows", "token_logprobs", "apply_logit_processors"))
        assert ((op, "ValueError") in seen) == (op in ("argmax", "sample_rows", "lm_head_logprobs"))
    assert {o for _, o in seen} == {"kernel", "reference", "reference-warn", "ValueError"}
    assert all(r[-1] == "reference" for r in table if r[1] == "cpu")


def test_route_returns_the_recorded_outcome(table):
    for r in table:
        assert route_row(r[:N_IN]) == r[-1], r


def test_wrappers_do_the_recorded_thing(table, shipped_knobs):
    for r in table:
        assert run_row(r[:N_IN]) == r[-1], r


def test_argument_check_raises_by_fault():
    """One fault each: TypeError for the dtype, ValueError for contiguity, shape and device."""
    check, i32 = ops._ck, torch.int32
    check(torch.zeros(2, 3, dtype=i32), "t", i32, (2, None), torch.device("cpu"))
    check(torch.zeros(2, 3, dtype=i32), "t", i32, None)
    with pytest.raises(TypeError):
        check(torch.zeros(2, 3), "t", i32, (2, 3))
    for bad, shape, dev in ((torch.zeros(3, 2, dtype=i32).t(), (2, 3), None), (torch.zeros(2, 3, dtype=i32), (2, 4), None),
                            (torch.zeros(2, 3, dtype=i32), (2,), None),
                            (torch.zeros(2, 3, dtype=i32), (2, 3), torch.device("meta"))):
        with pytest.raises(ValueError):
            check(bad, "t", i32, shape, dev)


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    knobs.update(knobs.Knobs().__dict__)
    out = [inp + [run_row(inp)] for inp in grid()]
    with open(TABLE, "w") as f:
        f.write('{"columns": ' + json.dumps(COLUMNS) + ',\n"rows": [\n')
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in out))
        f.write("\n]}\n")
    print(len(out), "rows,", os.path.getsize(TABLE), "bytes")
