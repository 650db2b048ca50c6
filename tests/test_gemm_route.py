"""The native calls of the dense GEMM host path against a table recorded before gemm.route existed.

tests/golden/gemm_routes.json holds, for the grid below, what gemm.linear, gemm.linear_swiglu and
quant.linear_fp8 hand to the native launchers: the function, then M, N, K, ws_floats, splits, mode and
variant in the launcher's argument order (gemm_pf takes no workspace and no splits: null), the type of
the result (T: a tensor, P: a SplitKPartial and its .splits, -: linear_swiglu's None) and its shape.
Pointers are not compared.  A row that reaches no launcher records "torch" (F.linear ran), or "none"
where linear_swiglu declined.

The harness drives the public entry points on meta tensors, with _ext.kernels replaced by a recorder
whose gemm_* methods return the launchers' effective slice count, and torch.cuda.current_stream /
is_current_stream_capturing replaced.  It touches no private name of ops.gemm or ops.quant, so this
file and the table pass unchanged at the commit before the route and at every commit after it: the
table was recorded there (``python tests/test_gemm_route.py --record`` rewrites it from whatever tree
it runs in), and checking a later tree against it is running this test."""
import json
import os
import sys
import types

import pytest
import torch

from distributed_llms_amd import _ext, knobs
from distributed_llms_amd.ops import gemm, quant

TABLE = os.path.join(os.path.dirname(__file__), "golden", "gemm_routes.json")
COLUMNS = ["entry", "m", "n", "k", "defer", "flag", "comm_cus", "knobs", "splits_in", "call", "result", "rsplits", "shape"]
N_IN = 9                                    # the first N_IN columns are inputs, the rest recorded

# 8B: qkv, o, gate|up, down, LM head; 70B: the same four and a 32000-row head; N % 256, N % 128, K % 64
SHAPES_8B = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336), (128256, 4096)]
SHAPES_MORE = [(10240, 8192), (8192, 8192), (57344, 8192), (8192, 28672), (32000, 4096), (4224, 4096), (4160, 4096),
               (4096, 4128)]
SHAPES = SHAPES_8B + SHAPES_MORE
MS = [1, 16, 64, 65, 128, 129, 192, 199, 200, 224, 225, 256, 257, 320, 384, 385, 512, 513, 640, 1024, 2048, 4096, 32768]
MS_MORE = [1, 224, 225, 256, 257, 513, 4096]   # thinned: SHAPES_MORE
MS_COMM = [64, 200, 256, 320, 512, 4096]
MS_KNOB = [64, 256, 320, 4096]
# knob overrides, each with the (N, K, swiglu) it can affect
QKV, O, GU, DOWN, HEAD = SHAPES_8B
KNOB_ROWS = [
    ({"wide": "none"}, [(QKV, 0), (GU, 1), (DOWN, 0)]),
    ({"wide": "all"}, [(QKV, 0), (GU, 1), (DOWN, 0)]),
    ({"wide": "gate_up,down"}, [(QKV, 0), (GU, 1), (DOWN, 0)]),
    ({"sq": "none"}, [(HEAD, 0), ((57344, 8192), 1)]),
    ({"sq_split": True}, [(QKV, 0), (DOWN, 0), (GU, 1)]),
    ({"sq_split": True, "pp_gate_up_min_m": 0}, [(GU, 1)]),
    ({"pp_persistent": False}, [(O, 0), (GU, 1)]),
    ({"pp_gate_up_min_m": 0}, [(GU, 1), ((57344, 8192), 1)]),
    ({"pp_down_min_k": 0}, [((8192, 28672), 0)]),
    ({"pp_down_min_k": 8192}, [(DOWN, 0)]),
    ({"pp_head_min_m": 0}, [(HEAD, 0)]),
    ({"wide_small_bm": 0}, [(O, 0)]),
    ({"pf_dynamic": "on"}, [(O, 0), (GU, 1)]),
]
FP8_SHAPES = [QKV, O, GU, DOWN]
FP8_MS = [64, 200, 256, 4096, 32768]
STREAM = 0x7E57                             # no real stream's handle: the meta workspace is cached beside the real ones


def grid():
    """The inputs of every row, in table order."""
    rows = []

    def add(entry, m, nk, defer=0, flag="", comm=0, kn=None, splits=0):
        rows.append([entry, m, nk[0], nk[1], defer, flag, comm, kn or {}, splits])

    for nk in SHAPES:
        for m in (MS if nk in SHAPES_8B else MS_MORE):
            add("lin", m, nk)
            add("lin", m, nk, defer=1)
            add("swi", m, nk)
    for nk in SHAPES:
        for m in MS_COMM:
            add("lin", m, nk, defer=1, comm=16)
            add("swi", m, nk, comm=16)
    for kn, cases in KNOB_ROWS:
        for nk, sw in cases:
            for m in MS_KNOB:
                add("swi" if sw else "lin", m, nk, defer=0 if sw else 1, kn=kn)
    for m in MS_KNOB:
        add("lin", m, HEAD, comm=16, kn={"head_beside_comm": "pp"})
    for defer in (0, 1):
        add("lin", 224, HEAD, defer=defer, kn={"wide_target_wgs": 4096})      # 4 slabs of 224 x 128256 do not fit
    for nk, sw in ((O, 0), (GU, 1)):        # a capture clears gemm_pf's dynamic-queue bit
        add("swi" if sw else "lin", 4096, nk, flag="capture", kn={"pf_dynamic": "on"})
        add("swi" if sw else "lin", 4096, nk, comm=16)
    for m in (64, 256, 4096):               # what no kernel takes
        for flag in ("bias", "fp32", "noncontig"):
            add("lin", m, QKV, flag=flag)
            if flag != "bias":
                add("swi", m, GU, flag=flag)
    for nk in FP8_SHAPES:
        for m in FP8_MS:
            add("fp8", m, nk)
            add("fp8", m, nk, defer=1)
            if nk == GU:
                add("fp8s", m, nk)
    for kn in ({"fp8_bm128": False}, {"fp8_group_m": 0}):
        for m in (200, 256, 4096):
            add("fp8", m, O, defer=1, kn=kn)
            add("fp8s", m, GU, kn=kn)
    for m in (64, 256, 4096):
        add("fp8", m, O, defer=1, comm=16)
        add("fp8", m, O, defer=1, splits=16)        # at M = 4096 the workspace holds 2 slabs, not 16
        add("fp8", m, O, defer=1, splits=12)        # 32 K-tiles in 12 slices of 3: 11 run
    return rows


class Recorder:
    """Stands in for the extension module: records what the launchers are given."""

    def __init__(self):
        self.calls = []

    def _split(self, name, kt, ws_floats, m, n, k, splits, mode, variant):
        self.calls.append([name, m, n, k, ws_floats, splits, mode, variant])
        return -(-kt // -(-kt // splits))

    def gemm_wide(self, c, a, b, ws, ws_floats, m, n, k, splits, mode, variant, stream):
        return self._split("gemm_wide", k // 64, ws_floats, m, n, k, splits, mode, variant)

    def gemm_pp(self, c, a, b, ws, ws_floats, m, n, k, splits, mode, variant, stream):
        return self._split("gemm_pp", k // 64, ws_floats, m, n, k, splits, mode, variant)

    def gemm_sq(self, c, a, b, ws, ws_floats, m, n, k, splits, mode, variant, stream):
        return self._split("gemm_sq", k // 64, ws_floats, m, n, k, splits, mode, variant)

    def gemm_wide_fp8(self, c, a, a_scale, b, b_scale, ws, ws_floats, m, n, k, splits, mode, variant, stream):
        return self._split("gemm_wide_fp8", k // 128, ws_floats, m, n, k, splits, mode, variant)

    def gemm_pf(self, c, a, b, m, n, k, mode, variant, stream):
        self.calls.append(["gemm_pf", m, n, k, None, None, mode, variant])


class MetaAct(quant.Fp8Act):
    """A quantized activation on the meta device that linear_fp8 takes for a GPU one."""
    __slots__ = ()
    is_cuda = True


def run_row(inputs):
    """One call of a public entry point under the row's knobs and comm reservation -> the recorded columns."""
    entry, m, n, k, defer, flag, comm, kn, splits = inputs
    rec = Recorder()
    saved = (_ext.kernels, torch.cuda.current_stream, torch.cuda.is_current_stream_capturing)
    _ext.kernels = lambda: rec
    torch.cuda.current_stream = lambda *a: types.SimpleNamespace(cuda_stream=STREAM)
    torch.cuda.is_current_stream_capturing = lambda: flag == "capture"
    if comm:
        gemm.reserve_cus_for_comm(comm)
    try:
        with knobs.override(**kn):
            dt = torch.float32 if flag == "fp32" else torch.bfloat16
            if entry.startswith("fp8"):
                x = MetaAct(torch.empty(m, k, dtype=quant.FP8, device="meta"), torch.empty(m, device="meta"), (m, k), dt)
                w = quant.Fp8Weight(torch.empty(n, k, dtype=quant.FP8, device="meta"), torch.empty(n, device="meta"))
                y = quant.linear_fp8(x, w, swiglu=entry == "fp8s", defer=bool(defer), splits=splits)
            else:
                x = torch.empty(m, 2 * k, dtype=dt, device="meta")[:, :k] if flag == "noncontig" else \
                    torch.empty(m, k, dtype=dt, device="meta")
                w = torch.empty(n, k, dtype=dt, device="meta")
                if entry == "swi":
                    y = gemm.linear_swiglu(x, w)
                else:
                    bias = torch.empty(n, dtype=dt, device="meta") if flag == "bias" else None
                    y = gemm.linear(x, w, bias, defer=bool(defer))
    finally:
        if comm:
            gemm.release_cus_for_comm()
        _ext.kernels, torch.cuda.current_stream, torch.cuda.is_current_stream_capturing = saved
    assert len(rec.calls) <= 1, rec.calls
    call = rec.calls[0] if rec.calls else ("none" if y is None else "torch")
    if y is None:
        return [call, "-", None, None]
    if isinstance(y, gemm.SplitKPartial):
        return [call, "P", y.splits, list(y.shape)]
    return [call, "T", None, list(y.shape)]


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


def test_table_covers_the_grid(table, shipped_knobs):
    assert [r[:N_IN] for r in table] == grid()
    rows = [dict(zip(COLUMNS, r)) for r in table]
    plain = [r for r in rows if not r["knobs"] and not r["comm_cus"] and not r["flag"] and not r["entry"].startswith("fp8")]
    for nk in SHAPES:
        for entry, defer in (("lin", 0), ("lin", 1), ("swi", 0)):
            got = {r["m"] for r in plain if (r["n"], r["k"]) == nk and r["entry"] == entry and r["defer"] == defer}
            assert got == set(MS if nk in SHAPES_8B else MS_MORE), (nk, entry, defer)
        assert {r["m"] for r in rows if (r["n"], r["k"]) == nk and r["comm_cus"] == 16} >= set(MS_COMM), nk
    assert any(n % 256 and not n % 128 for n, _ in SHAPES) and any(n % 128 for n, _ in SHAPES)
    assert any(k % 64 for _, k in SHAPES)
    # every launcher in every mode it can run (gemm_pf has no mode 2)
    seen = {(r["call"][0], r["call"][6]) for r in rows if isinstance(r["call"], list)}
    assert seen == {(f, mode) for f in ("gemm_wide", "gemm_pp", "gemm_sq", "gemm_wide_fp8") for mode in (0, 1, 2)} | \
        {("gemm_pf", 0), ("gemm_pf", 1)}
    # both dispatchers' fall-throughs, from a shape and from each operand reason
    assert {r["flag"] for r in rows if r["call"] == "torch"} == {"", "bias", "fp32", "noncontig"}
    assert {r["flag"] for r in rows if r["call"] == "none"} == {"", "fp32", "noncontig"}
    # every branch: the variant words name them (pp: head, down, gate|up 128 / 256 columns, medium M;
    # wide: unsplit, split, the 128-row o-projection tile; pf: static, dynamic queue; sq; fp8: nontemporal
    # decode, 128-row tiles, prefill plain and grouped)
    v = gemm
    variants = {(r["call"][0], r["call"][7]) for r in rows if isinstance(r["call"], list)}
    assert variants == {("gemm_pp", v.PP_HEAD_VARIANT), ("gemm_pp", v.PP_GATE_UP_VARIANT),
                        ("gemm_pp", v.PP_GATE_UP_VARIANT & ~1), ("gemm_pp", v.PP_PREFILL_VARIANT),
                        ("gemm_wide", 33), ("gemm_wide", 1), ("gemm_wide", 1 | 128 << 8), ("gemm_wide", 33 | 128 << 8),
                        ("gemm_sq", 4), ("gemm_pf", 0), ("gemm_pf", 16),
                        ("gemm_wide_fp8", 1), ("gemm_wide_fp8", 1 | 128 << 8), ("gemm_wide_fp8", 4), ("gemm_wide_fp8", 4 | 64)}
    down = [r for r in rows if r["call"][0] == "gemm_pp" and r["call"][7] == v.PP_GATE_UP_VARIANT and r["entry"] == "lin"]
    assert down and all(r["call"][5] > 1 for r in down)            # the long-K down projection: split
    # the stream capture clears gemm_pf's dynamic-queue bit; comm CUs set it
    assert all(r["call"][7] == 0 for r in rows if r["flag"] == "capture") and any(r["flag"] == "capture" for r in rows)
    assert any(r["call"][0] == "gemm_pf" and r["call"][7] == 16 and r["comm_cus"] and not r["knobs"] for r in rows)
    # the workspace clamp: fewer slices than asked for, and fewer than the planner's
    assert any(r["splits_in"] and 1 < r["call"][5] < r["splits_in"] for r in rows)
    clamped = [r for r in rows if r["knobs"] == {"wide_target_wgs": 4096} and r["m"] == 224]
    with knobs.override(wide_target_wgs=4096):
        assert clamped and all(r["call"][5] < gemm.wide_splits(r["m"], r["n"], r["k"]) for r in clamped)
    # deferred partials carry the launcher's effective slice count
    assert all(r["rsplits"] == -(-(r["k"] // (128 if r["entry"] == "fp8" else 64)) //
                                 -(-(r["k"] // (128 if r["entry"] == "fp8" else 64)) // r["call"][5]))
               for r in rows if r["result"] == "P")
    assert any(r["result"] == "P" and r["rsplits"] < r["call"][5] for r in rows)


def test_entry_points_reproduce_the_table(table, shipped_knobs):
    for r in table:
        assert run_row(r[:N_IN]) == r[N_IN:], r


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    knobs.update(knobs.Knobs().__dict__)
    out = [inp + run_row(inp) for inp in grid()]
    with open(TABLE, "w") as f:
        f.write('{"columns": ' + json.dumps(COLUMNS) + ',\n"rows": [\n')
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in out))
        f.write("\n]}\n")
    print(len(out), "rows,", os.path.getsize(TABLE), "bytes")
