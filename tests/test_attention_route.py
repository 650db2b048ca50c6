"""ops.prefill_route against a table recorded before the route existed.

tests/golden/attention_routes.json holds, for a thinned grid of prefill calls, what the host path then
decided in three places: the wrapper's choice (a forced version, the prefill_attn knob, split-context
eligibility, the auto version), the two demotions the native launcher applied on its own (the 32x32
kernels to 4 away from head_dim 128 / groups up to 16; the LDS kernels to 3 behind block tables wider
than PF_MAX_CHUNKS) and the stage's question whether the kernel rotates q itself.  Each row: the
inputs, the knob overrides, the CUs reserved for comm kernels, and the expected (version,
rope_in_kernel, nsplit, split_chunks).  A forced version was only ever given to the rotated-q wrapper,
so those rows ask with allow_rope_in_kernel off; rows that plan version 5 without a host-known context
(the wrapper reads it from the device) are not in the table and checked below."""
import json
import os

import pytest

from distributed_llms_amd import knobs, ops
from distributed_llms_amd.ops import gemm

HEADS = [(32, 8, 128), (64, 8, 128), (32, 8, 64), (12, 12, 64), (24, 4, 128)]
GRID = {"batch": [1, 8, 256], "max_q_len": [1, 20, 64, 65, 383, 384, 4096], "max_ctx": [None, 4095, 4096, 8192, 32768],
        "max_blocks": [256, 1024, 1025], "prefill_attn": [0, 3, 4, 5, 7, 9], "prefill_fused_rope": [1, 0],
        "prefill_split_min_ctx": [0, 256, 4096], "comm_cus": [0, 16], "allow_rope_in_kernel": [1, 0],
        "version": [0, 7], "nsplit": [None, 200]}


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(os.path.dirname(__file__), "golden", "attention_routes.json")) as f:
        t = json.load(f)
    return [dict(zip(t["columns"], row)) for row in t["rows"]]


def test_table_covers_the_grid(table):
    for h in HEADS:
        mine = [r for r in table if (r["num_heads"], r["num_kv_heads"], r["head_dim"]) == h]
        for name, values in GRID.items():
            assert {r[name] for r in mine} == set(values), (h, name)
    # the launcher's own choices, which no host test could see
    assert any(r["head_dim"] == 64 and r["prefill_attn"] in (7, 9) and r["exp_version"] == 4 for r in table)
    assert any(r["max_blocks"] == 1025 and r["prefill_attn"] in (0, 4, 7, 9) and r["exp_version"] == 3 for r in table)
    assert {r["exp_version"] for r in table} == {3, 4, 5, 7, 9}


def test_prefill_route_reproduces_the_table(table):
    for r in table:
        if r["comm_cus"]:
            gemm.reserve_cus_for_comm(r["comm_cus"])
        try:
            with knobs.override(prefill_attn=r["prefill_attn"], prefill_fused_rope=bool(r["prefill_fused_rope"]),
                                prefill_split_min_ctx=r["prefill_split_min_ctx"]):
                got = ops.prefill_route(r["batch"], r["num_heads"], r["num_kv_heads"], r["head_dim"], r["max_q_len"],
                                        r["max_ctx"], r["max_blocks"], version=r["version"], nsplit=r["nsplit"],
                                        allow_rope_in_kernel=bool(r["allow_rope_in_kernel"]))
        finally:
            if r["comm_cus"]:
                gemm.release_cus_for_comm()
        want = ops.PrefillRoute(r["exp_version"], bool(r["exp_rope_in_kernel"]), r["exp_nsplit"], r["exp_split_chunks"])
        assert got == want, r


def test_split_route_without_a_host_context_is_unplanned():
    with knobs.override(prefill_attn=ops.PREFILL_SPLIT):
        assert ops.prefill_route(1, 32, 8, 128, 20, None, 256) == ops.PrefillRoute(5, False, 0, 0)
    assert ops.prefill_route(1, 32, 8, 128, 20, None, 256, version=5, nsplit=7) == ops.PrefillRoute(5, False, 0, 0)
    assert ops.prefill_route(1, 32, 8, 128, 20, 4200, 256, version=5, nsplit=7) == ops.PrefillRoute(5, False, 7, 19)
    with pytest.raises(ValueError):
        ops.prefill_route(1, 32, 8, 128, 20, 4200, 256, version=5, nsplit=0)
