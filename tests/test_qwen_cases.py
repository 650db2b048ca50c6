"""CPU checks of tests/qwen_cases.py: the builders' preconditions hold for every shape the GPU test launches,
the acceptance rules reject torch emulations of wrong qkv_prep kernels, and ops/reference.py qkv_prep (the
CPU path and the contract) passes every case."""
import pytest
import torch

import qwen_cases as qc
from distributed_llms_amd import ops
from distributed_llms_amd.ops import reference as ref

SMALL = [(4, 2, 64), (4, 1, 128), (8, 2, 64)]


@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("tokens", qc.TOKENS)
@pytest.mark.parametrize("shape", qc.SHAPES, ids=str)
def test_reference_passes_every_case(shape, tokens, kind):
    case = qc.prep_case(*shape, tokens, kind)        # the builder asserts its own preconditions
    assert case.qkv.shape == (tokens, (shape[0] + 2 * shape[1]) * shape[2]) and case.qkv.dtype == torch.bfloat16
    assert (case.bias is None) == (kind == "norm") and (case.q_w is None) == kind.startswith("bias")
    buf, y = qc.run(case, ref.qkv_prep)
    msg = qc.mismatch(case, y)
    assert msg is None, msg
    qc.assert_guards(buf)
    buf2, y2 = qc.run(case, ops.qkv_prep_)          # the public op takes the reference off the GPU
    assert torch.equal(buf, buf2)


@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_emulated_kernel_passes(shape, kind):
    case = qc.prep_case(*shape, 257, kind)
    msg = qc.mismatch(case, qc.emulate(case))
    assert msg is None, msg


def test_norm_rows_cover_every_needle():
    for hq, hkv, d in qc.SHAPES:
        rows = qc.prep_case(hq, hkv, d, 257, "norm").rows
        for h in (0, hq - 1, hq, hq + hkv - 1):
            for c in qc.needle_columns(d):
                assert f"needle at head {h} column {c}" in rows
        assert {"zero", "tiny", "random"} <= set(rows)
        assert qc.prep_case(hq, hkv, d, 3, "both").rows == ["random", "zero", "tiny"]


@pytest.mark.parametrize("wrong,kinds", sorted(qc.WRONG.items()))
@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_rules_reject_wrong_kernels(shape, wrong, kinds):
    for kind in kinds:
        case = qc.prep_case(*shape, 257, kind)
        assert qc.mismatch(case, qc.emulate(case, wrong)) is not None, f"{wrong} passes the {kind} case"


def test_untouched_slots_are_not_written():
    """No bias: the v slots keep their bits whatever they hold (here NaN patterns); only q_w: k too."""
    hq, hkv, d = 4, 2, 64
    case = qc.prep_case(hq, hkv, d, 17, "norm")
    x = case.qkv.clone().view(17, hq + 2 * hkv, d)
    x[:, hq + hkv:] = qc.from_bits(torch.full((17, hkv, d), 0x7FC1))
    y = x.clone().view(17, -1)
    ref.qkv_prep(y, None, case.q_w, case.k_w, hq, hkv, d, qc.EPS)
    assert torch.equal(y.view(17, -1, d)[:, hq + hkv:].view(torch.int16), x[:, hq + hkv:].view(torch.int16))
    y = x.clone().view(17, -1)
    ref.qkv_prep(y, None, case.q_w, None, hq, hkv, d, qc.EPS)
    assert torch.equal(y.view(17, -1, d)[:, hq:].view(torch.int16), x[:, hq:].view(torch.int16))
    assert not torch.equal(y.view(17, -1, d)[:, :hq], x[:, :hq])


def test_op_checks_shapes():
    qkv = torch.zeros(3, 8 * 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="qkv must be"):
        ops.qkv_prep_(qkv, None, None, None, 4, 1, 64, 1e-6)
    with pytest.raises(ValueError, match="bias must be"):
        ops.qkv_prep_(qkv, torch.zeros(64, dtype=torch.bfloat16), None, None, 4, 2, 64, 1e-6)
    with pytest.raises(ValueError, match="q_w must be"):
        ops.qkv_prep_(qkv, None, torch.zeros(128, dtype=torch.bfloat16), None, 4, 2, 64, 1e-6)


def test_modes_cover_every_kind():
    """The three launch modes (bias-only, norm-only, both) and the case kinds that run in each."""
    assert sorted(k for ks in qc.MODES.values() for k in ks) == sorted(qc.KINDS)
    for mode, kinds in qc.MODES.items():
        for kind in kinds:
            case = qc.prep_case(4, 2, 64, 3, kind)
            assert (case.bias is not None) == (mode != "norm-only") and (case.q_w is not None) == (mode != "bias-only")
