"""Inputs and the acceptance rule shared by test_logprobs.py (CPU) and test_logprobs_gpu.py.

The reference is ops/reference.py token_logprobs (float64 numpy).  An implementation in lower
precision (the HIP kernel: float32 exp2, 2^40 fixed-point sum, one float32 ln Z) must give the
reference's top ids exactly -- the order is exact on bf16 keys -- and floats within
ATOL + RTOL * |lp| wherever the reference is finite; non-finite values must be equal.  Basis of
the bound: the relative error of Z is below 4e-6, one float32 rounding each goes to ln Z and to
the result, and a float32 emulation of the fixed-point sum stayed within 3.4e-6 at logit spread
10 (|lp| <= 88) and 7.6e-6 at spread 20 (|lp| <= 174).
"""
import numpy as np
import torch

from distributed_llms_amd.ops import reference as ref

# rows x vocab: a row shorter than the workgroup; an odd vocabulary (unaligned rows, ragged last
# group); the register capacity; more rows than CUs; the served vocabulary
SHAPES = [(3, 777), (5, 5003), (2, 131072), (300, 2048), (4, 128256)]
WANTS = (-1, 0, 1, 5, 20)
N_MAX = ref.MAX_LOGPROBS
ATOL, RTOL = 1e-5, 2.0 ** -22
NUM_HAND = 6


def hand_rows(vocab, g):
    """Six hand-built rows: all -inf; one finite entry in the ragged tail; two +inf maxima; NaN
    entries and a -0 / +0 tie at the top; all entries equal; the largest values at the row's end."""
    ninf = float("-inf")
    h = torch.full((NUM_HAND, vocab), ninf)
    h[1, vocab - 1] = -3.0
    h[2] = torch.randn(vocab, generator=g) * 3.0
    h[2, vocab // 2 + 1] = float("inf")
    h[2, 3] = float("inf")
    h[3] = -torch.rand(vocab, generator=g) * 8.0 - 0.5
    h[3, 0] = float("nan")
    h[3, vocab - 2] = float("nan")
    h[3, 5] = -0.0
    h[3, 2] = 0.0
    h[4] = 1.0
    m = min(32, vocab)
    h[5] = -20.0
    h[5, vocab - m:] = 10.0 - 0.25 * torch.arange(m - 1, -1, -1, dtype=torch.float32)
    return h.to(torch.bfloat16)


def make_case(rows, vocab):
    """bf16 logits [3 * rows + 6, vocab]: random rows at logit spread 3 and at spread 10 (even and
    odd rows of the first 2 * rows), tie-heavy rows (the spread-3 rows rounded to integers), then
    hand_rows.  ``want`` walks -1, 0, 1, 5, 20; ``ids`` walks index 0, V - 1, an index in the
    ragged tail, a random index, and two indices outside the row (V and -5)."""
    g = torch.Generator().manual_seed(rows * 1000003 + vocab)
    rand = torch.randn(2 * rows, vocab, generator=g)
    rand[0::2] *= 3.0
    rand[1::2] *= 10.0
    ties = (rand[0::2]).round()
    logits = torch.cat([rand.to(torch.bfloat16), ties.to(torch.bfloat16), hand_rows(vocab, g)])
    n = logits.shape[0]
    rng = np.random.default_rng(rows * 7919 + vocab)
    tail = vocab - 2 if vocab % 8 else vocab - 3
    pick = (0, vocab - 1, tail, None, vocab, -5)
    want = np.array([WANTS[(i + i // 5) % 5] for i in range(n)], dtype=np.int32)
    ids = np.array([rng.integers(0, vocab) if pick[i % 6] is None else pick[i % 6] for i in range(n)], dtype=np.int32)
    want[n - NUM_HAND:] = (20, 20, 20, 20, 5, 20)
    ids[n - NUM_HAND:] = (0, vocab - 1, 3, 0, tail, vocab - 1)
    return {"logits": logits, "ids": torch.from_numpy(ids), "want": torch.from_numpy(want)}


def reference(case, n_max=N_MAX):
    """(chosen, top_ids, top_lp) of the reference, as CPU tensors (float32 / int32 / float32)."""
    return ref.token_logprobs(case["logits"], case["ids"], case["want"], n_max)


def check_floats(got, exp, what):
    """Non-finite values equal exactly; elsewhere |err| <= ATOL + RTOL * |lp|.  Returns max |err|."""
    got = np.asarray(got, dtype=np.float64)
    exp = np.asarray(exp, dtype=np.float64)
    fin = np.isfinite(exp)
    assert np.array_equal(got[~fin], exp[~fin]), f"{what}: non-finite values differ"
    assert np.isfinite(got[fin]).all(), f"{what}: non-finite where the reference is finite"
    err = np.abs(got[fin] - exp[fin])
    bound = ATOL + RTOL * np.abs(exp[fin])
    worst = float(err.max()) if err.size else 0.0
    assert (err <= bound).all(), f"{what}: max |err| {worst:.3e}, worst excess {float((err - bound).max()):.3e}"
    return worst


def check(got, exp, label=""):
    """``got`` / ``exp``: (chosen, top_ids, top_lp) tensors.  Every row counts."""
    gc, gi, gl = (t.cpu() for t in got)
    ec, ei, el = (t.cpu() for t in exp)
    assert gi.dtype == torch.int32 and gc.dtype == torch.float32 and gl.dtype == torch.float32
    assert torch.equal(gi, ei), f"{label}: top ids differ in rows {(gi != ei).any(1).nonzero().flatten().tolist()[:8]}"
    e1 = check_floats(gc.numpy(), ec.numpy(), f"{label} chosen")
    e2 = check_floats(gl.numpy(), el.numpy(), f"{label} top_lp")
    return max(e1, e2)
