"""Inputs and the acceptance rule shared by test_processors.py (CPU) and test_processors_gpu.py.

The reference is ops/reference.py apply_logit_processors (numpy float32, one IEEE rounding per
operation, one round-to-nearest-even to bf16).  The HIP kernel must give the reference's bf16 bit
patterns: every element equal, except that a token some rule touches may hold any NaN where the
reference holds a NaN (NaN compares as NaN).  Tokens no rule touches, rows that did not ask and the
guard columns beside a strided row must keep their bits exactly.
"""
from types import SimpleNamespace

import numpy as np
import torch

from distributed_llms_amd.ops import reference as ref

# rows x vocab: a row shorter than the workgroup's stride; an odd vocabulary (unaligned rows, ragged
# last group; run with a row stride above the vocabulary too); the kernels' largest row; the served
# vocabulary
SHAPES = [(3, 777), (5, 5003), (2, 131072), (4, 128256)]
# what the rows of a case ask for, by row index: every rule at once with the EOS ban, nothing (no
# state row), bias and ban only, penalties only, a state row without the SAMPLE flag
KINDS = ("all", "none", "bias", "penalties", "flagless")
# bf16 patterns planted under every kind of token: +-inf, a signalling and a quiet NaN with
# payloads, -0, +0, the smallest subnormals
SPECIAL = (0x7F80, 0xFF80, 0x7FA5, 0xFFC1, 0x8000, 0x0000, 0x0001, 0x8001)
BIAS_PITCH = 304


def f32_bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def empty_state(state_rows, vocab, device="cpu"):
    """A LogitState look-alike (the tensors ops.* read), zeroed."""
    pitch = -(-vocab // 8) * 8
    return SimpleNamespace(
        vocab=vocab, state=torch.zeros(state_rows, pitch, dtype=torch.int32, device=device),
        bias_n=torch.zeros(state_rows, dtype=torch.int32, device=device),
        bias_ids=torch.zeros(state_rows, BIAS_PITCH, dtype=torch.int32, device=device),
        bias_vals=torch.zeros(state_rows, BIAS_PITCH, dtype=torch.float32, device=device))


def state_to(ls, device):
    return SimpleNamespace(vocab=ls.vocab, state=ls.state.to(device), bias_n=ls.bias_n.to(device),
                           bias_ids=ls.bias_ids.to(device), bias_vals=ls.bias_vals.to(device))


def proc_row(state_row=-1, prompt_len=0, flags=0, rep=1.0, pres=0.0, freq=0.0, min_tokens=0, start=0):
    r = np.zeros(ref.PROC_WORDS, dtype=np.int32)
    r[[ref.PROC_ROW, ref.PROC_PROMPT_LEN, ref.PROC_FLAGS, ref.PROC_MIN_TOKENS, ref.PROC_START]] = (
        state_row, prompt_len, flags, min_tokens, start)
    r[[ref.PROC_REP, ref.PROC_PRES, ref.PROC_FREQ]] = f32_bits([rep, pres, freq])
    return r


def make_apply_case(rows, vocab):
    """bf16 logits [rows, vocab] at spread 3 with SPECIAL planted under counted, prompt-only, biased
    and untouched tokens; a state of rows + 2 state rows used in reverse order (row r -> state row
    rows - r), the two others filled with a pattern nobody may read into a result; procs by KINDS.
    Returns a dict: logits, ls, procs, seq_lens, eos, touched (bool [rows, vocab])."""
    rng = np.random.default_rng(rows * 7919 + vocab)
    g = torch.Generator().manual_seed(rows * 1000003 + vocab)
    logits = (torch.randn(rows, vocab, generator=g) * 3.0).to(torch.bfloat16)
    lbits = logits.view(torch.int16).numpy().view(np.uint16)
    ls = empty_state(rows + 2, vocab)
    st = ls.state.numpy().view(np.uint32)
    st[0, :] = 0xA5A5A5A5 & ~ref.STATE_BIAS_BIT
    st[rows + 1, :] = 7
    eos = vocab - 1 if vocab % 8 else vocab // 2 + 3       # in the ragged last group when there is one
    procs = np.stack([proc_row() for _ in range(rows)])
    seq_lens = np.zeros(rows, dtype=np.int32)
    touched = np.zeros((rows, vocab), dtype=bool)
    ns = len(SPECIAL)
    for r in range(rows):
        kind = KINDS[r % len(KINDS)]
        if kind == "none":
            seq_lens[r] = 9
            continue
        s = rows - r
        toks = rng.permutation(vocab)
        # disjoint token sets: counted, prompt-only, biased (some of them counted / in the prompt too)
        n_cnt, n_pr = max(2 * ns + 3, vocab // 50), max(2 * ns, vocab // 40)
        counted, prompt = toks[:n_cnt], toks[n_cnt:n_cnt + n_pr]
        n_bias = 300 if kind in ("all", "bias") and r == 0 else 37
        pure = toks[n_cnt + n_pr:n_cnt + n_pr + n_bias - 2 * ns]
        biased = np.concatenate([pure, counted[ns:2 * ns], prompt[ns:2 * ns]])
        untouched = toks[n_cnt + n_pr + n_bias:n_cnt + n_pr + n_bias + ns]
        cnt = rng.integers(1, 40, size=n_cnt).astype(np.uint32)
        cnt[-3:] = (4096, 70000, (1 << 24) - 1)
        st[s, counted] = cnt
        st[s, prompt] |= np.uint32(ref.STATE_PROMPT_BIT)
        st[s, counted[::3]] |= np.uint32(ref.STATE_PROMPT_BIT)
        has_bias = kind in ("all", "bias")
        if has_bias:
            st[s, biased] |= np.uint32(ref.STATE_BIAS_BIT)
            ls.bias_n[s] = n_bias
            ls.bias_ids[s, :n_bias] = torch.from_numpy(biased.astype(np.int32))
            vals = rng.uniform(-100, 100, size=n_bias).astype(np.float32)
            vals[:3] = (100.0, -100.0, 0.0)
            ls.bias_vals[s, :n_bias] = torch.from_numpy(vals)
        for group in (counted[:ns], prompt[:ns], pure[:ns], untouched):
            lbits[r, group] = SPECIAL
        pen = kind in ("all", "penalties", "flagless")
        rep, pres, freq = ((1.3, 0.7, 0.05) if r % 2 == 0 else (0.8, -1.5, -0.011)) if pen else (1.0, 0.0, 0.0)
        # a ban in the rows that carry the bias (row 0: eos has a bias entry, so the bias pass owns it)
        min_tokens, prompt_len = (6, 4) if has_bias else (0, 4)
        seq_lens[r] = 4 + (3 if r % 2 == 0 else 8)          # output index 3 (< 6: banned) or 8 (not)
        if kind == "all" and r == 0 and eos not in biased:
            st[s, eos] |= np.uint32(ref.STATE_BIAS_BIT)
            ls.bias_ids[s, 5] = eos
            st[s, biased[5]] &= np.uint32(~ref.STATE_BIAS_BIT & 0xFFFFFFFF)
            biased = np.concatenate([biased[:5], [eos], biased[6:]])
        flags = 0 if kind == "flagless" else ref.PROC_SAMPLE
        procs[r] = proc_row(s, prompt_len, flags, rep, pres, freq, min_tokens)
        if flags:
            w = st[s, :vocab]
            c = (w & np.uint32(ref.STATE_COUNT_MASK)) > 0
            t = c.copy()
            if rep != 1.0:
                t |= (w & np.uint32(ref.STATE_PROMPT_BIT)) != 0
            if has_bias:
                t[biased] = True
            if seq_lens[r] - prompt_len < min_tokens:
                t[eos] = True
            touched[r] = t
    return {"logits": logits, "ls": ls, "procs": torch.from_numpy(procs), "seq_lens": torch.from_numpy(seq_lens),
            "eos": int(eos), "touched": touched}


def reference(case):
    """The reference's logits for ``case`` (a new CPU tensor)."""
    out = case["logits"].clone()
    ls = case["ls"]
    ref.apply_logit_processors(out, ls.state, case["procs"], case["seq_lens"], case["eos"], ls.bias_n, ls.bias_ids,
                               ls.bias_vals)
    return out


def check_bits(got, exp, before, touched, label=""):
    """bf16 tensors [rows, vocab]: equal bit patterns; where a rule touches the token and the
    reference holds a NaN, any NaN.  Returns how many elements the processors changed."""
    g = got.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
    e = exp.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
    b = before.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
    nan_g, nan_e = (g & 0x7FFF) > 0x7F80, (e & 0x7FFF) > 0x7F80
    ok = (g == e) | (nan_g & nan_e & touched)
    bad = np.argwhere(~ok)
    assert ok.all(), (f"{label}: {bad.shape[0]} elements differ, first (row, token) {bad[:4].tolist()}: got "
                      f"{[hex(g[i, j]) for i, j in bad[:4]]}, expected {[hex(e[i, j]) for i, j in bad[:4]]}, "
                      f"before {[hex(b[i, j]) for i, j in bad[:4]]}")
    assert ((e == b) | touched).all(), f"{label}: the reference changed a token no rule touches"
    return int((e != b).sum())
