"""Inputs, fp64 expectations and acceptance rules for csrc/kernels/qkv_prep.hip (the Qwen2 qkv bias and
the Qwen3 per-head q / k RMSNorm, in place on the dense qkv) -- shared by tests/test_qwen_gpu.py (GPU: the
launches) and tests/test_qwen_cases.py (CPU: the builders' preconditions, the proof that the rules reject
wrong kernels, and ops/reference.py qkv_prep itself).  On the pattern of tests/pertoken_cases.py, whose
bit-pattern generators and rules are reused.

A case is one launch: qkv [T, (hq + 2 hkv) d], an optional bias [(hq + 2 hkv) d] and optional q_w / k_w [d].
Kinds
  bias_int   bias only.  x and b are integers in [-128, 128]: the f32 sum is exact and a bf16 value
             (asserted), so the output is compared by bits
  bias_tie   bias only.  b = +-2^e and x has exponent e + 8: x + b lies half way between two bf16 values on
             at least 40 % of the elements (asserted); the output is compared by bits with bf16(fp64 sum),
             which pins round-to-nearest-even
  norm       q_w and k_w, no bias.  The v slots hold a sentinel bit pattern and must keep it
  both       bias, q_w and k_w.  x + b is exact in f32 (asserted); the fp64 reference norms that sum, and
             the v slots are compared by bits with bf16(x + b)
The norm kinds order their token rows so that every T keeps the most telling ones: a random row, the zero
row, the tiny row (eps dominates), then one needle row per boundary column (0, 7, 8, d/2 - 1, d/2, d - 8,
d - 1) in the first q head, the last k head, the last q head and the first k head, then random rows.

Acceptance rules (pertoken_cases): ``exact`` by bits, ``rel`` |y - ref64| <= (2^-8 + 2^-12) |ref64|.
"""
import functools
from collections import namedtuple

import torch

import gemm_exact_cases as gx
from gemm_exact_cases import BF16, F64, SENT16, gen
from pertoken_cases import (I16, assert_same_bits, from_bits, patterns, rel_mismatch, same_bits,  # noqa: F401
                            tie_share, trunc_bf16)

EPS = 1e-6
SHAPES = [(4, 2, 64), (8, 2, 64), (4, 1, 128), (28, 4, 128), (32, 8, 128)]
TOKENS = [1, 3, 17, 257]
KINDS = ["bias_int", "bias_tie", "norm", "both"]
MODES = {"bias-only": ("bias_int", "bias_tie"), "norm-only": ("norm",), "both": ("both",)}

# qkv / bias / q_w / k_w: the launch's operands (bias, q_w, k_w None when absent); expected: bf16 [T, slots, d]
# for the slots compared by bits; ref64: fp64 [T, hq + hkv, d] for the normed slots (None without a norm);
# rows: what each token row is
PrepCase = namedtuple("PrepCase", "kind qkv bias q_w k_w expected ref64 rows hq hkv d eps")


def needle_columns(d):
    return [0, 7, 8, d // 2 - 1, d // 2, d - 8, d - 1]


def norm_ref(r, w, eps=EPS):
    """fp64 r rsqrt(mean_d(r^2) + eps) w over the last dimension."""
    r, w = r.to(F64), w.to(F64)
    return r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps) * w


def _norm_rows(hq, hkv, d, tokens):
    """[(kind, head slot or None, column or None)] for ``tokens`` rows, in the order of the module docstring."""
    rows = [("random", None, None), ("zero", None, None), ("tiny", None, None)]
    for h in (0, hq + hkv - 1, hq - 1, hq):
        rows += [(f"needle at head {h} column {c}", h, c) for c in needle_columns(d)]
    rows += [("random", None, None)] * max(0, tokens - len(rows))
    return rows[:tokens]


@functools.lru_cache(maxsize=None)
def prep_case(hq, hkv, d, tokens, kind):
    nh = hq + 2 * hkv
    g = gen(hq, hkv, d, tokens, 600 + KINDS.index(kind))
    shape = (tokens, nh, d)
    if kind == "bias_int":
        x = torch.randint(-128, 129, shape, generator=g).to(BF16)
        b = torch.randint(-128, 129, (nh, d), generator=g).to(BF16)
        s32 = x.float() + b.float()
        assert torch.equal(s32.double(), x.double() + b.double()) and bool((s32.abs() <= 256).all())
        assert torch.equal(s32.to(BF16).float(), s32), "the integer sums must be bf16 values"
        return PrepCase(kind, x.view(tokens, -1), b.view(-1), None, None, s32.to(BF16), None,
                        ["integers"] * tokens, hq, hkv, d, EPS)
    if kind == "bias_tie":
        be = torch.randint(127 - 8, 127 + 1, (nh, d), generator=g)
        b = from_bits((torch.randint(0, 2, (nh, d), generator=g) << 15) | (be << 7))
        x = from_bits((torch.randint(0, 2, shape, generator=g) << 15) | ((be + 8).expand(shape) << 7)
                      | torch.randint(0, 128, shape, generator=g))
        s32 = x.float() + b.float()
        assert torch.equal(s32.double(), x.double() + b.double()), "x + b must be exact in f32"
        assert tie_share(s32) >= 0.4
        return PrepCase(kind, x.view(tokens, -1), b.view(-1), None, None, (x.double() + b.double()).float().to(BF16),
                        None, ["ties"] * tokens, hq, hkv, d, EPS)

    both = kind == "both"
    q_w, k_w = patterns(g, (d,), -4, 4), patterns(g, (d,), -4, 4)
    assert not torch.equal(q_w, k_w)
    b = patterns(g, (nh, d), -4, 4) if both else None
    rows = _norm_rows(hq, hkv, d, tokens)
    x = patterns(g, shape, -6, 6) if both else patterns(g, shape, -8, 8)       # the random rows
    for i, (what, head, col) in enumerate(rows):
        if what == "zero":
            x[i] = 0.0
        elif what == "tiny" and not both:
            x[i] = patterns(g, (nh, d), -21, -20)
        elif what == "tiny":
            # r = x + b is zero except at each head's smallest |b|, where x is -b one ulp further out: r = -+ulp(b)
            col_min = b.float().abs().argmin(-1, keepdim=True)
            bits = (-b).view(I16).long() & 0xFFFF
            x[i] = from_bits(bits.scatter(-1, col_min, bits.gather(-1, col_min) + 1))
        elif head is not None:
            x[i] = patterns(g, (nh, d), -7, -5)
            x[i, head, col] = 64.0 if i % 2 == 0 else -64.0
    r32 = x.float() + (b.float() if both else 0.0)
    assert torch.equal(r32.double(), x.double() + (b.double() if both else 0.0)), "x + b must be exact in f32"
    r64 = r32.double()
    for i, (what, head, col) in enumerate(rows):
        ms = r64[i, :hq + hkv].pow(2).mean(-1)
        if what == "tiny":
            assert bool((ms < EPS / 16).all()) and bool((ms > 0).all()), "eps must dominate the tiny row"
        elif what == "zero":
            assert both or bool((ms == 0).all())
        elif head is not None:
            assert abs(r64[i, head, col].item()) >= 32
            assert both or bool((ms[head] > 16 * ms[torch.arange(hq + hkv) != head]).all())
    ref64 = torch.cat([norm_ref(r64[:, :hq], q_w, EPS), norm_ref(r64[:, hq:hq + hkv], k_w, EPS)], dim=1)
    if both:
        expected = r32[:, hq + hkv:].to(BF16)
    else:
        x[:, hq + hkv:] = from_bits(torch.full((tokens, hkv, d), SENT16))
        expected = x[:, hq + hkv:].clone()
    return PrepCase(kind, x.reshape(tokens, -1).contiguous(), None if b is None else b.reshape(-1), q_w, k_w, expected,
                    ref64, [r[0] for r in rows], hq, hkv, d, EPS)


def run(case, fn, device="cpu"):
    """``fn(qkv, bias, q_w, k_w, hq, hkv, d, eps)`` in place on a copy of the case's qkv that sits between
    sentinel guard rows -> (buf, y): the whole int16 buffer and its [T, width] bf16 middle."""
    buf, y = gx.sentinel_out(case.qkv.shape[0], case.qkv.shape[1], device=device)
    y.copy_(case.qkv)
    dev = lambda t: None if t is None else t.to(device)
    fn(y, dev(case.bias), dev(case.q_w), dev(case.k_w), case.hq, case.hkv, case.d, case.eps)
    return buf, y


def mismatch(case, y):
    """None if the output ``y`` [T, width] passes the case's rules, else a message."""
    t, hq, hkv, d = y.shape[0], case.hq, case.hkv, case.d
    y = y.detach().cpu().view(t, hq + 2 * hkv, d)
    if case.ref64 is None:
        return same_bits(y, case.expected)
    msg = rel_mismatch(y[:, :hq + hkv], case.ref64, kinds=case.rows)
    if msg is not None:
        return "q / k slots: " + msg
    msg = same_bits(y[:, hq + hkv:], case.expected)
    return None if msg is None else "v slots: " + msg


def assert_guards(buf, what="qkv_prep"):
    g = gx.GUARD_ROWS
    gx.assert_untouched(buf[:g], what + ": guard rows before row 0")
    gx.assert_untouched(buf[-g:], what + ": guard rows after row T - 1")


def emulate(case, wrong=None):
    """The kernel's formula in f32 torch -- bf16((x + b) * rsqrt(ss / d + eps) * w) per head -- and its wrong
    forms (``wrong``): whole_row, norm_v, kw_for_q, boundary, neighbour_bias, round_sum, truncate, no_eps."""
    hq, hkv, d, t = case.hq, case.hkv, case.d, case.qkv.shape[0]
    nh = hq + 2 * hkv
    x = case.qkv.view(t, nh, d)
    y = x.clone()
    store = trunc_bf16 if wrong == "truncate" else (lambda v: v.to(BF16))
    last = nh if case.bias is not None or wrong == "norm_v" else hq + hkv
    r = x[:, :last].float()
    if case.bias is not None:
        b = case.bias.view(nh, d).float()
        r = r + (torch.roll(b, -1, 0) if wrong == "neighbour_bias" else b)
    if wrong == "round_sum":
        r = r.to(BF16).float()
    out = r.clone()
    if case.q_w is not None:
        eps = 0.0 if wrong == "no_eps" else case.eps
        edge = hq - 1 if wrong == "boundary" else hq
        w = torch.zeros(last, d)
        normed = torch.zeros(last, dtype=torch.bool)
        w[:edge], normed[:edge] = (case.k_w if wrong == "kw_for_q" else case.q_w).float(), True
        w[edge:edge + hkv], normed[edge:edge + hkv] = case.k_w.float(), True
        if wrong == "norm_v":
            w[hq + hkv:], normed[hq + hkv:] = case.k_w.float(), True
        ss = r.pow(2).sum(-1, keepdim=True)
        if wrong == "whole_row":
            ss = ss[:, :hq + hkv].sum(1, keepdim=True).expand_as(ss) / (hq + hkv)
        out = torch.where(normed.view(1, -1, 1), r * torch.rsqrt(ss / d + eps) * w, r)
    y[:, :last] = store(out)
    return y.view(t, -1)


# the case kinds that must reject each wrong form
WRONG = {"whole_row": ("norm", "both"), "norm_v": ("norm", "both"), "kw_for_q": ("norm", "both"),
         "boundary": ("norm", "both"), "neighbour_bias": ("bias_int", "bias_tie", "both"), "round_sum": ("both",),
         "truncate": ("bias_tie", "norm", "both"), "no_eps": ("norm", "both")}
