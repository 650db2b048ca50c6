"""Inputs and acceptance rules shared by test_sampler_seeded.py (CPU) and test_sampler_gpu.py.

The acceptance rule for an implementation whose masses are not float64 (the HIP kernel: float32
exp2, 2^40 fixed-point sums): its id must be in the reference's kept set and sit at the CDF
crossing, where a decision within EPS * Z of a boundary (a top-p membership threshold, the crossing
itself) accepts either neighbour.  EPS is measured, not assumed: MEASURED_GAP is the largest
sum_i |w32_i - w64_i| / Z64 over the sampled rows of every case below (w32: the reference's masses
recomputed in float32; the sum bounds the disagreement of every partial sum), and EPS is 8 times
that, for the kernel's different summation order and the hardware exp2.  test_sampler_seeded.py
re-measures the gap on the CPU and checks that the reference's own float32 form stays inside the
cap that the kernel is held to: at most 2 % of the random rows accepted only by the widened rule,
and no hand-built row.
"""
import numpy as np
import torch

from distributed_llms_amd.ops import reference as ref

SHAPES = [(1, 128256), (9, 50257), (4, 32000), (3, 777), (300, 4099)]
TEMPS_E4 = (0, 1, 7000, 10000, 20000)
TOP_PS_E4 = (1, 5000, 9000, 10000)
MEASURED_GAP = 9.2e-8
EPS = 8 * MEASURED_GAP
WIDENED_CAP = 0.02


def top_ks(vocab):
    return (0, 1, 2, 50, vocab, vocab + 5)


def make_case(rows, vocab):
    """bf16 logits [2 * rows + 2, vocab]: random at scale 3, their coarse-rounded copy (many
    ties), then two hand-built rows (one finite entry in the ragged tail; all -inf), with per-row
    params / seeds / pos mixing every temperature, top-k and top-p value.  -> dict of CPU tensors;
    ``hand`` marks the hand-built rows."""
    g = torch.Generator().manual_seed(rows * 1000003 + vocab)
    rand = (torch.randn(rows, vocab, generator=g) * 3.0).to(torch.bfloat16)
    coarse = rand.float().round().to(torch.bfloat16)
    hand = torch.full((2, vocab), float("-inf"), dtype=torch.bfloat16)
    hand[0, vocab - 1] = -3.0
    logits = torch.cat([rand, coarse, hand])
    n = logits.shape[0]
    rng = np.random.default_rng(rows * 7919 + vocab)
    ks = top_ks(vocab)
    params = np.empty((n, 3), dtype=np.int32)
    for i in range(n):
        # a fixed walk through the grid, so that small cases still mix the values
        params[i] = (TEMPS_E4[(i + i // 5) % 5], ks[(i // 2 + i // 7) % 6], TOP_PS_E4[(i + i // 3) % 4])
    params[n - 2] = (10000, 0, 10000)
    params[n - 1] = (7000, 50, 9000)
    seeds = rng.integers(-2 ** 63, 2 ** 63 - 1, size=n, dtype=np.int64)
    pos = rng.integers(0, 8192, size=n).astype(np.int32)
    is_hand = np.zeros(n, dtype=bool)
    is_hand[n - 2:] = True
    return {"logits": logits, "params": torch.from_numpy(params), "seeds": torch.from_numpy(seeds),
            "pos": torch.from_numpy(pos), "hand": is_hand}


def mass_gap(logits_row, temp_e4):
    """sum_i |w32_i - w64_i| / Z64 of one sampled row (see the module docstring)."""
    def masses(dt):
        l = np.array(logits_row, dtype=dt)
        l[np.isnan(l)] = -np.inf
        with np.errstate(invalid="ignore"):
            d = l - l.max()
            d[l == l.max()] = 0
            return np.exp(d / dt(temp_e4 * 1e-4))
    w64, w32 = masses(np.float64), masses(np.float32).astype(np.float64)
    return float(np.abs(w32 - w64).sum() / w64.sum())


def _accept_widened(l, temp_e4, k, p_e4, u, got, eps):
    """The widened rule for one sampled row with an entry above -inf (float64 throughout)."""
    v = l.shape[0]
    if not 0 <= got < v:
        return False
    l = np.array(l, dtype=np.float64)
    l[np.isnan(l)] = -np.inf
    with np.errstate(invalid="ignore"):
        d = l - l.max()
        d[l == l.max()] = 0
        x = d / (temp_e4 * 1e-4)
    w = np.exp(x)
    keepk = x >= np.sort(x)[::-1][k - 1] if 0 < k < v else np.ones(v, dtype=bool)   # exact: counts
    if not keepk[got]:
        return False
    zk = (w * keepk).sum()
    vals, inv = np.unique(x, return_inverse=True)                      # ascending values
    gmass = np.bincount(inv, weights=w * keepk, minlength=len(vals))
    above = (gmass[::-1].cumsum()[::-1] - gmass)[inv]                  # survivors' mass strictly above
    if p_e4 < 10000:
        p = max(p_e4, 0) * 1e-4
        sure = keepk & (above <= p * zk - eps * zk)
        maybe = keepk & (above <= p * zk + eps * zk)
    else:
        sure = maybe = keepk
    if not maybe[got]:
        return False
    # every kept set between the two: `sure` plus the j largest borderline value groups
    border = np.unique(x[maybe & ~sure])[::-1]
    for j in range(len(border) + 1):
        s = sure | (maybe & np.isin(x, border[:j]))
        if not s[got]:
            continue
        m = w * s
        c = m.cumsum()
        z = c[-1]
        if c[got] - m[got] - eps * z <= u * z <= c[got] + eps * z:
            return True
    return False


def check_ids(case, got, eps=EPS):
    """Hold ``got`` (ids of an implementation under test) to the acceptance rule.  Returns the
    number of random rows that needed the widened rule; asserts on everything else."""
    logits = case["logits"].float().numpy()
    params = case["params"].numpy()
    u = ref.sample_uniforms(case["seeds"].numpy(), case["pos"].numpy())
    want, kept, _ = ref.sample_rows_detail(logits, params, u)
    got = np.asarray(got)
    widened = 0
    for i in np.nonzero(got != want)[0]:
        t, k, p = (int(a) for a in params[i])
        finite = np.nanmax(np.where(np.isnan(logits[i]), -np.inf, logits[i])) > -np.inf
        assert t > 0 and finite, f"row {i}: greedy / all -inf rows are exact: got {got[i]}, want {want[i]}"
        assert not case["hand"][i], f"hand-built row {i}: got {got[i]}, want {want[i]}"
        assert _accept_widened(logits[i], t, k, p, u[i], int(got[i]), eps), \
            f"row {i} (params {params[i].tolist()}, u {u[i]}): got {got[i]}, want {want[i]}, " \
            f"kept {bool(kept[i, got[i]]) if 0 <= got[i] < logits.shape[1] else None}"
        widened += 1
    n_random = int((~case["hand"]).sum())
    assert widened <= WIDENED_CAP * n_random, f"{widened} of {n_random} rows needed the widened rule"
    return widened


# ---- the distribution case: one 37-entry row drawn at pos 0..65535
DIST_V, DIST_N, DIST_SEED = 37, 65536, 0x5EEDC0FFEE123457
DIST_PARAMS = (13000, 12, 9000)


def dist_row():
    g = torch.Generator().manual_seed(37)
    return (torch.randn(1, DIST_V, generator=g) * 2.0).to(torch.bfloat16)


def chi2_sf(x, dof):
    """P(chi-square with dof degrees of freedom > x), from the closed forms for integer dof."""
    import math
    h = x / 2.0
    if dof % 2 == 0:
        term, total = 1.0, 1.0
        for i in range(1, dof // 2):
            term *= h / i
            total += term
        return math.exp(-h) * total
    term, total = 1.0, 0.0
    for j in range((dof - 1) // 2):
        term = 1.0 if j == 0 else term * x / (2 * j + 1)
        total += term
    return math.erfc(math.sqrt(h)) + math.sqrt(2.0 * x / math.pi) * math.exp(-h) * total


def chi2_critical_999(dof):
    """The 99.9 % point of chi-square: chi2_sf(x, dof) = 0.001 by bisection."""
    lo, hi = 0.0, 1000.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if chi2_sf(mid, dof) > 1e-3 else (lo, mid)
    return hi


def check_distribution(ids):
    """No draw outside the kept set; chi-square of the counts against the reference's exact kept
    probabilities under the 99.9 % critical value."""
    row = dist_row().float().numpy()
    _, kept, w = ref.sample_rows_detail(row, np.array([DIST_PARAMS]), np.array([0.5]))
    kept, w = kept[0], w[0]
    probs = w * kept / (w * kept).sum()
    counts = np.bincount(np.asarray(ids), minlength=DIST_V)
    assert counts[~kept].sum() == 0, "draws outside the kept set"
    nz = probs > 0
    exp = probs[nz] * DIST_N
    chi2 = float(((counts[nz] - exp) ** 2 / exp).sum())
    dof = int(nz.sum()) - 1
    assert dof >= 3
    assert chi2 < chi2_critical_999(dof), f"chi2 {chi2:.2f} >= {chi2_critical_999(dof):.2f} (dof {dof})"
    return chi2, dof
