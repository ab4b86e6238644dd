"""Shared cases and the host reference of the validation-metric tests
(tests/test_metrics_cpu.py, tests/test_metrics_gpu.py,
tests/golden/make_metrics_golden.py).

A case is (n, pattern, seed); ``make_case`` draws its logits and labels from
``numpy.random.default_rng(seed)``.  ``host_reference`` is the exact host
computation the device must equal: a stable argsort of the scores, tie
groups, 2U in int64, and fp64 logloss / RMSE (p = the fp64 sigmoid rounded to
fp32), summed exactly (math.fsum).
"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

# csrc/metrics.hip's UNIT_KEYS and AUC_TILE_MIN: keys per sort unit, smallest AUC tile
UNIT = 4096
TILE = 2048

PATTERNS = ("distinct", "q16", "equal", "sep_pos", "sep_neg", "special", "one_pos", "one_neg")


def _cases():
    out = []
    for n in (2, 63, 64, 65):
        for p in ("distinct", "q16", "equal"):
            out.append((n, p))
    for n in (63, 64, 65):
        out.append((n, "special"))
    for n in (TILE - 1, TILE, TILE + 1, UNIT - 1, UNIT, UNIT + 1):   # one block's worth +- 1
        for p in ("distinct", "q16"):
            out.append((n, p))
    for p in PATTERNS:                                               # three blocks + 3
        out.append((3 * UNIT + 3, p))
    for p in ("distinct", "q16", "equal", "special"):                # several scatter units per bucket
        out.append((65539, p))
    out.append(((1 << 20) + 1, "distinct"))
    return [(n, p, 1000 + i) for i, (n, p) in enumerate(out)]


CASES = _cases()


def case_id(case):
    return f"{case[1]}-{case[0]}"


def make_case(case):
    """(logits fp32 [n], labels fp32 [n] of 0.0 / 1.0), both classes present."""
    n, pattern, seed = case
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.4).astype(np.float32)
    z = (rng.standard_normal(n) * 2.0).astype(np.float32)
    if pattern == "distinct":
        pass
    elif pattern == "q16":
        z = (rng.integers(0, 16, n).astype(np.float32) - 7.5) * np.float32(0.5)
    elif pattern == "equal":
        z = np.full(n, 0.375, np.float32)
    elif pattern in ("sep_pos", "sep_neg"):          # perfectly separated: AUC exactly 1.0 / 0.0
        s = 1.0 if pattern == "sep_pos" else -1.0
        z = (np.abs(z) + np.float32(0.25)) * np.where(y == 1, s, -s).astype(np.float32)
    elif pattern == "special":                       # +-0 tied, +-inf, denormals, duplicates
        vals = np.array([0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.0, -1.0,
                         1e38, -2.5e37], np.float32)
        k = max(1, n // 2)
        where = rng.choice(n, size=k, replace=False)
        z[where] = vals[rng.integers(0, len(vals), k)]
    elif pattern == "one_pos":
        y[:] = 0.0
        y[rng.integers(0, n)] = 1.0
    elif pattern == "one_neg":
        y[:] = 1.0
        y[rng.integers(0, n)] = 0.0
    else:
        raise ValueError(pattern)
    if pattern not in ("one_pos", "one_neg"):
        if pattern in ("sep_pos", "sep_neg"):
            if y.min() == y.max():                   # (never at these sizes)
                y[0], z[0] = 1.0 - y[0], -z[0]
        else:
            y[0], y[1] = 0.0, 1.0
    return np.ascontiguousarray(z, np.float32), np.ascontiguousarray(y, np.float32)


def exact_u2(z, y):
    """(2U, P, N) as Python ints: 2U = sum over positives i of
    2 #{neg j: z_j < z_i} + #{neg j: z_j == z_i}, IEEE equality."""
    z = np.asarray(z, np.float32)
    y = np.asarray(y, np.float32)
    order = np.argsort(z, kind="stable")
    zs, ys = z[order], y[order]
    head = np.flatnonzero(np.r_[True, zs[1:] != zs[:-1]])   # tie-group heads
    neg_g = np.add.reduceat((ys == 0).astype(np.int64), head)
    pos_g = np.add.reduceat((ys == 1).astype(np.int64), head)
    neg_before = np.cumsum(neg_g) - neg_g
    u2 = int(np.sum(pos_g * (2 * neg_before + neg_g), dtype=np.int64))
    return u2, int(pos_g.sum()), int(neg_g.sum())


def host_reference(z, y):
    """dict(u2, n_pos, n_neg, auc, logloss, rmse) -- what dcnr_eval_metrics
    must give (auc bit for bit, the fp64 sums to rounding)."""
    z = np.asarray(z, np.float32)
    y = np.asarray(y, np.float32)
    n = z.shape[0]
    u2, P, N = exact_u2(z, y)
    zd, yd = z.astype(np.float64), y.astype(np.float64)
    with np.errstate(all="ignore"):
        terms = np.maximum(zd, 0.0) - zd * yd + np.log1p(np.exp(-np.abs(zd)))
        p = (1.0 / (1.0 + np.exp(-zd))).astype(np.float32)
        d = yd - p.astype(np.float64)
        sq = d * d
    logloss = math.fsum(terms) / n if np.all(np.isfinite(terms)) else float(np.sum(terms) / n)
    rmse = math.sqrt(math.fsum(sq) / n)
    auc = u2 / (2.0 * P * N) if P * N else float("nan")
    return dict(u2=u2, n_pos=P, n_neg=N, auc=auc, logloss=logloss, rmse=rmse)


@lru_cache(maxsize=None)
def case_with_reference(case):
    """(z, y, host_reference) of a case, computed once per process; callers do
    not modify the arrays."""
    z, y = make_case(case)
    z.setflags(write=False)
    y.setflags(write=False)
    return z, y, host_reference(z, y)


def same_or_close(a, b, rel=0.0, abs_=0.0):
    """a == b up to the bounds; NaN matches NaN and an infinity its own sign
    (the logloss of a +-inf logit)."""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= max(abs_, rel * abs(b))
