"""Shared cases and the host reference of the per-group ranking-metric tests
(tests/test_grouped_metrics_cpu.py, tests/test_grouped_metrics_gpu.py,
tests/golden/make_grouped_metrics_golden.py).

A case is (n, pattern, layout, seed): the logits and labels are
``metrics_cases.make_case((n, pattern, seed))``, the group ids come from the
layout (drawn from the same seed + 1); a layout may overwrite labels so that
some groups hold a single class.  ``host_reference`` is the host computation
the device must equal: a stable sort of (group, -score), every count a Python
int, every mean ``math.fsum`` of the per-group doubles.
"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

import metrics_cases as mc

# the walk's tile is dcnr_eval_metrics' AUC tile and the sort is the same
# sort: csrc/metrics.hip's AUC_TILE_MIN and UNIT_KEYS, read from one place
TILE = mc.TILE
UNIT = mc.UNIT
WAVE = 64

KS = (1, 5, 10, 4096)
LAYOUTS = ("one", "own", "wave64", "mean8", "huge3", "gaps", "oneclass",
           "ng2", "ng2049", "ng4m", "ngmax")
# n_groups of the layouts that hold a few ids only: 3, 4, 5 and 6 sort passes
FEW = {"ng2": 2, "ng2049": (1 << 11) + 1, "ng4m": (1 << 22) + 1, "ngmax": (1 << 31) - 1}


def _cases():
    out = []
    for n in (2, 63, 64, 65):
        for p, lay in (("distinct", "one"), ("q16", "mean8"), ("equal", "own"), ("q16", "one"),
                       ("distinct", "wave64"), ("special", "mean8")):
            if p == "special" and n < 63:
                continue
            out.append((n, p, lay))
    for n in (TILE - 1, TILE, TILE + 1, UNIT - 1, UNIT, UNIT + 1):
        for p, lay in (("distinct", "one"), ("q16", "mean8"), ("q16", "wave64"), ("distinct", "huge3")):
            out.append((n, p, lay))
    n = 3 * UNIT + 3
    pats = ("distinct", "q16", "equal", "special")
    for j, lay in enumerate(LAYOUTS):
        out.append((n, pats[j % 4], lay))
    for p in pats:
        out.append((n, p, "mean8" if p != "q16" else "huge3"))
    out.append((n, "equal", "one"))
    out.append((n, "special", "one"))
    n = 65539
    for p, lay in (("distinct", "one"), ("q16", "mean8"), ("equal", "huge3"), ("special", "own"),
                   ("distinct", "gaps"), ("q16", "oneclass"), ("distinct", "wave64"),
                   ("q16", "ng2"), ("distinct", "ng2049"), ("q16", "ng4m"), ("special", "ngmax")):
        out.append((n, p, lay))
    # more than 64 tiles (the close kernel's second step), and tiles above TILE rows (n > 1024 TILE)
    out.append((65 * TILE + 5, "distinct", "one"))
    out.append((65 * TILE + 5, "q16", "huge3"))
    out.append((1024 * TILE + 4097, "q16", "one"))
    out.append((1024 * TILE + 4097, "distinct", "wave64"))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return [(n, p, lay, 3000 + i) for i, (n, p, lay) in enumerate(uniq)]


CASES = _cases()


def case_id(case):
    return f"{case[1]}-{case[2]}-{case[0]}"


def make_groups(n, layout, rng, y):
    """(groups int64 [n], n_groups, wants_records); may overwrite ``y``."""
    if layout == "one":
        return np.zeros(n, np.int64), 1, True
    if layout == "own":
        return rng.permutation(n).astype(np.int64), n, True
    if layout == "wave64":                       # sorted, the groups are the 64-row wave steps
        return rng.permutation(np.arange(n, dtype=np.int64) // WAVE), (n + WAVE - 1) // WAVE, True
    if layout == "mean8":
        ng = max(1, n // 8)
        return rng.integers(0, ng, n).astype(np.int64), ng, True
    if layout == "huge3":                        # three groups of ~20 % of the rows each, the rest alone
        ng = n + 3
        g = np.arange(n, dtype=np.int64) + 3
        pick = rng.random(n)
        for j, gid in enumerate((0, ng // 2, ng - 1)):
            g[(pick >= 0.2 * j) & (pick < 0.2 * (j + 1))] = gid
        return g, ng, True
    if layout == "gaps":                         # two of every three ids unused, and a tail of unused ids
        m = n // 8 + 1
        return 3 * rng.integers(0, m, n).astype(np.int64) + 1, 3 * m + 5, True
    if layout == "oneclass":                     # a third of the groups all negative, a third all positive
        ng = max(3, n // 8)
        g = rng.integers(0, ng, n).astype(np.int64)
        y[g % 3 == 0] = 0.0
        y[g % 3 == 1] = 1.0
        return g, ng, True
    if layout in FEW:                            # a few ids of a large range, both ends among them
        ng = FEW[layout]
        ids = np.unique(np.r_[0, ng - 1, rng.integers(0, ng, 5)]).astype(np.int64)
        return ids[rng.integers(0, len(ids), n)], ng, False
    raise ValueError(layout)


def make_case(case):
    """(logits fp32 [n], labels fp32 [n], groups int64 [n], n_groups, wants_records)."""
    n, pattern, layout, seed = case
    z, y = mc.make_case((n, pattern, seed))
    y = y.copy()
    g, ng, rec = make_groups(n, layout, np.random.default_rng(seed + 1), y)
    return z, y, np.ascontiguousarray(g, np.int64), int(ng), rec


def dcg_tables(k_max):
    """discount[i] = 1 / log2(i + 2), ideal = its running sum (sequential),
    float64 [k_max]: what dcnr.metrics.dcg_tables hands the device."""
    discount = 1.0 / np.log2(np.arange(k_max, dtype=np.float64) + 2.0)
    return discount, np.cumsum(discount)


def served_order(z, g):
    """Stable sort of (group, -score); -0.0 ties with +0.0 (z + 0.0)."""
    zc = np.asarray(z, np.float32) + np.float32(0.0)
    return np.lexsort((-zc.astype(np.float64), g)), zc


def host_reference(z, y, g, n_groups, ks=KS):
    """dict: ``gids`` (the present groups, ascending) with per-group int64
    arrays n, n_pos, auc_u2, first_pos_rank, hits [m, nk] and float64 dcg
    [m, nk] (summed in long double, then rounded once); the summary's counts
    as Python ints; the means as math.fsum of the per-group doubles, with the
    number of groups each averages."""
    z = np.asarray(z, np.float32)
    y = np.asarray(y, np.float32)
    g = np.asarray(g, np.int64)
    n = z.shape[0]
    nk = len(ks)
    assert np.finfo(np.longdouble).nmant >= 63, "host reference sums DCG in an 80-bit long double"
    order, zc = served_order(z, g)
    gs, zs, ys = g[order], zc[order], y[order]
    pos = (ys == 1.0)
    idx = np.arange(n, dtype=np.int64)
    ghead = np.r_[True, gs[1:] != gs[:-1]]
    hpos = np.flatnonzero(ghead)
    gids = gs[hpos]
    m = len(hpos)
    gi = np.cumsum(ghead) - 1                      # row -> ordinal of its group
    rank = idx - hpos[gi] + 1
    n_u = np.diff(np.r_[hpos, n]).astype(np.int64)
    P = np.add.reduceat(pos.astype(np.int64), hpos)
    N = n_u - P
    # 2U per group from its tie groups: pos_t * (2 * negatives below + neg_t)
    thead = ghead | np.r_[True, zs[1:] != zs[:-1]]
    tpos = np.flatnonzero(thead)
    pos_t = np.add.reduceat(pos.astype(np.int64), tpos)
    neg_t = np.add.reduceat((~pos).astype(np.int64), tpos)
    tg = gi[tpos]                                  # tie group -> group ordinal
    negcum = np.cumsum(neg_t)                      # negatives through tie group t, all groups
    neg_before_group = (np.cumsum(N) - N)[tg]
    neg_below = N[tg] - (negcum - neg_before_group)     # lower scores come later in the group
    u2 = np.zeros(m, np.int64)
    np.add.at(u2, tg, pos_t * (2 * neg_below + neg_t))
    big = np.int64(1) << 40
    fpr = np.minimum.reduceat(np.where(pos, rank, big), hpos)
    fpr = np.where(fpr == big, 0, fpr).astype(np.int64)
    hits = np.zeros((m, nk), np.int64)
    dcg = np.zeros((m, nk), np.float64)
    if nk:
        discount, ideal = dcg_tables(ks[-1])
        dl = discount.astype(np.longdouble)
        for j, k in enumerate(ks):
            inb = pos & (rank <= k)
            hits[:, j] = np.add.reduceat(inb.astype(np.int64), hpos)
            terms = np.where(inb, dl[np.minimum(rank, ks[-1]) - 1], np.longdouble(0))
            dcg[:, j] = np.add.reduceat(terms, hpos).astype(np.float64)
    aucg = (P > 0) & (N > 0)
    rk = P > 0
    auc_u = u2[aucg].astype(np.float64) / (2.0 * P[aucg].astype(np.float64) * N[aucg].astype(np.float64))
    m_auc, m_rk = int(aucg.sum()), int(rk.sum())
    rows_auc = int(n_u[aucg].sum())
    nan = float("nan")
    ref = dict(
        gids=gids, n_u=n_u, n_pos=P, auc_u2=u2, first_pos_rank=fpr, hits=hits, dcg=dcg,
        auc_groups=aucg, ranked_groups=rk, auc_u=auc_u,
        n=int(n), n_groups_present=int(m), n_groups_auc=m_auc, n_groups_ranked=m_rk, n_rows_auc=rows_auc,
        hit_groups=tuple(int((hits[rk, j] > 0).sum()) for j in range(nk)),
        gauc=math.fsum(n_u[aucg].astype(np.float64) * auc_u) / rows_auc if m_auc else nan,
        auc_macro=math.fsum(auc_u) / m_auc if m_auc else nan,
        mrr=math.fsum(1.0 / fpr[rk].astype(np.float64)) / m_rk if m_rk else nan,
    )
    hr, rc, nd, ndcg_u = [], [], [], np.zeros((m, nk), np.float64)
    for j, k in enumerate(ks):
        if not m_rk:
            hr.append(nan), rc.append(nan), nd.append(nan)
            continue
        Pr = P[rk]
        hr.append(ref["hit_groups"][j] / m_rk)
        rc.append(math.fsum(hits[rk, j].astype(np.float64) / Pr.astype(np.float64)) / m_rk)
        ndcg_u[rk, j] = dcg[rk, j] / ideal[np.minimum(k, Pr) - 1]
        nd.append(math.fsum(ndcg_u[rk, j]) / m_rk)
    ref.update(hit_rate=tuple(hr), recall=tuple(rc), ndcg=tuple(nd), ndcg_u=ndcg_u)
    return ref


@lru_cache(maxsize=None)
def case_with_reference(case):
    """(z, y, g, n_groups, wants_records, host_reference) of a case, computed
    once per process; callers do not modify the arrays."""
    z, y, g, ng, rec = make_case(case)
    for a in (z, y, g):
        a.setflags(write=False)
    return z, y, g, ng, rec, host_reference(z, y, g, ng)


def sampled(mask, limit=128):
    """Ordinals of at most ``limit`` of the groups ``mask`` marks, evenly
    spaced (all of them when there are no more): the groups the fixture holds
    sklearn's values for."""
    idx = np.flatnonzero(mask)
    if len(idx) <= limit:
        return idx
    return idx[np.linspace(0, len(idx) - 1, limit).astype(np.int64)]
