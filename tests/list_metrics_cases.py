"""Shared cases and the host reference of the list-metric tests
(tests/test_list_metrics_cpu.py, tests/test_list_metrics_gpu.py).

A case is a dict: ``rows`` int64 [n], ``offsets`` int64 [R + 1], ``counts``
int32 [R] or None, ``at``, ``table`` fp32 [n_items, d], ``scores`` fp32 [n],
``info`` fp64 [n_items], ``relevant`` (a list of R sets), ``ks``.
``host_reference(case, inv)`` is the host computation the device must match,
written from the definitions in include/dcnr.h: every count a Python int, the
pair cosines in fp64 from the fp32 table and the inverse norms it is GIVEN
(the library's own, so the stage is checked from its stored inputs), the Gini
numerator from the sorted counts in Python ints, membership by Python sets,
every mean ``math.fsum`` of the per-list doubles.
"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

# (name, R, at, d, n_items, layout)
SPECS = [
    ("mix", 257, 20, 64, 1000, "mix"),
    ("k1", 1, 1, 1, 1, "mix"),
    ("k2", 3, 2, 4, 7, "mix"),
    ("k33", 257, 33, 33, 1000, "mix"),
    ("k64", 3, 64, 100, 1000, "mix"),
    ("k128", 3, 128, 256, 1000, "mix"),
    ("k128few", 1, 128, 4, 7, "mix"),
    ("nullcounts", 5000, 20, 64, 1000, "full"),
    ("identical", 257, 20, 64, 1000, "identical"),
    ("equal", 3, 20, 4, 7, "equal"),
    ("broken", 257, 20, 33, 1000, "broken"),
    ("repeats", 3, 20, 4, 1000, "repeats"),
    # a workgroup's second step over its lists (more than 2048 x 4 lists a wave each, more than
    # 2048 lists a workgroup each); item counts of 1024 and more (past the counts kernel's LDS bins)
    ("steps", 9000, 20, 4, 1000, "mix"),
    ("steps33", 2100, 33, 4, 1000, "mix"),
    ("identical1100", 1100, 20, 4, 1000, "identical"),
]
BIG = ("nullcounts", "steps", "steps33")       # (the host-only checks leave these out)
NAMES = [s[0] for s in SPECS]


def cutoffs(at):
    return tuple(sorted({min(k, at) for k in (1, 5, 10, at)}))[:4]


def lengths(at):
    """The m every part can go wrong at, counts beyond ``at`` included."""
    return sorted({0, 1, 2, 3, max(at - 1, 0), at, at + 5})


def make_case(name):
    _, R, at, d, n_items, layout = next(s for s in SPECS if s[0] == name)
    rng = np.random.default_rng(7000 + NAMES.index(name))
    table = rng.standard_normal((n_items, d)).astype(np.float32)
    table[np.abs(table) < 1e-3] = 0.5          # no zero-norm rows (d = 1 included)
    if n_items >= 10:
        table[1:10] = table[0]                 # duplicate embedding rows: cosine 1
    info = -np.log2(rng.uniform(1e-4, 1.0, n_items))
    ks = cutoffs(at)
    lens = lengths(at)
    seg, cnt = [], []                          # segment length, measured count
    for r in range(R):
        if layout in ("full", "identical"):
            seg.append(at)
            cnt.append(at)
        elif layout == "equal":
            seg.append(n_items)
            cnt.append(n_items)
        else:
            c = lens[(len(lens) - 1 - r) % len(lens)] if R > 1 else lens[-2]
            cnt.append(c)
            seg.append(c + (r % 3))            # a count may stop short of its segment
    offsets = np.zeros(R + 1, np.int64)
    np.cumsum(seg, out=offsets[1:])
    n = int(offsets[R])
    rows = np.zeros(n, np.int64)
    first = None
    for r in range(R):
        L = seg[r]
        if layout == "identical" and first is not None:
            pick = first
        elif layout == "equal":
            pick = rng.permutation(n_items)
        elif layout == "repeats":              # a row repeated inside a list: its count exceeds R
            pick = rng.choice(n_items, size=L, replace=False)
            pick[::2] = 11
        else:
            pick = rng.choice(n_items, size=L, replace=L > n_items)
            if layout == "mix" and L >= 3 and n_items >= 10 and r % 4 == 0:
                pick[:3] = (0, 1, 2)           # three copies of one embedding in a list
        first = pick if first is None else first
        rows[offsets[r]:offsets[r + 1]] = pick
    counts = None if layout in ("full", "identical", "equal") else np.array(cnt, np.int32)
    scores = rng.standard_normal(n).astype(np.float32) * 3
    # held-out sets: empty; the row at rank 1, at rank ks[j], at ks[j] + 1, at rank `at` and
    # just behind it; a stranger; several.  The kind steps once per cycle of the lengths and the
    # cutoff once per cycle of the kinds, so every (length, kind, cutoff) occurs (_heldout_ok)
    relevant = []
    nl = len(lens)
    for r in range(R):
        lst = rows[offsets[r]:offsets[r + 1]]
        if R > nl:
            kind, j = (r // nl) % 7, ks[(r // (7 * nl)) % len(ks)]
        elif R > 1:        # few lists, the longest first: behind `at`, at ks[0] + 1, at ks[-2]
            kind, j = (4, 3, 2)[r % 3], (ks[-1], ks[0], ks[-2] if len(ks) > 1 else ks[0])[r % 3]
        else:
            kind, j = 2, ks[-1]
        s = set()
        if kind == 1 and len(lst) >= 1:
            s = {int(lst[0])}
        elif kind == 2 and len(lst) >= j:
            s = {int(lst[j - 1])}
        elif kind == 3 and len(lst) > j:
            s = {int(lst[j])}
        elif kind == 4 and len(lst) > at:
            s = {int(lst[at - 1]), int(lst[at])}
        elif kind == 5:
            s = {int(rng.integers(0, n_items))}
        elif kind == 6:
            s = set(int(v) for v in lst[1::3]) | {int(rng.integers(0, n_items))}
        relevant.append(s)
    if layout == "repeats":                    # (a repeated held-out row would count once per position)
        relevant = [s - {11} for s in relevant]
    if layout == "broken":
        counts = counts.copy()
        rows[offsets[5]] = -1                  # a marked answer (seg[5] >= 1 by construction below)
        rows[offsets[9]] = n_items             # a row past the table
        rows[offsets[100] + 1] = -7            # a negative row that is no mark
        rows[offsets[30] + 1] = -1             # a -1 behind the first position
        offsets[200] = offsets[199] - 3        # not monotone: list 199 is bad, list 200 overlaps
        offsets[R] = n + 5                     # the last segment leaves the buffer
        counts[60] = -1
        counts[61] = seg[61] + 1               # beyond its segment
        counts[200] = 2
    return dict(name=name, R=R, at=at, d=d, n_items=n_items, rows=rows, offsets=offsets,
                counts=counts, table=table, scores=scores, info=info, relevant=relevant, ks=ks)


def _broken_ok():
    """The lists the 'broken' case touches hold the rows it overwrites."""
    _, R, at, *_ = next(s for s in SPECS if s[0] == "broken")
    lens = lengths(at)
    cnt = lambda r: lens[(len(lens) - 1 - r) % len(lens)]
    assert cnt(5) >= 1 and cnt(9) >= 1 and cnt(100) >= 2 and cnt(30) >= 2, [cnt(r) for r in (5, 9, 100, 30)]


_broken_ok()


def placements(case):
    """Where the held-out rows of the well-formed lists fall: a set of tags."""
    at, ks, rows, off, counts = case["at"], case["ks"], case["rows"], case["offsets"], case["counts"]
    tags = set()
    for r in range(case["R"]):
        o, o1 = int(off[r]), int(off[r + 1])
        if o < 0 or o1 < o or o1 > rows.size:
            continue
        cnt = o1 - o if counts is None else int(counts[r])
        if cnt < 0 or cnt > o1 - o:
            continue
        lst, m = rows[o:o1].tolist(), min(cnt, at)
        for v in case["relevant"][r]:
            if v not in lst:
                tags.add("stranger")
                continue
            p = lst.index(v)                       # its first position
            if p == 0 and m >= 1:
                tags.add("rank1")
            for k in ks:
                if p == k - 1 and p < m:
                    tags.add(("at", k))
                if p == k and p < m:
                    tags.add(("after", k))
            if p >= at and cnt > at:
                tags.add("beyond_at")              # measured list full, the row just outside it
            elif p >= m:
                tags.add("behind_count")
    return tags


def _heldout_ok():
    """The held-out rows sit where the cases claim: at rank 1, at every cutoff, one behind every
    cutoff below ``at``, and at position ``at`` of a list whose count exceeds ``at``."""
    for name in ("mix", "k33", "k2", "k64", "k128"):
        c = make_case(name)
        tags, at, ks = placements(c), c["at"], c["ks"]
        want = {"beyond_at", ("at", at)}
        if c["R"] > 100:
            want |= {"rank1", "stranger", "behind_count"} | {("at", k) for k in ks} | \
                {("after", k) for k in ks if k < at}
        assert want <= tags, (name, sorted(map(str, want - tags)))


_heldout_ok()


def numpy_inv_norms(table):
    """fp32 inverse row norms on the host (the CPU tests' stand-in for the
    library's own)."""
    t = table.astype(np.float64)
    return (1.0 / np.sqrt((t * t).sum(1))).astype(np.float32)


def discount_tables(k_max):
    from dcnr.metrics import dcg_tables
    return dcg_tables(k_max)


def gini_numerator(counts):
    """sum over i = 1 .. n of (2 i - n - 1) c_(i), the counts ascending: Python ints."""
    c = sorted(int(v) for v in counts)
    n = len(c)
    return sum((2 * (i + 1) - n - 1) * v for i, v in enumerate(c))


@lru_cache(maxsize=None)
def _triu(m):
    return np.triu_indices(m, 1)


def host_reference(case, inv):
    R, at, n_items, ks = case["R"], case["at"], case["n_items"], case["ks"]
    rows, off, counts = case["rows"], case["offsets"], case["counts"]
    n = rows.size
    T = case["table"].astype(np.float64)
    invd = np.asarray(inv, np.float32).astype(np.float64)
    sc = case["scores"].astype(np.float64)
    info = case["info"]
    nk = len(ks)
    disc, ideal = discount_tables(ks[-1]) if nk else (None, None)
    expo = [0] * n_items
    rec = dict(m=np.zeros(R, np.int64), n_rel=np.zeros(R, np.int64),
               first_hit_rank=np.zeros(R, np.int64), hits=np.zeros((R, nk), np.int64),
               pair_cos_sum=np.zeros(R), score_sum=np.zeros(R), info_sum=np.zeros(R),
               dcg=np.zeros((R, nk)), abs_score_sum=np.zeros(R))
    n_bad = n_marked = n_scored = n_pairs = n_entries = n_rel_lists = 0
    hit_lists = [0] * nk
    ild_t, mrr_t = [], []
    recall_t, ndcg_t = [[] for _ in ks], [[] for _ in ks]
    for r in range(R):
        o, o1 = int(off[r]), int(off[r + 1])
        if o < 0 or o1 < o or o1 > n:
            n_bad += 1
            continue
        cnt = o1 - o if counts is None else int(counts[r])
        if cnt < 0 or cnt > o1 - o:
            n_bad += 1
            continue
        m = min(cnt, at)
        lst = [int(v) for v in rows[o:o + m]]
        if o1 > o and rows[o] == -1:
            n_marked += 1
            continue
        if any(v < 0 or v >= n_items for v in lst):
            n_bad += 1
            continue
        rel = case["relevant"][r]
        rec["m"][r], rec["n_rel"][r] = m, len(rel)
        n_scored += m >= 1
        n_entries += m
        for v in lst:
            expo[v] += 1
        rec["score_sum"][r] = math.fsum(sc[o:o + m])
        rec["abs_score_sum"][r] = math.fsum(np.abs(sc[o:o + m]))
        rec["info_sum"][r] = math.fsum(info[lst]) if m else 0.0
        if m >= 2:
            X = T[lst]
            cos = (X @ X.T) * np.outer(invd[lst], invd[lst])
            pc = math.fsum(cos[_triu(m)])
            rec["pair_cos_sum"][r] = pc
            n_pairs += 1
            ild_t.append(1.0 - pc / (m * (m - 1) // 2))
        if rel:
            n_rel_lists += 1
            where = [p for p, v in enumerate(lst) if v in rel]
            fhr = where[0] + 1 if where else 0
            rec["first_hit_rank"][r] = fhr
            mrr_t.append(1.0 / fhr if fhr else 0.0)
            for j, k in enumerate(ks):
                h = [p for p in where if p < k]
                dcg = math.fsum(disc[p] for p in h)
                rec["hits"][r, j], rec["dcg"][r, j] = len(h), dcg
                hit_lists[j] += len(h) > 0
                recall_t[j].append(len(h) / len(rel))
                ndcg_t[j].append(dcg / ideal[min(k, len(rel)) - 1])
    mean = lambda t, m: math.fsum(t) / m if m else math.nan
    n_distinct = sum(1 for c in expo if c)
    gnum = gini_numerator(expo)
    return dict(
        n_lists=R, n_lists_scored=int(n_scored), n_lists_pairs=n_pairs, n_marked=n_marked,
        n_bad_list=n_bad, n_entries=n_entries, n_distinct_items=n_distinct, gini_num=gnum,
        n_rel_lists=n_rel_lists, hit_lists=tuple(hit_lists),
        ild=mean(ild_t, n_pairs), mrr=mean(mrr_t, n_rel_lists),
        mean_score=mean(rec["score_sum"], n_entries), mean_info=mean(rec["info_sum"], n_entries),
        mean_abs_score=mean(rec["abs_score_sum"], n_entries),
        coverage=n_distinct / n_items,
        gini=gnum / (n_items * n_entries) if n_entries else math.nan,
        hit_rate=tuple(hit_lists[j] / n_rel_lists if n_rel_lists else math.nan for j in range(nk)),
        recall=tuple(mean(recall_t[j], n_rel_lists) for j in range(nk)),
        ndcg=tuple(mean(ndcg_t[j], n_rel_lists) for j in range(nk)),
        records=rec, exposure=expo)
