"""Shared by test_admit_cpu.py and test_admit_gpu.py: the dict that numbers raw
ids by first appearance, id batches with known and new ids mixed, frames cut in
a fit part P and a later part S, and appended rows for the neighbour table."""
import numpy as np

import neighbor_update_rule as rule
import prepare_common as pc
import transform_common as tc

RESERVED = tc.RESERVED
INT64_MAX = (1 << 63) - 1
FIVE = ("user", "item", "target", "cat", "num")


def dict_insert(table, raw):
    """The yardstick: ``table`` (id -> index, grown in place) numbers every
    id it does not hold ``len(table)`` at its first appearance, as
    ``enumerate(df[col].unique())`` does.  Returns (indices [M], new ids)."""
    out, new = [], []
    for v in np.asarray(raw, dtype=np.int64).reshape(-1).tolist():
        if v not in table:
            table[v] = len(table)
            new.append(v)
        out.append(table[v])
    return np.array(out, dtype=np.int64), np.array(new, dtype=np.int64)


def mixed_batch(rng, known, M, n_new, low32=False):
    """M ids: about half drawn from ``known``, the rest from ``n_new`` ids the
    map does not hold (each at least once when M allows), shuffled.  ``low32``:
    the new ids agree in their low 32 bits."""
    known = np.asarray(known, dtype=np.int64)
    top = int(np.abs(known).max()) + 1 if known.size else 1
    if low32:
        fresh = (np.arange(1, n_new + 1, dtype=np.int64) << 32) + (top & 0xFFFFFFFF) + (1 << 50)
    else:
        fresh = top + 1 + rng.permutation(4 * n_new + 4)[:n_new].astype(np.int64) * 3
    fresh = fresh[~np.isin(fresh, known)]
    n_known = M // 2 if known.size else 0
    q = np.concatenate([rng.choice(known, n_known) if n_known else np.zeros(0, np.int64),
                        rng.choice(fresh, M - n_known) if fresh.size else np.zeros(0, np.int64)])
    q[:min(fresh.size, q.size)] = fresh[:q.size]
    rng.shuffle(q)
    return q.astype(np.int64)


def split_case(seed, M, M2, use_filter=True, n_users=None, n_items=None):
    """A random frame of M + M2 rows, P the first M and S the rest: every
    category of S occurs in P and none is missing there (a fit drops a row
    with a missing category, train.py's dropna, where ``transform`` keeps it);
    S's users and hotels go beyond P's.  Returns (whole, P's case)."""
    whole = pc.random_case(seed, M + M2, n_users=n_users or (M + M2) // 2, n_items=n_items or (M + M2) // 5,
                           use_filter=use_filter)
    for c, k in enumerate(whole["cat"]):
        k[M:][k[M:] < 0] = k[:M][k[:M] >= 0][0]
        assert np.isin(k[M:], k[:M]).all(), f"category column {c}: S holds a key P does not"
    fit_case = dict(whole, **dict(zip(FIVE, tc.part(whole, 0, M))))
    return whole, fit_case


def appended_rows(table, m, seed):
    """m rows to append to ``table``: an exact copy of row 5 (ties break by
    row), a zero row, a pair whose nearest are each other (at a distance far
    above float32's rounding: no tie that two ways of summing would break
    differently), rows next to old rows, then random ones -- as many kinds as
    m allows, in that order."""
    rng = np.random.default_rng(seed)
    N, d = table.shape
    noise = lambda k: rng.standard_normal((k, d)).astype(np.float32)
    far = noise(1)
    kinds = [table[5:6].copy(), np.zeros((1, d), np.float32), 40 * far, 3 * far + np.float32(0.2) * noise(1),
             np.float32(1.5) * table[rng.integers(0, N, 3)] + np.float32(0.05) * noise(3)]
    v = np.concatenate(kinds)[:m]
    if m > v.shape[0]:
        v = np.concatenate([v, noise(m - v.shape[0])])
    return v.astype(np.float32)


def grown_distances(table, new):
    return rule.distances(np.concatenate([table, new]).astype(np.float32))
