"""F13: neighbours within a row set, from the library the reference uses.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_within_golden.py

Writes tests/golden/f13_knn_within.npz.  The reference's index is
scikit-learn's ``NearestNeighbors(metric='cosine', algorithm='brute')``
(main.py:268-270); "the k nearest rows of a set" is that index fitted on
``table[set]``.  Spec: ``np.random.default_rng(20261020)``; a standard-normal
fp32 table 5003 x 24; sets of 1, 7, 40, 300, 2500 and 5003 rows
(``rng.choice`` without replacement, sorted); k = min(10, set size); per set
the queries are the set's first two rows (one for the 1-row set) and 6 random
normal queries.  Stored per set s: ``set{s}`` (rows, int64), ``q{s}``,
``dist{s}`` fp32 and ``idx{s}`` (positions within the set, int64).  The script
prints the share of positions whose distance has no neighbour within 2e-6 and
the smallest gap.
"""
from __future__ import annotations

import os

import numpy as np
from sklearn.neighbors import NearestNeighbors

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (1, 7, 40, 300, 2500, 5003)
ATOL = 2e-6


def main():
    rng = np.random.default_rng(20261020)
    N, d = 5003, 24
    table = rng.standard_normal((N, d), dtype=np.float32)
    out = {"table": table, "n_sets": np.int64(len(SIZES))}
    n_iso = n_all = 0
    gap = np.inf
    for s, n in enumerate(SIZES):
        rows = np.sort(rng.choice(N, n, replace=False)).astype(np.int64)
        q = np.concatenate([table[rows[:min(2, n)]], rng.standard_normal((6, d), dtype=np.float32)])
        k = min(10, n)
        index = NearestNeighbors(n_neighbors=k, metric="cosine", algorithm="brute").fit(table[rows])
        dist, idx = index.kneighbors(q)
        out[f"set{s}"] = rows
        out[f"q{s}"] = q.astype(np.float32)
        out[f"dist{s}"] = dist.astype(np.float32)
        out[f"idx{s}"] = idx.astype(np.int64)
        if k > 1:
            diff = np.diff(dist, axis=1)
            near = diff <= ATOL
            iso = np.ones(dist.shape, bool)
            iso[:, 1:] &= ~near
            iso[:, :-1] &= ~near
            gap = min(gap, float(diff.min()))
        else:
            iso = np.ones(dist.shape, bool)
        n_iso += int(iso.sum())
        n_all += iso.size
    np.savez_compressed(os.path.join(HERE, "f13_knn_within.npz"), **out)
    print(f"isolated share {n_iso / n_all:.4f}, smallest gap {gap:.3g}")


if __name__ == "__main__":
    main()
