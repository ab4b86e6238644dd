"""Writes tests/golden/f12_grouped_metrics.npz: for every case of
tests/grouped_metrics_cases.py what scikit-learn gives group by group,

    auc_<i>    sklearn.metrics.roc_auc_score(y_u, z_u) of the case's AUC groups
    ndcg_<i>   sklearn.metrics.ndcg_score([y_u], [z_u], k=k) for each cutoff of
               KS, [groups, len(KS)]: ``distinct`` cases only (sklearn averages
               over ties, the metric follows the served order) and ranked
               groups of at least 2 rows (sklearn refuses a single document)

for the groups ``grouped_metrics_cases.sampled`` picks: all of a case's
groups up to 128, 128 evenly spaced ones beyond, which keeps the file small.
Results only; the inputs are regenerated from the cases' seeds.  Runs on the
CPU:

    python tests/golden/make_grouped_metrics_golden.py

sklearn refuses infinite scores, so they are replaced by +-FLT_MAX as in
make_metrics_golden.py (order-preserving; AUC depends on the order alone).
"""
import os
import sys

import numpy as np
from sklearn.metrics import ndcg_score, roc_auc_score

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import grouped_metrics_cases as gm  # noqa: E402


def main():
    out = {"names": np.array([gm.case_id(c) for c in gm.CASES])}
    fmax = float(np.finfo(np.float32).max)
    for i, case in enumerate(gm.CASES):
        z, y, g, ng, _, ref = gm.case_with_reference(case)
        zf = z.astype(np.float64)
        if np.isinf(z).any():
            assert not np.any(np.abs(z[np.isfinite(z)]) == fmax)
            zf = np.clip(zf, -fmax, fmax)
        order = np.argsort(g, kind="stable")
        start = np.searchsorted(g[order], ref["gids"])
        rows = lambda o: order[start[o]:start[o] + ref["n_u"][o]]   # noqa: E731
        out[f"auc_{i}"] = np.array([roc_auc_score(y[rows(o)], zf[rows(o)])
                                    for o in gm.sampled(ref["auc_groups"])], np.float64)
        if case[1] == "distinct":
            pick = gm.sampled(ref["ranked_groups"] & (ref["n_u"] >= 2))
            out[f"ndcg_{i}"] = np.array([[ndcg_score(y[rows(o)][None], zf[rows(o)][None], k=k)
                                          for k in gm.KS] for o in pick], np.float64).reshape(-1, len(gm.KS))
    path = os.path.join(HERE, "f12_grouped_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(gm.CASES)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
