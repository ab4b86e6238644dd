"""Writes tests/golden/f10_metrics.npz: for every case of tests/metrics_cases.py
the values the reference's own calls give (train.py:255-265, 366-387):

    sk_auc      sklearn.metrics.roc_auc_score(y, z)
    rmse_torch  sqrt(sklearn.metrics.mean_squared_error(y, torch.sigmoid(z)))   (fp32 sigmoid)
    bce_torch   nn.BCEWithLogitsLoss()(z, y) on fp64 inputs

and the exact 2U, P, N.  Expected outputs only; the inputs are regenerated
from the cases' seeds.  Runs on the CPU:

    python tests/golden/make_metrics_golden.py

sklearn refuses infinite scores, so roc_auc_score gets them with +-inf
replaced by +-FLT_MAX, which no case holds as a finite score (asserted): an
order-preserving map, and AUC depends on the order alone.
"""
import os
import sys

import numpy as np
import torch
from sklearn.metrics import mean_squared_error, roc_auc_score

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import metrics_cases as mc  # noqa: E402


def main():
    names, sk_auc, rmse_t, bce_t, u2, npos, nneg = [], [], [], [], [], [], []
    fmax = np.finfo(np.float32).max
    for case in mc.CASES:
        z, y = mc.make_case(case)
        zf = z.astype(np.float64)
        if np.isinf(z).any():
            assert not np.any(np.abs(z[np.isfinite(z)]) == fmax)
            zf = np.clip(zf, -float(fmax), float(fmax))
        names.append(mc.case_id(case))
        sk_auc.append(roc_auc_score(y, zf))
        p32 = torch.sigmoid(torch.from_numpy(z.copy())).numpy()
        rmse_t.append(float(np.sqrt(mean_squared_error(y, p32))))
        bce_t.append(torch.nn.BCEWithLogitsLoss()(torch.from_numpy(z.copy()).double(),
                                                  torch.from_numpy(y.copy()).double()).item())
        a, b, c = mc.exact_u2(z, y)
        u2.append(a), npos.append(b), nneg.append(c)
    out = os.path.join(HERE, "f10_metrics.npz")
    np.savez_compressed(out, names=np.array(names), sk_auc=np.array(sk_auc, np.float64),
                        rmse_torch=np.array(rmse_t, np.float64), bce_torch=np.array(bce_t, np.float64),
                        u2=np.array(u2, np.int64), n_pos=np.array(npos, np.int64),
                        n_neg=np.array(nneg, np.int64))
    print(f"wrote {out}: {len(names)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
