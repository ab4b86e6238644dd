#!/usr/bin/env python
"""Times dcnr_eval_group_metrics (per-group GAUC, NDCG@k, hit rate, recall,
MRR) against dcnr_eval_metrics on the same n and against the same metrics
written with torch ops on the device, in one process.

    python tools/bench_grouped_metrics.py [--sizes 1048576 4194304] [--iters 30]
                                          [--torch-iters 20] [--out FILE.json]

Per size, three group layouts:
  zipf   ids drawn with probability ~ 1 / rank over 2^17 users (a few users
         with thousands of rows, most with a handful), n_groups = 2^17
  one    every row in one group, n_groups = 1 (3 sort passes, one list of n)
  own    every row its own group, n_groups = n (every lane finishes a group)
Per layout, after a warm-up, the median (and min / max) of --iters calls timed
with device events, inputs resident and workspace preallocated:
  group_call_ms      dcnr_eval_group_metrics, summary only (per_group = NULL)
  group_records_ms   the same with the n_groups records written
  eval_metrics_ms    dcnr_eval_metrics on the same logits and labels
  torch_ms           torch_group_metrics below: two stable torch.sort calls
                     and cumsum / index_add_ / scatter_reduce on the device
Before anything is timed the torch version is checked against the new call:
every count equal, every mean within 1e-9.  Prints one JSON line (and writes
it to --out).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hybrid-hotel-recommendation-system-based-on-friends-recommendations_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import numpy as np  # noqa: E402
import torch  # noqa: E402

KS = (5, 10, 20)
N_USERS = 1 << 17


def torch_group_metrics(z, y, g, ks, discount, ideal):
    """The summary of dcnr_eval_group_metrics with torch ops on the device
    (fp64 sums by index_add_: their order is not fixed)."""
    n = z.shape[0]
    dev = z.device
    zc = z + 0.0                                           # -0.0 ties with +0.0
    o1 = torch.sort(zc, descending=True, stable=True).indices
    order = o1[torch.sort(g[o1], stable=True).indices]     # stable by group: (group, -score, position)
    gs, zs, pos = g[order], zc[order], y[order] == 1.0
    idx = torch.arange(n, device=dev)
    one = torch.ones(1, dtype=torch.bool, device=dev)
    ghead = torch.cat([one, gs[1:] != gs[:-1]])
    thead = ghead | torch.cat([one, zs[1:] != zs[:-1]])
    hpos = torch.nonzero(ghead).reshape(-1)
    m = hpos.shape[0]
    gi = torch.cumsum(ghead, 0) - 1
    G = hpos[gi]
    T = torch.cummax(torch.where(thead, idx, torch.zeros_like(idx)), 0).values
    rank = idx - G + 1
    posl = pos.long()
    PB = torch.cumsum(posl, 0) - posl
    c = torch.where(pos, (idx - T) - (PB - PB[T]), (PB - PB[G]) + (PB[T] - PB[G]))
    zl = lambda: torch.zeros(m, dtype=torch.int64, device=dev)   # noqa: E731
    n_u = zl().index_add_(0, gi, torch.ones_like(posl))
    P = zl().index_add_(0, gi, posl)
    N = n_u - P
    u2 = zl().index_add_(0, gi, c)
    big = 1 << 40
    fpr = torch.full((m,), big, dtype=torch.int64, device=dev).scatter_reduce_(
        0, gi, torch.where(pos, rank, torch.full_like(rank, big)), "amin")
    aucg, rk = (P > 0) & (N > 0), P > 0
    auc_u = u2[aucg].double() / (2.0 * P[aucg].double() * N[aucg].double())
    out = {"n_groups_present": m, "n_groups_auc": int(aucg.sum()), "n_groups_ranked": int(rk.sum()),
           "n_rows_auc": int(n_u[aucg].sum()),
           "gauc": float((n_u[aucg].double() * auc_u).sum() / n_u[aucg].sum()),
           "auc_macro": float(auc_u.mean()), "mrr": float((1.0 / fpr[rk].double()).mean()),
           "hit_groups": [], "hit_rate": [], "recall": [], "ndcg": []}
    Pr = P[rk]
    for k in ks:
        inb = pos & (rank <= k)
        hits = zl().index_add_(0, gi, inb.long())[rk]
        w = torch.where(inb, discount[torch.clamp(rank, max=ks[-1]) - 1], torch.zeros((), dtype=torch.float64,
                                                                                      device=dev))
        dcg = torch.zeros(m, dtype=torch.float64, device=dev).index_add_(0, gi, w)[rk]
        out["hit_groups"].append(int((hits > 0).sum()))
        out["hit_rate"].append(float((hits > 0).double().mean()))
        out["recall"].append(float((hits.double() / Pr.double()).mean()))
        out["ndcg"].append(float((dcg / ideal[torch.clamp(Pr, max=k) - 1]).mean()))
    return out


def zipf_ids(rng, n):
    p = 1.0 / np.arange(1, N_USERS + 1, dtype=np.float64)
    ids = rng.choice(N_USERS, size=n, p=p / p.sum())
    return rng.permutation(N_USERS)[ids].astype(np.int64)      # heavy users at arbitrary ids


def same(a, b):
    """Within 1e-9; a mean over no group is NaN on both sides (every row its
    own group: no group has both classes)."""
    return (a != a and b != b) or abs(a - b) <= 1e-9


def timed(fn, iters):
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "runs": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 20, 1 << 22])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--torch-iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_grouped_metrics.py needs the HIP device")
    from dcnr import _lib, metrics
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = _lib.stream_ptr(dev)
    disc, ideal = (torch.from_numpy(a).to(dev) for a in metrics.dcg_tables(KS[-1]))
    ks_arr = (ctypes.c_int32 * len(KS))(*KS)
    out = {"device": torch.cuda.get_device_name(0), "ks": list(KS), "timing": "device events, median",
           "sizes": {}}
    for n in args.sizes:
        rng = np.random.default_rng(n)
        z = torch.from_numpy((rng.standard_normal(n) * 2.0).astype(np.float32)).to(dev)
        y = torch.from_numpy((rng.random(n) < 0.4).astype(np.float32)).to(dev)
        res_m = torch.empty(72, dtype=torch.uint8, device=dev)
        ws_m = torch.empty(metrics.workspace_bytes(n), dtype=torch.uint8, device=dev)

        def eval_call():
            _lib.check(lib.dcnr_eval_metrics(z.data_ptr(), y.data_ptr(), n, res_m.data_ptr(), ws_m.data_ptr(),
                                             ws_m.numel(), stream), "dcnr_eval_metrics")

        for _ in range(args.warmup):
            eval_call()
        per_n = {"eval_metrics_ms": timed(eval_call, args.iters), "layouts": {}}
        layouts = {"zipf": (zipf_ids(rng, n), N_USERS), "one": (np.zeros(n, np.int64), 1),
                   "own": (rng.permutation(n).astype(np.int64), n)}
        for name, (g_h, ng) in layouts.items():
            g = torch.from_numpy(g_h).to(dev)
            ws = torch.empty(metrics.group_workspace_bytes(n, ng), dtype=torch.uint8, device=dev)
            res = torch.empty(216, dtype=torch.uint8, device=dev)
            rec = torch.empty((ng, 12), dtype=torch.int64, device=dev)

            def group_call(records=False):
                _lib.check(lib.dcnr_eval_group_metrics(
                    z.data_ptr(), y.data_ptr(), g.data_ptr(), n, ng, ks_arr, len(KS), disc.data_ptr(),
                    ideal.data_ptr(), res.data_ptr(), rec.data_ptr() if records else None, ws.data_ptr(),
                    ws.numel(), stream), "dcnr_eval_group_metrics")

            # the torch version against the new call, before anything is timed
            m = metrics.group_metrics(z, y, g, ks=KS, n_groups=ng)
            t = torch_group_metrics(z, y, g, KS, disc, ideal)
            for f in ("n_groups_present", "n_groups_auc", "n_groups_ranked", "n_rows_auc"):
                assert getattr(m, f) == t[f], (name, f, getattr(m, f), t[f])
            assert list(m.hit_groups) == t["hit_groups"], (name, m.hit_groups, t["hit_groups"])
            for f in ("gauc", "auc_macro", "mrr"):
                assert same(getattr(m, f), t[f]), (name, f, getattr(m, f), t[f])
            for f in ("hit_rate", "recall", "ndcg"):
                assert all(same(a, b) for a, b in zip(getattr(m, f), t[f])), (name, f)
            for _ in range(args.warmup):
                group_call()
                group_call(True)
                torch_group_metrics(z, y, g, KS, disc, ideal)
            torch.cuda.synchronize()
            lay = {"n_groups": ng, "sort_passes": (32 + (ng - 1).bit_length() + 10) // 11,
                   "largest_group": int(np.bincount(g_h).max()) if ng < n else 1,
                   "group_call_ms": timed(group_call, args.iters),
                   "group_records_ms": timed(lambda: group_call(True), args.iters),
                   "torch_ms": timed(lambda: torch_group_metrics(z, y, g, KS, disc, ideal), args.torch_iters),
                   "gauc": None if m.gauc != m.gauc else m.gauc, "mrr": m.mrr, "ndcg": list(m.ndcg), "checked_against_torch": True}
            lay["group_over_eval_metrics"] = round(lay["group_call_ms"]["median_ms"] /
                                                   per_n["eval_metrics_ms"]["median_ms"], 2)
            lay["torch_over_group"] = round(lay["torch_ms"]["median_ms"] / lay["group_call_ms"]["median_ms"], 1)
            per_n["layouts"][name] = lay
            del g, ws, rec
        out["sizes"][str(n)] = per_n
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
