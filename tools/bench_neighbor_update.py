#!/usr/bin/env python
"""Times the in-place update of the item neighbour table
(``NearestNeighbors.update_rows``: dcnr_cosine_neighbor_table_update, the one
host wait, dcnr_cosine_neighbor_table_rows) against the full rebuild, in one
process.

    python tools/bench_neighbor_update.py [--rows 1000000] [--dim 64] [--k 11]
                                          [--m 1 32 1024 16384] [--rounds 3]

Workload: bench.py's configs[4] index, a seeded random normal table, its
neighbour table built once.  Per m and round: m rows drawn at random get new
random vectors.  Reported per round:
  update_s   HIP events around the whole ``update_rows`` call on the stream,
             the refresh of the norms and the packed rows and the one wait
             included (the host's wall clock beside it)
  phases     the same change driven through the two native calls with events
             between them: refresh | filter + merge | re-search
  stats      rows changed / affected / merged / searched again
and, per round, the full rebuild (dcnr_cosine_neighbor_table over every row)
on the same table.  After every update the table is compared with nothing:
the tests do that; here the update of round r is the starting point of round
r + 1.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hybrid-hotel-recommendation-system-based-on-friends-recommendations_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def ev():
    return torch.cuda.Event(enable_timing=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--k", type=int, default=11)
    ap.add_argument("--m", type=int, nargs="+", default=[1, 32, 1024, 16384])
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_neighbor_update.py needs the HIP device")
    import dcnr
    dev = torch.device("cuda:0")
    N, d, k = args.rows, args.dim, args.k
    g = torch.Generator(device=dev).manual_seed(7)
    table = torch.randn(N, d, device=dev, generator=g)
    nn_ = dcnr.NearestNeighbors(n_neighbors=k).fit(table)
    nbr = nn_.build_neighbor_table()
    rng = np.random.default_rng(11)
    out = {"workload": f"{N} x {d} random normal table, k = {k}", "rounds": args.rounds,
           "packed_copy": nn_._packed is not None, "rebuild_s": [], "m": {}}

    def rebuild():
        a, b = ev(), ev()
        torch.cuda.synchronize()
        a.record()
        nn_._build_into(nbr)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / 1e3

    rebuild()   # warm-up
    out["rebuild_s"] = [round(rebuild(), 4) for _ in range(args.rounds)]
    for m in args.m:
        res = {"update_s": [], "wall_s": [], "phases_s": [], "stats": []}
        for rnd in range(args.rounds + 1):        # round 0: warm-up
            rows = np.sort(rng.choice(N, m, replace=False))
            vec = torch.randn(m, d, device=dev, generator=g)
            a, b = ev(), ev()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            stats = nn_.update_rows(rows, vec, return_stats=True, rebuild=False)
            b.record()
            b.synchronize()
            wall = time.perf_counter() - t0
            # the same kind of change again, phase by phase
            rows = np.sort(rng.choice(N, m, replace=False))
            vec = torch.randn(m, d, device=dev, generator=g)
            e = [ev() for _ in range(4)]
            torch.cuda.synchronize()
            e[0].record()
            nn_._refresh_rows(rows, vec)
            e[1].record()
            nn_._update_table(rows, nbr, True, events=e[2:])
            torch.cuda.synchronize()
            if rnd:
                res["update_s"].append(round(a.elapsed_time(b) / 1e3, 6))
                res["wall_s"].append(round(wall, 6))
                res["phases_s"].append({"refresh": round(e[0].elapsed_time(e[1]) / 1e3, 6),
                                        "filter_merge": round(e[1].elapsed_time(e[2]) / 1e3, 6),
                                        "research": round(e[2].elapsed_time(e[3]) / 1e3, 6)})
                res["stats"].append(stats)
        res["update_s_median"] = statistics.median(res["update_s"])
        res["rebuild_over_update"] = round(statistics.median(out["rebuild_s"]) / res["update_s_median"], 1)
        res["faster_in_every_round"] = max(res["update_s"]) < min(out["rebuild_s"])
        out["m"][str(m)] = res
    out["rebuild_s_after"] = [round(rebuild(), 4) for _ in range(args.rounds)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
