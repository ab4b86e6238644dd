#!/usr/bin/env python
"""Times a batch of /recommendations requests given as user ids
(``RankingPipeline.recommend_users``: the reviews and the friend graph on the
device) against the route a caller had before it, in the same process:
``InteractionStore.sources_host`` in numpy for every request, then
``recommend_many``.

    python tools/bench_user_requests.py [--batches 1 8 64 256] [--iters 20] [--rounds 5]
    python tools/bench_user_requests.py --one-batch 64     # for a kernel trace of its own
    python tools/bench_user_requests.py --kernel-stats run_kernel_stats.csv ...
                                                # adds that trace's kernel times to the table
    python tools/bench_user_requests.py --neighbor-table   # neighbours from the item neighbour table

Workload: tools/bench_requests.py's (bench.py's configs[4] leg: a 1M x 64 item
table, the bench model in bf16, lambda 0.7, top 20) with a synthetic store:
20000 reviewers, 8 friends each on average, 20 reviews each of which a fifth
are >= 8 and a fifth <= 4 -- 32 positives per friends-mode request on average,
drawn with a skew towards popular hotels so that friends do agree.  Medians
as tools/bench_requests.py takes them.  Per batch size R, ms per batch of

  users            recommend_users (recommended_by lists included)
  users_no_lists   recommend_users(recommended_by=False): what ``host`` computes
  host             sources_host per request + recommend_many
  host_lists       ``host`` + recommended_by_host per answer (reads the rows back)

and the ratio of padded to distinct positives: the top-k queries the host
bound costs over the distinct rows ``host`` searches.  The answers of the
routes are compared ("answers_differ").  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hybrid-hotel-recommendation-system-based-on-friends-recommendations_amd")
for p in (PKG, ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_requests import N_ITEMS, build, timed  # noqa: E402

N_REVIEWERS, FRIENDS_EACH, REVIEWS_EACH = 20000, 8, 20
KERNELS = ("req_sources_kernel", "req_recommended_by_kernel", "req_by_gather_kernel")


def make_store():
    import dcnr
    rng = np.random.default_rng(11)
    M = N_REVIEWERS * REVIEWS_EACH
    rev = np.repeat(np.arange(N_REVIEWERS), REVIEWS_EACH)
    item = np.minimum((rng.random(M) ** 4 * N_ITEMS).astype(np.int64), N_ITEMS - 1)
    rating = rng.choice([9.0, 2.0, 6.0, 6.0, 6.0], M)
    order = rng.permutation(M)
    E = N_REVIEWERS * FRIENDS_EACH // 2
    fa, fb = rng.integers(0, N_REVIEWERS, E), rng.integers(0, N_REVIEWERS, E)
    return dcnr.InteractionStore(rev[order], item[order], rating[order], fa, fb,
                                 n_items=N_ITEMS, n_reviewers=N_REVIEWERS)


def kernel_times(path):
    """avg microseconds and calls of the new kernels in a rocprofv3 --stats kernel CSV"""
    out = {}
    for row in csv.DictReader(open(path)):
        for k in KERNELS:
            if k in row["Name"]:
                out[k] = {"calls": int(row["Calls"]),
                          "avg_us": round(float(row["AverageNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--one-batch", type=int, default=0,
                    help="warm up, then run one recommend_users call of this size and exit")
    ap.add_argument("--kernel-stats", default=None,
                    help="a rocprofv3 --kernel-trace --stats CSV of a --one-batch run")
    ap.add_argument("--neighbor-table", action="store_true",
                    help="serve the neighbours from the item neighbour table, built at start")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_user_requests.py needs the HIP device")
    dev = torch.device("cuda:0")
    pipe, g = build(dev, args.neighbor_table)
    store = make_store()
    store.on(dev)
    rng = np.random.default_rng(3)

    def requests(R):
        return (torch.randint(0, 1_000_000, (R,), generator=g, device=dev).tolist(),
                rng.integers(0, N_REVIEWERS, R))

    if args.one_batch:
        users, rv = requests(args.one_batch)
        for _ in range(args.warmup + 1):
            pipe.recommend_users(store, users, rv, "friends", lambda_param=0.7)
            torch.cuda.synchronize()
        print(json.dumps({"one_batch": args.one_batch}))
        return

    out = {"workload": "bench_cfg5 (1M x 64 item table, bench model bf16, lambda 0.7, top 20); "
                       f"store: {N_REVIEWERS} reviewers x {REVIEWS_EACH} reviews, "
                       f"{FRIENDS_EACH} friends on average, friends mode",
           "iters": args.iters, "rounds": args.rounds, "neighbor_table": args.neighbor_table,
           "batches": {}}
    if args.kernel_stats:
        out["kernel_us"] = kernel_times(args.kernel_stats)
    for R in args.batches:
        users, rv = requests(R)

        def by_users(lists=True):
            return pipe.recommend_users(store, users, rv, "friends", lambda_param=0.7,
                                        recommended_by=lists)

        def host():
            src = [store.sources_host(int(u), "friends") for u in rv]
            return pipe.recommend_many(users, [s[0] for s in src], lambda_param=0.7,
                                       excluded=[s[1] for s in src])

        def host_lists():
            res = host()
            return res, [store.recommended_by_host(int(u), rows.cpu()) for u, (rows, _) in
                         zip(rv, res)]

        routes = {"users": by_users, "users_no_lists": lambda: by_users(False), "host": host,
                  "host_lists": host_lists}
        for _ in range(args.warmup):
            got, want = by_users(), host_lists()
        for r, ((gr, gl), (wr, wl)) in enumerate(zip(got, want[0])):
            if not (torch.equal(gr, wr) and torch.equal(gl, wl) and
                    got.to_lists(r)[2] == want[1][r]):
                out.setdefault("answers_differ", []).append(R)
                break
        iters = max(5, args.iters // max(1, R // 32))
        rows = {name: [] for name in routes}
        for _ in range(args.rounds):
            for name, fn in routes.items():
                rows[name].append(timed(fn, iters))
        distinct, padded = int(got.n_positives.sum()), int(got.positives_bound.sum())
        res = {"iters": iters, "positives_per_request": round(distinct / R, 1),
               "padded_over_distinct_positives": round(padded / max(1, distinct), 3),
               "answered_on_host": int(got.on_host.sum())}
        for name, v in rows.items():
            ms = [h for h, _ in v]
            res[name] = {"ms_per_batch": round(statistics.median(ms), 4),
                         "ms_best_median": round(min(ms), 4), "ms_worst_median": round(max(ms), 4),
                         "requests_per_s": round(R / statistics.median(ms) * 1e3, 1)}
        res["speedup_users_no_lists_over_host"] = round(
            res["host"]["ms_per_batch"] / res["users_no_lists"]["ms_per_batch"], 2)
        res["speedup_users_over_host_lists"] = round(
            res["host_lists"]["ms_per_batch"] / res["users"]["ms_per_batch"], 2)
        out["batches"][str(R)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
