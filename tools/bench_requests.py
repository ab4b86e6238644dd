#!/usr/bin/env python
"""Times a batch of /recommendations requests served by one
``RankingPipeline.recommend_many`` call against the route a service had before
it: the loop of ``recommend()`` over the same requests, in the same process.

    python tools/bench_requests.py [--batches 1 8 64 256] [--iters 20] [--rounds 5]
    python tools/bench_requests.py --one-batch 64      # for a kernel trace of its own
    python tools/bench_requests.py --neighbor-table    # the pipeline reads the item neighbour table
    python tools/bench_requests.py --large 1 4 --no-loop   # large requests in every batch

Workload: bench.py's configs[4] leg (bench_cfg5) -- a 1M x 64 item table, the
bench model in bf16, 32 random positive hotels per request, lambda 0.7, top 20.
Per batch size R: warm-up, then --rounds medians, each over --iters timed
repetitions of the batched call and max(5, iters / (R / 8)) of the loop (a
repetition of the loop is R requests; both counts are in the output), host
clock around a synchronising repetition and HIP events around the same span,
alternating the two routes.  Reported per route: ms per batch (the median of
the medians, the best and the worst median), requests/s, and which eval
forward each route ran, observed from the library's launch counts by kernel
class (the fused tower starts at 16384 rows where it covers the model; this
model's input is wider than it takes).  The answers of the two routes are
compared; batch sizes at which they differ are listed under "answers_differ"
(none is expected while both take the same forward).  With --neighbor-table the
pipeline is built with ``neighbor_table=True`` (both routes then look their
neighbours up; the build's seconds are reported).  Prints one JSON line.

``--large N`` puts N requests of 400 to 2000 random positives (seeded) into
every batch, in place of its first N: requests above the one-workgroup
kernels' 4096-row capacity, which ``recommend_many`` answers in its large lane
(before it: through ``recommend()``).  Several values of N run one after the
other in one process, 0 being the plain workload; a batch with large requests
is reported under "R+Nlarge".  The large requests take ``--large-lambda``
(default 1.0: a tree without the large lane cannot answer lambda < 1 above 4096
candidates, and the same command must run on both).  ``--no-loop`` leaves the
loop of ``recommend()`` out (it is the same code in both trees).  Results are
kept under profiles/large_requests/.
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

import torch  # noqa: E402

N_ITEMS = 1_000_000


def build(dev, neighbor_table=False):
    import dcnr
    from bench import CFG
    torch.manual_seed(5)
    m = dcnr.DCN_RecSys(1_000_000, N_ITEMS, CFG["cat_dims"], CFG["n_num"],
                        dict(CFG["params"], emb_dim=64), precision="bf16").to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(7)
    item_cat = torch.randint(0, 1000, (N_ITEMS, 12), generator=g, device=dev)
    item_num = torch.rand((N_ITEMS, 8), generator=g, device=dev)
    return dcnr.RankingPipeline(m, item_cat, item_num, neighbor_table=neighbor_table), g


def forward_seen(fn):
    """which eval forward fn() ran, observed: the library's launch counts by kernel class
    around one call (the fused tower is a class of its own)"""
    from dcnr import _lib
    _lib.profile_enable(True)
    _lib.profile_collect()
    fn()
    seen = _lib.profile_collect()
    _lib.profile_enable(False)
    return "fused tower" if seen["tower"][1] else "layer by layer"


def requests(R, g, dev, n_large=0):
    users = torch.randint(0, 1_000_000, (R,), generator=g, device=dev).tolist()
    pos = [torch.randint(0, N_ITEMS, (32,), generator=g, device=dev).tolist() for _ in range(R)]
    if n_large:
        import numpy as np
        rng = np.random.default_rng(1000 * R + n_large)
        for r in range(min(n_large, R)):
            pos[r] = rng.integers(0, N_ITEMS, int(rng.integers(400, 2001))).tolist()
    return users, pos


def timed(fn, iters):
    """median ms of fn() by the host clock and by HIP events, each repetition synchronised"""
    host, evs = [], []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        evs.append(a.elapsed_time(b))
    return statistics.median(host), statistics.median(evs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--one-batch", type=int, default=0,
                    help="warm up, then run one batched call of this size and exit")
    ap.add_argument("--neighbor-table", action="store_true",
                    help="serve the neighbours from the item neighbour table, built at start")
    ap.add_argument("--large", type=int, nargs="+", default=[0],
                    help="requests of 400 to 2000 positives in every batch (several: one after the other)")
    ap.add_argument("--large-lambda", type=float, default=1.0, help="lambda_param of the large requests")
    ap.add_argument("--no-loop", action="store_true", help="time the batched call only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_requests.py needs the HIP device")
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    pipe, g = build(dev, args.neighbor_table)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0

    if args.one_batch:
        n_large = min(args.large[0], args.one_batch)
        users, pos = requests(args.one_batch, g, dev, n_large)
        lam = [args.large_lambda] * n_large + [0.7] * (args.one_batch - n_large)
        for _ in range(args.warmup):
            pipe.recommend_many(users, pos, lambda_param=lam)
        torch.cuda.synchronize()
        pipe.recommend_many(users, pos, lambda_param=lam)
        torch.cuda.synchronize()
        print(json.dumps({"one_batch": args.one_batch, "large": n_large}))
        return

    out = {"workload": "bench_cfg5: 1M x 64 item table, bench model bf16, 32 positives per "
                       "request, lambda 0.7, top 20", "iters": args.iters, "rounds": args.rounds,
           "neighbor_table": args.neighbor_table, "pipeline_build_s": round(build_s, 3),
           "batches": {}}
    out["large_lambda"] = args.large_lambda
    for R, n_large in [(R, n) for R in args.batches for n in args.large]:
        users, pos = requests(R, g, dev, n_large)
        n_large = min(n_large, R)
        lam = [args.large_lambda] * n_large + [0.7] * (R - n_large)

        def many():
            return pipe.recommend_many(users, pos, lambda_param=lam)

        def loop():
            return [pipe.recommend(users[r], pos[r], lambda_param=lam[r]) for r in range(R)]

        routes = {"many": many} if args.no_loop else {"many": many, "loop": loop}
        for _ in range(args.warmup):
            got = {name: fn() for name, fn in routes.items()}
        for (gr, gl), (wr, wl) in zip(got["many"], got.get("loop", got["many"])):
            if not (torch.equal(gr, wr) and torch.equal(gl, wl)):
                out.setdefault("answers_differ", []).append([R, n_large])
                break
        n_cand = sum(pipe.candidates(p).numel() for p in pos)
        rows = {name: [] for name in routes}
        loop_iters = max(5, args.iters // max(1, R // 8))   # a repetition is R requests
        for _ in range(args.rounds):
            for name, fn in routes.items():
                rows[name].append(timed(fn, args.iters if name == "many" else loop_iters))
        res = {"candidates": n_cand, "large": n_large,
               "positives_of_large": [len(p) for p in pos[:n_large]],
               "answered": {"large_lane": len(getattr(got["many"], "large", ())),
                            "host": len(getattr(got["many"], "on_host", ()))},
               "iters_many": args.iters, "iters_loop": loop_iters}
        for name, fn in routes.items():
            res["forward_" + name] = forward_seen(fn)
        for name, v in rows.items():
            host = [h for h, _ in v]
            res[name] = {"ms_per_batch": round(statistics.median(host), 4),
                         "ms_best_median": round(min(host), 4),
                         "ms_worst_median": round(max(host), 4),
                         "event_ms_per_batch": round(statistics.median(e for _, e in v), 4),
                         "requests_per_s": round(R / statistics.median(host) * 1e3, 1)}
        if "loop" in routes:
            res["speedup"] = round(res["loop"]["ms_per_batch"] / res["many"]["ms_per_batch"], 2)
            res["many_worst_at_or_below_loop_worst"] = (res["many"]["ms_worst_median"]
                                                        <= res["loop"]["ms_worst_median"])
        out["batches"][str(R) if not n_large else f"{R}+{n_large}large"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
