#!/usr/bin/env python
"""Times the set-scoped neighbour search (dcnr_cosine_topk_within) against the
two routes a pipeline without it has.

    python tools/bench_within.py [--rows 1000000] [--dim 64] [--k 10]
                                 [--requests 1 32 256] [--set-rows 200 2000 20000]
                                 [--rounds 5]

Workload: bench.py's configs[4] index, a seeded random normal table; requests
of 8 positives each (rows of the table), every request naming one of 64
registered sets of equal size (random rows, ascending); each positive asks for
its k nearest rows of the set other than itself, which is what the request
path asks with n_neighbors = k + 1.  One more point searches a single set that
is the whole table (32 requests).

Per point, in one process on one device, HIP events around the calls, no host
wait inside, median / best / worst of --rounds after a warm-up:
  within   the one dcnr_cosine_topk_within call (buffers allocated before);
  global   (a) dcnr_cosine_topk_packed over the whole table for the same
           queries, k + 1 neighbours: the step the call replaces in the request
           path -- another answer, a comparable cost;
  refit    (b) the other route to the same answer: per distinct set, an index
           fitted on table[set] and queried with that set's positives, the fit
           included (host work and allocations are part of that route, so its
           interval is wall time on the stream).
and the within call's workspace bytes.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hybrid-hotel-recommendation-system-based-on-friends-recommendations_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_SETS, POSITIVES = 64, 8


def event_us(fn, rounds):
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return {"us_median": round(statistics.median(out), 1), "us_best": round(min(out), 1),
            "us_worst": round(max(out), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--requests", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--set-rows", type=int, nargs="+", default=[200, 2000, 20000])
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_within.py needs the HIP device")
    import dcnr
    from dcnr import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    N, d, k = args.rows, args.dim, args.k
    table = torch.randn(N, d, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    nn_ = dcnr.NearestNeighbors(n_neighbors=k + 1).fit(table)
    t, inv = nn_._table, nn_._inv
    packed = nn_._packed.data_ptr() if nn_._packed is not None else None
    stream = _lib.stream_ptr(dev)
    rng = np.random.default_rng(7)
    out = {"workload": f"{N} x {d} random normal table, k = {k} within / {k + 1} global, "
                       f"{POSITIVES} positives per request, {N_SETS} sets", "rounds": args.rounds,
           "packed_copy": packed is not None, "points": []}

    def point(R, sets, label):
        S, n = len(sets), len(sets[0])
        Q = R * POSITIVES
        which = rng.integers(0, S, R)
        pos = torch.from_numpy(rng.integers(0, N, Q)).to(dev)
        q = t[pos].contiguous()
        set_rows = torch.from_numpy(np.concatenate(sets)).to(dev)
        set_off = torch.arange(S + 1, dtype=torch.int64, device=dev) * n
        seg_off = torch.arange(R + 1, dtype=torch.int64, device=dev) * POSITIVES
        seg_set = torch.from_numpy(which.astype(np.int32)).to(dev)
        idx = torch.empty((Q, k), dtype=torch.int64, device=dev)
        dist = torch.empty((Q, k), dtype=torch.float32, device=dev)
        nb = int(lib.dcnr_cosine_topk_within_workspace_size(Q, k, d, n))
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)

        def within():
            _lib.check(lib.dcnr_cosine_topk_within(
                t.data_ptr(), inv.data_ptr(), N, d, q.data_ptr(), Q, pos.data_ptr(), seg_off.data_ptr(), R,
                seg_set.data_ptr(), set_rows.data_ptr(), set_rows.numel(), set_off.data_ptr(), S, n, k, k,
                idx.data_ptr(), dist.data_ptr(), None, ws.data_ptr(), nb, stream), "dcnr_cosine_topk_within")
        gnb = int(lib.dcnr_cosine_topk_workspace_size(N, Q, k + 1))
        gws = torch.empty(gnb, dtype=torch.uint8, device=dev)
        gidx = torch.empty((Q, k + 1), dtype=torch.int64, device=dev)
        gdist = torch.empty((Q, k + 1), dtype=torch.float32, device=dev)

        def whole():
            _lib.check(lib.dcnr_cosine_topk_packed(
                t.data_ptr(), inv.data_ptr(), packed, N, d, q.data_ptr(), Q, k + 1, gidx.data_ptr(),
                gdist.data_ptr(), gws.data_ptr(), gnb, stream), "dcnr_cosine_topk")
        d_sets = [set_rows[s * n:(s + 1) * n] for s in range(S)]
        by_set = {int(s): torch.from_numpy(np.flatnonzero(np.repeat(which, POSITIVES) == s)).to(dev)
                  for s in np.unique(which)}

        def refit():
            for s, qs in by_set.items():
                sub = dcnr.NearestNeighbors(n_neighbors=k + 1).fit(t[d_sets[s]])
                sub.kneighbors_device(q[qs], min(k + 1, n))
        res = {"point": label, "requests": R, "queries": Q, "set_rows": n, "distinct_sets": len(by_set),
               "workspace_bytes": nb}
        for name, fn in (("within", within), ("global", whole), ("refit", refit)):
            if name == "refit" and n == N:
                continue   # (the set is the table: the route is the global search)
            fn()   # warm-up
            res[name] = event_us(fn, args.rounds)
        out["points"].append(res)

    for n in args.set_rows:
        sets = [np.sort(rng.choice(N, n, replace=False)).astype(np.int64) for _ in range(N_SETS)]
        for R in args.requests:
            point(R, sets, f"R={R}, sets of {n}")
    point(32, [np.arange(N, dtype=np.int64)], "R=32, one set = the table")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
