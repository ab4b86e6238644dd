#!/usr/bin/env python
"""Times the build of the item neighbour table
(``NearestNeighbors.build_neighbor_table``, dcnr_cosine_neighbor_table) and the
scan behind it at other chunk widths.

    python tools/bench_neighbor_table.py [--rows 1000000] [--dim 64] [--k 11]
                                         [--chunks 256 1024 4096] [--rounds 3]

Workload: bench.py's configs[4] index, a seeded random normal table.  The build
walks the table's rows in chunks of queries through the batched top-k, the
query pointer inside the table.  The library ships one chunk width; to choose
it, this tool drives the same walk itself through dcnr_cosine_topk_packed at
each candidate width (the shipped build adds one int64 -> int32 narrowing
launch per chunk) and reports, per width, the seconds for the whole table
(median, best and worst of --rounds; HIP events around the walk, no host wait
inside it) and the bytes of one chunk's scratch: the search's workspace plus the
chunk's int64 indices and distances.  Then the shipped build, the same way, with
its workspace.  Prints one JSON line.
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

import torch  # noqa: E402


def event_seconds(fn, rounds):
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / 1e3)
    return {"s_median": round(statistics.median(out), 4), "s_best": round(min(out), 4),
            "s_worst": round(max(out), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--k", type=int, default=11)
    ap.add_argument("--chunks", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_neighbor_table.py needs the HIP device")
    import dcnr
    from dcnr import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    N, d, k = args.rows, args.dim, args.k
    table = torch.randn(N, d, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    nn_ = dcnr.NearestNeighbors(n_neighbors=k).fit(table)
    t, inv = nn_._table, nn_._inv
    packed = nn_._packed.data_ptr() if nn_._packed is not None else None
    stream = _lib.stream_ptr(dev)
    out = {"workload": f"{N} x {d} random normal table, k = {k}", "rounds": args.rounds,
           "packed_copy": packed is not None, "chunks": {}}
    for C in args.chunks:
        nb = int(lib.dcnr_cosine_topk_workspace_size(N, C, k))
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        idx = torch.empty((C, k), dtype=torch.int64, device=dev)
        dist = torch.empty((C, k), dtype=torch.float32, device=dev)

        def walk():
            for lo in range(0, N, C):
                _lib.check(lib.dcnr_cosine_topk_packed(
                    t.data_ptr(), inv.data_ptr(), packed, N, d, t.data_ptr() + 4 * d * lo,
                    min(C, N - lo), k, idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), nb, stream),
                    "dcnr_cosine_topk")
        walk()   # warm-up
        res = event_seconds(walk, args.rounds)
        res["workspace_bytes"] = nb + idx.numel() * 8 + dist.numel() * 4
        out["chunks"][str(C)] = res
        del ws, idx, dist
    nn_.build_neighbor_table()   # warm-up
    res = event_seconds(nn_.build_neighbor_table, args.rounds)
    res["workspace_bytes"] = int(lib.dcnr_cosine_neighbor_table_workspace_size(N, k))
    res["table_bytes"] = nn_.neighbor_table_.numel() * 4
    out["shipped_build"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
