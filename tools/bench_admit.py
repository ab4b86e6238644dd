#!/usr/bin/env python
"""Times the two device routes of admission against what they replace, in one
process on one device.

    python tools/bench_admit.py [--ids 16777216] [--known 1048576] [--new 1048576]
                                [--rows 1048576] [--dim 64] [--k 11] [--append 1,1024,16384]
                                [--rounds 5] [--host-rounds 3] [--skip insert|append]

Insert.  ``IdMap.insert`` of --ids raw ids into a map that holds --known: --new
of them distinct new ids, each first seen somewhere in the batch, the rest known
ids, shuffled.  Two timings of the device route: the call as a user makes it
(the table is first rebuilt at capacity >= 2 (n + M)), and the native call alone
on a table already sized for the ids it will hold (``capacity=``).  Against
``insert_host`` on the same batch; the three results are compared before any
timing.  Reported with the insert's bytes: ``bytes_needed`` = what the
contract needs (raw in, out, one 16-byte slot per query, new_ids and the new
slots) and ``bytes_moved`` = what the passes read and write, counted from the
shapes (find 32 M; claim, mark, scan, head and rest 48 M more; 80 bytes per row
with an unknown id for its slot traffic), over the native call's time, beside
the rate of a device copy of the same size measured here.

Append.  ``NearestNeighbors.append_rows`` of m new rows (--append) onto a
fitted --rows x --dim table with its k-column neighbour table, ``vectors=`` and
``storage=`` forms, against ``fit`` + ``build_neighbor_table`` on the grown
table -- the only route there was.  Each result is compared with the rebuild's
before timing.  The host clock runs around calls that end in a stream
synchronise.  Per figure: the median, the best and the worst of --rounds runs,
the two routes alternating.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hybrid-hotel-recommendation-system-based-on-friends-recommendations_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def spread(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_best": round(min(ms), 4),
            "ms_worst": round(max(ms), 4), "runs": len(ms)}


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def pow2_at_least(n):
    c = 1
    while c < n:
        c <<= 1
    return c


def bench_insert(dev, args):
    import dcnr
    rng = np.random.default_rng(1)
    n, M, n_new = args.known, args.ids, args.new
    every = rng.permutation(2 * (n + n_new)).astype(np.int64)[:n + n_new] * ((1 << 32) + 1) - (1 << 40)
    ids, fresh = every[:n], every[n:]
    raw = np.concatenate([fresh, ids[rng.integers(0, n, M - n_new)]])
    rng.shuffle(raw)
    d_ids, d_raw = torch.from_numpy(ids).to(dev), torch.from_numpy(raw).to(dev)
    tight = pow2_at_least(2 * (n + n_new))

    def device_map(capacity=None):
        return dcnr.IdMap(d_ids, device=dev, capacity=capacity)

    host = dcnr.IdMap(ids, device="cpu")
    t0 = time.perf_counter()
    want_out, want_new = host.insert_host(raw)
    host_ms = [1e3 * (time.perf_counter() - t0)]
    assert want_new.size == n_new
    for cap in (None, tight):
        m = device_map(cap)
        out, new = m.insert(d_raw, capacity=cap)
        assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(new.cpu().numpy(), want_new)
        assert torch.equal(m.lookup(m.ids), torch.arange(len(m), device=dev))
        del m, out, new
    for _ in range(args.host_rounds - 1):
        host = dcnr.IdMap(ids, device="cpu")
        t0 = time.perf_counter()
        host.insert_host(raw)
        host_ms.append(1e3 * (time.perf_counter() - t0))
    call_ms, native_ms, copy_ms = [], [], []
    unknown_rows = int((want_out >= n).sum())
    needed = 32 * M + 24 * n_new
    moved = 80 * M + 80 * unknown_rows
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    for r in range(args.rounds + 1):                # round 0 warms up
        m = device_map()
        ms_call, _ = clock(lambda: m.insert(d_raw))
        m = device_map(tight)
        ms_native, _ = clock(lambda: m.insert(d_raw, capacity=tight))
        ms_copy, _ = clock(lambda: dst.copy_(src))
        if r:
            call_ms.append(ms_call)
            native_ms.append(ms_native)
            copy_ms.append(ms_copy)
        del m
    res = {"ids": M, "known": n, "new": n_new, "rows_with_an_unknown_id": unknown_rows,
           "capacity_call": pow2_at_least(2 * (n + M)), "capacity_native": tight, "results_equal": True,
           "insert_call": spread(call_ms), "insert_native": spread(native_ms), "insert_host": spread(host_ms),
           "copy_same_bytes": spread(copy_ms), "bytes_needed": needed, "bytes_moved": moved}
    t = res["insert_native"]["ms_median"]
    res["speedup_call_vs_host"] = round(res["insert_host"]["ms_median"] / res["insert_call"]["ms_median"], 2)
    res["speedup_native_vs_host"] = round(res["insert_host"]["ms_median"] / t, 2)
    res["moved_gb_per_s"] = round(moved / (1e6 * t), 1)
    res["needed_gb_per_s"] = round(needed / (1e6 * t), 1)
    res["copy_gb_per_s"] = round(moved / (1e6 * res["copy_same_bytes"]["ms_median"]), 1)
    res["fraction_of_copy"] = round(res["copy_same_bytes"]["ms_median"] / t, 3)
    return res


def bench_append(dev, args):
    import dcnr
    from dcnr.knn import rebuild_is_cheaper
    N, d, k = args.rows, args.dim, args.k
    sizes = [int(s) for s in args.append.split(",") if s]
    g = torch.Generator(device=dev).manual_seed(2)
    base = torch.randn(N + max(sizes), d, device=dev, generator=g)
    nn_ = dcnr.NearestNeighbors(n_neighbors=k).fit(base[:N].clone())
    nn_.build_neighbor_table()
    torch.cuda.synchronize()
    state = (nn_._table, nn_._inv, nn_._packed, nn_.neighbor_table_)

    def restore():
        nn_._table, nn_._inv, nn_._packed, nn_.neighbor_table_ = state
        nn_.n_samples_fit_ = N

    def rebuild(grown):
        fresh = dcnr.NearestNeighbors(n_neighbors=k).fit(grown)
        fresh.build_neighbor_table()
        return fresh

    res = {"rows": N, "dim": d, "k": k, "results_equal": True, "append": {}}
    for m in sizes:
        grown = base[:N + m].clone()
        new = grown[N:].clone()
        one = {"rebuild_is_cheaper": bool(rebuild_is_cheaper(m, k, N + m))}
        want = rebuild(grown)
        for form in ("vectors", "storage"):
            restore()
            _, stats = nn_.append_rows(return_stats=True, **({"vectors": new} if form == "vectors" else
                                                             {"storage": grown}))
            assert torch.equal(nn_.neighbor_table_, want.neighbor_table_), (m, form)
            assert torch.equal(nn_._inv, want._inv), (m, form)
            assert want._packed is None or torch.equal(nn_._packed, want._packed), (m, form)
            one["stats"] = {k_: (bool(v) if isinstance(v, bool) else int(v)) for k_, v in stats.items()}
        del want
        ms = {"vectors": [], "storage": [], "rebuild": []}
        for r in range(args.rounds + 1):            # round 0 warms up; the routes alternate
            for form in ("vectors", "storage"):
                restore()
                t, _ = clock(lambda: nn_.append_rows(**({"vectors": new} if form == "vectors" else
                                                        {"storage": grown})))
                if r:
                    ms[form].append(t)
            t, _ = clock(lambda: rebuild(grown))
            if r:
                ms["rebuild"].append(t)
        one.update({f"append_{f}": spread(ms[f]) for f in ("vectors", "storage")})
        one["fit_and_build"] = spread(ms["rebuild"])
        one["speedup_storage"] = round(one["fit_and_build"]["ms_median"] / one["append_storage"]["ms_median"], 2)
        one["speedup_vectors"] = round(one["fit_and_build"]["ms_median"] / one["append_vectors"]["ms_median"], 2)
        res["append"][str(m)] = one
        restore()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, default=1 << 24)
    ap.add_argument("--known", type=int, default=1 << 20)
    ap.add_argument("--new", type=int, default=1 << 20)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--k", type=int, default=11)
    ap.add_argument("--append", default="1,1024,16384")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--skip", choices=["insert", "append"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_admit.py needs the HIP device")
    dev = torch.device("cuda:0")
    res = {}
    if args.skip != "insert":
        res["insert"] = bench_insert(dev, args)
    if args.skip != "append":
        res["append"] = bench_append(dev, args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
