#!/usr/bin/env python
"""Times InteractionStore.remove against the route a store without it has.

    python tools/bench_store_remove.py [--log2-reviews 20 24 26] [--batches 1 1000 100000]
                                       [--rounds 5] [--out profiles/store_remove/NAME.json]

Stores: as tools/bench_store_append.py builds them (M reviews, U = M / 16
reviewers, E = M / 8 friendship rows, 4096 hotels), uploaded to the device
before anything is timed.  Batches: b reviews drawn from all over main_df and
b / 10 friendships (at least one) drawn from the rows of friendships_df.

Per point, in one process on one device, median / best / worst of --rounds
after a warm-up, every round from the same store state:
  (a) remove   wall clock of store.remove(batch) with a device synchronize
               inside the timed region, split into the host part and the device
               part (upload, the two dcnr_csr_remove calls, the wait), and the
               bytes uploaded; in rounds of their own, the library's HIP-event
               time of the dcnr_csr_remove launches, and from it the achieved
               bytes/s against the bytes the pass must move (old + new payloads
               and offsets, read once and written once, and the positions);
  (b) rebuild  wall clock of InteractionStore(tables without those rows) +
               .on(dev) + a device synchronize: the yardstick.  The tables are
               filtered before the clock starts.
Prints one JSON line (and writes it to --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_store_append import N_ITEMS, fork, stats, tables  # noqa: E402  (sets the package path)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-reviews", type=int, nargs="+", default=[20, 24, 26])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1000, 100000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_store_remove.py needs the HIP device")
    import dcnr
    from dcnr import _lib
    dev = torch.device("cuda:0")
    out = {"workload": "random tables, U = M / 16, E = M / 8, 4096 hotels; batch of b reviews and "
                       "max(1, b / 10) friendships of the tables", "device": torch.cuda.get_device_name(0),
           "processes": 1, "rounds": args.rounds, "ms": "median / best / worst", "points": []}
    for lg in args.log2_reviews:
        M = 1 << lg
        U, E = M // 16, M // 8
        rng = np.random.default_rng(lg)
        rev, item, rating, fa, fb = tables(rng, U, M, E)
        store = dcnr.InteractionStore(rev, item, rating, fa, fb, n_items=N_ITEMS, n_reviewers=U)
        store.on(dev)
        torch.cuda.synchronize()
        pair_key = np.minimum(fa, fb) * U + np.maximum(fa, fb)
        for b in args.batches:
            rows = np.sort(rng.choice(M, b, replace=False))
            e = rng.choice(E, max(1, b // 10), replace=False)
            batch = (rev[rows], rows, fa[e], fb[e])
            keep_r = np.ones(M, bool)
            keep_r[rows] = False
            keep_f = ~np.isin(pair_key, pair_key[e])
            rest = (rev[keep_r], item[keep_r], rating[keep_r], fa[keep_f], fb[keep_f])

            def one_remove(profile):
                s = fork(store)
                torch.cuda.synchronize()
                if profile:
                    _lib.profile_collect()
                t = time.perf_counter()
                s.remove(*batch)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t
                return wall, s

            def rebuild():
                torch.cuda.synchronize()
                t = time.perf_counter()
                s = dcnr.InteractionStore(*rest, n_items=N_ITEMS, n_reviewers=U)
                s.on(dev)
                torch.cuda.synchronize()
                return time.perf_counter() - t, s

            one_remove(False)   # warm-up
            wall, host, device = [], [], []
            for _ in range(args.rounds):
                w, s = one_remove(False)
                wall.append(w)
                host.append(s.last_remove["host_s"])
                device.append(s.last_remove["device_s"])
            upload = s.last_remove["upload_bytes"]
            # what the two passes must move: payloads and offsets, read once, written once
            moved = upload
            for name, n_pay in (("review_rows", 2), ("friend_rows", 1)):
                old_n = store.on(dev)[1][name].numel()
                new_n = s.on(dev)[1][name].numel()
                if new_n != old_n:
                    moved += 4 * n_pay * (old_n + new_n) + 8 * 2 * (U + 1)
            _lib.profile_enable(True)
            kern = []
            for _ in range(args.rounds):
                one_remove(True)
                ms, launches = _lib.profile_collect()["serve"]
                kern.append(ms * 1e-3)
            _lib.profile_enable(False)
            _, r = rebuild()    # warm-up; and the two routes agree
            assert r.n_reviews == s.n_reviews and np.array_equal(r.friend_rows, s.friend_rows)
            assert np.array_equal(r.review_item, s.review_item) and np.array_equal(r.n_pos, s.n_pos)
            del r
            reb = [rebuild()[0] for _ in range(args.rounds)]
            k_med = statistics.median(kern)
            out["points"].append({
                "log2_reviews": lg, "reviews": M, "reviewers": U, "friend_rows": int(store.friend_rows.size),
                "batch_reviews": b, "batch_friendships": int(e.size),
                "removed_friend_rows": int(store.friend_rows.size - s.friend_rows.size),
                "remove_wall_ms": stats(wall), "remove_host_ms": stats(host),
                "remove_device_part_ms": stats(device), "remove_upload_bytes": int(upload),
                "remove_kernels_ms": stats(kern), "remove_launches": int(launches),
                "remove_bytes_moved": int(moved),
                "remove_gb_per_s": round(moved / k_med / 1e9, 1) if k_med > 0 else None,
                "rebuild_wall_ms": stats(reb),
                "rebuild_over_remove": round(statistics.median(reb) / statistics.median(wall), 2)})
            print(json.dumps(out["points"][-1]), file=sys.stderr, flush=True)
        del store
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
