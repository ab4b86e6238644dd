#!/usr/bin/env python
"""Times InteractionStore.append against the route a store without it has.

    python tools/bench_store_append.py [--log2-reviews 20 24 26] [--batches 1 1000 100000]
                                       [--rounds 5] [--out profiles/store_append/NAME.json]

Stores: f11_common.random_tables-like data (seeded; repeated (reviewer, hotel)
pairs, self / repeated / reversed friend pairs, NaN ratings) with M reviews,
U = M / 16 reviewers, E = M / 8 friendship rows, 4096 hotels, uploaded to the
device before anything is timed.  Batches: b reviews and b / 10 friendships
(at least one) of the same distribution.

Per point, in one process on one device, median / best / worst of --rounds
after a warm-up, every round from the same store state:
  (a) append   wall clock of store.append(batch) with a device synchronize
               inside the timed region, split into the host part and the device
               part (upload, the two dcnr_csr_insert calls, the wait), and the
               bytes uploaded; in rounds of their own, the library's HIP-event
               time of the dcnr_csr_insert launches, and from it the achieved
               bytes/s against the bytes the pass must move (old + new payloads
               and offsets, read once and written once);
  (b) rebuild  wall clock of InteractionStore(concatenated tables) + .on(dev)
               + a device synchronize: the yardstick.
Prints one JSON line (and writes it to --out).
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hybrid-hotel-recommendation-system-based-on-friends-recommendations_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_ITEMS = 4096


def tables(rng, U, M, E):
    rev = rng.integers(0, U - U // 10, M)
    item = rng.integers(0, N_ITEMS, M)
    rating = rng.integers(1, 11, M).astype(np.float64)
    if M >= 8:
        rep = rng.choice(M, M // 8, replace=False)
        src = rng.integers(0, M, rep.size)
        rev[rep], item[rep] = rev[src], item[src]
        rating[rng.choice(M, max(1, M // 20), replace=False)] = np.nan
    fa = rng.integers(U // 20, U, E)
    fb = rng.integers(U // 20, U, E)
    n = E // 10
    fb[:E // 30] = fa[:E // 30]
    fa[E - n:], fb[E - n:] = fb[:n].copy(), fa[:n].copy()
    return rev, item, rating, fa, fb


def stats(xs, unit=1e3, nd=3):
    return {"median": round(statistics.median(xs) * unit, nd), "best": round(min(xs) * unit, nd),
            "worst": round(max(xs) * unit, nd)}


def fork(store):
    """The same store state again: append replaces arrays and device tensors,
    it writes into none, so a shallow copy shares them safely."""
    s = copy.copy(store)
    s._dev, s._prev, s._dev_lock = dict(store._dev), {}, threading.Lock()
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-reviews", type=int, nargs="+", default=[20, 24, 26])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1000, 100000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_store_append.py needs the HIP device")
    import dcnr
    from dcnr import _lib
    dev = torch.device("cuda:0")
    out = {"workload": "random tables, U = M / 16, E = M / 8, 4096 hotels; batch of b reviews and "
                       "max(1, b / 10) friendships", "device": torch.cuda.get_device_name(0),
           "processes": 1, "rounds": args.rounds, "ms": "median / best / worst", "points": []}
    for lg in args.log2_reviews:
        M = 1 << lg
        U, E = M // 16, M // 8
        rng = np.random.default_rng(lg)
        base = tables(rng, U, M, E)
        t0 = time.perf_counter()
        store = dcnr.InteractionStore(*base, n_items=N_ITEMS, n_reviewers=U)
        store.on(dev)
        torch.cuda.synchronize()
        first_build_s = time.perf_counter() - t0
        for b in args.batches:
            batch = tables(rng, U, b, max(1, b // 10))
            whole = tuple(np.concatenate([x, y]) for x, y in zip(base, batch))

            def one_append(profile):
                s = fork(store)
                torch.cuda.synchronize()
                if profile:
                    _lib.profile_collect()
                t = time.perf_counter()
                s.append(*batch)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t
                return wall, s

            def rebuild():
                torch.cuda.synchronize()
                t = time.perf_counter()
                s = dcnr.InteractionStore(*whole, n_items=N_ITEMS, n_reviewers=U)
                s.on(dev)
                torch.cuda.synchronize()
                return time.perf_counter() - t

            one_append(False)   # warm-up
            wall, host, device = [], [], []
            for _ in range(args.rounds):
                w, s = one_append(False)
                wall.append(w)
                host.append(s.last_append["host_s"])
                device.append(s.last_append["device_s"])
            upload = s.last_append["upload_bytes"]
            # what the two passes must move: payloads and offsets, read once, written once
            moved = 0
            for name, n_pay in (("review_rows", 2), ("friend_rows", 1)):
                old_n = store.on(dev)[1][name].numel()
                new_n = s.on(dev)[1][name].numel()
                if new_n != old_n:
                    moved += 4 * n_pay * (old_n + new_n) + 8 * 2 * (U + 1)
            _lib.profile_enable(True)
            kern = []
            for _ in range(args.rounds):
                one_append(True)
                ms, launches = _lib.profile_collect()["serve"]
                kern.append(ms * 1e-3)
            _lib.profile_enable(False)
            rebuild()           # warm-up
            reb = [rebuild() for _ in range(args.rounds)]
            k_med = statistics.median(kern)
            out["points"].append({
                "log2_reviews": lg, "reviews": M, "reviewers": U, "friend_rows": int(store.friend_rows.size),
                "batch_reviews": b, "batch_friendships": max(1, b // 10),
                "append_wall_ms": stats(wall), "append_host_ms": stats(host),
                "append_device_part_ms": stats(device), "append_upload_bytes": int(upload),
                "insert_kernels_ms": stats(kern), "insert_launches": int(launches),
                "insert_bytes_moved": int(moved),
                "insert_gb_per_s": round(moved / k_med / 1e9, 1) if k_med > 0 else None,
                "rebuild_wall_ms": stats(reb),
                "rebuild_over_append": round(statistics.median(reb) / statistics.median(wall), 2)})
            print(json.dumps(out["points"][-1]), file=sys.stderr, flush=True)
        out.setdefault("first_build_s", {})[str(lg)] = round(first_build_s, 2)
        del store
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
