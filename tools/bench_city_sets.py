#!/usr/bin/env python
"""Times the device build of the city / popular sets (dcnr_city_sets_build,
dcnr.CitySets) against the host route over the same columns.

    python tools/bench_city_sets.py [--log2-reviews 20 24 26] [--tables even100 even10000 skew100]
                                    [--batches 1 1000 100000] [--rounds 5]
                                    [--out profiles/city_sets/NAME.json]

Tables: M main_df rows over C cities, 100 000 hotels, every hotel in one city,
user_reviews_count an integer in [0, 5000) (so every city's cut falls inside a
tie group); ``even``: the rows spread evenly over the cities, ``skew``: city 0
holds half of them.  top = 100.

Per point, in one process on one device, median / best / worst of --rounds
after a warm-up:
  (a) build    HIP events around dcnr_city_sets_build over the resident columns
               (buffers allocated beforehand, cap as CitySets guesses it), and
               the GB/s over the bytes the four input columns occupy (20 M);
  (b) host     the route without the device, once: the by-city index and then
               city_rows_host / top_rows_host / popular_rows_host of every
               city, from the same columns; its sets must equal the device's;
  (c) append / remove of b rows: wall clock with a device synchronize inside
               the timed region, split into the host part (the new numpy
               columns) and the device part (upload of the batch, the tail copy
               or compaction, the build, its one readback), every round from
               the same state.
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
sys.path.insert(0, os.path.join(ROOT, "hybrid-hotel-recommendation-system-based-on-friends-recommendations_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_ITEMS, TOP = 100_000, 100
TABLES = {"even100": (100, False), "even10000": (10_000, False), "skew100": (100, True)}


def stats(xs, unit=1e3, nd=3):
    return {"median": round(statistics.median(xs) * unit, nd), "best": round(min(xs) * unit, nd),
            "worst": round(max(xs) * unit, nd)}


def table(rng, M, C, skew):
    city = rng.integers(0, C, M)
    if skew:
        city[rng.random(M) < 0.5] = 0
    item = city + C * rng.integers(0, N_ITEMS // C, M)      # a hotel's city is its row mod C
    return item, city, rng.integers(0, 5000, M).astype(np.float64)


def fork(cs):
    """The same state again: append / remove replace arrays and device tensors,
    they write into none, so a shallow copy shares them safely."""
    s = copy.copy(cs)
    s._dev, s._prev, s._dev_lock = dict(cs._dev), {}, threading.Lock()
    return s


def timed_builds(dev, gen, C, rounds):
    """(seconds per build by HIP events, status) of dcnr_city_sets_build over a
    generation's resident columns."""
    from dcnr import _lib
    lib = _lib.load()
    M = gen.n_reviews
    nb = int(lib.dcnr_city_sets_workspace_size(M, N_ITEMS, C, TOP))
    cap = max(1, min(M, N_ITEMS) + min(M, C * TOP))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    off = torch.empty(2 * C + 2, dtype=torch.int64, device=dev)
    rows = torch.empty(cap, dtype=torch.int64, device=dev)
    top = torch.empty(C * TOP, dtype=torch.int32, device=dev)
    st = torch.empty(1, dtype=torch.int32, device=dev)
    secs = []
    for i in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.dcnr_city_sets_build(
            gen.review_item.data_ptr(), gen.review_city.data_ptr(), gen.review_popularity.data_ptr(),
            gen.review_row.data_ptr(), M, N_ITEMS, C, TOP, off.data_ptr(), rows.data_ptr(), cap,
            top.data_ptr(), st.data_ptr(), None, None, ws.data_ptr(), nb, _lib.stream_ptr(dev)),
            "dcnr_city_sets_build")
        e1.record()
        e1.synchronize()
        if i:   # (the first is the warm-up)
            secs.append(e0.elapsed_time(e1) * 1e-3)
    assert int(st.item()) == 0 and torch.equal(off, gen.set_offsets) and \
        torch.equal(rows[:gen.set_rows.numel()], gen.set_rows)
    return secs, nb


def host_route(cs, gen):
    """Every city's three sets with numpy, timed; and compared with the device's."""
    from dcnr.cities import CityColumns
    c0 = cs._cols
    t = time.perf_counter()
    cols = CityColumns(c0.item, c0.city, c0.key, c0.row, c0.n_items, c0.n_cities, c0.top)   # (no index yet)
    sets = [(cols.city_rows(c), cols.top_rows(c), cols.popular_rows(c)) for c in range(cs.n_cities)]
    sec = time.perf_counter() - t
    C = cs.n_cities
    want_rows = np.concatenate([s[0] for s in sets] + [s[2] for s in sets])
    want_off = np.concatenate([[0], np.cumsum([s[0].size for s in sets] + [s[2].size for s in sets])])
    assert np.array_equal(gen.host_offsets[:2 * C + 1], want_off) and gen.host_offsets[-1] == want_off[-1]
    assert np.array_equal(gen.set_rows.cpu().numpy(), want_rows)
    top = gen.top_rows.cpu().numpy()
    for c in range(0, C, max(1, C // 50)):
        assert np.array_equal(top[c][top[c] >= 0], sets[c][1])
    return sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-reviews", type=int, nargs="+", default=[20, 24, 26])
    ap.add_argument("--tables", nargs="+", default=list(TABLES), choices=list(TABLES))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1000, 100000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_city_sets.py needs the HIP device")
    import dcnr
    dev = torch.device("cuda:0")
    out = {"workload": f"M rows over C cities, {N_ITEMS} hotels, top = {TOP}; even: rows spread evenly, "
                       "skew: city 0 holds half", "device": torch.cuda.get_device_name(0), "processes": 1,
           "rounds": args.rounds, "ms": "median / best / worst", "points": []}
    for lg in args.log2_reviews:
        M = 1 << lg
        for name in args.tables:
            C, skew = TABLES[name]
            rng = np.random.default_rng(lg * 7 + C + skew)
            item, city, key = table(rng, M, C, skew)
            cs = dcnr.CitySets(item, city, key, n_items=N_ITEMS, n_cities=C, top=TOP)
            gen = cs.on(dev)
            torch.cuda.synchronize()
            build, ws_bytes = timed_builds(dev, gen, C, args.rounds)
            host_s = host_route(cs, gen)
            b_med = statistics.median(build)
            point = {"table": name, "log2_reviews": lg, "reviews": M, "cities": C,
                     "largest_city_rows": int(np.bincount(city, minlength=C).max()),
                     "set_rows": int(gen.set_rows.numel()), "workspace_bytes": ws_bytes,
                     "build_ms": stats(build), "input_bytes": 20 * M,
                     "build_gb_per_s": round(20 * M / b_med / 1e9, 2),
                     "host_route_ms": round(host_s * 1e3, 1),
                     "host_over_build": round(host_s / b_med, 1), "updates": []}
            for b in args.batches:
                if b >= M:
                    continue
                new = table(rng, b, C, skew)
                gone = np.sort(rng.choice(M, b, replace=False))
                for op, call in (("append", lambda s: s.append(*new)), ("remove", lambda s: s.remove(gone))):
                    wall, host, device = [], [], []
                    for i in range(args.rounds + 1):
                        s = fork(cs)
                        torch.cuda.synchronize()
                        t = time.perf_counter()
                        call(s)
                        torch.cuda.synchronize()
                        if i:
                            wall.append(time.perf_counter() - t)
                            host.append(s.last_update["host_s"])
                            device.append(s.last_update["device_s"])
                    point["updates"].append({"op": op, "batch": b, "wall_ms": stats(wall),
                                             "host_ms": stats(host), "device_part_ms": stats(device),
                                             "upload_bytes": int(s.last_update["upload_bytes"])})
                    del s
            out["points"].append(point)
            print(json.dumps(point), file=sys.stderr, flush=True)
            del cs, gen
            torch.cuda.empty_cache()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
