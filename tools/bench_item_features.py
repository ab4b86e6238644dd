#!/usr/bin/env python
"""Times the device build of the hotel feature tables (dcnr_item_features_build,
dcnr.ItemFeatures) against the host route over the same columns.

    python tools/bench_item_features.py [--log2-reviews 20 24] [--batches 1 1000 100000]
                                        [--rounds 5] [--out profiles/item_features/NAME.json]

Tables: M main_df rows over 100 000 hotels drawn uniformly (so nearly every
hotel's first row lies in the first few hundred thousand rows), n_cat = 2 codes
and n_num = 11 values per row, a min-max scaler fitted to the values.

Per point, in one process on one device, median / best / worst of --rounds
after a warm-up:
  (a) build    HIP events around --builds back-to-back calls of
               dcnr_item_features_build over the resident columns (buffers
               allocated beforehand), divided by their number: once with the
               review_row column as ``ItemFeatures`` holds it, once with NULL
               (the rows numbered by position).  With it the byte model, the
               time those bytes take at the HBM rate a streaming copy reaches
               (6.3 TB/s) and the fraction of that floor the build reaches:
                 scan     4 M (review_item) + 4 M (review_row, if given)
                 scratch  4 n_items written, 4 n_items read
                 tables   n_items (8 n_cat + 4 n_num + 4) written
                 gather   per hotel with a row: its codes, its values and its
                          review_row word, each rounded up to the 128-byte
                          requests the memory system reads in
  (b) host     the route without the device, once: numpy's first occurrence
               per hotel (np.unique(return_index=True)), the gather and the
               scaler, from the same columns; its tables must equal the
               device's byte for byte;
  (c) append / remove / set_values of b rows: wall clock with a device
               synchronize inside the timed region, split into the host part
               and the device part (upload of the batch, the tail copy,
               compaction or scatter, the build, its one readback), every
               round from the same state.
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

N_ITEMS, N_CAT, N_NUM = 100_000, 2, 11
HBM_BYTES_PER_S = 6.3e12   # what a streaming copy reaches on the MI355X
REQUEST = 128              # bytes per memory request


def stats(xs, unit=1e3, nd=4):
    return {"median": round(statistics.median(xs) * unit, nd), "best": round(min(xs) * unit, nd),
            "worst": round(max(xs) * unit, nd)}


def table(rng, M):
    return (rng.integers(0, N_ITEMS, M), rng.integers(0, 300, (M, N_CAT)),
            rng.random((M, N_NUM)) * 10)


def byte_model(M, n_with_row, with_rows):
    up = lambda b: -(-b // REQUEST) * REQUEST
    parts = {"scan": (8 if with_rows else 4) * M, "scratch": 8 * N_ITEMS,
             "tables": N_ITEMS * (8 * N_CAT + 4 * N_NUM + 4),
             "gather": n_with_row * (up(4 * N_CAT) + up(8 * N_NUM) + (up(4) if with_rows else 0))}
    parts["total"] = sum(parts.values())
    return parts


def fork(ft):
    """The same state again: the calls replace arrays and device tensors, they
    write into none, so a shallow copy shares them safely."""
    s = copy.copy(ft)
    s._dev, s._prev, s._dev_lock = dict(ft._dev), {}, threading.Lock()
    return s


def timed_builds(dev, gen, with_rows, rounds, builds):
    """Seconds per build by HIP events over a generation's resident columns."""
    from dcnr import _lib
    lib = _lib.load()
    M = gen.n_reviews
    nb = int(lib.dcnr_item_features_workspace_size(M, N_ITEMS, N_CAT, N_NUM))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    first = torch.empty(N_ITEMS, dtype=torch.int32, device=dev)
    cat = torch.empty((N_ITEMS, N_CAT), dtype=torch.int64, device=dev)
    num = torch.empty((N_ITEMS, N_NUM), dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    secs = []
    for i in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(builds):
            _lib.check(lib.dcnr_item_features_build(
                gen.review_item.data_ptr(), gen.review_row.data_ptr() if with_rows else None,
                gen.review_cat.data_ptr(), gen.review_num.data_ptr(), gen.scaler_scale.data_ptr(),
                gen.scaler_min.data_ptr(), M, N_ITEMS, N_CAT, N_NUM, first.data_ptr(), cat.data_ptr(),
                num.data_ptr(), counts.data_ptr(), None, ws.data_ptr(), nb, _lib.stream_ptr(dev)),
                "dcnr_item_features_build")
        e1.record()
        e1.synchronize()
        if i:   # (the first is the warm-up)
            secs.append(e0.elapsed_time(e1) * 1e-3 / builds)
    assert counts.tolist() == [gen.n_with_row, 0] and torch.equal(cat, gen.item_cat) and \
        torch.equal(num.view(torch.int32), gen.item_num.view(torch.int32))
    return secs, nb


def host_route(ft, gen):
    """The three tables with numpy, timed; and compared with the device's."""
    from dcnr.item_features import FeatureColumns
    c = ft._cols
    t = time.perf_counter()
    first, cat, num = FeatureColumns(c.item, c.row, c.cat, c.num, c.scale, c.min, c.n_items).tables()
    sec = time.perf_counter() - t
    assert gen.first_row.cpu().numpy().tobytes() == first.tobytes()
    assert gen.item_cat.cpu().numpy().tobytes() == cat.tobytes()
    assert gen.item_num.cpu().numpy().tobytes() == num.tobytes()
    return sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-reviews", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1000, 100000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--builds", type=int, default=50, help="back-to-back builds per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_item_features.py needs the HIP device")
    import dcnr
    dev = torch.device("cuda:0")
    out = {"workload": f"M rows over {N_ITEMS} hotels drawn uniformly, n_cat = {N_CAT}, n_num = {N_NUM}",
           "device": torch.cuda.get_device_name(0), "processes": 1, "rounds": args.rounds,
           "builds_per_window": args.builds, "ms": "median / best / worst",
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "points": []}
    for lg in args.log2_reviews:
        M = 1 << lg
        rng = np.random.default_rng(lg)
        item, cat, num = table(rng, M)
        lo, hi = num.min(axis=0), num.max(axis=0)
        scale = 1.0 / (hi - lo)
        ft = dcnr.ItemFeatures(item, cat, num, scale, -lo * scale, n_items=N_ITEMS)
        gen = ft.on(dev)
        torch.cuda.synchronize()
        point = {"log2_reviews": lg, "reviews": M, "hotels_with_a_row": gen.n_with_row, "builds": []}
        for with_rows in (True, False):
            secs, ws_bytes = timed_builds(dev, gen, with_rows, args.rounds, args.builds)
            med = statistics.median(secs)
            model = byte_model(M, gen.n_with_row, with_rows)
            floor = model["total"] / HBM_BYTES_PER_S
            point["builds"].append({"review_row": "given" if with_rows else "NULL", "build_ms": stats(secs),
                                    "model_bytes": model, "hbm_floor_ms": round(floor * 1e3, 4),
                                    "floor_over_build": round(floor / med, 3),
                                    "model_gb_per_s": round(model["total"] / med / 1e9, 1)})
        point["workspace_bytes"] = ws_bytes
        host_s = host_route(ft, gen)
        point["host_route_ms"] = round(host_s * 1e3, 1)
        point["host_over_build"] = round(host_s / (point["builds"][0]["build_ms"]["median"] * 1e-3), 1)
        point["updates"] = []
        for b in args.batches:
            if b >= M:
                continue
            new = table(rng, b)
            gone = np.sort(rng.choice(M, b, replace=False))
            vals = rng.random((b, N_NUM))
            for op, call in (("append", lambda s: s.append(*new)), ("remove", lambda s: s.remove(gone)),
                             ("set_values", lambda s: s.set_values(gone, vals))):
                wall, host, device = [], [], []
                for i in range(args.rounds + 1):
                    s = fork(ft)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    call(s)
                    torch.cuda.synchronize()
                    if i:
                        wall.append(time.perf_counter() - t)
                        host.append(s.last_update["host_s"])
                        device.append(s.last_update["device_s"])
                point["updates"].append({"op": op, "batch": b, "wall_ms": stats(wall, nd=3),
                                         "host_ms": stats(host, nd=3), "device_part_ms": stats(device, nd=3),
                                         "upload_bytes": int(s.last_update["upload_bytes"])})
                del s
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del ft, gen
        torch.cuda.empty_cache()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
