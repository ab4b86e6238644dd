#!/usr/bin/env python
"""Times prepare_data on the device (dcnr_train_table_build, dcnr.prepare_data)
against the numpy yardstick over the same columns.

    python tools/bench_train_table.py [--log2-rows 20 22] [--rounds 5] [--host-rounds 3]
                                      [--native-only]
                                      [--out profiles/train_table/bench_train_table.json]

Frame: M rows, 8 raw numeric columns (2 % NaN) and the reference's 3 derived
ones (n_num = 11), 2 categorical columns (300 and 6 keys, 1 % missing), about
M / 8 users and M / 64 items drawn uniformly, the reference's noise filter on a
1..10 rating column (it keeps 7 rows in 10).

Per point, in one process on one device, median / best / worst of the rounds
after a warm-up:
  (a) native   HIP events around --builds back-to-back dcnr_train_table_build
               calls over resident columns (buffers allocated beforehand),
               divided by their number; with the byte model of the passes the
               call makes (byte_model below), the time those bytes take at the
               HBM rate a streaming copy reaches (6.3 TB/s) and the fraction of
               that floor the call reaches
  (b) prepare  dcnr.prepare_data end to end, wall clock with a device
               synchronize inside the timed region: from device-resident columns
               and from host columns (the upload inside)
  (c) host     dcnr.prepare_data_host on the same arrays plus the upload of its
               eight tensors; its outputs must equal the device's
Prints one JSON line (and writes it to --out).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hybrid-hotel-recommendation-system-based-on-friends-recommendations_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_RAW, N_CAT = 8, 2
DERIVED = [("ratio", 0, 1), ("ratio", 5, 7), ("diff", 3, 4)]
FILTER = (3, 4.0, 8.0)
HBM_BYTES_PER_S = 6.3e12   # what a streaming copy reaches on the MI355X
SORT_PASSES, SELECT_PASSES = 6, 6


def stats(xs, unit=1e3, nd=3):
    return {"median": round(statistics.median(xs) * unit, nd), "best": round(min(xs) * unit, nd),
            "worst": round(max(xs) * unit, nd)}


def frame(M, seed):
    rng = np.random.default_rng(seed)
    raw = np.round(rng.normal(50.0, 20.0, (M, N_RAW)), 2)
    raw[:, 1] = rng.integers(0, 6, M)          # stars, zeros among them
    raw[:, 3] = rng.integers(1, 11, M)         # the rating the filter reads
    raw[rng.random((M, N_RAW)) < 0.02] = np.nan
    cat = [rng.integers(0, 300, M), rng.integers(0, 6, M)]
    for k in cat:
        k[rng.random(M) < 0.01] = -1
    return dict(user=rng.integers(0, max(1, M // 8), M) * 7919 - 12345,
                item=rng.integers(0, max(1, M // 64), M) + (1 << 40), target=rng.integers(0, 2, M),
                cat=cat, num=raw, noise_filter=FILTER, derived=DERIVED)


def byte_model(M, n, n_num):
    """The bytes the passes of dcnr_train_table_build move (inputs read once per
    pass that needs them, outputs written once): M input rows, n surviving."""
    cols = 2 + N_CAT
    parts = {
        "rows": M * (8 * N_RAW + 8 * N_CAT) + M * (8 * n_num + 1 + 4),
        "survivor_scan_emit": 12 * M + M * (1 + 4 + 1) + 8 * n,
        "median_select": SELECT_PASSES * M * n_num * (8 + 1),
        "minmax": M * n_num * (8 + 1),
        "transform": n * (8 * n_num + 4) + n * 4 * n_num,
        "records": cols * (16 * M + 12 * n),
        "sort": cols * SORT_PASSES * 48 * M,
        "heads_scans_codes": 2 * (16 * n + 8 * n + 24 * n + 24 * n + 16 * n)
        + N_CAT * (16 * n + 4 * n + 12 * n + 28 * n + 8 * n),
    }
    parts["total"] = sum(parts.values())
    return parts


def native(dev, cols, M, rounds, builds):
    """Seconds per dcnr_train_table_build by HIP events; the counts."""
    from dcnr import _lib, prepare as P
    lib = _lib.load()
    user, item, target, key, raw = cols
    dv = P._derived_arg(DERIVED, N_RAW)
    n_num = N_RAW + len(dv)
    nb = int(lib.dcnr_train_table_workspace_size(M, N_CAT, N_RAW, len(dv)))
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    ws = new(nb, torch.uint8)
    out = [new(M, torch.int32), new((M, 2), torch.int64), new((M, N_CAT), torch.int64),
           new((M, n_num), torch.float32), new(M, torch.float32), new(M, torch.int64), new(M, torch.int64),
           new((N_CAT, M), torch.int64), new((5, n_num), torch.float64)]
    counts = new(P.N_COUNTS + N_CAT, torch.int32)
    a = P.TrainTableArgs(user.data_ptr(), item.data_ptr(), target.data_ptr(), key.data_ptr(), raw.data_ptr(), M,
                         N_CAT, N_RAW, FILTER[0], FILTER[1], FILTER[2], len(dv), dv.ctypes.data,
                         *[t.data_ptr() for t in out], None, counts.data_ptr(), None)
    secs = []
    for i in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(builds):
            _lib.check(lib.dcnr_train_table_build(ctypes.byref(a), ws.data_ptr(), nb, _lib.stream_ptr(dev)),
                       "dcnr_train_table_build")
        e1.record()
        e1.synchronize()
        if i:   # (the first is the warm-up)
            secs.append(e0.elapsed_time(e1) * 1e-3 / builds)
    return secs, nb, counts.cpu().tolist()


def wall(fn, rounds):
    secs = []
    for i in range(rounds + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        if i:
            secs.append(time.perf_counter() - t)
    return secs, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--builds", type=int, default=5, help="back-to-back native calls per timed window")
    ap.add_argument("--native-only", action="store_true", help="leg (a) alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_train_table.py needs the HIP device")
    import dcnr
    dev = torch.device("cuda:0")
    n_num = N_RAW + len(DERIVED)
    out = {"workload": f"M rows, n_num = {n_num} ({len(DERIVED)} derived), n_cat = {N_CAT}, ~M/8 users, "
                       "~M/64 items, noise filter on",
           "device": torch.cuda.get_device_name(0), "processes": 1, "rounds": args.rounds,
           "host_rounds": args.host_rounds, "builds_per_window": args.builds, "ms": "median / best / worst",
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "points": []}
    for lg in args.log2_rows:
        M = 1 << lg
        case = frame(M, lg)
        on = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x)).to(device=dev, dtype=dt)
        cols = (on(case["user"], torch.int64), on(case["item"], torch.int64), on(case["target"], torch.uint8),
                on(np.stack(case["cat"], axis=1), torch.int64), on(case["num"], torch.float64))
        secs, ws_bytes, counts = native(dev, cols, M, args.rounds, args.builds)
        n = counts[0]
        model = byte_model(M, n, n_num)
        med = statistics.median(secs)
        floor = model["total"] / HBM_BYTES_PER_S
        point = {"log2_rows": lg, "rows": M, "surviving": n, "users": counts[1], "items": counts[2],
                 "after_filter": counts[3], "workspace_bytes": ws_bytes, "native_ms": stats(secs),
                 "model_bytes": model, "hbm_floor_ms": round(floor * 1e3, 3),
                 "floor_over_native": round(floor / med, 3), "model_gb_per_s": round(model["total"] / med / 1e9, 1)}
        if args.native_only:
            out["points"].append(point)
            continue
        resident = dict(user=cols[0], item=cols[1], target=cols[2], cat=cols[3], num=cols[4])
        kw = dict(noise_filter=FILTER, derived=DERIVED, device=dev)
        s, p = wall(lambda: dcnr.prepare_data(**resident, **kw), args.rounds)
        point["prepare_data_resident_ms"] = stats(s)
        host_in = dict(user=case["user"], item=case["item"], target=case["target"], cat=case["cat"], num=case["num"])
        s, _ = wall(lambda: dcnr.prepare_data(**host_in, **kw), args.rounds)
        point["prepare_data_from_host_ms"] = stats(s)

        def host_route():
            h = dcnr.prepare_data_host(**host_in, noise_filter=FILTER, derived=DERIVED)
            return h, [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in h.train + h.val]
        s, (h, up) = wall(host_route, args.host_rounds)
        point["host_yardstick_plus_upload_ms"] = stats(s, nd=1)
        point["host_over_prepare_data_from_host"] = round(
            statistics.median(s) * 1e3 / point["prepare_data_from_host_ms"]["median"], 1)
        for a, b in zip(p.train + p.val, up):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
        assert p.model_dims == h.model_dims and np.array_equal(p.scale_, h.scale_)
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del cols, resident, p, h, up
        torch.cuda.empty_cache()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
