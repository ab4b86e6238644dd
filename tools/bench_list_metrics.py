#!/usr/bin/env python
"""Times dcnr_eval_list_metrics against the route a caller has without it: the
same figures written with torch ops on the device, in one process.

    python tools/bench_list_metrics.py [--lists 256 4096 65536 1000000] [--iters 20]
                                       [--out profiles/list_metrics/bench_list_metrics.json]

A table of --items x --dim fp32 embeddings (1M x 64), R lists of --at (20)
uniformly drawn items with their logits, the inputs resident and the workspace
preallocated.  Per R, after a warm-up of both routes, --iters rounds that
alternate the two; a round's figure is a host clock around `inner` calls that
end in one device synchronise, divided by `inner`.  `inner` is set per route
and R from one timed call after the warm-up so that a window lasts at least
--window-ms (20 ms).  Median, min and max per route:
  call_ms     dcnr_eval_list_metrics, summary only (scores given, no held-out
              sets): four launches (clear, lists, counts, final)
  records_ms  the same with the R records written
  torch_ms    torch_list_metrics below: gather + bmm + triu for the pair
              cosines, bincount + sort for coverage and Gini
Before anything is timed the torch figures are checked against the call's:
the integers equal, ild and mean_score within 1e-5.  gather_GBps is the bytes
of the embedding rows the lists name (R * at * dim * 4) over call_ms: the rate
of the whole call, not of one kernel.  Prints one JSON line (and writes it to
--out).
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
PKG = os.path.join(ROOT, "hybrid-hotel-recommendation-system-based-on-friends-recommendations_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def torch_list_metrics(rows, scores, table, inv, R, at):
    """ild, mean_score, n_distinct_items and gini_num with torch ops on the device."""
    n_items = table.shape[0]
    e = table[rows] * inv[rows].unsqueeze(1)                     # the gather, normalised
    e = e.view(R, at, -1)
    g = torch.bmm(e, e.transpose(1, 2))                          # [R, at, at] cosines
    pc = torch.triu(g, diagonal=1).sum((1, 2), dtype=torch.float64)
    ild = (1.0 - pc / (at * (at - 1) // 2)).mean()
    c = torch.bincount(rows, minlength=n_items)
    s = torch.sort(c).values
    w = 2 * torch.arange(1, n_items + 1, device=rows.device) - n_items - 1
    return ild, scores.sum(dtype=torch.float64) / rows.numel(), (c > 0).sum(), (w * s).sum()


def clocked(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "rounds": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", type=int, nargs="+", default=[256, 4096, 65536, 1000000])
    ap.add_argument("--items", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--at", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_list_metrics.py needs the HIP device")
    from dcnr import _lib, metrics
    from dcnr.serving import row_inv_norms
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = _lib.stream_ptr(dev)
    n_items, d, at = args.items, args.dim, args.at
    gen = torch.Generator(device=dev).manual_seed(1)
    table = torch.randn((n_items, d), generator=gen, device=dev)
    inv = row_inv_norms(table)
    ks = (ctypes.c_int32 * 1)(0)
    out = {"device": torch.cuda.get_device_name(0), "n_items": n_items, "dim": d, "at": at,
           "timing": "host clock around `inner` calls ending in one synchronise (a window of at "
                     "least window_ms), per call; median over rounds alternating the routes",
           "window_ms": args.window_ms, "lists": {}}
    for R in args.lists:
        n = R * at
        rng = np.random.default_rng(R)
        rows = torch.from_numpy(rng.integers(0, n_items, n)).to(dev)
        scores = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
        offsets = torch.arange(0, n + 1, at, dtype=torch.int64, device=dev)
        ws = torch.empty(metrics.list_workspace_bytes(R, n_items), dtype=torch.uint8, device=dev)
        res = torch.empty(248, dtype=torch.uint8, device=dev)
        rec = torch.empty((R, 14), dtype=torch.int64, device=dev)

        def call(records=False):
            _lib.check(lib.dcnr_eval_list_metrics(
                rows.data_ptr(), n, offsets.data_ptr(), None, R, at, table.data_ptr(), inv.data_ptr(), d,
                n_items, scores.data_ptr(), None, None, 0, None, ks, 0, None, None, res.data_ptr(),
                rec.data_ptr() if records else None, ws.data_ptr(), ws.numel(), stream),
                "dcnr_eval_list_metrics")

        def torch_route():
            return torch_list_metrics(rows, scores, table, inv, R, at)

        # the torch figures against the call's, before anything is timed
        m = metrics.list_metrics_raw(rows, offsets, None, table=table, inv_norms=inv, at=at,
                                     scores=scores, ks=(), ws=ws)
        t_ild, t_score, t_distinct, t_gnum = (v.item() for v in torch_route())
        assert (m.n_distinct_items, m.gini_num, m.n_entries) == (t_distinct, t_gnum, n), (m, t_distinct, t_gnum)
        assert abs(m.ild - t_ild) <= 1e-5 and abs(m.mean_score - t_score) <= 1e-5, (m.ild, t_ild)
        for _ in range(args.warmup):
            call()
            call(True)
            torch_route()
        # calls per timed window: at least --window-ms of work
        inner = max(1, int(np.ceil(args.window_ms / clocked(call, 5))))
        t_inner = max(1, int(np.ceil(args.window_ms / clocked(torch_route, 2))))
        a, b, c = [], [], []
        for _ in range(args.iters):
            a.append(clocked(call, inner))
            c.append(clocked(torch_route, t_inner))
            b.append(clocked(lambda: call(True), inner))
        per = {"entries": n, "call_ms": stats(a), "records_ms": stats(b), "torch_ms": stats(c),
               "inner_calls": inner, "torch_inner_calls": t_inner,
               "ild": m.ild, "coverage": m.coverage, "gini": m.gini, "checked_against_torch": True}
        per["spread_pct"] = {k: round(100.0 * (per[k]["max_ms"] - per[k]["min_ms"]) / per[k]["median_ms"], 1)
                             for k in ("call_ms", "records_ms", "torch_ms")}
        per["gather_GBps"] = round(n * d * 4 / (per["call_ms"]["median_ms"] * 1e-3) / 1e9, 1)
        per["torch_over_call"] = round(per["torch_ms"]["median_ms"] / per["call_ms"]["median_ms"], 2)
        out["lists"][str(R)] = per
        del rows, scores, offsets, ws, rec
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
