"""Cosine nearest neighbours on libdcnr: drop-in for the
``sklearn.neighbors.NearestNeighbors(metric='cosine', algorithm='brute')``
index the reference builds at startup (main.py:268-270) and queries per
positive hotel (main.py:200) and per /similar_items request (main.py:300).

``kneighbors`` keeps sklearn's contract (numpy in, numpy ``(dist, idx)`` out,
ascending distance, the query row itself included when it is in the index --
callers drop position 0 as main.py does).  Ties are ordered by row index
(sklearn's argsort order among exactly equal distances is unspecified).
``kneighbors_device`` takes/returns device tensors for batched callers.

``build_neighbor_table`` precomputes the answer for every row of the fitted
table (the only queries the reference ever makes: main.py:200, 300), so that a
server looks neighbours up instead of scanning.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

# the batched scan (knn.hip scan v4) serves d = 32 / 64; its admission bound
# samples the first V4_S = 65536 rows.  Tables of more than PACKED_MIN_ROWS
# rows get the fit-time bf16 copy
PACKED_D = (32, 64)
PACKED_MIN_ROWS = 32768
# changed rows one dcnr_cosine_neighbor_table_update call takes (knn.hip UPD_MAX_M)
UPDATE_MAX_ROWS = 16384


class NearestNeighbors:
    def __init__(self, n_neighbors=5, metric='cosine', algorithm='brute', device='cuda'):
        if metric != 'cosine':
            raise NotImplementedError("dcnr.NearestNeighbors implements metric='cosine' only "
                                      "(the reference's only use, main.py:268)")
        if algorithm not in ('brute', 'auto'):
            raise NotImplementedError("dcnr.NearestNeighbors is a brute-force index")
        self.n_neighbors = n_neighbors
        self.metric = metric
        self.algorithm = algorithm
        self.device = torch.device(device)
        self._table = None
        self._inv = None
        self._packed = None
        self.neighbor_table_ = None
        self._pin = None   # update_rows' pinned count words

    def fit(self, X, y=None):
        t = torch.as_tensor(np.asarray(X, dtype=np.float32) if not torch.is_tensor(X) else X)
        t = t.to(self.device, torch.float32).contiguous()
        if t.dim() != 2:
            raise ValueError("Expected 2D array")
        if self.device.type != 'cuda':
            raise RuntimeError("dcnr.NearestNeighbors runs on the HIP device only")
        self._table = t
        self.neighbor_table_ = None   # (of the table fitted before)
        self._inv = torch.empty(t.shape[0], dtype=torch.float32, device=self.device)
        lib = _lib.load()
        _lib.check(lib.dcnr_row_inv_norms(t.data_ptr(), t.shape[0], t.shape[1], self._inv.data_ptr(),
                                          _lib.stream_ptr(self.device)), "dcnr_row_inv_norms")
        self._packed = None
        if t.shape[1] in PACKED_D and t.shape[0] > PACKED_MIN_ROWS:
            # bf16 copy of the normalised rows for the batched coarse scan
            # (2 B / element beside the fp32 table; same results without it)
            self._packed = torch.empty(t.shape, dtype=torch.int16, device=self.device)
            _lib.check(lib.dcnr_cosine_pack_rows(t.data_ptr(), self._inv.data_ptr(), t.shape[0],
                                                 t.shape[1], self._packed.data_ptr(),
                                                 _lib.stream_ptr(self.device)),
                       "dcnr_cosine_pack_rows")
        self.n_samples_fit_ = t.shape[0]
        self.n_features_in_ = t.shape[1]
        return self

    def kneighbors_device(self, q: torch.Tensor, k: int):
        if self._table is None:
            raise RuntimeError("This NearestNeighbors instance is not fitted yet")
        lib = _lib.load()
        q = q.to(self.device, torch.float32).reshape(-1, self._table.shape[1]).contiguous()
        Q = q.shape[0]
        N, d = self._table.shape
        if k > N:
            raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, "
                             f"n_samples_fit = {N}, n_samples = {Q}")
        idx = torch.empty((Q, k), dtype=torch.int64, device=self.device)
        dist = torch.empty((Q, k), dtype=torch.float32, device=self.device)
        nb = int(lib.dcnr_cosine_topk_workspace_size(N, Q, k))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=self.device)
        packed = self._packed.data_ptr() if self._packed is not None else None
        _lib.check(lib.dcnr_cosine_topk_packed(self._table.data_ptr(), self._inv.data_ptr(), packed,
                                               N, d, q.data_ptr(), Q, k, idx.data_ptr(),
                                               dist.data_ptr(), ws.data_ptr(), ws.numel(),
                                               _lib.stream_ptr(self.device)),
                   "dcnr_cosine_topk")
        return dist, idx

    def kneighbors_within_device(self, q, k, set_rows, set_offsets, seg_offsets, seg_set, max_set_rows,
                                 exclude=None, out=None, seg_status=None):
        """The k nearest rows within a row set (dcnr_cosine_topk_within), on
        device tensors.  Queries [seg_offsets[g], seg_offsets[g+1]) search the
        rows ``set_rows[set_offsets[s]:set_offsets[s+1]]`` of set ``s =
        seg_set[g]`` (int64 CSR, ascending rows; ``seg_set`` int32, negative =
        segment skipped); ``max_set_rows`` is a host bound on the longest set
        named.  ``exclude`` (int64 [Q], -1 = none) leaves one row out per
        query.  ``out`` = (idx int64, dist fp32), each [Q, >= k] with unit
        column stride and one row stride -- column slices of wider buffers
        will do: columns [0, k) of the rows of segments that are not skipped
        are overwritten, everything else is kept.  Without it fresh [Q, k]
        tensors are used (a skipped segment's rows then read (-1, inf)).
        Returns ``(dist, idx)``; with fewer than k eligible rows the tail is
        (-1, FLT_MAX).  ``seg_status`` (int32 [G]) receives DCNR_REQ_BAD_DATA
        for a segment whose device data failed a check."""
        if self._table is None:
            raise RuntimeError("This NearestNeighbors instance is not fitted yet")
        k = int(k)
        if not 1 <= k <= 64:
            raise ValueError(f"kneighbors_within_device: n_neighbors = {k} outside [1, 64]")
        N, d = self._table.shape
        q = q.to(self.device, torch.float32).reshape(-1, d).contiguous()
        Q = q.shape[0]

        def same_dev(t):   # ('cuda' names the current device)
            return t.device.type == self.device.type and self.device.index in (None, t.device.index)

        def dev(t, dtype, what):
            if not same_dev(t) or t.dtype != dtype or not t.is_contiguous():
                raise ValueError(f"kneighbors_within_device: {what} must be a contiguous {dtype} tensor "
                                 f"on {self.device}")
            return t
        set_rows = dev(set_rows, torch.int64, "set_rows")
        set_offsets = dev(set_offsets, torch.int64, "set_offsets")
        seg_offsets = dev(seg_offsets, torch.int64, "seg_offsets")
        seg_set = dev(seg_set, torch.int32, "seg_set")
        G, S = seg_set.numel(), set_offsets.numel() - 1
        if seg_offsets.numel() != G + 1 or S < 0:
            raise ValueError("kneighbors_within_device: seg_offsets needs one entry more than seg_set, "
                             "set_offsets at least one")
        if exclude is not None and dev(exclude, torch.int64, "exclude").numel() != Q:
            raise ValueError("kneighbors_within_device: exclude needs one entry per query")
        if seg_status is not None and dev(seg_status, torch.int32, "seg_status").numel() != G:
            raise ValueError("kneighbors_within_device: seg_status needs one entry per segment")
        if out is None:
            idx = torch.full((Q, k), -1, dtype=torch.int64, device=self.device)
            dist = torch.full((Q, k), torch.finfo(torch.float32).max, dtype=torch.float32, device=self.device)
        else:
            idx, dist = out
            ok = (idx.dtype == torch.int64 and dist.dtype == torch.float32 and same_dev(idx) and same_dev(dist)
                  and idx.dim() == 2 and dist.dim() == 2
                  and idx.shape[0] == Q and dist.shape[0] == Q and idx.shape[1] >= k and dist.shape[1] >= k
                  and (Q == 0 or (idx.stride(1) == 1 and dist.stride(1) == 1
                                  and idx.stride(0) == dist.stride(0) >= k)))
            if not ok:
                raise ValueError("kneighbors_within_device: out = (idx int64, dist fp32), both [Q, >= k] "
                                 "with unit column stride and the same row stride")
        ld = idx.stride(0) if Q > 0 else k
        lib = _lib.load()
        nb = int(lib.dcnr_cosine_topk_within_workspace_size(Q, k, d, int(max_set_rows)))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=self.device)
        _lib.check(lib.dcnr_cosine_topk_within(
            self._table.data_ptr(), self._inv.data_ptr(), N, d, q.data_ptr(), Q,
            exclude.data_ptr() if exclude is not None else None, seg_offsets.data_ptr(), G,
            seg_set.data_ptr(), set_rows.data_ptr() if set_rows.numel() else None, set_rows.numel(),
            set_offsets.data_ptr(), S, int(max_set_rows), k, ld, idx.data_ptr(), dist.data_ptr(),
            seg_status.data_ptr() if seg_status is not None else None, ws.data_ptr(), ws.numel(),
            _lib.stream_ptr(self.device)), "dcnr_cosine_topk_within")
        return dist, idx

    def _within_rows(self, rows):
        """A host row list as kneighbors(within=) takes it: validated, sorted,
        de-duplicated int64."""
        r = np.unique(np.asarray(rows, dtype=np.int64).reshape(-1))
        N = self._table.shape[0]
        if r.size and (r[0] < 0 or r[-1] >= N):
            raise ValueError(f"within: row {int(r[0] if r[0] < 0 else r[-1])} outside the index [0, {N})")
        return r

    def build_neighbor_table(self, k=None, rows=None, return_distance=False):
        """The item neighbour table (dcnr_cosine_neighbor_table): int32
        [rows, k] on the device, row r exactly ``kneighbors_device(table[r:r+1],
        k)[1]`` -- the row's k nearest, ascending by (distance, row), the row
        itself not treated specially.  ``k`` defaults to ``n_neighbors``;
        ``rows`` = (lo, hi) builds that range only (a build in pieces gives
        the same rows).  A full build is kept as ``neighbor_table_`` until the
        next ``fit``.  ``return_distance``: (distances fp32, table)."""
        if self._table is None:
            raise RuntimeError("This NearestNeighbors instance is not fitted yet")
        lib = _lib.load()
        N, d = self._table.shape
        k = self.n_neighbors if k is None else int(k)
        lo, hi = (0, N) if rows is None else (int(rows[0]), int(rows[1]))
        if not 0 <= lo <= hi <= N:
            raise ValueError(f"build_neighbor_table: rows ({lo}, {hi}) outside [0, {N}]")
        if not 1 <= k <= N:
            raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, "
                             f"n_samples_fit = {N}")
        nbr = torch.empty((hi - lo, k), dtype=torch.int32, device=self.device)
        dist = torch.empty((hi - lo, k), dtype=torch.float32, device=self.device) \
            if return_distance else None
        nb = int(lib.dcnr_cosine_neighbor_table_workspace_size(N, k))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=self.device)
        packed = self._packed.data_ptr() if self._packed is not None else None
        _lib.check(lib.dcnr_cosine_neighbor_table(self._table.data_ptr(), self._inv.data_ptr(), packed,
                                                  N, d, k, lo, hi, nbr.data_ptr(),
                                                  dist.data_ptr() if return_distance else None,
                                                  ws.data_ptr(), ws.numel(),
                                                  _lib.stream_ptr(self.device)),
                   "dcnr_cosine_neighbor_table")
        if (lo, hi) == (0, N):
            self.neighbor_table_ = nbr
        return (dist, nbr) if return_distance else nbr

    def update_rows(self, rows, vectors=None, table=None, return_stats=False, rebuild=None):
        """New vectors for some rows of the fitted table, with everything
        derived from it brought back to exactly what ``fit`` +
        ``build_neighbor_table`` give on the new table: ``_inv``, ``_packed``
        and the neighbour table, the work growing with the number of rows.

        rows     distinct row ids inside [0, N) (ValueError otherwise, nothing
                 changed); none at all is a no-op
        vectors  [m, d], written into the table; None: those rows of the
                 fitted table were already modified in place (a pipeline's
                 index shares the model's item table when that is fp32 on the
                 device: ``fit`` does not copy it)
        table    int32 [N, kt] on the device, contiguous, updated in place;
                 default ``neighbor_table_``; with neither only the norms and
                 the packed copy are refreshed
        rebuild  None: the range build takes over from the incremental update
                 where that is estimated at half a rebuild or more
                 (``rebuild_is_cheaper``); True / False force either path
                 (the result is the same)

        Precondition: ``table`` was exact for the embeddings before the
        change -- built from them, or updated through here ever since.  More
        rows than one native call takes (UPDATE_MAX_ROWS) are applied as
        consecutive changes (written in place already, they are rebuilt: the
        vectors in between are gone).  Ordered on the current stream, with one
        host wait (for the number of rows to search again); not safe against
        requests in flight on other streams.  ``return_stats``: a dict of the
        rows changed / affected / merged / searched again (read back only
        then; ``rebuilt`` when the range build ran)."""
        if self._table is None:
            raise RuntimeError("This NearestNeighbors instance is not fitted yet")
        N, d = self._table.shape
        r = np.asarray(rows.cpu() if torch.is_tensor(rows) else rows).reshape(-1)
        if r.size and not np.issubdtype(r.dtype, np.integer):
            raise ValueError("update_rows: rows must be integers")
        r = r.astype(np.int64)
        if r.size and (r.min() < 0 or r.max() >= N):
            raise ValueError(f"update_rows: rows outside [0, {N})")
        order = np.argsort(r, kind="stable")
        r = r[order]
        if np.any(r[1:] == r[:-1]):
            raise ValueError("update_rows: duplicate rows")
        if vectors is not None:
            v = torch.as_tensor(np.asarray(vectors, dtype=np.float32)) if not torch.is_tensor(vectors) \
                else vectors
            v = v.to(self.device, torch.float32).reshape(-1, d)
            if v.shape[0] != r.size:
                raise ValueError(f"update_rows: {r.size} rows, {v.shape[0]} vectors")
            v = v[torch.from_numpy(order).to(self.device)]
        table = self._table_arg("update_rows", table)
        stats = dict(changed=int(r.size), affected=0, merged=0, researched=0, rebuilt=False)
        m = int(r.size)
        if m == 0:
            return stats if return_stats else None
        kt = table.shape[1] if table is not None else 0
        full = table is not None and (bool(rebuild) if rebuild is not None
                                      else rebuild_is_cheaper(m, kt, N))
        if table is not None and not full and vectors is None and m > UPDATE_MAX_ROWS:
            full = True
        if table is None or full:
            self._refresh_rows(r, None if vectors is None else v)
            if full:
                self._build_into(table)
                stats.update(rebuilt=True, researched=N)
        else:
            for lo in range(0, m, UPDATE_MAX_ROWS):
                hi = min(m, lo + UPDATE_MAX_ROWS)
                self._refresh_rows(r[lo:hi], None if vectors is None else v[lo:hi])
                c = self._update_table(r[lo:hi], table, return_stats)
                if return_stats:
                    _add_counts(stats, c)
        return stats if return_stats else None

    def append_rows(self, vectors=None, table=None, storage=None, return_stats=False, rebuild=None):
        """Append m rows to the fitted table, with everything derived from it
        ending exactly as ``fit`` + ``build_neighbor_table(kt)`` give it on the
        grown table: ``_inv``, ``_packed`` and the neighbour table.

        vectors  [m, d]: copied behind the fitted table
        storage  instead: an fp32 device tensor [N + m, d], contiguous, whose
                 first N rows equal the fitted table and whose last m rows are
                 the new vectors; adopted without a copy (a pipeline's index
                 shares the model's grown item table as it shared the old one)
        table    int32 [N, kt] on the device, exact for the fitted table;
                 default ``neighbor_table_``; with neither only the norms and
                 the packed copy grow

        Returns the grown [N + m, kt] neighbour table (None without one), also
        kept as ``neighbor_table_`` when that was the table grown (otherwise a
        kept ``neighbor_table_`` is dropped: it is not the index's any more); with
        ``return_stats`` ``(table, stats)``, the stats as ``update_rows``'.

        The appended rows are the changed rows of the grown table: no list of
        an old row can hold a new row, so an old row is either untouched or
        gains new rows.  ``update_rows``' filter finds the rows that may gain
        (a superset, by a margin far above float32's rounding), and they are
        searched as the build searches them, the new rows with them whatever
        their lists hold (they are filled with row 0 first).  The filter's rows
        do not go through ``update_rows``' merge: it scores a kept entry again,
        and at a million rows some two neighbours lie within one float32 step,
        where the merge and the search need not order them alike (measured:
        DESIGN.md section 8, "Admitting new rows").  More than
        UPDATE_MAX_ROWS rows are appended as consecutive appends, each onto the
        exact table of the rows before it; ``rebuild`` as in ``update_rows``.
        Ordered on the current stream; not safe against requests in flight on
        other streams."""
        if self._table is None:
            raise RuntimeError("This NearestNeighbors instance is not fitted yet")
        N, d = self._table.shape
        if (vectors is None) == (storage is None):
            raise ValueError("append_rows: give vectors or storage, not both")
        if storage is not None:
            if (not torch.is_tensor(storage) or storage.dtype != torch.float32 or storage.dim() != 2
                    or storage.shape[1] != d or storage.shape[0] < N or storage.device != self._table.device
                    or not storage.is_contiguous()):
                raise ValueError(f"append_rows: storage must be a contiguous fp32 [>= {N}, {d}] tensor on "
                                 f"{self._table.device}")
            grown = storage.detach()
        else:
            v = torch.as_tensor(np.asarray(vectors, dtype=np.float32)) if not torch.is_tensor(vectors) \
                else vectors
            v = v.detach().to(self.device, torch.float32).reshape(-1, d)
            grown = torch.cat([self._table, v], dim=0)
        m = int(grown.shape[0]) - N
        own = table is None or table is self.neighbor_table_
        table = self._table_arg("append_rows", table)
        stats = dict(changed=m, affected=0, merged=0, researched=0, rebuilt=False)
        if m == 0:
            if storage is not None:
                self._table = grown
            return (table, stats) if return_stats else table
        # the norms and packed rows of the new rows, by the fit's kernels (each
        # row's bits depend on that row alone)
        lib = _lib.load()
        stream = _lib.stream_ptr(self.device)
        new = grown[N:]
        inv = torch.empty(N + m, dtype=torch.float32, device=self.device)
        inv[:N] = self._inv
        _lib.check(lib.dcnr_row_inv_norms(new.data_ptr(), m, d, inv[N:].data_ptr(), stream), "dcnr_row_inv_norms")
        packed = None
        if d in PACKED_D and N + m > PACKED_MIN_ROWS:
            packed = torch.empty((N + m, d), dtype=torch.int16, device=self.device)
            if self._packed is not None:
                packed[:N] = self._packed
                lo = N
            else:   # the table has just grown past the point where the fit packs
                lo = 0
            _lib.check(lib.dcnr_cosine_pack_rows(grown[lo:].data_ptr(), inv[lo:].data_ptr(), N + m - lo, d,
                                                 packed[lo:].data_ptr(), stream), "dcnr_cosine_pack_rows")
        if table is not None:
            kt = table.shape[1]
            nbr = torch.zeros((N + m, kt), dtype=torch.int32, device=self.device)   # new lists: row 0
            nbr[:N] = table
        self._table, self._inv, self._packed = grown, inv, packed
        self.n_samples_fit_ = N + m
        if table is None:
            return (None, stats) if return_stats else None
        full = bool(rebuild) if rebuild is not None else rebuild_is_cheaper(m, kt, N + m)
        if full:
            self._build_into(nbr)
            stats.update(rebuilt=True, researched=N + m)
        else:
            try:
                for lo in range(N, N + m, UPDATE_MAX_ROWS):
                    hi = min(N + m, lo + UPDATE_MAX_ROWS)
                    # an append of rows [lo, hi) onto the exact table of rows [0, lo)
                    self._table, self._inv = grown[:hi], inv[:hi]
                    self._packed = None if packed is None else packed[:hi]
                    c = self._update_table(np.arange(lo, hi, dtype=np.int64), nbr[:hi], return_stats, merge=False)
                    if return_stats:
                        _add_counts(stats, c)
            finally:
                self._table, self._inv, self._packed = grown, inv, packed
        # a kept table that was not the one grown no longer matches the index
        self.neighbor_table_ = nbr if own else None
        return (nbr, stats) if return_stats else nbr

    def _table_arg(self, what, table):
        """The neighbour table ``what`` works on: ``table``, by default
        ``neighbor_table_``, checked against the fitted table; None with neither."""
        table = self.neighbor_table_ if table is None else table
        N = self._table.shape[0]
        if table is not None:
            if (not torch.is_tensor(table) or table.dtype != torch.int32 or table.dim() != 2
                    or table.shape[0] != N or not 1 <= table.shape[1] <= N
                    or table.device != self._table.device or not table.is_contiguous()):
                raise ValueError(f"{what}: table must be a contiguous int32 [{N}, kt] tensor on "
                                 f"{self._table.device}")
        return table

    def _refresh_rows(self, r, v):
        """Writes v (or nothing) into rows r of the table and recomputes their
        inverse norms and packed rows with the fit's kernels on the gathered
        rows (each row's bits depend on that row alone)."""
        lib = _lib.load()
        d = self._table.shape[1]
        sel = torch.from_numpy(r).to(self.device)
        if v is not None:
            self._table[sel] = v
        g = self._table[sel].contiguous()
        inv = torch.empty(r.size, dtype=torch.float32, device=self.device)
        stream = _lib.stream_ptr(self.device)
        _lib.check(lib.dcnr_row_inv_norms(g.data_ptr(), r.size, d, inv.data_ptr(), stream),
                   "dcnr_row_inv_norms")
        self._inv[sel] = inv
        if self._packed is not None:
            pk = torch.empty((r.size, d), dtype=torch.int16, device=self.device)
            _lib.check(lib.dcnr_cosine_pack_rows(g.data_ptr(), inv.data_ptr(), r.size, d, pk.data_ptr(),
                                                 stream), "dcnr_cosine_pack_rows")
            self._packed[sel] = pk

    def _build_into(self, table):
        """The range build of every row, written over ``table``."""
        lib = _lib.load()
        N, d = self._table.shape
        kt = table.shape[1]
        nb = int(lib.dcnr_cosine_neighbor_table_workspace_size(N, kt))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=self.device)
        packed = self._packed.data_ptr() if self._packed is not None else None
        _lib.check(lib.dcnr_cosine_neighbor_table(self._table.data_ptr(), self._inv.data_ptr(), packed,
                                                  N, d, kt, 0, N, table.data_ptr(), None, ws.data_ptr(),
                                                  ws.numel(), _lib.stream_ptr(self.device)),
                   "dcnr_cosine_neighbor_table")

    def _update_table(self, r, table, want_counts, events=None, merge=True):
        """One native update of the sorted rows r (norms and packed rows
        already new): filter and merge, the one wait, the re-search.  Returns
        the four counts (the pinned mirror's) when asked.  ``events``: two
        torch events, recorded behind the first call and behind the second
        (tools/bench_neighbor_update.py).  ``merge=False``: no merge -- every
        row the filter finds is searched again (dcnr_cosine_neighbor_table_affected)."""
        lib = _lib.load()
        N, d = self._table.shape
        kt, m = table.shape[1], int(r.size)
        changed = np.ascontiguousarray(r, dtype=np.int32)
        nb = int(lib.dcnr_cosine_neighbor_table_update_workspace_size(N, d, kt, m))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=self.device)
        counts = torch.empty(4, dtype=torch.int32, device=self.device)
        research = torch.empty(N, dtype=torch.int32, device=self.device)
        if self._pin is None:
            self._pin = torch.zeros(4, dtype=torch.int32).pin_memory()
        packed = self._packed.data_ptr() if self._packed is not None else None
        stream = _lib.stream_ptr(self.device)
        first = lib.dcnr_cosine_neighbor_table_update if merge else lib.dcnr_cosine_neighbor_table_affected
        _lib.check(first(
            self._table.data_ptr(), self._inv.data_ptr(), packed, N, d, kt, changed.ctypes.data, m,
            table.data_ptr(), counts.data_ptr(), self._pin.data_ptr(), research.data_ptr(), ws.data_ptr(),
            ws.numel(), stream), "dcnr_cosine_neighbor_table_update" if merge else
            "dcnr_cosine_neighbor_table_affected")
        if events:
            events[0].record()
        torch.cuda.current_stream(self.device).synchronize()   # the update's one wait
        c = self._pin.tolist()
        _lib.check(lib.dcnr_cosine_neighbor_table_rows(
            self._table.data_ptr(), self._inv.data_ptr(), packed, N, d, kt, research.data_ptr(), c[3],
            table.data_ptr(), ws.data_ptr(), ws.numel(), stream), "dcnr_cosine_neighbor_table_rows")
        if events:
            events[1].record()
        return c if want_counts else None

    def kneighbors(self, X=None, n_neighbors=None, return_distance=True, within=None):
        """sklearn's ``kneighbors``.  ``within`` (an iterable of rows of the
        index; not in sklearn) restricts the search to those rows for every
        query: the answer is what an index fitted on ``table[sorted rows]``
        returns, as rows of this index.  The rows are validated (one outside
        the index raises ``ValueError``), sorted and de-duplicated here.
        Unlike sklearn, ``n_neighbors`` above the set's size is no error: the
        lists come back padded with row -1 at distance inf."""
        k = self.n_neighbors if n_neighbors is None else int(n_neighbors)
        if k <= 0:
            raise ValueError(f"Expected n_neighbors > 0. Got {k}")
        q = torch.as_tensor(np.asarray(X, dtype=np.float32)) if not torch.is_tensor(X) else X
        if q.shape[0] == 0:   # sklearn's check_array
            raise ValueError(f"Found array with 0 sample(s) (shape={tuple(q.shape)}) while a minimum "
                             "of 1 is required by NearestNeighbors.")
        if within is not None:
            if self._table is None:
                raise RuntimeError("This NearestNeighbors instance is not fitted yet")
            rows = self._within_rows(within)
            Q = int(q.reshape(-1, self._table.shape[1]).shape[0])
            i64 = lambda a: torch.tensor(a, dtype=torch.int64, device=self.device)
            dist, idx = self.kneighbors_within_device(
                q, k, torch.from_numpy(rows).to(self.device), i64([0, rows.size]), i64([0, Q]),
                torch.zeros(1, dtype=torch.int32, device=self.device), int(rows.size))
            dist = dist.cpu().numpy()
            dist[dist == np.finfo(np.float32).max] = np.inf
            return (dist, idx.cpu().numpy()) if return_distance else idx.cpu().numpy()
        dist, idx = self.kneighbors_device(q, k)
        idx_np = idx.cpu().numpy()
        if return_distance:
            return dist.cpu().numpy(), idx_np
        return idx_np


def _add_counts(stats, c):
    """The four count words of one native update, added to the stats."""
    stats["affected"] += c[1]
    stats["merged"] += c[2]
    stats["researched"] += c[3]


def rebuild_is_cheaper(m: int, kt: int, N: int) -> bool:
    """update_rows' fallback point, in pair distances against the rebuild's
    N^2.  About m (kt + 1) rows are searched again as the build searches them
    (the changed rows and the lists a changed row left a hole in: m N (kt + 1)
    pairs).  Before that the merge takes m distances for each of about
    2 m (kt + 1) affected rows, at 29 times the scan's cost per pair
    (measured at 1M x 64, k = 11: 47.5 ms at m = 16384 against the rebuild's
    254 ms) -- counted above m = 1024, under which the
    merge stays below a millisecond.  The rebuild runs when the estimate
    reaches half of it: m >= 19.5 k at 1M rows, k = 11 (measured there: the
    update is 2.9 times faster than the rebuild at m = 16384, one native
    call's limit; the model puts the crossover near 30 k)."""
    pairs = m * N * (kt + 1)
    if m > 1024:
        pairs += 58 * (kt + 1) * m * m
    return 2 * pairs >= N * N


def index_shard(n: int, rank: int, world: int):
    """Rows [lo, hi) of an n-row index held by ``rank``: balanced, covering
    every row (unlike parallel.shard_range, which trims a batch)."""
    if world < 1 or not (0 <= rank < world):
        raise ValueError("bad rank/world")
    return n * rank // world, n * (rank + 1) // world


class ShardedNearestNeighbors:
    """The cosine index row-sharded over a process group (SURVEY.md 8(e),
    cfg5): rank r holds rows ``index_shard(N, r, world)`` of the table, scans
    only those (``dcnr_cosine_topk``), and the ranks' k-lists -- global row
    ids -- are all-gathered (world * Q * k candidates, one exchange step) and
    merged on the device by ``dcnr_topk_merge``.  Every rank returns exactly
    what ``NearestNeighbors`` over the whole table returns, ties included
    (ascending (dist, row)); the per-row distance does not depend on which
    rank computes it.  Same ``kneighbors`` contract as the single index
    (main.py:200, 300); every rank must call with the same queries."""

    def __init__(self, n_neighbors=5, metric='cosine', algorithm='brute', device='cuda',
                 group=None):
        import torch.distributed as dist
        self._local = NearestNeighbors(n_neighbors, metric, algorithm, device)
        self.n_neighbors = n_neighbors
        self.device = self._local.device
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.lo = self.hi = 0
        self.n_samples_fit_ = None

    def fit(self, X, y=None):
        """X: the whole table (every rank passes the same one; only the
        rank's rows are copied to the device)."""
        n = X.shape[0]
        if n < self.world:
            raise ValueError(f"{n} rows cannot be split over {self.world} ranks")
        self.lo, self.hi = index_shard(n, self.rank, self.world)
        self._local.fit(X[self.lo:self.hi])
        self.n_samples_fit_ = n
        self.n_features_in_ = X.shape[1]
        return self

    def kneighbors_device(self, q: torch.Tensor, k: int):
        import torch.distributed as dist
        if self.n_samples_fit_ is None:
            raise RuntimeError("This ShardedNearestNeighbors instance is not fitted yet")
        if k > self.n_samples_fit_:
            raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, "
                             f"n_samples_fit = {self.n_samples_fit_}")
        q = q.to(self.device, torch.float32).reshape(-1, self.n_features_in_).contiguous()
        Q = q.shape[0]
        kl = min(k, self.hi - self.lo)
        d_loc, i_loc = self._local.kneighbors_device(q, kl)
        dl = torch.full((Q, k), torch.finfo(torch.float32).max, dtype=torch.float32,
                        device=self.device)
        il = torch.full((Q, k), -1, dtype=torch.int64, device=self.device)
        dl[:, :kl] = d_loc
        il[:, :kl] = i_loc + self.lo
        dg = [torch.empty_like(dl) for _ in range(self.world)]
        ig = [torch.empty_like(il) for _ in range(self.world)]
        dist.all_gather(dg, dl, group=self.group)
        dist.all_gather(ig, il, group=self.group)
        dall = torch.stack(dg).contiguous()
        iall = torch.stack(ig).contiguous()
        idx = torch.empty((Q, k), dtype=torch.int64, device=self.device)
        dd = torch.empty((Q, k), dtype=torch.float32, device=self.device)
        lib = _lib.load()
        _lib.check(lib.dcnr_topk_merge(dall.data_ptr(), iall.data_ptr(), self.world, Q, k,
                                       idx.data_ptr(), dd.data_ptr(),
                                       _lib.stream_ptr(self.device)), "dcnr_topk_merge")
        return dd, idx

    def kneighbors(self, X=None, n_neighbors=None, return_distance=True):
        k = self.n_neighbors if n_neighbors is None else int(n_neighbors)
        if k <= 0:
            raise ValueError(f"Expected n_neighbors > 0. Got {k}")
        q = torch.as_tensor(np.asarray(X, dtype=np.float32)) if not torch.is_tensor(X) else X
        if q.shape[0] == 0:   # sklearn's check_array
            raise ValueError(f"Found array with 0 sample(s) (shape={tuple(q.shape)}) while a minimum "
                             "of 1 is required by NearestNeighbors.")
        dist_, idx = self.kneighbors_device(q, k)
        idx_np = idx.cpu().numpy()
        if return_distance:
            return dist_.cpu().numpy(), idx_np
        return idx_np
