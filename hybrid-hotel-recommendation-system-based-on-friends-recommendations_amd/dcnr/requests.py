"""A batch of /recommendations requests: what ``RankingPipeline``'s batched
entry points (``recommend_many``, ``lambda_sweep``, ``recommend_users``) share.
``pack_requests`` is the host half on plain values (no pipeline, no device):
it validates the rows and lays out the arrays to upload.  ``_RequestBatch`` is
the device half as one sequence: one pinned upload, candidates, the call's one
wait, forward, rank + MMR, and the answers with the host's spliced in.

A request whose bound ``need`` = positives * k + fallback rows exceeds SV_MAX
cannot be promised to fit the one-workgroup kernels.  ``pack_requests`` marks
those (``large``); a caller that opts in (``large_lane_split``, then
``_RequestBatch(large=...)``) has them answered by the large lane
(csrc/serving_large.hip) in the same pass: its candidates are launched behind
the small lane's, from the same neighbour source, its mirrors are read at the
same wait, and it is scored by a forward of its own, so the small lane's
answers keep the bits they have without it."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

SV_MAX = 4096   # csrc/serving.hip: candidates per union / rank / MMR call
REQ_OVERFLOW, REQ_BAD_DATA = 1, 2   # DCNR_REQ_* status bits of the batched calls


def _row_set(rows, n_rows, what) -> np.ndarray:
    """A row set as the kernels read it: int64, ascending, distinct, inside the table."""
    if torch.is_tensor(rows):
        rows = rows.cpu().numpy()
    a = np.unique(np.asarray(list(rows) if not isinstance(rows, np.ndarray) else rows,
                             dtype=np.int64).reshape(-1))
    if a.size and (a[0] < 0 or a[-1] >= n_rows):
        raise ValueError(f"{what}: row outside [0, {n_rows})")
    return a


def set_entries(entries, n_reg, first_adhoc, n_rows, adhoc, name, sep):
    """Set arguments (each None, a ``register_sets`` index or an iterable of
    rows) as int32 indices into one CSR, -1 for None: a registered set is its
    own index, the others are appended to ``adhoc`` as row sets and stand from
    ``first_adhoc`` on.  ``name`` (formatted with the entry's place ``r``) and
    ``sep`` word the ValueErrors."""
    idx = np.full(len(entries), -1, np.int32)
    for r, e in enumerate(entries):
        if e is None:
            continue
        if isinstance(e, (int, np.integer)):
            if not 0 <= e < n_reg:
                raise ValueError(f"{name.format(r=r)}{sep}{e} is not a registered set")
            idx[r] = e
        else:
            adhoc.append(_row_set(e, n_rows, name.format(r=r)))
            idx[r] = first_adhoc + len(adhoc) - 1
    return idx


def rounds_to_one(lam64, lam32):
    """recommend() decides "lambda < 1" on the Python double and computes with
    its float32: a lambda that rounds to 1.0f from below would take its MMR
    branch where the batched kernels would not, so it goes the one-request way."""
    return (lam64 < 1.0) != (lam32 < 1.0)


class PackedRequests:
    """What ``pack_requests`` lays out.  ``arrays``: the named arrays to
    upload, in order; ``pos``, ``pos_off``, ``lam`` (float32), ``topk``: those
    of them the host reads again; ``lam64``; ``odd``: the requests whose lambda
    ``rounds_to_one``; ``cap``: the longest candidate list's bound.  ``S`` sets
    stand in the CSR the set indices name (0: nothing about sets is uploaded),
    its last ``n_adhoc`` rows this call's own.  ``within_*``: None unless some
    request names a set for its neighbours.  ``need`` [R]: every request's
    bound, its staged list plus its fallback set's rows (``fallback_len`` [R],
    0 where it names none); ``large``: the requests (ascending int32) whose
    bound exceeds SV_MAX -- the others can never overflow."""
    S = n_adhoc = 0
    within_idx = within_longest = within_any_global = None


def pack_requests(users, positive_rows, lambda_param, top_k, allowed, excluded, fallback,
                  neighbors_within=None, *, n_users, n_rows, k, reg_off, city=None):
    """The host half of ``recommend_many``: validates the rows (ValueError) and
    returns the ``PackedRequests``.  Without set arguments nothing about sets
    is built or uploaded (the index arrays go as null: no filters).

    n_users, n_rows, k   the user table's and the hotel tables' rows, n_neighbors
    reg_off   the registered sets' host offsets [n_reg + 1]
    city      None, or (host_offsets, n_cities, the R codes, neighbors_in_city)
              of a city generation: its 2C + 1 sets stand behind the registered
              ones, in front of the per-call ones"""
    # (few numpy calls: at R = 1 this host work is latency the device waits for.
    # A row read as unsigned is in range iff it is below the table's length)
    R = users.size
    if users.view(np.uint64).max() >= n_users:
        raise ValueError(f"recommend_many: user row outside [0, {n_users})")
    pos = [np.asarray(p.cpu() if torch.is_tensor(p) else p, dtype=np.int64).reshape(-1)
           for p in positive_rows]
    lens = [p.size for p in pos]
    pos_off = np.zeros(R + 1, np.int64)
    if R == 1:
        pos_all, pos_off[1] = pos[0], lens[0]
    else:
        pos_all = np.concatenate(pos)
        np.cumsum(lens, out=pos_off[1:])
    if pos_all.size and pos_all.view(np.uint64).max() >= n_rows:
        raise ValueError(f"recommend_many: positive row outside [0, {n_rows})")
    lam64 = np.full(R, lambda_param, np.float64) if np.isscalar(lambda_param) else \
        np.array(lambda_param, np.float64).reshape(R)
    lam = lam64.astype(np.float32)   # what the kernels (and dcnr_mmr_rerank) compute with
    topk = np.full(R, top_k, np.int32) if np.isscalar(top_k) else \
        np.array(top_k, np.int32).reshape(R)
    if (top_k if np.isscalar(top_k) else topk.min()) < 1:
        raise ValueError("recommend_many: top_k must be at least 1")
    p = PackedRequests()
    p.arrays = dict(pos=pos_all, pos_off=pos_off, users=users, lam=lam, topk=topk)
    p.pos, p.pos_off, p.lam, p.lam64, p.topk = pos_all, pos_off, lam, lam64, topk
    p.odd = rounds_to_one(lam64, lam)
    need = np.array(lens, np.int64) * k   # a request's slot: its staged list (+ its fallback set)
    idx = None
    if allowed is not None or excluded is not None or fallback is not None or \
            neighbors_within is not None or city is not None:
        # registered sets by index, per-call ones appended to the CSR
        n_reg = reg_off.size - 1
        if city is not None:   # the generation's sets between the two
            reg_off = np.concatenate([reg_off, reg_off[-1] + city[0][1:]])
        adhoc = []

        def set_indices(entries, what):
            if entries is None:
                return np.full(R, -1, np.int32)
            if len(entries) != R:
                raise ValueError(f"recommend_many: {what} needs one entry per request")
            return set_entries(entries, n_reg, reg_off.size - 1, n_rows, adhoc,
                               f"recommend_many: {what}[{{r}}]", " = ")

        idx = [set_indices(allowed, "allowed"), set_indices(excluded, "excluded"),
               set_indices(fallback, "fallback"), set_indices(neighbors_within, "neighbors_within")]
        if city is not None:
            _, C, codes, in_city = city
            known = codes >= 0
            idx[0] = (n_reg + np.where(known, codes, 2 * C)).astype(np.int32)
            idx[2] = (n_reg + np.where(known, C + codes, 2 * C)).astype(np.int32)
            if in_city:
                idx[3] = idx[0].copy()
    # lists whose entries are all None name no set: nothing about sets is uploaded
    if idx is not None and max(i.max() for i in idx) >= 0:
        a_idx, e_idx, f_idx, w_idx = idx
        adhoc_rows = np.concatenate(adhoc) if adhoc else np.zeros(0, np.int64)
        set_off = np.concatenate([reg_off, reg_off[-1] + np.cumsum([a.size for a in adhoc],
                                                                     dtype=np.int64)])
        set_len = np.append(np.diff(set_off), 0)   # [-1] = 0: no fallback named
        need = need + set_len[f_idx]
        p.arrays.update(set_off=set_off, adhoc_rows=adhoc_rows, allowed=a_idx, excluded=e_idx,
                        fallback=f_idx)
        p.S, p.n_adhoc = set_off.size - 1, adhoc_rows.size
        if w_idx.max() >= 0:   # (else the neighbour step is the global one, untouched)
            p.arrays["within"] = w_idx
            p.within_idx = w_idx
            p.within_longest = int(set_len[w_idx[w_idx >= 0]].max())
            p.within_any_global = bool(((w_idx < 0) & (np.array(lens) > 0)).any())
    p.cap = int(min(SV_MAX, max(1, int(need.max()))))
    p.need = need
    p.fallback_len = need - np.array(lens, np.int64) * k
    p.large = np.flatnonzero(need > SV_MAX).astype(np.int32)
    return p


def large_lane_split(p, budget):
    """Which of the packed requests ``p`` the large lane answers under a budget
    of ``budget`` staged entries: (lanes, on_host), request indices ascending.
    The large requests are taken in request order while the sum of their
    bounds stays within the budget; one that does not fit, and one whose lambda
    ``rounds_to_one``, is answered on the host (``recommend()``: never
    truncated).  With ``lanes``: ``stage_off`` [L + 1], the bounds' offsets."""
    lanes, host, total = [], [], 0
    for r in p.large.tolist():
        if p.odd[r] or total + int(p.need[r]) > budget:
            host.append(r)
        else:
            lanes.append(r)
            total += int(p.need[r])
    lanes = np.array(lanes, np.int32)
    stage_off = np.zeros(lanes.size + 1, np.int64)
    np.cumsum(p.need[lanes], out=stage_off[1:])
    return lanes, np.array(host, np.int32), stage_off


class _RequestBatch:
    """One batched call's device half, the same sequence for every entry point.
    The constructor stages ``arrays`` in the thread's pinned buffer and uploads
    them in one non-blocking copy; behind them in the pinned buffer stand the
    device's mirrors (the request offsets and the candidate status; with
    ``sources`` the source counts and status too) and, from ``self.tail`` on,
    ``tail`` free bytes.  Then ``candidates``, ``wait`` -- the call's ONE wait,
    after which ``seg`` [R + 1] (the requests' offsets among the ``n``
    candidates) and ``st`` [R] (the status words, or-ed) are known --,
    ``score``, ``rank_mmr`` and ``answers``.  ``what`` names the entry point to
    a caller whose batch the device rejects.  Device words, [R] each: count,
    status, out_count; with ``sources`` src_count [2 R], src_status, by_status.

    ``large``: None, or (lanes, stage_off) of ``large_lane_split`` with at
    least one lane: ``arrays`` then carries ``large_req`` (the lanes),
    ``large_stage_off``, ``large_lam`` and ``large_topk`` (the lanes' lambdas
    and top_k), and the large lane runs beside every step: its candidates in
    ``candidates``, its mirrors (``lseg`` [L + 1], ``ln``) read in ``wait``,
    then ``large_score`` and ``large_rank_mmr``."""

    def __init__(self, pipe, what, R, arrays, sources=False, tail=0, large=None):
        self.pipe, self.what, self.R, self.sources = pipe, what, R, sources
        self.large = large
        self.L = L = 0 if large is None else int(large[0].size)
        self.dev = dev = pipe.device
        at, total = {}, 0
        for name, a in arrays.items():
            at[name] = total
            total += (a.nbytes + 7) & ~7
        pad = (4 * R + 7) & ~7
        self._o_off, self._o_st = total, total + 8 * (R + 1)
        self._o_cnt = self._o_st + pad           # (the two mirrors of ``sources``)
        self._o_sst = self._o_cnt + 8 * R
        self.tail = self._o_sst + pad if sources else self._o_cnt
        if L:   # the large lane's mirrors: offsets [L + 1], status [L]
            self._o_loff = self.tail
            self._o_lst = self._o_loff + 8 * (L + 1)
            self.tail = self._o_lst + ((4 * L + 7) & ~7)
        self.pin, self.host = pin, host = pipe._pinned(self.tail + tail)
        for name, a in arrays.items():
            host[at[name]:at[name] + a.nbytes] = a.view(np.uint8)
        self._dbuf = pin[:total].to(dev, non_blocking=True)
        self._at, self._base, self._pin = at, self._dbuf.data_ptr(), pin.data_ptr()
        self.pin_src_count, self.pin_src_status = self._pin + self._o_cnt, self._pin + self._o_sst
        self.stream = _lib.stream_ptr(dev)
        self._words = torch.empty((7 if sources else 3) * R, dtype=torch.int32, device=dev)
        (self.count, self.status, self.out_count, self.src_count, _, self.src_status,
         self.by_status) = (self._words.data_ptr() + 4 * R * j for j in range(7))   # (3: no sources)

    def ptr(self, name):
        """The uploaded array's device address, None for one that did not travel."""
        return self._base + self._at[name] if name in self._at else None

    def view(self, name, n, dtype):
        """The first n elements of an uploaded array as a device tensor."""
        o = self._at[name]
        return self._dbuf[o:o + n * dtype.itemsize].view(dtype)

    def set_rows(self, reg_rows, n_adhoc, extra=0):
        """The call's set CSR rows on the device: ``reg_rows``, the uploaded
        per-call sets' behind them, then room for ``extra`` more."""
        parts = [reg_rows]
        if n_adhoc:
            parts.append(self.view("adhoc_rows", n_adhoc, torch.int64))
        if extra:
            parts.append(torch.empty(extra, dtype=torch.int64, device=self.dev))
        return torch.cat(parts) if len(parts) > 1 else reg_rows

    def candidates(self, d_pos, set_rows, S, min_candidates, cap, within=None):
        """Every request's candidates, at most ``cap`` each, from the positives ``d_pos``
        (on the device, segmented by the uploaded ``pos_off``) and the uploaded set
        indices into the ``S`` sets of ``set_rows``.  ``within``: None, or (the longest set
        a request seeks its neighbours in, whether a request with positives names none)."""
        pipe, R, Q = self.pipe, self.R, d_pos.numel()
        self.Q, self.cap = Q, cap
        self.slots = torch.empty((R, cap), dtype=torch.int64, device=self.dev)
        self.offsets = torch.empty(R + 1, dtype=torch.int64, device=self.dev)
        if within is not None:
            within = (set_rows, self.view("set_off", S + 1, torch.int64),
                      self.view("pos_off", R + 1, torch.int64),
                      self.view("within", R, torch.int32)) + tuple(within)
        sets = (set_rows.data_ptr() if set_rows.numel() else None, set_rows.numel(),
                self.ptr("set_off"), S, self.ptr("allowed"), self.ptr("excluded"), self.ptr("fallback"),
                int(min_candidates), pipe.n_rows)
        idx = pipe._requests_candidates(
            d_pos.data_ptr() if Q else None, d_pos, self.ptr("pos_off"), R, Q, *sets, cap,
            self.slots.data_ptr(), self.count, self.status,
            self.offsets.data_ptr(), self._pin + self._o_off, self._pin + self._o_st, self.stream,
            within=within)
        if self.L:
            self._large_candidates(d_pos, idx, sets)

    def _large_candidates(self, d_pos, idx, sets):
        """The large lane's candidates, launched behind the small lane's from the neighbour
        source that call read: ``idx`` (the top-k lists or the set-scoped overlay), or the
        pipeline's neighbour table where ``idx`` is None."""
        pipe, L, dev = self.pipe, self.L, self.dev
        n = self.ln_staged = int(self.large[1][-1])
        lib = _lib.load()
        self._lnb = int(lib.dcnr_requests_large_workspace_size(L, n))
        self._lws = torch.empty(self._lnb, dtype=torch.uint8, device=dev)
        self.lrows = torch.empty(n, dtype=torch.int64, device=dev)
        self.loffsets = torch.empty(L + 1, dtype=torch.int64, device=dev)
        self._lwords = torch.empty(3 * L, dtype=torch.int32, device=dev)
        self.lcount, self.lstatus, self.lout_count = (self._lwords.data_ptr() + 4 * L * j
                                                      for j in range(3))
        nbr = pipe._nbr if idx is None else None
        _lib.check(lib.dcnr_requests_large_candidates(
            d_pos.data_ptr() if self.Q else None, self.ptr("pos_off"), self.R, self.Q,
            None if idx is None else idx.data_ptr(), None if nbr is None else nbr.data_ptr(),
            0 if nbr is None else nbr.shape[1], pipe.n_neighbors, *sets, self.ptr("large_req"),
            self.ptr("large_stage_off"), L, n, self.lrows.data_ptr(), self.lcount, self.lstatus,
            self.loffsets.data_ptr(), self._pin + self._o_loff, self._pin + self._o_lst,
            self._lws.data_ptr(), self._lnb, self.stream), "dcnr_requests_large_candidates")

    def wait(self):
        """The rank workspace (allocated while the device works), the wait, the mirrors read."""
        R, host, dev = self.R, self.host, self.dev
        self._nb = int(_lib.load().dcnr_requests_workspace_size(R, self.Q, self.pipe.n_neighbors,
                                                                self.cap))
        self._ws = torch.empty(self._nb, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()   # the call's one wait
        self.seg = host[self._o_off:self._o_st].view(np.int64)
        self.n = int(self.seg[R])
        self.st = host[self._o_st:self._o_st + 4 * R].view(np.int32)
        if self.sources:
            self.src_counts = host[self._o_cnt:self._o_sst].view(np.int32).reshape(R, 2)
            self.st = self.st | host[self._o_sst:self._o_sst + 4 * R].view(np.int32)
        if self.L:
            self.lseg = host[self._o_loff:self._o_lst].view(np.int64)
            self.ln = int(self.lseg[self.L])
            lst = host[self._o_lst:self._o_lst + 4 * self.L].view(np.int32)
            if lst.any():
                raise RuntimeError(f"{self.what}: the device rejected validated input")
        if (self.st & REQ_BAD_DATA).any():
            raise RuntimeError(f"{self.what}: the device rejected validated input")

    def score(self):
        """The ranking batch of the n candidates and one forward: logits [n]."""
        pipe, n = self.pipe, self.n
        if not n:   # nothing is launched
            return torch.empty(0, dtype=torch.float32, device=self.dev)
        batch, args = pipe._ranking_outputs(n)
        _lib.check(_lib.load().dcnr_requests_ranking_batch(
            self.slots.data_ptr(), self.cap, self.offsets.data_ptr(), self.R, n, self.ptr("users"),
            *args, self.stream), "dcnr_requests_ranking_batch")
        return pipe.model(*batch).reshape(-1).to(torch.float32).contiguous()

    def rank_mmr(self, logits, lam_ptr, count_ptr):
        """Rank + MMR of every segment of ``logits`` (read only) under the lambdas [R] at
        ``lam_ptr`` -> (rows, logits) [n], their lengths to ``count_ptr`` (n = 0: no launch)."""
        n, table, inv = self.n, self.pipe.index._table, self.pipe.index._inv
        out_rows = torch.empty(n, dtype=torch.int64, device=self.dev)
        out_logits = torch.empty(n, dtype=torch.float32, device=self.dev)
        if n:
            _lib.check(_lib.load().dcnr_requests_rank_mmr(
                logits.data_ptr(), n, self.slots.data_ptr(), self.cap, self.offsets.data_ptr(),
                self.R, table.data_ptr(), inv.data_ptr(), table.shape[1], table.shape[0],
                lam_ptr, self.ptr("topk"), out_rows.data_ptr(), out_logits.data_ptr(),
                count_ptr, self.status, self._ws.data_ptr(), self._nb, self.stream),
                "dcnr_requests_rank_mmr")
        return out_rows, out_logits

    def large_score(self):
        """The ranking batch of the large lane's ln candidates and a forward of its own."""
        pipe, n = self.pipe, self.ln
        if not n:   # nothing is launched
            return torch.empty(0, dtype=torch.float32, device=self.dev)
        batch, args = pipe._ranking_outputs(n)
        _lib.check(_lib.load().dcnr_requests_large_ranking_batch(
            self.lrows.data_ptr(), self.loffsets.data_ptr(), self.L, n, self.ptr("large_req"),
            self.R, self.ptr("users"), *args, self.stream), "dcnr_requests_large_ranking_batch")
        return pipe.model(*batch).reshape(-1).to(torch.float32).contiguous()

    def large_rank_mmr(self, logits):
        """Rank + MMR of the large lane's segments -> {request: (rows, logits)}, views into
        its two result tensors of the lengths ``answer_lengths`` gives the small lane's."""
        n, L = self.ln, self.L
        table, inv = self.pipe.index._table, self.pipe.index._inv
        out_rows = torch.empty(n, dtype=torch.int64, device=self.dev)
        out_logits = torch.empty(n, dtype=torch.float32, device=self.dev)
        if n:
            _lib.check(_lib.load().dcnr_requests_large_rank_mmr(
                logits.data_ptr(), n, self.lrows.data_ptr(), self.loffsets.data_ptr(), L,
                table.data_ptr(), inv.data_ptr(), table.shape[1], table.shape[0],
                self.ptr("large_lam"), self.ptr("large_topk"), out_rows.data_ptr(),
                out_logits.data_ptr(), self.lout_count, self.lstatus, self._lws.data_ptr(),
                self._lnb, self.stream), "dcnr_requests_large_rank_mmr")
        lanes, n_seg = self.large[0], np.diff(self.lseg)
        return {int(r): (out_rows[int(o):int(o) + int(c)], out_logits[int(o):int(o) + int(c)])
                for r, o, c in zip(lanes, self.lseg[:-1], n_seg)}, n_seg

    def answer_lengths(self, lam32, topk):
        """How many items each request's answer holds (one lambda and top_k, or R of each)."""
        n_seg = np.diff(self.seg)
        # every candidate is a table row, so the MMR finds min(top_k, n_seg) items
        return np.where(lam32 < 1.0, np.minimum(topk, n_seg), n_seg)

    def answers(self, out_rows, out_logits, lengths, on_host, host_answer):
        """The R answers: views into (out_rows, out_logits) of ``lengths``
        items, ``host_answer(r)`` for the requests flagged in ``on_host``."""
        def view(r):
            o, c = int(self.seg[r]), int(lengths[r])
            return out_rows[o:o + c], out_logits[o:o + c]
        return [host_answer(r) if on_host[r] else view(r) for r in range(self.R)]
