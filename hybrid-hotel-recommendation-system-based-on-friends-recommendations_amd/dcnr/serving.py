"""The /recommendations and /similar_items scoring core on libdcnr.

Mirrors the reference's serving functions (main.py) with their device work in
HIP kernels (serving.hip, knn.hip, the DCN-R forward):

  rerank_with_mmr(ranked_items_with_scores, lambda_param, top_k=20)
      main.py:133-169, same signature; reads ``ml_artifacts['item_embeddings']``
      and ``ml_artifacts['artifacts']['item_id_mapping']`` like the reference
      (this module's ``ml_artifacts`` dict), greedy MMR in one launch
      (dcnr_mmr_rerank).
  RankingPipeline
      the device-resident request path: cosine neighbours of the positive
      hotels for ALL positives in one batched top-k (main.py:196-203 calls
      kneighbors once per hotel), the candidate union (dcnr_candidate_union),
      the ranking batch of preprocess_for_ranking (main.py:215-230) gathered
      from per-item feature tables (dcnr_ranking_batch), the eval-mode DCN-R
      forward (main.py:319-322), the stable descending sort (main.py:325,
      dcnr_rank_by_score) and MMR (main.py:327-332).

Everything works on internal row indices (the reference's ``item_id_mapping``
values); mapping external ids stays with the caller, as in main.py.  The
pandas filters of _generate_candidates (city, negative reviews, popular-hotel
fill-up, main.py:204-212) are host set operations and take ``allowed`` /
``excluded`` row sets here.

``RankingPipeline.recommend_many`` answers a batch of requests in one device
pass (dcnr_requests_*: one workgroup per request, the filters as binary
searches in row sets kept on the device by ``register_sets``, one forward over
all candidates, one host wait); ``similar_items_many`` is its /similar_items
companion.  The requests of a batch whose bound of candidates exceeds the
one-workgroup kernels' 4096 (SV_MAX) take the large lane of the same pass
(dcnr_requests_large_*, serving_large.hip: grids over the entries, a forward of
their own, the same one wait) up to ``RankingPipeline.large_lane_budget``
staged entries; ``recommend()``'s MMR above SV_MAX ranked candidates is
dcnr_mmr_rerank_large (``mmr_positions_large``).  ``RankingPipeline.recommend_users`` is the same pass from user
ids: the positives, the negatives and the ``recommended_by`` lists (main.py:
172-194, 336-351) come from a ``dcnr.InteractionStore`` on the device
(dcnr_requests_sources, dcnr_requests_recommended_by).  The pass itself (pack,
one pinned upload, candidates, the one wait, forward, rank + MMR, the host's
answers spliced in) is ``dcnr.requests``: ``pack_requests`` and one
``_RequestBatch`` per call, which the three batched entry points feed and read.

``RankingPipeline.list_metrics`` measures answers already served
(``dcnr.list_metrics`` against the pipeline's own table), and
``RankingPipeline.lambda_sweep`` answers one batch for several values of
``lambda_param`` from ONE candidates pass and ONE forward, each lambda's
answers measured on the device where rank + MMR left them.

``RankingPipeline(..., neighbor_table=True)`` builds the item neighbour table
once (``NearestNeighbors.build_neighbor_table``): every neighbour query of the
request path is a row of the fitted table, so ``candidates``, ``recommend``,
``recommend_many``, ``recommend_users``, ``similar_items`` and
``similar_items_many`` then read their neighbours from it and scan nothing;
the answers are the same bits.
"""
from __future__ import annotations

import ctypes
import functools
import threading
from typing import Any, Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .knn import NearestNeighbors
from .requests import (REQ_OVERFLOW, SV_MAX, _RequestBatch, _row_set, large_lane_split, pack_requests,
                       rounds_to_one, set_entries)

ml_artifacts: Dict[str, Any] = {}

def _dev_table(emb, device):
    """(table fp32 [n, d] on device, inverse row norms [n]) cached per source array."""
    cache = ml_artifacts.setdefault('_dcnr_tables', {})
    key = id(emb)
    hit = cache.get(key)
    if hit is not None and hit[0] is emb:
        return hit[1], hit[2]
    t = torch.as_tensor(np.asarray(emb, dtype=np.float32) if not torch.is_tensor(emb) else emb)
    t = t.to(device, torch.float32).contiguous()
    inv = row_inv_norms(t)
    cache[key] = (emb, t, inv)
    return t, inv


def row_inv_norms(t: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    inv = torch.empty(t.shape[0], dtype=torch.float32, device=t.device)
    _lib.check(lib.dcnr_row_inv_norms(t.data_ptr(), t.shape[0], t.shape[1], inv.data_ptr(),
                                      _lib.stream_ptr(t.device)), "dcnr_row_inv_norms")
    return inv


def mmr_positions(table: torch.Tensor, inv: torch.Tensor, rows: torch.Tensor,
                  scores: torch.Tensor, lambda_param: float, top_k: int = 20) -> torch.Tensor:
    """Device MMR over candidates in ranked order: returns int64 positions
    (into the ranked list) of the re-ranked items (dcnr_mmr_rerank).  At most
    SV_MAX candidates (one workgroup's LDS holds every candidate's running
    max-similarity); more raise ValueError."""
    lib = _lib.load()
    dev = table.device
    n = rows.numel()
    if n > SV_MAX:
        raise ValueError(f"mmr_positions: {n} candidates exceed the device MMR's {SV_MAX}")
    out = torch.empty(max(1, top_k), dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    if n == 0:
        return out[:0]
    rows = rows.to(dev, torch.int64).contiguous()
    scores = scores.to(dev, torch.float32).contiguous()
    _lib.check(lib.dcnr_mmr_rerank(table.data_ptr(), inv.data_ptr(), table.shape[1],
                                   rows.data_ptr(), scores.data_ptr(), n, float(lambda_param),
                                   int(top_k), out.data_ptr(), cnt.data_ptr(),
                                   _lib.stream_ptr(dev)), "dcnr_mmr_rerank")
    return out[:int(cnt.item())]


def mmr_positions_large(table: torch.Tensor, inv: torch.Tensor, rows: torch.Tensor,
                        scores: torch.Tensor, lambda_param: float, top_k: int = 20) -> torch.Tensor:
    """``mmr_positions`` for any number of candidates (dcnr_mmr_rerank_large:
    every candidate's running max-similarity lives in a workspace, the
    arithmetic and its order are ``mmr_positions``', so are the picks)."""
    lib = _lib.load()
    dev = table.device
    n = rows.numel()
    out = torch.empty(max(1, top_k), dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    if n == 0:
        return out[:0]
    rows = rows.to(dev, torch.int64).contiguous()
    scores = scores.to(dev, torch.float32).contiguous()
    nb = int(lib.dcnr_mmr_rerank_large_workspace_size(n))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.check(lib.dcnr_mmr_rerank_large(table.data_ptr(), inv.data_ptr(), table.shape[1],
                                         rows.data_ptr(), scores.data_ptr(), n, float(lambda_param),
                                         int(top_k), out.data_ptr(), cnt.data_ptr(), ws.data_ptr(), nb,
                                         _lib.stream_ptr(dev)), "dcnr_mmr_rerank_large")
    return out[:int(cnt.item())]


def rerank_with_mmr(ranked_items_with_scores: List[Tuple[float, int]], lambda_param: float,
                    top_k: int = 20) -> List[int]:
    """main.py:133-169: greedy Maximal Marginal Relevance over (score, item_id)
    pairs given in ranked order; returns the re-ranked item ids."""
    if not ranked_items_with_scores:
        return []
    emb = ml_artifacts['item_embeddings']
    mapping = ml_artifacts['artifacts']['item_id_mapping']
    device = ml_artifacts.get('device', torch.device('cuda'))
    if isinstance(device, str):
        device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError("dcnr.serving runs on the HIP device only")
    table, inv = _dev_table(emb, device)
    ids = [item_id for _, item_id in ranked_items_with_scores]
    rows = torch.tensor([mapping.get(i, -1) if mapping.get(i) is not None else -1 for i in ids],
                        dtype=torch.int64)
    scores = torch.tensor(np.asarray([s for s, _ in ranked_items_with_scores], dtype=np.float32))
    pos = mmr_positions(table, inv, rows, scores, lambda_param, top_k).cpu().tolist()
    return [ids[p] for p in pos]


def _one_generation(fn):
    """A scoring entry point of ``RankingPipeline``: with ``item_features``, the
    outermost call on a thread takes the newest generation once; everything the
    call launches, the entry points it calls included, scores from that one.
    A list it returns keeps the generation (``_features_held``).  A pipeline
    built from arrays goes straight through."""
    @functools.wraps(fn)
    def call(self, *args, **kwargs):
        if self._features is None or getattr(self._tls, "feat", None) is not None:
            return fn(self, *args, **kwargs)
        gen = self._tls.feat = self._features.on(self.device)
        try:
            out = fn(self, *args, **kwargs)
        finally:
            self._tls.feat = None
        if type(out) is list:
            out = Answers(out)
        if isinstance(out, list):
            out._features_held = gen
        return out
    return call


class Answers(list):
    """What ``recommend_many`` returns when a request left the small lane, or
    from a pipeline with ``item_features``: the list of R (ranked rows,
    logits) pairs.  ``large``: the requests (indices, ascending) the large
    lane answered; ``on_host``: those ``recommend()`` answered (both empty
    where every request took the small lane).  From a pipeline with
    ``item_features`` it keeps the feature generation the call scored from."""
    large = ()
    on_host = ()


class UserAnswers(list):
    """What ``RankingPipeline.recommend_users`` returns: a list of R (ranked
    rows, logits) pairs, views into ``rows`` / ``logits`` [n] as
    ``recommend_many``'s are, and the recommended_by lists of every position of
    those two tensors, on the device:

      by_offsets [n + 1], by_reviewers   a CSR over the positions: position i
                   was recommended by by_reviewers[by_offsets[i] : by_offsets[i + 1]]
                   (store reviewer indices, in the reference's order); positions
                   behind a request's answer have empty lists
      by_count [n], lists                the same lists where the host can find
                   them without reading by_offsets: request r's reviewers,
                   position by position, from lists[list offset of r] on

    ``to_lists(r)`` turns answer r into Python lists with one copy to the
    host.  A request that was answered on the host (``on_host[r]``) has no
    positions in the tensors; ``to_lists`` serves it from the store's host
    copies.  ``n_positives`` / ``positives_bound``: per request the distinct
    positives the device found and the padded length they were searched at."""

    def to_lists(self, r: int):
        """(hotel rows, logits, recommended_by lists) of answer r."""
        rows, logits = self[r]
        if self.on_host[r]:
            rows = rows.cpu()
            return (rows.tolist(), logits.cpu().tolist(),
                    self._store.recommended_by_host(int(self._rv[r]), rows))
        o, c = int(self._seg[r]), int(self._cnt[r])
        l0, l1 = int(self._list_off[r]), int(self._list_off[r + 1])
        pack = torch.cat([rows, logits.view(torch.int32).to(torch.int64),
                          self.by_count[o:o + c].to(torch.int64),
                          self.lists[l0:l1].to(torch.int64)]).cpu().numpy()
        ends = np.cumsum(pack[2 * c:3 * c])
        who = pack[3 * c:]
        by = [who[e - m:e].tolist() for e, m in zip(ends, pack[2 * c:3 * c])]
        return (pack[:c].tolist(), pack[c:2 * c].astype(np.int32).view(np.float32).tolist(), by)


class SweepResult(list):
    """What ``RankingPipeline.lambda_sweep`` returns: a list of (answers,
    ListMetrics) pairs, one per lambda of ``lambdas``; ``skipped``: the
    request indices left out of every lambda's lists and metrics."""
    lambdas = ()
    skipped = ()


class RankingPipeline:
    """Device-resident request path of /recommendations and /similar_items.

    model      dcnr.DCN_RecSys (eval mode is set here), on the HIP device
    item_embeddings  [n_items, d] (the exported item_embedding weights,
               train.py:393-394); default: the model's own item table
    item_cat   int64 [n_items, n_cat]: each hotel's encoded categorical codes
    item_num   fp32 [n_items, n_num]: each hotel's scaled numeric features
    item_features  a ``dcnr.ItemFeatures`` in place of the two arrays (give the
               pair or this; anything else is a ValueError, as are widths that
               do not fit the model): the tables then follow the object's
               ``append`` / ``remove`` / ``set_values`` / ``set_scaler``.  Every
               scoring entry point (``ranking_batch``, ``score``, ``recommend``,
               ``recommend_many``, ``recommend_users``, ``lambda_sweep``) takes
               ``item_features.on(device)`` once when it is entered and scores
               every launch of the call from that one generation -- the
               requests a batched call answers through ``recommend()``
               included -- and the batched calls' answers keep it alive.
               ``item_cat`` / ``item_num`` read the newest generation.
               Serialise the object's changes against requests
    large_lane_budget  (attribute, default 2^20) the staged entries --
               positives * n_neighbors + fallback rows, summed over a batch's
               large requests -- ``recommend_many``'s large lane takes in one
               call; large requests past it are answered by ``recommend()``.
               The lane's workspace is 49 bytes and its candidate buffer 8
               bytes per staged entry: 57 MiB at the default
    neighbor_table  False: every request scans the index.  True: the item
               neighbour table is built here with k = n_neighbors; an int:
               with that k (>= n_neighbors; /similar_items reads it up to
               n = k - 1); an int32 array or tensor [n_items, kt]: a table built
               before (``build_neighbor_table``, ``load_artifacts``) is adopted.
               ValueError for a table of another shape or kt < n_neighbors.
    """

    def __init__(self, model, item_cat=None, item_num=None, item_embeddings=None,
                 n_neighbors: int = 11, neighbor_table=False, item_features=None):
        dev = model.final_linear.weight.device
        if dev.type != 'cuda':
            raise RuntimeError("RankingPipeline runs on the HIP device only")
        self.model = model.eval()
        self.device = dev
        emb = model.item_embedding.weight.detach() if item_embeddings is None else item_embeddings
        self.index = NearestNeighbors(n_neighbors=n_neighbors, metric='cosine',
                                      algorithm='brute', device=dev).fit(emb)
        self._tls = threading.local()
        self._features = item_features
        if item_features is not None:
            if item_cat is not None or item_num is not None:
                raise ValueError("RankingPipeline: give item_cat and item_num, or item_features")
            dims = getattr(model, "_dims", None)
            want = (len(model.cat_embeddings), item_features.n_num if dims is None else dims["n_num"])
            if (item_features.n_cat, item_features.n_num) != want:
                raise ValueError(f"RankingPipeline: item_features holds {item_features.n_cat} "
                                 f"categorical and {item_features.n_num} numeric columns, the model "
                                 f"takes {want[0]} and {want[1]}")
            self._tables = None
            self.n_items = item_features.n_items
        else:
            if item_cat is None or item_num is None:
                raise ValueError("RankingPipeline: give item_cat and item_num, or item_features")
            self._tables = (torch.as_tensor(item_cat).to(dev, torch.int64).contiguous(),
                            torch.as_tensor(item_num).to(dev, torch.float32).contiguous())
            self.n_items = self._tables[0].shape[0]
            if self._tables[1].shape[0] != self.n_items:
                raise ValueError("item_cat and item_num must have one row per item")
        self.n_neighbors = n_neighbors
        # hotel rows every table holds (index, item_cat, item_num): what a
        # batched request may name
        self.n_rows = min(self.n_items, self.index._table.shape[0])
        # register_sets: (rows on the device, host offsets [S + 1]); replaced
        # as a whole, so a call in flight keeps the pair it started with
        self._no_rows = torch.empty(0, dtype=torch.int64, device=dev)
        self._sets = (self._no_rows, np.zeros(1, np.int64))
        self._sets_lock = threading.Lock()
        self._city_joined = None   # (registered rows, CitySets generation, the two joined)
        self._nbr = self._neighbor_table(neighbor_table)
        self.large_lane_budget = 1 << 20

    def _feature_tables(self):
        """(item_cat, item_num) this call scores from: the arrays the pipeline
        was built from, or the ``ItemFeatures`` generation the entry point
        took (outside one: the newest)."""
        if self._tables is not None:
            return self._tables
        gen = getattr(self._tls, "feat", None) or self._features.on(self.device)
        return gen.item_cat, gen.item_num

    item_cat = property(lambda self: self._feature_tables()[0])
    item_num = property(lambda self: self._feature_tables()[1])

    def _neighbor_table(self, arg):
        """The constructor's ``neighbor_table`` as int32 [n_items, kt] on the device, or None."""
        n, k = self.index._table.shape[0], self.n_neighbors
        if arg is None or arg is False:
            return None
        if arg is True or isinstance(arg, (int, np.integer)):
            kt = k if arg is True else int(arg)
            if kt < k:
                raise ValueError(f"neighbor_table: k = {kt} is below n_neighbors = {k}")
            return self.index.build_neighbor_table(kt)
        t = torch.as_tensor(arg)
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != n or t.shape[1] < k:
            raise ValueError(f"neighbor_table: expected int32 [{n}, kt >= {k}], got "
                             f"{str(t.dtype).replace('torch.', '')} {list(t.shape)}")
        return t.to(self.device).contiguous()

    def update_item_embeddings(self, rows, vectors, update_model: bool = True, return_stats=False):
        """New embeddings for some hotels: ``index.update_rows`` on the
        index's table, norms, packed copy and the neighbour table this
        pipeline serves from, all as a pipeline built fresh on the new
        embeddings would hold them.  The index's table IS the model's item
        table when that was fp32 on the device at construction (``fit`` does
        not copy it), and the one write serves both; otherwise, with
        ``update_model``, the same rows of ``model.item_embedding`` are
        written too (a pipeline built on ``item_embeddings`` of another shape
        than the model's table leaves the model alone).  Ordered on the
        current stream; not safe against requests in flight on other
        streams."""
        out = self.index.update_rows(rows, vectors, table=self._nbr, return_stats=return_stats)
        w = self.model.item_embedding.weight
        t = self.index._table
        if update_model and w.data_ptr() != t.data_ptr() and w.shape == t.shape:
            r = torch.as_tensor(np.asarray(rows.cpu() if torch.is_tensor(rows) else rows).reshape(-1),
                                dtype=torch.int64, device=w.device)
            v = torch.as_tensor(np.asarray(vectors, dtype=np.float32)) if not torch.is_tensor(vectors) \
                else vectors
            with torch.no_grad():
                w[r] = v.to(w.device, w.dtype).reshape(-1, w.shape[1])
        return out

    def append_items(self, item_cat=None, item_num=None, item_features=None, return_stats=False):
        """Admit the hotels the model's item table has grown by
        (``model.grow_(n_items=...)`` first): rows [N, N + m) of the model's
        table go through ``index.append_rows`` -- as ``storage`` when the grown
        weight is fp32 on the device, so the index shares the model's table as
        it shared the old one -- and the neighbour table this pipeline serves
        from grows with them, all as a pipeline built fresh on the grown model
        would hold them.  Old rows of the model's table that no longer equal
        the index's (training steps since) are first brought in through
        ``index.update_rows``.  The new hotels' features: ``item_cat`` [m, n_cat]
        and ``item_num`` [m, n_num] for a pipeline built from arrays, or an
        ``ItemFeatures`` built with the new ``n_items``, which replaces the old
        one.  ``n_items`` / ``n_rows`` follow.  Ordered on the current stream;
        not safe against requests in flight on other streams."""
        w = self.model.item_embedding.weight.detach()
        N = int(self.index._table.shape[0])
        m = int(w.shape[0]) - N
        if m < 0 or w.shape[1] != self.index._table.shape[1]:
            raise ValueError(f"append_items: the model's item table {list(w.shape)} does not extend the "
                             f"index's {list(self.index._table.shape)}")
        if self._tables is None:
            if item_features is None or item_cat is not None or item_num is not None:
                raise ValueError("append_items: this pipeline serves from item_features; give the new one")
            if (item_features.n_cat, item_features.n_num) != (self._features.n_cat, self._features.n_num):
                raise ValueError("append_items: item_features has other columns than the one it replaces")
            if item_features.n_items != self.n_items + m:
                raise ValueError(f"append_items: item_features holds {item_features.n_items} hotels, "
                                 f"the grown table {self.n_items + m}")
            tables = None
        else:
            if item_features is not None or item_cat is None or item_num is None:
                raise ValueError("append_items: this pipeline serves from arrays; give the new rows' "
                                 "item_cat and item_num")
            old_cat, old_num = self._tables
            cat = torch.as_tensor(item_cat).to(self.device, torch.int64).reshape(-1, old_cat.shape[1])
            num = torch.as_tensor(item_num).to(self.device, torch.float32).reshape(-1, old_num.shape[1])
            if cat.shape[0] != m or num.shape[0] != m:
                raise ValueError(f"append_items: {m} new hotels, {cat.shape[0]} item_cat and "
                                 f"{num.shape[0]} item_num rows")
            tables = (torch.cat([old_cat, cat]).contiguous(), torch.cat([old_num, num]).contiguous())
        stats = {}
        old = self.index._table
        if w.data_ptr() != old.data_ptr():
            moved = torch.nonzero((w[:N] != old.to(w.dtype)).any(dim=1)).reshape(-1)
            if moved.numel():
                s = self.index.update_rows(moved, w[moved], table=self._nbr, return_stats=return_stats)
                stats["updated"] = s
        shared = w.dtype == torch.float32 and w.device == old.device and w.is_contiguous()
        out = self.index.append_rows(vectors=None if shared else w[N:], storage=w if shared else None,
                                     table=self._nbr, return_stats=return_stats)
        if return_stats:
            out, s = out
            stats.update(s)
        if self._nbr is not None:
            self._nbr = out
        if tables is None:
            self._features = item_features
        else:
            self._tables = tables
        self.n_items += m
        self.n_rows = min(self.n_items, self.index._table.shape[0])
        self._city_joined = None
        return stats if return_stats else None

    # ---------------------------------------------------------- /similar_items
    def similar_items(self, item_row: int, n: int = 10, within=None) -> torch.Tensor:
        """main.py:294-303: the n nearest hotels, the hotel itself dropped
        (kneighbors(n_neighbors=n+1)[1:]).  ``within`` (a ``register_sets``
        index or an iterable of rows): the n nearest rows of that set other
        than the hotel itself, whether or not the hotel is in the set -- fewer
        than n when the set is smaller."""
        if within is not None:
            row = self.similar_items_many([int(item_row)], n, within=[within])[0]
            return row[row >= 0]
        if self._nbr is not None and n + 1 <= self._nbr.shape[1]:
            return self._nbr[int(item_row), 1:n + 1].to(torch.int64)
        q = self.index._table[int(item_row)].reshape(1, -1)
        _, idx = self.index.kneighbors_device(q, n + 1)
        return idx[0, 1:]

    # ------------------------------------------------------- /recommendations
    def candidates(self, positive_rows, within=None) -> torch.Tensor:
        """_generate_candidates' union (main.py:196-203): the positive hotels
        and their n_neighbors-1 nearest neighbours, distinct rows ascending.
        ``within`` (a ``register_sets`` index or an iterable of rows): the
        neighbours are each positive's n_neighbors-1 nearest rows of that set
        other than itself (a scan of the set; the neighbour table, which holds
        global neighbours, is not consulted)."""
        lib = _lib.load()
        pos = torch.as_tensor(positive_rows, dtype=torch.int64).reshape(-1).to(self.device)
        Q = pos.numel()
        if Q == 0:
            return pos
        k = self.n_neighbors
        nbr = self._nbr
        if within is not None:
            nbr = None
            rows, off, w_idx, longest = self._within_csr([within])
            idx = self._within_overlay(pos, None, rows, off,
                                       torch.tensor([0, Q], dtype=torch.int64, device=self.device),
                                       torch.from_numpy(w_idx).to(self.device), longest)
        elif nbr is None:
            _, idx = self.index.kneighbors_device(self.index._table[pos], k)
        qc = max(1, SV_MAX // k)     # the union kernel's one-workgroup capacity
        outs = []
        for q0 in range(0, Q, qc):   # > SV_MAX entries: per-chunk unions, then merged
            p_ = pos[q0:q0 + qc].contiguous()
            out = torch.empty(p_.numel() * k, dtype=torch.int64, device=self.device)
            cnt = torch.zeros(1, dtype=torch.int32, device=self.device)
            if nbr is not None:   # the neighbours looked up, nothing scanned
                _lib.check(lib.dcnr_candidate_union_table(p_.data_ptr(), p_.numel(), nbr.data_ptr(),
                                                          nbr.shape[1], nbr.shape[0], k,
                                                          out.data_ptr(), cnt.data_ptr(),
                                                          _lib.stream_ptr(self.device)),
                           "dcnr_candidate_union_table")
            else:
                i_ = idx[q0:q0 + qc].contiguous()
                _lib.check(lib.dcnr_candidate_union(p_.data_ptr(), p_.numel(), i_.data_ptr(), k,
                                                    out.data_ptr(), cnt.data_ptr(),
                                                    _lib.stream_ptr(self.device)),
                           "dcnr_candidate_union")
            c = int(cnt.item())
            if c < 0:
                raise ValueError("candidates: a positive row or a neighbour table entry lies "
                                 "outside the table")
            outs.append(out[:c])
        if len(outs) == 1:
            return outs[0]
        return torch.unique(torch.cat(outs))   # ascending distinct rows, as one call gives

    def _ranking_outputs(self, n):
        """The model inputs (user ids, item ids, cat, num) of n rows to fill,
        and the arguments both ranking-batch calls end with, item_cat to num
        (a pointer is null where the model has no such column)."""
        item_cat, item_num = self._feature_tables()
        K, F = item_cat.shape[1], item_num.shape[1]
        u = torch.empty(n, dtype=torch.int64, device=self.device)
        i = torch.empty(n, dtype=torch.int64, device=self.device)
        c = torch.empty((n, K), dtype=torch.int64, device=self.device)
        x = torch.empty((n, F), dtype=torch.float32, device=self.device)
        return (u, i, c, x), (item_cat.data_ptr() if K else None, K,
                              item_num.data_ptr() if F else None, F, self.n_items,
                              u.data_ptr(), i.data_ptr(), c.data_ptr() if K else None,
                              x.data_ptr() if F else None)

    @_one_generation
    def ranking_batch(self, user_row: int, item_rows: torch.Tensor):
        """preprocess_for_ranking (main.py:215-230) on the device."""
        lib = _lib.load()
        item_rows = item_rows.to(self.device, torch.int64).contiguous()
        n = item_rows.numel()
        batch, args = self._ranking_outputs(n)
        _lib.check(lib.dcnr_ranking_batch(item_rows.data_ptr(), n, int(user_row), *args,
                                          _lib.stream_ptr(self.device)), "dcnr_ranking_batch")
        return batch

    @_one_generation
    @torch.no_grad()
    def score(self, user_row: int, item_rows: torch.Tensor) -> torch.Tensor:
        """Eval-mode DCN-R logits of (user, hotel) pairs (main.py:319-322)."""
        if item_rows.numel() == 0:
            return torch.empty(0, dtype=torch.float32, device=self.device)
        return self.model(*self.ranking_batch(user_row, item_rows)).reshape(-1)

    def rank(self, scores: torch.Tensor) -> torch.Tensor:
        """Positions in descending score order, ties by position (main.py:325).
        Above SV_MAX candidates (the LDS sort's capacity) a stable device sort
        of -score gives the same order."""
        lib = _lib.load()
        n = scores.numel()
        if n > SV_MAX:
            return torch.sort(-scores.to(self.device, torch.float32), stable=True).indices
        order = torch.empty(n, dtype=torch.int64, device=self.device)
        if n:
            s = scores.to(torch.float32).contiguous()
            _lib.check(lib.dcnr_rank_by_score(s.data_ptr(), n, order.data_ptr(),
                                              _lib.stream_ptr(self.device)), "dcnr_rank_by_score")
        return order

    @_one_generation
    @torch.no_grad()
    def recommend(self, user_row: int, positive_rows, lambda_param: float = 1.0,
                  top_k: int = 20, allowed: Optional[Iterable[int]] = None,
                  excluded: Optional[Iterable[int]] = None,
                  fallback: Optional[Iterable[int]] = None, min_candidates: int = 20,
                  neighbors_within=None):
        """The scoring core of /recommendations (main.py:309-332) on hotel rows:
        candidates -> [fallback] -> [filters] -> ranking batch -> logits ->
        sort -> MMR when lambda_param < 1.  ``fallback`` (the city's most
        reviewed hotels) joins the candidates when fewer than
        ``min_candidates`` were found (main.py:204-207).  Returns (ranked
        rows, their logits) on the device.  ``neighbors_within`` goes to
        ``candidates``: the positives' neighbours are sought inside that set
        (the usual call names the city as ``allowed`` and here)."""
        cand = self.candidates(positive_rows, within=neighbors_within)
        if fallback is not None and cand.numel() < min_candidates:
            extra = torch.as_tensor(list(fallback), dtype=torch.int64).to(self.device)
            cand = torch.unique(torch.cat([cand, extra]))
        if allowed is not None or excluded is not None:   # host set filters (main.py:210-212)
            keep = set(cand.tolist())
            if allowed is not None:
                keep &= set(int(a) for a in allowed)
            if excluded is not None:
                keep -= set(int(e) for e in excluded)
            cand = torch.tensor(sorted(keep), dtype=torch.int64, device=self.device)
        if cand.numel() == 0:   # "No suitable candidates found." (main.py:311-312)
            return cand, torch.empty(0, dtype=torch.float32, device=self.device)
        scores = self.score(user_row, cand)
        order = self.rank(scores)
        ranked, rscores = cand[order], scores[order]
        if lambda_param < 1.0 and ranked.numel():
            mmr = mmr_positions if ranked.numel() <= SV_MAX else mmr_positions_large
            pos = mmr(self.index._table, self.index._inv, ranked, rscores, lambda_param, top_k)
            return ranked[pos], rscores[pos]
        return ranked, rscores

    # ------------------------------------------------- a batch of requests
    def similar_items_many(self, item_rows, n: int = 10, within=None) -> torch.Tensor:
        """R /similar_items queries (main.py:294-303) in one top-k call:
        int64 [R, n], row r what ``similar_items(item_rows[r], n)`` returns.

        ``within``: None; one set for every query (a ``register_sets`` index,
        or rows as an array, tensor, set or range); or a list / tuple of R
        entries, each None, an index or an iterable of rows.  Row r then holds
        the n nearest rows of its set other than the item itself, padded with
        -1 when the set is smaller; entries that are None keep the global
        answer.  One set-scoped kernel call serves all R (queries in a run
        of equal entries share one pass over the set)."""
        rows = np.asarray(item_rows, dtype=np.int64).reshape(-1)
        if rows.size and (rows.min() < 0 or rows.max() >= self.index._table.shape[0]):
            raise ValueError("similar_items_many: item row outside the index")
        if rows.size == 0:
            return torch.empty((0, n), dtype=torch.int64, device=self.device)
        d_rows = torch.from_numpy(rows).to(self.device)
        if within is not None:
            return self._similar_within(d_rows, int(n), within)
        if self._nbr is not None and n + 1 <= self._nbr.shape[1]:
            return self._nbr[d_rows][:, 1:n + 1].to(torch.int64)
        _, idx = self.index.kneighbors_device(self.index._table[d_rows], n + 1)
        return idx[:, 1:]

    def _within_csr(self, entries):
        """Set arguments of the one-request calls (None, a ``register_sets``
        index, an iterable of rows) as one CSR behind the registered sets:
        (rows on the device, offsets int64 on the device, set index per entry
        as int32 with -1 for None, the longest named set)."""
        reg_rows, reg_off = self._sets
        n_reg = reg_off.size - 1
        adhoc = []
        idx = set_entries(entries, n_reg, n_reg, self.n_rows, adhoc, "within", ": ")
        off = np.concatenate([reg_off, reg_off[-1] + np.cumsum([a.size for a in adhoc], dtype=np.int64)])
        rows = reg_rows
        if adhoc:
            rows = torch.cat([reg_rows, torch.from_numpy(np.concatenate(adhoc)).to(self.device)])
        named = idx[idx >= 0]
        longest = int(np.diff(off)[named].max()) if named.size else 0
        return rows, torch.from_numpy(off).to(self.device), idx, longest

    def _within_overlay(self, d_pos, idx, set_rows, set_off, seg_off, seg_set, longest):
        """knn_idx [Q][k] of the candidate kernels with the set-scoped
        neighbours laid over it: column 0 is the positive's place (the kernels
        drop it), columns 1 .. k-1 of every segment that names a set are
        written by dcnr_cosine_topk_within (exclude = the positive itself).
        ``idx``: the global answers of the segments that name none, or None
        when every segment names one."""
        k = self.n_neighbors
        Q = d_pos.numel()
        if idx is None:
            idx = torch.full((Q, k), -1, dtype=torch.int64, device=self.device)
        if k > 1 and Q:
            dist = torch.empty((Q, k), dtype=torch.float32, device=self.device)
            self.index.kneighbors_within_device(self.index._table[d_pos], k - 1, set_rows, set_off, seg_off,
                                                seg_set, longest, exclude=d_pos,
                                                out=(idx[:, 1:], dist[:, 1:]))
        return idx

    def _similar_within(self, d_rows, n, within):
        R = d_rows.numel()
        entries = list(within) if isinstance(within, (list, tuple)) else [within] * R
        if len(entries) != R:
            raise ValueError("similar_items_many: within needs one entry per item row (a list or "
                             "tuple), or one set for all")
        # equal entries share one CSR slot; runs of them one segment
        slot, uniq = {}, []
        for e in entries:
            key = id(e) if not isinstance(e, (int, np.integer, type(None))) else ("i", e)
            if key not in slot:
                slot[key] = len(uniq)
                uniq.append(e)
        rows, off, u_idx, longest = self._within_csr(uniq)
        per = np.array([u_idx[slot[id(e) if not isinstance(e, (int, np.integer, type(None))) else ("i", e)]]
                        for e in entries], np.int32)
        starts = np.flatnonzero(np.r_[True, per[1:] != per[:-1]])
        seg_off = torch.from_numpy(np.r_[starts, R].astype(np.int64)).to(self.device)
        seg_set = torch.from_numpy(np.ascontiguousarray(per[starts])).to(self.device)
        out = None
        if (per < 0).any():   # the global answers first, the sets' laid over them
            if self._nbr is not None and n + 1 <= self._nbr.shape[1]:
                idx = self._nbr[d_rows][:, 1:n + 1].to(torch.int64)
                dist = torch.empty((R, n), dtype=torch.float32, device=self.device)
            else:
                dist, idx = self.index.kneighbors_device(self.index._table[d_rows], n + 1)
                idx, dist = idx[:, 1:], dist[:, 1:]
            out = (idx, dist)
        _, idx = self.index.kneighbors_within_device(self.index._table[d_rows], n, rows, off, seg_off, seg_set,
                                                     longest, exclude=d_rows, out=out)
        return idx

    def _requests_candidates(self, pos_ptr, d_pos, pos_off_ptr, R, Q, *rest, within=None):
        """dcnr_requests_candidates behind ONE top-k call over all requests'
        positives d_pos [Q] -- or, with a neighbour table, its table form and no
        scan.  ``rest``: the arguments from set_rows on.  ``within`` (requests
        that name a set for their neighbours): (set_rows, set_off, pos_off, set
        index per request -- device tensors --, the longest named set, whether a
        request with positives names none).  Those requests' neighbours come
        from one set-scoped call laid over the global answers (the table's rows,
        gathered, or the scan's), which only the others keep.  Returns the
        knn_idx [Q][k] the kernel read, None where it read the neighbour table."""
        lib = _lib.load()
        k, nbr = self.n_neighbors, self._nbr
        if nbr is not None and (within is None or not Q):
            _lib.check(lib.dcnr_requests_candidates_table(
                pos_ptr, pos_off_ptr, R, Q, nbr.data_ptr(), nbr.shape[1], k, *rest),
                "dcnr_requests_candidates_table")
            return None
        idx = None
        if Q and (within is None or within[5]):   # someone keeps global neighbours
            idx = nbr[d_pos][:, :k].to(torch.int64) if nbr is not None else \
                self.index.kneighbors_device(self.index._table[d_pos], k)[1]
        if Q and within is not None:
            idx = self._within_overlay(d_pos, idx, *within[:5])
        _lib.check(lib.dcnr_requests_candidates(
            pos_ptr, pos_off_ptr, R, Q, idx.data_ptr() if Q else None, k, *rest),
            "dcnr_requests_candidates")
        return idx

    def register_sets(self, sets) -> List[int]:
        """Upload row sets (a city's hotels, its most reviewed hotels ...) once,
        sorted and distinct, and return their indices for ``recommend_many``'s
        ``allowed`` / ``excluded`` / ``fallback``.  A later call appends; indices
        stay valid."""
        new = [_row_set(s, self.n_rows, "register_sets") for s in sets]
        with self._sets_lock:
            rows, off = self._sets
            first = off.size - 1
            if new:
                add = torch.from_numpy(np.concatenate(new)).to(self.device)
                lens = np.array([a.size for a in new], np.int64)
                rows = torch.cat([rows, add])
                # published only once written: a call on another stream may read it at once
                torch.cuda.current_stream(self.device).synchronize()
                self._sets = (rows, np.concatenate([off, off[-1] + np.cumsum(lens)]))
        return list(range(first, first + len(new)))

    @_one_generation
    @torch.no_grad()
    def recommend_many(self, user_rows, positive_rows, lambda_param=1.0, top_k=20,
                       allowed=None, excluded=None, fallback=None, min_candidates: int = 20,
                       neighbors_within=None, city_sets=None, cities=None,
                       neighbors_in_city: bool = False):
        """``recommend()`` for R requests in one device pass: returns a list of
        R pairs (ranked rows, their logits), each equal to what ``recommend``
        returns for that request alone, as views into the result tensors of
        its lane.  The list is an ``Answers`` (its ``large`` / ``on_host`` name
        the requests that did not take the small lane) when some request took
        the large lane or ``recommend()``, or the pipeline has
        ``item_features``; else the plain list it has always been.

        user_rows      R user rows
        positive_rows  R sequences of hotel rows (may be empty)
        lambda_param, top_k   a scalar or R values
        allowed, excluded, fallback   None, or R entries, each None, an index
                       from ``register_sets`` or an iterable of rows (uploaded
                       for this call)
        neighbors_within   None, or R entries of the same forms: the set each
                       request's positives seek their neighbours in
                       (``recommend``'s ``neighbors_within``; the usual call
                       names the city here and as ``allowed``).  Requests
                       whose entry is None keep their global neighbours; the
                       others' come from ONE set-scoped search over all their
                       positives (dcnr_cosine_topk_within, the requests as its
                       segments) laid over them, whether or not the pipeline
                       has a neighbour table.  Still one wait.
        city_sets, cities, neighbors_in_city   a ``dcnr.CitySets`` and R city
                       codes (-1: a city the table does not know): request
                       r's ``allowed`` is city(cities[r]), its ``fallback``
                       popular(cities[r]) and, with ``neighbors_in_city``, its
                       ``neighbors_within`` city(cities[r]); those arguments
                       must then be None (ValueError), ``excluded`` stays
                       free.  The sets are the newest generation's on this
                       device, joined to the call's set CSR behind the
                       registered sets: nothing but R codes' worth of indices
                       and the generation's offsets travels.  An unknown city
                       gets the empty set, so its answer is empty
                       (main.py:209-212)

        One packed, pinned, non-blocking copy carries every host input; one
        top-k call serves all positives; each request's set work runs in its
        own workgroup; one forward scores all candidates.  The call waits for
        the device ONCE: after the candidate kernels, to read the forward's
        batch size (the last of the request offsets the device mirrors into
        pinned memory).  Rows are validated on the host before anything is
        launched (ValueError).  A request whose bound of candidates (its
        positives * n_neighbors + its fallback set's rows) exceeds the
        one-workgroup kernels' capacity (SV_MAX) takes the large lane: its
        candidates are found by grids over all such requests' entries behind
        the same upload, from the same neighbour source and before the same
        wait; a forward of its own scores them (so the other answers are the
        bits they are without it), a radix sort ranks them and one workgroup
        per request runs its MMR (``Answers.large``).  ``recommend()`` answers
        only a request whose lambda rounds to 1.0f from below, a large request
        past ``large_lane_budget`` staged entries, and one the small lane
        reports as overflowing although its bound fits -- spliced in, never
        truncated (``Answers.on_host``).

        The index and the feature tables must hold the same hotels (equal row
        counts; ValueError otherwise -- ``recommend()`` clamps there).  Nothing
        is read back after the forward, so a request whose logits hold a NaN
        or -inf (they have no rank; ``recommend()`` is undefined there too) is
        not reported: the device marks its whole answer, rows -1 and logits
        NaN."""
        users = self._users_arg("recommend_many", user_rows)
        R = users.size
        if len(positive_rows) != R:
            raise ValueError("recommend_many: one positive list per user row")
        if R == 0:
            return []
        city = self._city_arg("recommend_many", city_sets, cities, neighbors_in_city, R, allowed,
                              fallback, neighbors_within)
        p, b = self._many_front(users, positive_rows, lambda_param, top_k, allowed, excluded, fallback,
                                min_candidates, neighbors_within=neighbors_within, city=city,
                                large_lane=True)
        out_rows, out_logits = b.rank_mmr(b.score(), b.ptr("lam"), b.out_count)
        on_host = ((b.st & REQ_OVERFLOW) | p.odd).astype(bool)
        large = {}
        if b.L:
            lanes = b.large[0]
            large, n_seg = b.large_rank_mmr(b.large_score())
            cut = np.where(p.lam[lanes] < 1.0, np.minimum(p.topk[lanes], n_seg), n_seg)
            large = {r: (rows[:c], z[:c]) for (r, (rows, z)), c in zip(large.items(), cut.tolist())}
            on_host[lanes] = False

        def host(r):   # above the batched kernels' capacity, or a lambda that rounds to 1.0f
            return self._on_host(r, users, p, p.pos[p.pos_off[r]:p.pos_off[r + 1]],
                                 self._set_arg(None if excluded is None else excluded[r]),
                                 min_candidates, (city, allowed, fallback, neighbors_within))
        small = b.answers(out_rows, out_logits, b.answer_lengths(p.lam, p.topk), on_host, host)
        if not large and not on_host.any():   # every request in the small lane: the plain list, as ever
            return small
        res = Answers(large.get(r, a) for r, a in enumerate(small))
        res.large, res.on_host = sorted(large), np.flatnonzero(on_host).tolist()
        return res

    def _users_arg(self, what, user_rows):
        """``user_rows`` of the batched call ``what`` as an array, the tables' row counts checked."""
        if self.index._table.shape[0] != self.n_items:
            raise ValueError(f"{what}: the index holds {self.index._table.shape[0]} rows, "
                             f"item_cat / item_num {self.n_items}")
        return np.asarray(user_rows, dtype=np.int64).reshape(-1)

    def _pack(self, users, positive_rows, lambda_param, top_k, allowed, excluded, fallback,
              neighbors_within=None, city=None):
        """``pack_requests`` on this pipeline's tables (``city``: from ``_city_arg``), and the
        device rows of the sets the packed indices name in front of the per-call ones."""
        reg_rows, reg_off = self._sets
        p = pack_requests(users, positive_rows, lambda_param, top_k, allowed, excluded, fallback,
                          neighbors_within, n_users=self.model.user_embedding.weight.shape[0],
                          n_rows=self.n_rows, k=self.n_neighbors, reg_off=reg_off,
                          city=None if city is None else (city[0].host_offsets, city[0].n_cities,
                                                          city[1], city[2]))
        if not p.S:
            return p, self._no_rows
        return p, reg_rows if city is None else self._city_join(reg_rows, city[0])

    def _many_front(self, users, positive_rows, lambda_param, top_k, allowed, excluded, fallback,
                    min_candidates, extra=None, tail=0, neighbors_within=None, city=None,
                    large_lane=False):
        """``recommend_many`` up to its one wait: the packed requests and their
        ``_RequestBatch``, staged (``extra``: further named arrays to carry along;
        ``tail``: as ``_RequestBatch``'s), the candidates found and waited for.
        ``large_lane``: the caller opts in to the large lane for the requests
        ``large_lane_split`` gives it under ``large_lane_budget`` (the batch's
        ``large``); without it every request goes the small lane's way."""
        p, reg_rows = self._pack(users, positive_rows, lambda_param, top_k, allowed, excluded,
                                 fallback, neighbors_within, city)
        large = None
        if large_lane and p.large.size:
            lanes, _, stage_off = large_lane_split(p, self.large_lane_budget)
            if lanes.size:
                large = (lanes, stage_off)
                extra = dict(extra or {}, large_req=lanes, large_stage_off=stage_off,
                             large_lam=p.lam[lanes], large_topk=p.topk[lanes])
        b = _RequestBatch(self, "recommend_many", users.size, dict(p.arrays, **(extra or {})),
                          tail=tail, large=large)
        b.candidates(b.view("pos", p.pos.size, torch.int64), b.set_rows(reg_rows, p.n_adhoc), p.S,
                     min_candidates, p.cap,
                     None if p.within_idx is None else (p.within_longest, p.within_any_global))
        b.wait()
        return p, b

    def _on_host(self, r, users, p, positives, excluded, min_candidates, sets):
        """Request r of a batched call answered by ``recommend()``.  ``sets``: the call's
        (city, allowed, fallback, neighbors_within), turned into rows here (a city's from
        the host columns of the generation the batched call used)."""
        city, allowed, fallback, neighbors_within = sets
        if city is not None:
            gen, codes, in_city = city
            rows = gen.host.city_rows(int(codes[r]))
            sets = dict(allowed=rows, fallback=gen.host.popular_rows(int(codes[r])))
            if in_city:
                sets["neighbors_within"] = rows
        else:
            pick = lambda v: None if v is None else self._set_arg(v[r])
            sets = dict(allowed=pick(allowed), fallback=pick(fallback),
                        neighbors_within=pick(neighbors_within))
        return self.recommend(int(users[r]), positives, float(p.lam64[r]), int(p.topk[r]),
                              excluded=excluded, min_candidates=min_candidates, **sets)

    # ------------------------------------------------ what the answers look like
    def _blank_relevant(self, relevant, R, skipped):
        """``relevant`` as the host CSR of ``dcnr.metrics.relevant_csr``, the
        sets of the ``skipped`` requests emptied."""
        from . import metrics as mt
        rows, off = mt.relevant_csr(relevant, R, self.index._table.shape[0])
        if len(skipped):
            keep = np.ones(R, bool)
            keep[np.asarray(skipped, np.int64)] = False
            lens = np.diff(off)
            rows = rows[np.repeat(keep, lens)]
            off = np.zeros(R + 1, np.int64)
            np.cumsum(lens * keep, out=off[1:])
        return rows, off

    def list_metrics(self, answers, *, at: int = 20, info=None, relevant=None, ks=(5, 10, 20),
                     per_list: bool = False):
        """``dcnr.list_metrics`` of what ``recommend_many`` / ``recommend_users``
        returned: a list of (rows, logits) pairs, concatenated on the device
        (their lengths are known on the host; an answer that came from the
        one-request path is concatenated like any other), measured against
        this pipeline's index table, the logits as ``scores``.  An entry that
        is None (a request ``lambda_sweep`` skipped) is an empty list whose
        ``relevant`` set is ignored.  ``info`` / ``relevant`` / ``ks`` /
        ``per_list`` as in ``dcnr.list_metrics``."""
        from . import metrics as mt
        dev = self.device
        R = len(answers)
        table, inv = self.index._table, self.index._inv
        lens = np.array([0 if a is None else int(a[0].numel()) for a in answers], np.int64)
        off = np.zeros(R + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        n = int(off[R])
        _, at, ks = mt._list_check(n, R + 1, None, tuple(table.shape), inv.numel(), at, None,
                                   None if info is None else len(info), ks)
        rel = None
        if relevant is not None:
            skipped = [r for r, a in enumerate(answers) if a is None]
            rel = tuple(torch.from_numpy(a).to(dev) for a in self._blank_relevant(relevant, R, skipped))
        if info is not None:
            info = torch.as_tensor(info, dtype=torch.float64).reshape(-1).to(dev)
        some = [a for a in answers if a is not None and a[0].numel()]
        if some:
            rows = torch.cat([a[0].to(dev, torch.int64) for a in some])
            scores = torch.cat([a[1].to(dev, torch.float32) for a in some])
        else:
            rows = torch.empty(0, dtype=torch.int64, device=dev)
            scores = torch.empty(0, dtype=torch.float32, device=dev)
        return mt.list_metrics_raw(rows, torch.from_numpy(off).to(dev), None, table=table, inv_norms=inv,
                                   at=at, scores=scores, info=info, relevant=rel, ks=ks,
                                   per_list=per_list)

    @_one_generation
    @torch.no_grad()
    def lambda_sweep(self, user_rows, positive_rows, lambdas, top_k: int = 20, allowed=None,
                     excluded=None, fallback=None, min_candidates: int = 20, relevant=None,
                     info=None, ks=(5, 10, 20), neighbors_within=None):
        """``recommend_many`` for several values of ``lambda_param`` with the
        list metrics of each, the candidates scored ONCE: the front of
        ``recommend_many`` (one upload, one top-k or table lookup, one
        candidates pass, the one wait) and one forward; then per lambda one
        rank + MMR launch and one ``dcnr_eval_list_metrics`` launch that reads
        the answers and their counts where the first left them.  The
        summaries are read together after the last launch.

        lambdas     the values to compare (each one value for all requests)
        top_k       one value, at most 128: the MMR's length and the metrics' ``at``
        relevant, info, ks   as in ``dcnr.list_metrics`` (one entry per request)
        neighbors_within     as in ``recommend_many``

        Returns ``SweepResult``: a list of ``(answers, ListMetrics)``, one per
        lambda, ``answers`` as ``recommend_many`` returns them; ``.lambdas``;
        ``.skipped``: the indices of requests the batched kernels hand back
        (candidates above SV_MAX -- or every request, when some lambda rounds
        to 1.0f from below: decided on the host, nothing is launched then).
        Their entry in every ``answers`` is None, never a truncated list, and
        they take part in no metric but ``n_lists``: serve them with
        ``recommend()``."""
        from . import metrics as mt
        dev = self.device
        users = self._users_arg("lambda_sweep", user_rows)
        R = users.size
        if len(positive_rows) != R:
            raise ValueError("lambda_sweep: one positive list per user row")
        lam64 = np.asarray(list(lambdas), np.float64).reshape(-1)
        L = lam64.size
        if L == 0 or R == 0:
            raise ValueError("lambda_sweep: no lambda, or no request")
        if not np.isscalar(top_k):
            raise ValueError("lambda_sweep: one top_k for all requests")
        table, inv = self.index._table, self.index._inv
        _, at, ks = mt._list_check(0, R + 1, R, tuple(table.shape), inv.numel(), top_k, None,
                                   None if info is None else len(info), ks)
        out = SweepResult()
        out.lambdas = tuple(float(v) for v in lam64)
        rel_host = None
        if relevant is not None:   # validated before anything is launched
            rel_host = mt.relevant_csr(relevant, R, table.shape[0])
        if info is not None:
            info = torch.as_tensor(info, dtype=torch.float64).reshape(-1).to(dev)
        lam32 = lam64.astype(np.float32)
        if rounds_to_one(lam64, lam32).any():
            # such a lambda goes the one-request way, so the batched kernels serve no request of
            # this sweep.  Known here: the rows are validated as usual and nothing is launched.
            self._pack(users, positive_rows, float(lam64[0]), int(top_k), allowed, excluded,
                       fallback, neighbors_within)
            out.skipped = list(range(R))
            for _ in range(L):
                out.append(([None] * R, mt.empty_list_metrics(R, ks)))
            return out
        lams = np.repeat(lam32, R)                     # [L][R]: one lambda array per launch
        tail = 8 * (rel_host[0].size + R + 1) if rel_host is not None else 0
        _, b = self._many_front(users, positive_rows, float(lam64[0]), int(top_k), allowed, excluded,
                                fallback, min_candidates, extra={"lams": lams}, tail=tail,
                                neighbors_within=neighbors_within)
        skip = (b.st & REQ_OVERFLOW).astype(bool)
        out.skipped = np.flatnonzero(skip).tolist()
        # ---- the held-out sets without the skipped requests': pinned, no wait
        rel = None
        if rel_host is not None:
            rr, ro = self._blank_relevant(rel_host, R, out.skipped)
            o = b.tail
            b.host[o:o + 8 * (R + 1)] = ro.view(np.uint8)
            b.host[o + 8 * (R + 1):o + 8 * (R + 1) + 8 * rr.size] = rr.view(np.uint8)
            d_rel = b.pin[o:o + 8 * (R + 1 + rr.size)].to(dev, non_blocking=True).view(torch.int64)
            rel = (d_rel[R + 1:], d_rel[:R + 1])
        nsum = ctypes.sizeof(_lib.ListSummaryStruct)
        sums = torch.empty((L, nsum), dtype=torch.uint8, device=dev)
        mws = torch.empty(mt.list_workspace_bytes(R, table.shape[0]), dtype=torch.uint8, device=dev)
        logits = b.score()
        per = []
        for j in range(L):
            counts = torch.empty(R, dtype=torch.int32, device=dev)   # this lambda's out_count
            if not b.n:
                counts.zero_()
            rows_j, logits_j = b.rank_mmr(logits, b.ptr("lams") + 4 * R * j, counts.data_ptr())
            mt._list_launch(rows_j, b.offsets, counts, table, inv, at,
                            logits_j, info, rel, ks, False, mws, out=sums[j])
            per.append(b.answers(rows_j, logits_j, b.answer_lengths(lam32[j], int(top_k)), skip,
                                 lambda r: None))
        raw = sums.cpu().numpy()                           # every summary, one copy
        for j in range(L):
            out.append((per[j], mt._list_result(raw[j].tobytes(), ks, None)))
        return out

    # --------------------------------------------- a batch of requests by user
    @_one_generation
    @torch.no_grad()
    def recommend_users(self, store, user_rows, reviewers, modes, lambda_param=1.0, top_k=20,
                        allowed=None, fallback=None, min_candidates: int = 20,
                        recommended_by: bool = True, neighbors_within=None, city_sets=None,
                        cities=None, neighbors_in_city: bool = False):
        """``recommend_many`` from user ids: each request's positives, its
        excluded set (the negatives, main.py:193-194, 211) and the
        ``recommended_by`` lists of its answer (main.py:336-351) come from a
        ``dcnr.InteractionStore`` on the device.

        store       dcnr.InteractionStore over this pipeline's hotel rows
        user_rows   R model user rows (main.py:217 stays the caller's)
        reviewers   R store indices, -1 for a user the store does not know
        modes       'friends' / 'personal', one value or R
        lambda_param, top_k, allowed, fallback, min_candidates, neighbors_within,
        city_sets, cities, neighbors_in_city
                    as in ``recommend_many`` (``excluded`` is the negatives)

        Returns a ``UserAnswers``: a list of R (ranked rows, logits) pairs,
        each equal to what ``recommend_many`` gives for ``sources_host``'s
        positives and negatives, with the recommended_by CSR over the result
        tensor's positions as device tensors and ``to_lists(r)``.

        One packed pinned upload (no positives travel), one wait, as in
        ``recommend_many``.  The device cannot tell the host how many distinct
        positives it found without a second wait, so each request gets
        segments as long as the store's host counts bound them (the sum over
        its sources of their distinct positives / negatives) and the kernel
        fills a segment's tail with repeats: the candidate union is a set
        union and the excluded filter a binary search in an ascending set, so
        the candidates are those of the distinct rows.  A request whose friends
        or staged review rows exceed SV_MAX, or whose bound of positives times
        n_neighbors does (known from the counts before anything is launched),
        and one the candidate kernel reports as overflowing, is answered by
        ``sources_host`` + ``recommend()`` + ``recommended_by_host`` and
        spliced in, never truncated."""
        from . import interactions as ia
        lib = _lib.load()
        dev = self.device
        users = self._users_arg("recommend_users", user_rows)
        if store.n_items > self.n_rows:
            raise ValueError(f"recommend_users: the store names {store.n_items} hotel rows, the "
                             f"pipeline holds {self.n_rows}")
        R = users.size
        rv = np.asarray(reviewers, dtype=np.int64).reshape(-1)
        if rv.size != R:
            raise ValueError("recommend_users: one reviewer index per user row")
        if R == 0:
            return UserAnswers()
        if rv.min() < -1 or rv.max() >= store.n_reviewers:
            raise ValueError(f"recommend_users: reviewer outside [-1, {store.n_reviewers})")
        md = np.full(R, ia.mode_code(modes), np.int32) if isinstance(modes, (str, int, np.integer)) \
            else np.array([ia.mode_code(m_) for m_ in modes], np.int32)
        if md.size != R:
            raise ValueError("recommend_users: one mode, or one per request")
        # lambda, top_k and the allowed / fallback indices as recommend_many packs them
        city = self._city_arg("recommend_users", city_sets, cities, neighbors_in_city, R, allowed,
                              fallback, neighbors_within)
        p, reg_rows = self._pack(users, [()] * R, lambda_param, top_k, allowed, None, fallback,
                                 neighbors_within, city)
        k = self.n_neighbors
        # ---- what the store's host counts say about each request
        n_src, staged, pos_b, neg_b, n_fr, fr_rows, by_b = store.bounds(rv, md)
        on_host = (n_src > SV_MAX) | (staged > SV_MAX) | (pos_b * k > SV_MAX) | p.odd
        if recommended_by:
            on_host |= (n_fr > SV_MAX) | (fr_rows > SV_MAX)
        else:
            by_b = np.zeros(R, np.int64)
        dev_rv = np.where(on_host, -1, rv).astype(np.int32)   # answered on the host: no sources here
        zero = lambda a: np.where(on_host, 0, a)
        pos_off, list_off = np.zeros(R + 1, np.int64), np.zeros(R + 1, np.int64)
        np.cumsum(zero(pos_b), out=pos_off[1:])
        np.cumsum(zero(by_b), out=list_off[1:])
        Q, L = int(pos_off[R]), int(list_off[R])
        # the requests' negatives behind the registered and per-call sets, one CSR
        set_off = p.arrays.get("set_off", np.zeros(1, np.int64))
        S0, n0 = set_off.size - 1, int(set_off[-1])
        neg_b = zero(neg_b)
        set_off = np.concatenate([set_off, n0 + np.cumsum(neg_b)])
        NB = int(set_off[-1]) - n0
        e_idx = np.where(neg_b > 0, S0 + np.arange(R), -1).astype(np.int32)
        # no positives travel (the device finds them); offsets as the store's counts bound them
        arrays = dict(p.arrays, pos_off=pos_off, set_off=set_off, list_off=list_off, excluded=e_idx,
                      reviewers=dev_rv, modes=md)
        del arrays["pos"]
        f_len = 0
        if "fallback" in arrays:
            if on_host.any():   # (no fallback either: nothing of theirs is scored)
                arrays["fallback"] = np.where(on_host, -1, arrays["fallback"]).astype(np.int32)
            f_len = np.diff(set_off)[arrays["fallback"]] * (arrays["fallback"] >= 0)
        cap = int(min(SV_MAX, max(1, int((zero(pos_b) * k + f_len).max()))))
        b = _RequestBatch(self, "recommend_users", R, arrays, sources=True)
        set_rows = b.set_rows(reg_rows, p.n_adhoc, NB)
        desc, held = store.on(dev)   # the generation this call's kernels read: kept with the answers
        d_pos = torch.empty(Q, dtype=torch.int64, device=dev)
        _lib.check(lib.dcnr_requests_sources(
            desc, b.ptr("reviewers"), b.ptr("modes"), R, self.n_rows, b.ptr("pos_off"), Q,
            d_pos.data_ptr() if Q else None, b.ptr("set_off") + 8 * S0, n0, n0 + NB,
            set_rows.data_ptr() if NB else None, b.src_count, b.src_status, b.pin_src_count,
            b.pin_src_status, b.stream), "dcnr_requests_sources")
        within = None
        if p.within_idx is not None:   # the requests as the set-scoped search's segments
            within = (p.within_longest, bool(((p.within_idx < 0) & (zero(pos_b) > 0)).any()))
        b.candidates(d_pos, set_rows, S0 + R, min_candidates, cap, within)
        lists = torch.empty(L, dtype=torch.int32, device=dev)
        by_reviewers = torch.empty(L, dtype=torch.int32, device=dev)
        b.wait()
        n, seg = b.n, b.seg.copy()
        on_host = on_host | (b.st & REQ_OVERFLOW).astype(bool)
        out_rows, out_logits = b.rank_mmr(b.score(), b.ptr("lam"), b.out_count)
        by_count = torch.empty(n, dtype=torch.int32, device=dev)
        by_offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if recommended_by and n:
            _lib.check(lib.dcnr_requests_recommended_by(
                desc, b.ptr("reviewers"), R, self.n_rows, out_rows.data_ptr(), n,
                b.offsets.data_ptr(), b.out_count, b.ptr("list_off"), L,
                lists.data_ptr() if L else None, by_count.data_ptr(), by_offsets.data_ptr(),
                by_reviewers.data_ptr() if L else None, b.by_status, b.stream),
                "dcnr_requests_recommended_by")
        elif n:
            by_count.zero_()
        cnt = b.answer_lengths(p.lam, p.topk)
        res = UserAnswers()
        res.by_offsets, res.by_reviewers, res.by_count, res.lists = (by_offsets, by_reviewers,
                                                                    by_count, lists)
        res.rows, res.logits = out_rows, out_logits
        res._seg, res._cnt, res._list_off, res._store, res._rv = seg, cnt, list_off, store, rv
        res._held = held
        res._city_held = city[0] if city is not None else None
        res.n_positives, res.positives_bound = b.src_counts[:, 0].copy(), zero(pos_b)
        res.on_host = on_host

        def host(r):   # above the batched kernels' capacity: the store's host copies
            p_r, n_r = store.sources_host(int(rv[r]), int(md[r]))
            return self._on_host(r, users, p, p_r, n_r, min_candidates,
                                 (city, allowed, fallback, neighbors_within))
        res.extend(b.answers(out_rows, out_logits, cnt, on_host, host))
        return res

    def _city_arg(self, what, city_sets, cities, in_city, R, allowed, fallback, neighbors_within):
        """``city_sets`` / ``cities`` / ``neighbors_in_city`` of a batched call:
        None, or (the generation on this device, the R codes, the flag)."""
        if cities is None:
            if in_city:
                raise ValueError(f"{what}: neighbors_in_city needs cities")
            return None
        if city_sets is None:
            raise ValueError(f"{what}: cities needs city_sets")
        if allowed is not None or fallback is not None or (in_city and neighbors_within is not None):
            raise ValueError(f"{what}: with cities, allowed and fallback (and with neighbors_in_city, "
                             "neighbors_within) come from the city and must be None")
        codes = np.asarray(cities, dtype=np.int64).reshape(-1)
        if codes.size != R:
            raise ValueError(f"{what}: one city code per request")
        if codes.min() < -1 or codes.max() >= city_sets.n_cities:
            raise ValueError(f"{what}: city code outside [-1, {city_sets.n_cities})")
        if city_sets.n_items > self.n_rows:
            raise ValueError(f"{what}: the city sets name {city_sets.n_items} hotel rows, the "
                             f"pipeline holds {self.n_rows}")
        return city_sets.on(self.device), codes, bool(in_city)

    def _city_join(self, reg_rows, gen):
        """The registered sets' rows with the generation's behind them, on the
        device; joined once per (registered sets, generation)."""
        if reg_rows.numel() == 0:
            return gen.set_rows
        hit = self._city_joined
        if hit is None or hit[0] is not reg_rows or hit[1] is not gen:
            joined = torch.cat([reg_rows, gen.set_rows])
            # published only once written: a call on another stream may read it at once
            torch.cuda.current_stream(self.device).synchronize()
            hit = self._city_joined = (reg_rows, gen, joined)
        return hit[2]

    def _pinned(self, nbytes):
        """This thread's pinned staging buffer (tensor, numpy view), grown as
        needed.  One per thread: a call has waited for the device before it
        returns, so nothing of it is in flight when the thread's next call
        writes the buffer."""
        buf = getattr(self._tls, "pin", None)
        if buf is None or buf[0].numel() < nbytes:
            t = torch.empty(max(4096, 2 * nbytes), dtype=torch.uint8, pin_memory=True)
            buf = self._tls.pin = (t, t.numpy())
        return buf

    def _set_arg(self, e):
        """A recommend_many set entry as ``recommend()`` takes it (rows)."""
        if e is None or not isinstance(e, (int, np.integer)):
            return e
        rows, off = self._sets
        return rows[int(off[e]):int(off[e + 1])].tolist()
