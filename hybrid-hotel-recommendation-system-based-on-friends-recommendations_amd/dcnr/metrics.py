"""Validation metrics on the device: the reference's epoch end
(train.py:229-233, 255-265, 366-387) without copying the logits to the host.

  eval_metrics(logits, labels)   BCEWithLogitsLoss, roc_auc_score and
                                 sqrt(mean_squared_error(y, sigmoid(z))) in one
                                 native call (dcnr_eval_metrics) and one
                                 72-byte device-to-host copy
  roc_auc_score(y_true, y_score) sklearn's argument order
  evaluate(model, collab, cat, num, y, batch_size=None)
                                 the eval-mode forward over the whole split
                                 (train.py:229-232) into one logits buffer,
                                 then eval_metrics over all of it
  group_metrics(logits, labels, groups, ks=(5, 10, 20))
                                 per-group ranking metrics (GAUC, NDCG@k, hit
                                 rate / recall@k, MRR) of each group's list in
                                 served order: one native call
                                 (dcnr_eval_group_metrics), one 216-byte copy
  evaluate_ranking(model, collab, cat, num, y, group_by='user', ks=...)
                                 evaluate and group_metrics from one forward
  list_metrics(rows, offsets, counts, table=..., at=20, ...)
                                 what served lists look like (intra-list
                                 diversity, coverage, Gini of the exposure,
                                 mean logit / item weight, held-out hits): one
                                 native call (dcnr_eval_list_metrics) on the
                                 lists where the batched serving calls left
                                 them, one 248-byte copy
  popularity_information(counts) -log2 of each item's smoothed share: the
                                 ``info`` weight whose mean is novelty

AUC is exact (the midrank Mann-Whitney statistic over a full device sort of the
scores, ties included): ``auc_u2`` is the integer 2U and ``auc`` is
``auc_u2 / (2.0 * n_pos * n_neg)``.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _lib

class Metrics(NamedTuple):
    logloss: float
    auc: float
    rmse: float
    n: int
    n_pos: int
    n_neg: int
    auc_u2: int
    n_bad_label: int
    n_nan: int


def workspace_bytes(n: int) -> int:
    return int(_lib.load().dcnr_eval_metrics_workspace_size(int(n)))


def eval_metrics_raw(logits: torch.Tensor, labels: torch.Tensor, ws: torch.Tensor | None = None) -> Metrics:
    """dcnr_eval_metrics on fp32 device tensors, the struct as it comes (no
    checks on the counters).  ``ws``: a uint8 device workspace of at least
    ``workspace_bytes(n)`` bytes (allocated when None)."""
    lib = _lib.load()
    z = logits.detach().reshape(-1).to(torch.float32).contiguous()
    if z.device.type != 'cuda':
        raise RuntimeError("dcnr.eval_metrics runs on the HIP device only")
    y = labels.detach().reshape(-1).to(device=z.device, dtype=torch.float32).contiguous()
    n = z.shape[0]
    if y.shape[0] != n:
        raise ValueError(f"Found input variables with inconsistent numbers of samples: [{y.shape[0]}, {n}]")
    with torch.cuda.device(z.device):
        if ws is None:
            ws = torch.empty(workspace_bytes(n), dtype=torch.uint8, device=z.device)
        out = torch.empty(ctypes.sizeof(_lib.MetricsStruct), dtype=torch.uint8, device=z.device)
        _lib.check(lib.dcnr_eval_metrics(z.data_ptr(), y.data_ptr(), n, out.data_ptr(),
                                         ws.data_ptr() if ws.numel() else None, ws.numel(),
                                         _lib.stream_ptr(z.device)), "dcnr_eval_metrics")
        m = _lib.MetricsStruct.from_buffer_copy(out.cpu().numpy().tobytes())   # the one D2H copy
    return Metrics(float(m.logloss), float(m.auc), float(m.rmse), int(m.n), int(m.n_pos), int(m.n_neg),
                   int(m.auc_u2), int(m.n_bad_label), int(m.n_nan))


def eval_metrics(logits: torch.Tensor, labels: torch.Tensor) -> Metrics:
    """Logloss, exact ROC AUC and RMSE of ``logits`` against 0/1 ``labels``
    (device tensors).  Raises ValueError where sklearn's roc_auc_score does: a
    NaN score, a label that is not 0 or 1, only one class present."""
    m = eval_metrics_raw(logits, labels)
    if m.n_nan:
        raise ValueError("Input contains NaN.")
    if m.n_bad_label:
        raise ValueError("labels must be 0 or 1: continuous format is not supported")
    if m.n_pos == 0 or m.n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    return m


def _as_device_f32(a, device):
    if isinstance(a, torch.Tensor):
        return a.detach().to(device=device, dtype=torch.float32)
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=device)


def roc_auc_score(y_true, y_score) -> float:
    """sklearn.metrics.roc_auc_score(y_true, y_score) for binary labels
    (train.py:258, 380), on the device; tensors or numpy arrays."""
    dev = None
    for a in (y_score, y_true):
        if isinstance(a, torch.Tensor) and a.device.type == 'cuda':
            dev = a.device
            break
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError("dcnr.roc_auc_score runs on the HIP device only")
        dev = torch.device('cuda', torch.cuda.current_device())
    return eval_metrics(_as_device_f32(y_score, dev), _as_device_f32(y_true, dev)).auc


class GroupMetrics(NamedTuple):
    """dcnr_group_summary; per-cutoff fields are tuples aligned with ``ks``.
    ``records``: None, or a dict of [n_groups] device tensors (n, n_pos,
    auc_u2, first_pos_rank int64; hits [n_groups, len(ks)] int64; dcg
    [n_groups, len(ks)] float64)."""
    gauc: float
    auc_macro: float
    mrr: float
    ks: tuple
    hit_rate: tuple
    recall: tuple
    ndcg: tuple
    n: int
    n_groups_present: int
    n_groups_auc: int
    n_groups_ranked: int
    n_rows_auc: int
    n_bad_label: int
    n_nan: int
    n_bad_group: int
    hit_groups: tuple
    records: dict | None = None


def dcg_tables(k_max: int):
    """(discount, ideal) float64 [k_max]: discount[i] = 1 / log2(i + 2) and its
    running sum (numpy.cumsum: sequential, so ideal[i] is discount[0] + ... +
    discount[i] added in that order) -- the doubles the device divides by."""
    discount = 1.0 / np.log2(np.arange(k_max, dtype=np.float64) + 2.0)
    return discount, np.cumsum(discount)


_tables = {}


def _device_tables(k_max, device):
    key = (int(k_max), str(device))
    if key not in _tables:
        d, i = dcg_tables(k_max)
        _tables[key] = (torch.from_numpy(d).to(device), torch.from_numpy(i).to(device))
    return _tables[key]


def group_workspace_bytes(n: int, n_groups: int) -> int:
    return int(_lib.load().dcnr_eval_group_metrics_workspace_size(int(n), int(n_groups)))


def group_metrics_raw(logits, labels, groups, ks=(5, 10, 20), n_groups=None, per_group=False) -> GroupMetrics:
    """dcnr_eval_group_metrics on device tensors, the summary as it comes (no
    checks on the counters).  ``n_groups`` must be given here: the ids are not
    looked at on the host."""
    lib = _lib.load()
    z = logits.detach().reshape(-1).to(torch.float32).contiguous()
    if z.device.type != 'cuda':
        raise RuntimeError("dcnr.group_metrics runs on the HIP device only")
    y = labels.detach().reshape(-1).to(device=z.device, dtype=torch.float32).contiguous()
    g = groups.detach().reshape(-1).to(device=z.device, dtype=torch.int64).contiguous()
    n = z.shape[0]
    if y.shape[0] != n or g.shape[0] != n:
        raise ValueError(f"Found input variables with inconsistent numbers of samples: "
                         f"[{y.shape[0]}, {g.shape[0]}, {n}]")
    if n_groups is None:
        raise ValueError("group_metrics_raw needs n_groups")
    ks = tuple(int(k) for k in ks)
    nk = len(ks)
    if nk > _lib.GROUP_MAX_K:
        raise ValueError(f"at most {_lib.GROUP_MAX_K} cutoffs")
    n_groups = int(n_groups)
    ks_arr = (ctypes.c_int32 * max(1, nk))(*ks)
    with torch.cuda.device(z.device):
        disc, ideal = _device_tables(ks[-1], z.device) if nk and 1 <= ks[-1] <= (1 << 20) else (None, None)
        ws = torch.empty(group_workspace_bytes(n, n_groups), dtype=torch.uint8, device=z.device)
        out = torch.empty(ctypes.sizeof(_lib.GroupSummaryStruct), dtype=torch.uint8, device=z.device)
        rec = None
        if per_group:
            rec = torch.empty((max(n_groups, 0), ctypes.sizeof(_lib.GroupRecordStruct) // 8),
                              dtype=torch.int64, device=z.device)
        _lib.check(lib.dcnr_eval_group_metrics(
            z.data_ptr(), y.data_ptr(), g.data_ptr(), n, n_groups, ks_arr, nk,
            disc.data_ptr() if disc is not None else None,
            ideal.data_ptr() if ideal is not None else None, out.data_ptr(),
            rec.data_ptr() if rec is not None else None, ws.data_ptr() if ws.numel() else None,
            ws.numel(), _lib.stream_ptr(z.device)), "dcnr_eval_group_metrics")
        m = _lib.GroupSummaryStruct.from_buffer_copy(out.cpu().numpy().tobytes())   # the one D2H copy
    records = None
    if rec is not None:
        records = {"n": rec[:, 0], "n_pos": rec[:, 1], "auc_u2": rec[:, 2], "first_pos_rank": rec[:, 3],
                   "hits": rec[:, 4:4 + nk], "dcg": rec[:, 8:8 + nk].view(torch.float64)}
    return GroupMetrics(float(m.gauc), float(m.auc_macro), float(m.mrr), ks,
                        tuple(float(m.hit_rate[j]) for j in range(nk)),
                        tuple(float(m.recall[j]) for j in range(nk)),
                        tuple(float(m.ndcg[j]) for j in range(nk)),
                        int(m.n), int(m.n_groups_present), int(m.n_groups_auc), int(m.n_groups_ranked),
                        int(m.n_rows_auc), int(m.n_bad_label), int(m.n_nan), int(m.n_bad_group),
                        tuple(int(m.hit_groups[j]) for j in range(nk)), records)


def group_metrics(logits, labels, groups, ks=(5, 10, 20), n_groups=None, per_group=False) -> GroupMetrics:
    """Per-group ranking metrics of ``logits`` against 0/1 ``labels`` with
    ``groups`` [N] int64 naming each row's group (device tensors): GAUC, the
    macro mean of the per-group AUC, MRR, and hit rate / recall / NDCG at each
    cutoff of ``ks``, every group's rows ranked as the service shows them
    (descending logit, ties in input order).  ``n_groups=None`` takes
    ``groups.max() + 1``.  Raises ValueError for a NaN score, a label that is
    not 0 or 1 and a group id outside [0, n_groups).  Groups with a single
    class are not an error: they are left out of the AUC means (no positive:
    out of the ranking means too), and the counts say how many took part."""
    if n_groups is None:
        n_groups = int(groups.max()) + 1 if groups.numel() else 1
    m = group_metrics_raw(logits, labels, groups, ks, n_groups, per_group)
    if m.n_nan:
        raise ValueError("Input contains NaN.")
    if m.n_bad_label:
        raise ValueError("labels must be 0 or 1: continuous format is not supported")
    if m.n_bad_group:
        raise ValueError(f"{m.n_bad_group} group ids are outside [0, {n_groups})")
    return m


LIST_MAX_AT = 128   # dcnr_eval_list_metrics: 1 <= at <= 128


class ListMetrics(NamedTuple):
    """dcnr_list_summary; per-cutoff fields are tuples aligned with ``ks``.
    ``records``: None, or a dict of [R] device tensors (m, n_rel,
    first_hit_rank int64; hits [R, len(ks)] int64; pair_cos_sum, score_sum,
    info_sum float64; dcg [R, len(ks)] float64)."""
    ild: float
    coverage: float
    gini: float
    mean_score: float
    mean_info: float
    mrr: float
    ks: tuple
    hit_rate: tuple
    recall: tuple
    ndcg: tuple
    n_lists: int
    n_lists_scored: int
    n_lists_pairs: int
    n_marked: int
    n_bad_list: int
    n_entries: int
    n_distinct_items: int
    gini_num: int
    n_rel_lists: int
    hit_lists: tuple
    records: dict | None = None


def popularity_information(counts) -> np.ndarray:
    """Self-information of each item under add-one smoothing, float64
    [n_items]: ``-log2((c_i + 1) / (sum(c) + n_items))`` -- finite for an item
    never seen, never negative; the ``info`` of ``list_metrics`` (its mean is
    the lists' novelty)."""
    c = np.asarray(counts.cpu() if torch.is_tensor(counts) else counts, dtype=np.float64).reshape(-1)
    if c.size and c.min() < 0:
        raise ValueError("popularity_information: negative count")
    return -np.log2((c + 1.0) / (c.sum() + c.size))


def list_workspace_bytes(R: int, n_items: int) -> int:
    return int(_lib.load().dcnr_eval_list_metrics_workspace_size(int(R), int(n_items)))


def relevant_csr(relevant, R: int, n_items: int):
    """The held-out sets as the CSR dcnr_eval_list_metrics reads, on the host:
    (rows int64, offsets int64 [R + 1]), each set ascending and distinct.
    ``relevant``: a list of R iterables of item rows (None = empty), or a
    TUPLE ``(rows, offsets)`` of arrays whose sets need be neither."""
    if isinstance(relevant, tuple):
        if len(relevant) != 2:
            raise ValueError("relevant: a list of R iterables or a (rows, offsets) tuple")
        as_np = lambda a: np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.int64).reshape(-1)
        rows, off = as_np(relevant[0]), as_np(relevant[1])
        if off.size != R + 1:
            raise ValueError(f"relevant: {off.size} offsets for {R} lists")
        if off[0] < 0 or off[-1] > rows.size or (np.diff(off) < 0).any():
            raise ValueError("relevant: offsets not monotone or outside the rows")
        lens = np.diff(off)
        rows = rows[off[0]:off[-1]]
    else:
        if len(relevant) != R:
            raise ValueError(f"relevant: {len(relevant)} sets for {R} lists")
        sets = [np.asarray(list(s) if s is not None else [], dtype=np.int64).reshape(-1) for s in relevant]
        lens = np.array([s.size for s in sets], np.int64)
        rows = np.concatenate(sets) if sets else np.zeros(0, np.int64)
    if rows.size and (rows.min() < 0 or rows.max() >= n_items):
        raise ValueError(f"relevant: item row outside [0, {n_items})")
    seg = np.repeat(np.arange(R, dtype=np.int64), lens)
    key = np.unique(seg * int(n_items) + rows)            # sorted by (list, row), duplicates gone
    seg, rows = key // int(n_items), key % int(n_items)
    off = np.zeros(R + 1, np.int64)
    np.cumsum(np.bincount(seg, minlength=R), out=off[1:])
    return np.ascontiguousarray(rows), off


def _list_check(n, n_off, n_counts, table_shape, n_inv, at, n_scores, n_info, ks):
    """The ValueErrors of list_metrics that need no device."""
    ks = tuple(int(k) for k in ks)
    at = int(at)
    if not 1 <= at <= LIST_MAX_AT:
        raise ValueError(f"list_metrics: at = {at} outside [1, {LIST_MAX_AT}]")
    if len(ks) > _lib.GROUP_MAX_K:
        raise ValueError(f"at most {_lib.GROUP_MAX_K} cutoffs")
    if any(k < 1 for k in ks) or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"list_metrics: ks = {ks} must be positive and strictly ascending")
    if ks and ks[-1] > at:
        raise ValueError(f"list_metrics: cutoff {ks[-1]} above at = {at}")
    if n_off < 1:
        raise ValueError("list_metrics: offsets needs R + 1 entries")
    R = n_off - 1
    if n_counts is not None and n_counts != R:
        raise ValueError(f"list_metrics: {n_counts} counts for {R} lists")
    if len(table_shape) != 2 or table_shape[0] < 1:
        raise ValueError("list_metrics: table must be [n_items, d] with n_items >= 1")
    if n_inv is not None and n_inv != table_shape[0]:
        raise ValueError(f"list_metrics: {n_inv} inverse norms for {table_shape[0]} table rows")
    if n_scores is not None and n_scores != n:
        raise ValueError(f"list_metrics: {n_scores} scores beside {n} rows")
    if n_info is not None and n_info != table_shape[0]:
        raise ValueError(f"list_metrics: {n_info} info weights for {table_shape[0]} items")
    return R, at, ks


def _list_launch(rows, offsets, counts, table, inv, at, scores, info, rel, ks, per_list, ws, out=None):
    """Enqueue dcnr_eval_list_metrics on the current stream; every argument a
    device tensor of the right dtype (or None), ``rel`` a (rows, offsets) pair
    or None.  Returns (summary bytes on the device, records or None): nothing
    is read back here."""
    lib = _lib.load()
    dev = rows.device
    R, n, nk = offsets.numel() - 1, rows.numel(), len(ks)
    n_items, d = table.shape
    ks_arr = (ctypes.c_int32 * max(1, nk))(*ks)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        disc, ideal = _device_tables(ks[-1], dev) if nk else (None, None)
        if ws is None:
            ws = torch.empty(list_workspace_bytes(R, n_items), dtype=torch.uint8, device=dev)
        if out is None:
            out = torch.empty(ctypes.sizeof(_lib.ListSummaryStruct), dtype=torch.uint8, device=dev)
        rec = None
        if per_list:
            rec = torch.empty((R, ctypes.sizeof(_lib.ListRecordStruct) // 8), dtype=torch.int64, device=dev)
        _lib.check(lib.dcnr_eval_list_metrics(
            ptr(rows), n, offsets.data_ptr(), counts.data_ptr() if counts is not None else None, R, at,
            table.data_ptr(), inv.data_ptr(), d, n_items, ptr(scores) if scores is not None else None,
            info.data_ptr() if info is not None else None,
            ptr(rel[0]) if rel is not None else None, rel[0].numel() if rel is not None else 0,
            rel[1].data_ptr() if rel is not None else None, ks_arr, nk,
            ptr(disc), ptr(ideal), out.data_ptr(), ptr(rec), ptr(ws), ws.numel(),
            _lib.stream_ptr(dev)), "dcnr_eval_list_metrics")
    return out, rec


def _list_result(raw: bytes, ks, rec) -> ListMetrics:
    m = _lib.ListSummaryStruct.from_buffer_copy(raw)
    nk = len(ks)
    records = None
    if rec is not None:
        f64 = lambda a: a.view(torch.float64)
        records = {"m": rec[:, 0], "n_rel": rec[:, 1], "first_hit_rank": rec[:, 2],
                   "hits": rec[:, 3:3 + nk], "pair_cos_sum": f64(rec[:, 7]), "score_sum": f64(rec[:, 8]),
                   "info_sum": f64(rec[:, 9]), "dcg": f64(rec[:, 10:10 + nk])}
    return ListMetrics(float(m.ild), float(m.coverage), float(m.gini), float(m.mean_score),
                       float(m.mean_info), float(m.mrr), tuple(ks),
                       tuple(float(m.hit_rate[j]) for j in range(nk)),
                       tuple(float(m.recall[j]) for j in range(nk)),
                       tuple(float(m.ndcg[j]) for j in range(nk)),
                       int(m.n_lists), int(m.n_lists_scored), int(m.n_lists_pairs), int(m.n_marked),
                       int(m.n_bad_list), int(m.n_entries), int(m.n_distinct_items), int(m.gini_num),
                       int(m.n_rel_lists), tuple(int(m.hit_lists[j]) for j in range(nk)), records)


def empty_list_metrics(R: int, ks) -> ListMetrics:
    """What dcnr_eval_list_metrics gives for R lists that are all empty and
    have no held-out sets: the counts 0, coverage 0, every mean NaN."""
    nan, nk = float("nan"), len(ks)
    return ListMetrics(nan, 0.0, nan, nan, nan, nan, tuple(ks), (nan,) * nk, (nan,) * nk, (nan,) * nk,
                       int(R), 0, 0, 0, 0, 0, 0, 0, 0, (0,) * nk, None)


def list_metrics_raw(rows, offsets, counts=None, *, table, inv_norms, at=20, scores=None, info=None,
                     relevant=None, ks=(5, 10, 20), per_list=False, ws=None) -> ListMetrics:
    """dcnr_eval_list_metrics on device tensors as they come: ``relevant`` is a
    device ``(rows, offsets)`` pair whose sets are already ascending and
    distinct, ``info`` a float64 device tensor, ``ws`` a uint8 device workspace
    of at least ``list_workspace_bytes(R, n_items)`` bytes (allocated when
    None).  One wait: the 248-byte copy of the summary."""
    R, at, ks = _list_check(rows.numel(), offsets.numel(), None if counts is None else counts.numel(),
                            tuple(table.shape), inv_norms.numel(), at,
                            None if scores is None else scores.numel(),
                            None if info is None else info.numel(), ks)
    if relevant is not None and relevant[1].numel() != R + 1:
        raise ValueError(f"relevant: {relevant[1].numel()} offsets for {R} lists")
    if rows.device.type != 'cuda':
        raise RuntimeError("dcnr.list_metrics runs on the HIP device only")
    out, rec = _list_launch(rows, offsets, counts, table, inv_norms, at, scores, info, relevant, ks,
                            per_list, ws)
    return _list_result(out.cpu().numpy().tobytes(), ks, rec)   # the one D2H copy


def list_metrics(rows, offsets, counts=None, *, table, inv_norms=None, at=20, scores=None, info=None,
                 relevant=None, ks=(5, 10, 20), per_list=False) -> ListMetrics:
    """What R served lists look like, measured on the device where the batched
    serving calls left them.  List r is ``rows[offsets[r] : offsets[r] +
    counts[r]]`` (``counts=None``: whole segments), measured on its first
    ``min(count, at)`` positions.

    table, inv_norms  the item embeddings [n_items, d] and their inverse norms
                   (None: ``dcnr.serving.row_inv_norms(table)``)
    scores         the logits beside ``rows`` (mean_score), or None
    info           a float64 weight per item, e.g. ``popularity_information``
                   (mean_info), or None
    relevant       held-out items per list: a list of R iterables, or a TUPLE
                   (rows, offsets); sorted and de-duplicated here, on the host
    ks             up to 4 ascending cutoffs <= at for hit rate / recall / NDCG

    ``ild`` is the mean over lists of 1 - the mean pairwise cosine;
    ``coverage`` the share of items in some list; ``gini`` the Gini coefficient
    of the items' exposure counts (0: every item shown equally often).  A list
    whose first row is -1 (an answer the device marked) and a list with a bad
    offset, count or row is skipped and counted in ``n_marked`` /
    ``n_bad_list``.  Waits once, to read the summary."""
    as_t = lambda a, dt: a.detach() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=dt)
    rows, offsets = as_t(rows, torch.int64).reshape(-1), as_t(offsets, torch.int64).reshape(-1)
    table = as_t(table, torch.float32)
    if counts is not None:
        counts = as_t(counts, torch.int32).reshape(-1)
    if scores is not None:
        scores = as_t(scores, torch.float32).reshape(-1)
    if info is not None:
        info = as_t(info, torch.float64).reshape(-1)
    if inv_norms is not None:
        inv_norms = as_t(inv_norms, torch.float32).reshape(-1)
    R, at, ks = _list_check(rows.numel(), offsets.numel(), None if counts is None else counts.numel(),
                            tuple(table.shape), None if inv_norms is None else inv_norms.numel(), at,
                            None if scores is None else scores.numel(),
                            None if info is None else info.numel(), ks)
    rel = relevant_csr(relevant, R, table.shape[0]) if relevant is not None else None
    dev = next((t.device for t in (rows, table, offsets) if t.device.type == 'cuda'), None)
    if dev is None:
        raise RuntimeError("dcnr.list_metrics runs on the HIP device only")
    on = lambda t, dt: None if t is None else t.to(device=dev, dtype=dt).contiguous()
    table = on(table, torch.float32)
    if inv_norms is None:
        from .serving import row_inv_norms
        inv_norms = row_inv_norms(table)
    if rel is not None:
        rel = tuple(torch.from_numpy(a).to(dev) for a in rel)
    return list_metrics_raw(on(rows, torch.int64), on(offsets, torch.int64), on(counts, torch.int32),
                            table=table, inv_norms=on(inv_norms, torch.float32), at=at,
                            scores=on(scores, torch.float32), info=on(info, torch.float64),
                            relevant=rel, ks=ks, per_list=per_list)


def _eval_logits(model, collab, cat, num, batch_size):
    """(device, collab on it, logits [N]) of one eval-mode forward over the
    split in chunks of ``batch_size``, the model's mode restored."""
    dev = model._check_device()
    collab, cat, num = (t.to(dev) for t in (collab, cat, num))   # train.py:230-231
    N = collab.shape[0]
    if N == 0:
        raise ValueError("evaluate: empty split")
    step = N if batch_size is None else int(batch_size)
    if step < 1:
        raise ValueError("batch_size must be >= 1")
    logits = torch.empty(N, dtype=torch.float32, device=dev)
    was_training = model.training
    model.eval()
    try:
        for lo in range(0, N, step):
            hi = min(N, lo + step)
            logits[lo:hi] = model(collab[lo:hi, 0], collab[lo:hi, 1], cat[lo:hi], num[lo:hi]).reshape(-1)
    finally:
        model.train(was_training)
    return dev, collab, logits


@torch.no_grad()
def evaluate_ranking(model, collab, cat, num, y, group_by='user', ks=(5, 10, 20), batch_size=None):
    """``evaluate`` and the per-group ranking metrics from one forward:
    ``(Metrics, GroupMetrics)`` of the same logits buffer.  ``group_by``:
    'user' (``collab[:, 0]``), 'item' (``collab[:, 1]``) or an int64 tensor [N]
    of group ids."""
    dev, collab, logits = _eval_logits(model, collab, cat, num, batch_size)
    if isinstance(group_by, str):
        if group_by not in ('user', 'item'):
            raise ValueError("group_by is 'user', 'item' or a tensor of group ids")
        groups = collab[:, 0 if group_by == 'user' else 1]
    else:
        groups = torch.as_tensor(group_by).to(dev)
    y = y.to(dev)
    return eval_metrics(logits, y), group_metrics(logits, y, groups, ks=ks)


@torch.no_grad()
def evaluate(model, collab, cat, num, y, batch_size=None) -> Metrics:
    """The reference's validation pass (train.py:229-233, 255-265): eval-mode
    forward of the whole split -- ``collab`` [N, 2] holds (user, item) as
    X_collab does -- in chunks of ``batch_size`` when given, the logits in one
    device buffer, then the metrics over all N (the reference's single
    validation batch).  The model's train / eval mode is restored."""
    dev, _, logits = _eval_logits(model, collab, cat, num, batch_size)
    return eval_metrics(logits, y.to(dev))
