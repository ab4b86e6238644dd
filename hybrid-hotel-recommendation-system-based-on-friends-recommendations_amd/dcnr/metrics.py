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
