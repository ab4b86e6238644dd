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


@torch.no_grad()
def evaluate(model, collab, cat, num, y, batch_size=None) -> Metrics:
    """The reference's validation pass (train.py:229-233, 255-265): eval-mode
    forward of the whole split -- ``collab`` [N, 2] holds (user, item) as
    X_collab does -- in chunks of ``batch_size`` when given, the logits in one
    device buffer, then the metrics over all N (the reference's single
    validation batch).  The model's train / eval mode is restored."""
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
    return eval_metrics(logits, y.to(dev))
