"""The reference's ``prepare_data`` (train.py:36-87) and the filter and derived
columns its driver runs before it (train.py:280-287), on the device.

``prepare_data`` turns main_df's raw review columns into the reference's
``(collab, cat, num, y)`` training and validation tensors and its preprocessing
artifacts, bit for bit, with one native call (dcnr_train_table_build), one read
of its pinned count words, a host ``RandomState`` permutation and one
dcnr_gather_rows per split.  What comes out plugs into ``DeviceLoader``,
``FusedTrainer.fit``, ``DCN_RecSys(*model_dims, params)`` and
``ItemFeatures.set_scaler``.  ``prepare_data_host`` is the numpy yardstick of the
same contract; it needs neither pandas nor scikit-learn.
Both results keep the fit's ``derived`` and ``noise_filter``, and their
``preprocessor()`` applies the fit to other rows (dcnr/transform.py).

Arguments of both: ``user``, ``item`` [M] raw ids (any int64); ``target`` [M]
0 / 1; ``cat`` a list of n_cat columns, each either int64 keys (negative:
missing) or values (``category_keys`` makes their keys); ``num`` [M][n_raw]
float64.  ``noise_filter=(column, lo, hi)`` keeps the rows whose raw column is
``>= hi`` or ``<= lo``; ``derived`` is a sequence of ``("ratio" | "diff", i, j)``
over raw columns, appended behind them in that order.
"""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .data import DeviceLoader

REQ_BAD_DATA = 2          # DCNR_REQ_BAD_DATA
N_COUNTS = 5              # DCNR_TRAIN_TABLE_COUNTS
DERIVED_OPS = {"ratio": 0, "diff": 1}   # DCNR_DERIVED_*


class TrainTableArgs(ctypes.Structure):
    """dcnr_train_table_args."""
    _fields_ = [
        ("user", ctypes.c_void_p), ("item", ctypes.c_void_p), ("target", ctypes.c_void_p),
        ("cat_key", ctypes.c_void_p), ("raw", ctypes.c_void_p),
        ("M", ctypes.c_int64), ("n_cat", ctypes.c_int32), ("n_raw", ctypes.c_int32),
        ("filter_col", ctypes.c_int32), ("filter_lo", ctypes.c_double), ("filter_hi", ctypes.c_double),
        ("n_derived", ctypes.c_int32), ("derived", ctypes.c_void_p),
        ("row", ctypes.c_void_p), ("collab", ctypes.c_void_p), ("cat", ctypes.c_void_p),
        ("num", ctypes.c_void_p), ("y", ctypes.c_void_p),
        ("user_ids", ctypes.c_void_p), ("item_ids", ctypes.c_void_p), ("cat_keys", ctypes.c_void_p),
        ("stats", ctypes.c_void_p), ("host_stats", ctypes.c_void_p),
        ("counts", ctypes.c_void_p), ("host_counts", ctypes.c_void_p),
    ]


# ------------------------------------------------------------------ categories
def _is_missing(v) -> bool:
    return v is None or (isinstance(v, (float, np.floating)) and v != v)


def category_keys(values) -> Tuple[np.ndarray, list]:
    """(keys int64 [M], categories): the key of a value is its rank among the
    sorted distinct non-missing values, as ``astype('category').cat.codes``
    numbers them; ``None`` and NaN get -1.  Integer input passes through as its
    own key (a negative one means missing); its categories are the sorted
    distinct non-negative keys."""
    a = np.asarray(values)
    if a.dtype.kind in "iub":
        keys = a.astype(np.int64).reshape(-1)
        return keys, np.unique(keys[keys >= 0]).tolist()
    a = a.reshape(-1)
    if a.dtype.kind == "f":
        miss = np.isnan(a)
        cats, inv = np.unique(a[~miss], return_inverse=True)
    elif a.dtype.kind in "US":
        miss = np.zeros(a.size, dtype=bool)
        cats, inv = np.unique(a, return_inverse=True)
    else:
        miss = np.fromiter((_is_missing(v) for v in a), dtype=bool, count=a.size)
        cats = sorted(set(a[~miss].tolist()))
        code = {c: i for i, c in enumerate(cats)}
        inv = np.fromiter((code[v] for v in a[~miss].tolist()), dtype=np.int64, count=int((~miss).sum()))
        cats = np.asarray(cats, dtype=object)
    keys = np.full(a.size, -1, dtype=np.int64)
    keys[~miss] = inv
    return keys, cats.tolist()


def _derived_arg(derived, n_raw: int) -> np.ndarray:
    out = np.zeros((len(derived), 3), dtype=np.int32)
    for d, (op, i, j) in enumerate(derived):
        if op not in DERIVED_OPS:
            raise ValueError(f"derived column {d}: op {op!r} is neither 'ratio' nor 'diff'")
        if not (0 <= int(i) < n_raw and 0 <= int(j) < n_raw):
            raise ValueError(f"derived column {d}: columns ({i}, {j}) outside [0, {n_raw})")
        out[d] = (DERIVED_OPS[op], int(i), int(j))
    return out


def _filter_arg(noise_filter, n_raw: int):
    if noise_filter is None:
        return -1, 0.0, 0.0
    col, lo, hi = noise_filter
    if not 0 <= int(col) < n_raw:
        raise ValueError(f"noise_filter column {col} outside [0, {n_raw})")
    return int(col), float(lo), float(hi)


def split_indices(n: int, test_size: float = 0.2, random_state: int = 42):
    """(train, val) positions of ``train_test_split(arange(n), test_size=,
    random_state=)``: ``n_test = ceil(test_size * n)``, the rest trains;
    validation is the head of ``RandomState(random_state).permutation(n)``."""
    if n <= 0:
        raise ValueError("With n_samples=0 the resulting train set will be empty.")
    n_test = int(math.ceil(test_size * n))
    n_train = n - n_test
    if n_train <= 0:
        raise ValueError(f"With n_samples={n} and test_size={test_size} the resulting train set "
                         "will be empty.")
    perm = np.random.RandomState(random_state).permutation(n)
    return perm[n_test:n_test + n_train].astype(np.int64), perm[:n_test].astype(np.int64)


# -------------------------------------------------------------------- results
def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


class _Prepared:
    """What both fronts return (numpy arrays from ``prepare_data_host``, device
    tensors from ``prepare_data``)."""
    cat_names: List[str]
    numerical_cols: Optional[List[str]] = None

    def _categories(self, c):
        cats = self._cat_categories[c]
        keys = _host(self.cat_keys[c]).tolist()
        return keys if cats is None else [cats[k] for k in keys]

    @property
    def user_id_mapping(self) -> dict:
        if self._user_map is None:
            self._user_map = {int(v): i for i, v in enumerate(_host(self.user_ids).tolist())}
        return self._user_map

    @property
    def item_id_mapping(self) -> dict:
        if self._item_map is None:
            self._item_map = {int(v): i for i, v in enumerate(_host(self.item_ids).tolist())}
        return self._item_map

    @property
    def cat_encoders(self) -> dict:
        if self._encoders is None:
            self._encoders = {name: {c: i for i, c in enumerate(self._categories(k))}
                              for k, name in enumerate(self.cat_names)}
        return self._encoders

    def preprocessor(self):
        """The fitted state as a ``Preprocessor``: ``transform`` encodes rows the
        fit has not seen (dcnr/transform.py)."""
        from .transform import Preprocessor
        return Preprocessor(self.user_ids, self.item_ids, self.cat_keys, self._cat_categories, self.median_,
                            self.scale_, self.min_, self.cat_names, derived=self.derived,
                            noise_filter=self.noise_filter)

    def artifacts(self) -> dict:
        """The reference's ``artifacts`` dict (train.py:80-84); the scaler entry
        holds MinMaxScaler's fitted arrays (joblib stays with the caller)."""
        n_num = int(self.scale_.size)
        return {
            "user_id_mapping": self.user_id_mapping, "item_id_mapping": self.item_id_mapping,
            "scaler": {"scale_": self.scale_, "min_": self.min_, "data_min_": self.data_min_,
                       "data_max_": self.data_max_, "data_range_": self.data_max_ - self.data_min_},
            "cat_encoders": self.cat_encoders,
            "numerical_cols": self.numerical_cols or [f"num{c}" for c in range(n_num)],
            "categorical_cols": list(self.cat_names),
        }


class HostPrepared(_Prepared):
    pass


class PreparedData(_Prepared):
    """``prepare_data``'s result: ``train`` and ``val`` (collab, cat, num, y)
    device tensors in ``DeviceLoader``'s and ``FusedTrainer.fit``'s order,
    ``rows_train`` / ``rows_val`` their input positions, ``model_dims`` for
    ``DCN_RecSys(*model_dims, params)``, the fitted ``scale_``, ``min_``,
    ``data_min_``, ``data_max_`` and ``median_`` as host float64, and the id maps
    and category encoders in the reference's ``artifacts`` layout (built from the
    id and key lists when first read).  ``full`` and ``rows`` are the unsplit
    tables."""

    def loader(self, batch_size: int, shuffle: bool = True, generator=None) -> DeviceLoader:
        """A ``DeviceLoader`` over ``train`` (the tensors are used where they
        are)."""
        return DeviceLoader(*self.train, batch_size=batch_size, shuffle=shuffle, generator=generator,
                            device=self.train[0].device)


def _finish(out: _Prepared, cat_names, n_num, derived=(), noise_filter=None):
    out.cat_names = list(cat_names)
    out.derived = [(str(op), int(i), int(j)) for op, i, j in derived]
    out.noise_filter = None if noise_filter is None else tuple(noise_filter)
    out._user_map = out._item_map = out._encoders = None
    out.model_dims = (int(len(out.user_ids)), int(len(out.item_ids)),
                      {name: int(len(out.cat_keys[k])) for k, name in enumerate(cat_names)}, int(n_num))
    return out


def _cat_columns(cat, M):
    """Per column (keys or a device tensor, categories or None)."""
    if cat is None:
        return []
    if isinstance(cat, torch.Tensor):
        if cat.dim() == 1:
            cat = cat.reshape(M, 1)
        return [(cat[:, c], None) for c in range(cat.shape[1])]
    cols = []
    for col in cat:
        if isinstance(col, torch.Tensor):
            cols.append((col.reshape(-1), None))
            continue
        a = np.asarray(col)
        if a.dtype.kind in "iub":
            cols.append((a.astype(np.int64).reshape(-1), None))
        else:
            cols.append(category_keys(a))
    return cols


def _names(cat_names, n_cat):
    names = list(cat_names) if cat_names is not None else [f"cat{c}" for c in range(n_cat)]
    if len(names) != n_cat:
        raise ValueError(f"{len(names)} cat_names for {n_cat} categorical columns")
    return names


# --------------------------------------------------------------- numpy yardstick
def _median(v: np.ndarray) -> float:
    """Of the non-NaN float64 values v: v[k/2], or (v[k/2-1] + v[k/2]) / 2."""
    k = v.size
    if k == 0:
        return float("nan")
    s = np.sort(v)
    if k % 2:
        return float(s[k // 2])
    with np.errstate(all="ignore"):
        return float((s[k // 2 - 1] + s[k // 2]) / np.float64(2.0))


def prepare_data_host(user, item, target, cat, num, *, cat_names=None, noise_filter=None, derived=(),
                      test_size=0.2, random_state=42) -> HostPrepared:
    """The contract in numpy (the yardstick of ``prepare_data``)."""
    to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    user = to_np(user).astype(np.int64).reshape(-1)
    item = to_np(item).astype(np.int64).reshape(-1)
    M = user.size
    target = to_np(target).reshape(-1)
    raw = to_np(num).astype(np.float64) if num is not None else np.zeros((M, 0))
    raw = raw.reshape(M, 1) if raw.ndim == 1 else raw
    if raw.ndim != 2 or raw.shape[0] != M:
        raise ValueError("num must be [M, columns]")
    n_raw = raw.shape[1]
    cols = [(to_np(k).astype(np.int64), c) for k, c in _cat_columns(cat, M)]
    names = _names(cat_names, len(cols))
    dv = _derived_arg(derived, n_raw)
    fcol, lo, hi = _filter_arg(noise_filter, n_raw)

    with np.errstate(all="ignore"):
        keep = np.ones(M, dtype=bool) if fcol < 0 else (raw[:, fcol] >= hi) | (raw[:, fcol] <= lo)
        extra = []
        for op, i, j in dv:
            if op == DERIVED_OPS["ratio"]:
                v = raw[:, i] / raw[:, j]
                v[~np.isfinite(v)] = 0.0
            else:
                v = raw[:, i] - raw[:, j]
            extra.append(v)
        x = np.column_stack([raw] + extra) if extra else raw.copy()
        n_num = x.shape[1]
        x = x[keep]
        median = np.array([_median(x[~np.isnan(x[:, c]), c]) for c in range(n_num)], dtype=np.float64)
        for c in range(n_num):
            x[np.isnan(x[:, c]), c] = median[c]
        key = np.stack([k[keep] for k, _ in cols], axis=1) if cols else np.zeros((x.shape[0], 0), np.int64)
        live = (key >= 0).all(axis=1)
        rows = np.flatnonzero(keep)[live].astype(np.int32)
        x, key = x[live], key[live]
        n = rows.size

        def first_appearance(ids):
            uniq, first, inv = np.unique(ids, return_index=True, return_inverse=True)
            order = np.argsort(first, kind="stable")
            code = np.empty(order.size, dtype=np.int64)
            code[order] = np.arange(order.size)
            return uniq[order], code[inv.reshape(-1)]
        user_ids, ucode = first_appearance(user[rows])
        item_ids, icode = first_appearance(item[rows])
        cat_keys, codes = [], []
        for c in range(len(cols)):
            present, inv = np.unique(key[:, c], return_inverse=True)
            cat_keys.append(present)
            codes.append(inv.reshape(-1).astype(np.int64))
        if np.isinf(x).any():
            raise ValueError("Input X contains infinity or a value too large for dtype('float64').")
        if n == 0:
            raise ValueError("Found array with 0 sample(s) while a minimum of 1 is required.")
        nan = np.float64("nan")
        all_nan = np.isnan(x).all(axis=0)
        safe = np.where(np.isnan(x), np.inf, x)
        data_min = np.where(all_nan, nan, safe.min(axis=0))
        safe = np.where(np.isnan(x), -np.inf, x)
        data_max = np.where(all_nan, nan, safe.max(axis=0))
        rng = data_max - data_min
        div = rng.copy()
        div[div < 10.0 * np.finfo(np.float64).eps] = 1.0
        scale = 1.0 / div
        mn = 0.0 - data_min * scale
        xs = x * scale
        xs = xs + mn
        num_out = xs.astype(np.float32)

    out = HostPrepared()
    out.rows = rows
    out.full = (np.stack([ucode, icode], axis=1).reshape(n, 2),
                np.stack(codes, axis=1) if codes else np.zeros((n, 0), np.int64),
                num_out, (target[rows] != 0).astype(np.float32))
    out.user_ids, out.item_ids, out.cat_keys = user_ids, item_ids, cat_keys
    out._cat_categories = [c for _, c in cols]
    out.median_, out.data_min_, out.data_max_, out.scale_, out.min_ = median, data_min, data_max, scale, mn
    out.n_after_filter = int(keep.sum())
    _finish(out, names, n_num, derived, noise_filter)
    tr, va = split_indices(n, test_size, random_state)
    out.train = tuple(t[tr] for t in out.full)
    out.val = tuple(t[va] for t in out.full)
    out.rows_train, out.rows_val = rows[tr], rows[va]
    return out


# --------------------------------------------------------------------- device
def train_table(user, item, target, cat_key, raw, *, noise_filter=None, derived=(), device="cuda"):
    """dcnr_train_table_build over device (or host) columns: the unsplit tables
    as a dict of device tensors and host arrays, after the one host wait.
    ``cat_key`` is int64 [M][n_cat], ``raw`` float64 [M][n_raw], ``target`` uint8."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("prepare_data runs on the HIP device; prepare_data_host is the numpy path")
    lib = _lib.load()
    on = lambda t, dt: torch.as_tensor(t).to(device=dev, dtype=dt).contiguous()
    user, item = on(user, torch.int64).reshape(-1), on(item, torch.int64).reshape(-1)
    M = int(user.numel())
    target = torch.as_tensor(target).to(dev).reshape(-1)
    target = (target != 0).to(torch.uint8) if target.dtype != torch.uint8 else target.contiguous()
    two_d = lambda t: t.reshape(M, 1) if t.dim() == 1 else t
    cat_key = two_d(on(cat_key, torch.int64)) if cat_key is not None else \
        torch.zeros((M, 0), dtype=torch.int64, device=dev)
    raw = two_d(on(raw, torch.float64)) if raw is not None else \
        torch.zeros((M, 0), dtype=torch.float64, device=dev)
    if cat_key.dim() != 2 or raw.dim() != 2:
        raise ValueError("cat_key and num must be [M, columns]")
    if any(int(t.shape[0]) != M for t in (item, target, cat_key, raw)):
        raise ValueError("Size mismatch between columns")
    n_cat, n_raw = int(cat_key.shape[1]), int(raw.shape[1])
    dv = _derived_arg(derived, n_raw)
    n_num = n_raw + len(dv)
    fcol, lo, hi = _filter_arg(noise_filter, n_raw)
    with torch.cuda.device(dev):
        nb = int(lib.dcnr_train_table_workspace_size(M, n_cat, n_raw, len(dv)))
        if nb == 0:
            raise RuntimeError(f"prepare_data: the device build does not take this shape "
                               f"(M={M}, n_cat={n_cat}, n_num={n_num})")
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        ws = new(nb, torch.uint8)
        row, collab, cat = new(M, torch.int32), new((M, 2), torch.int64), new((M, n_cat), torch.int64)
        num, y = new((M, n_num), torch.float32), new(M, torch.float32)
        user_ids, item_ids, cat_keys = new(M, torch.int64), new(M, torch.int64), new((n_cat, M), torch.int64)
        stats, counts = new((5, n_num), torch.float64), new(N_COUNTS + n_cat, torch.int32)
        pin_counts = torch.zeros(N_COUNTS + n_cat, dtype=torch.int32).pin_memory()
        pin_stats = torch.zeros((5, n_num), dtype=torch.float64).pin_memory()
        p = lambda t: t.data_ptr() if t.numel() else None
        a = TrainTableArgs(p(user), p(item), p(target), p(cat_key), p(raw), M, n_cat, n_raw, fcol, lo, hi,
                           len(dv), dv.ctypes.data if len(dv) else None, p(row), p(collab), p(cat), p(num),
                           p(y), p(user_ids), p(item_ids), p(cat_keys), p(stats), p(pin_stats),
                           counts.data_ptr(), pin_counts.data_ptr())
        _lib.check(lib.dcnr_train_table_build(ctypes.byref(a), p(ws), nb, _lib.stream_ptr(dev)),
                   "dcnr_train_table_build")
        torch.cuda.current_stream(dev).synchronize()   # the one host wait
    c = pin_counts.numpy().copy()
    n, n_users, n_items, n_after, status = (int(v) for v in c[:N_COUNTS])
    st = pin_stats.numpy().copy()
    return dict(n=n, n_users=n_users, n_items=n_items, n_after_filter=n_after, status=status,
                cat_counts=[int(v) for v in c[N_COUNTS:]], stats=st, n_num=n_num,
                row=row[:n], collab=collab[:n], cat=cat[:n], num=num[:n], y=y[:n],
                user_ids=user_ids[:n_users], item_ids=item_ids[:n_items],
                cat_keys=[cat_keys[k, :int(c[N_COUNTS + k])] for k in range(n_cat)],
                counts=counts, device_stats=stats)


def prepare_data(user, item, target, cat, num, *, cat_names=None, noise_filter=None, derived=(),
                 test_size=0.2, random_state=42, device="cuda") -> PreparedData:
    """The reference's filter, derived columns and ``prepare_data`` on the device
    (see the module docstring).  Raises ``ValueError`` where the reference does:
    a surviving +-inf, no surviving row, an empty train set."""
    dev = torch.device(device)
    user_t = torch.as_tensor(user)
    M = int(user_t.numel())
    cols = _cat_columns(cat, M)
    names = _names(cat_names, len(cols))
    if cols:
        cat_key = torch.stack([torch.as_tensor(k).to(device=dev, dtype=torch.int64).reshape(-1)
                               for k, _ in cols], dim=1)
    else:
        cat_key = None
    t = train_table(user_t, item, target, cat_key, num, noise_filter=noise_filter, derived=derived,
                    device=dev)
    if t["status"] & REQ_BAD_DATA:
        raise ValueError("Input X contains infinity or a value too large for dtype('float64').")
    n = t["n"]
    if n == 0:
        raise ValueError("Found array with 0 sample(s) while a minimum of 1 is required.")
    tr, va = split_indices(n, test_size, random_state)   # (raises before any gather)

    out = PreparedData()
    out.rows = t["row"]
    out.full = (t["collab"], t["cat"], t["num"], t["y"])
    out.user_ids, out.item_ids, out.cat_keys = t["user_ids"], t["item_ids"], t["cat_keys"]
    out._cat_categories = [c for _, c in cols]
    out.median_, out.data_min_, out.data_max_, out.scale_, out.min_ = (t["stats"][q] for q in range(5))
    out.n_after_filter = t["n_after_filter"]
    _finish(out, names, t["n_num"], derived, noise_filter)

    lib = _lib.load()
    src = list(out.full) + [out.rows]
    row_bytes = (ctypes.c_int64 * 5)(*[s.element_size() * (s[0].numel() if s.dim() > 1 else 1) for s in src])

    def gather(idx):
        idx = torch.from_numpy(idx).to(dev)
        B = int(idx.numel())
        dst = [torch.empty((B,) + tuple(s.shape[1:]), dtype=s.dtype, device=dev) for s in src]
        # (a column of width 0 has nothing to move and no pointer to give)
        live = [k for k, s in enumerate(src) if row_bytes[k] > 0]
        if B and live:
            rb = (ctypes.c_int64 * len(live))(*[row_bytes[k] for k in live])
            with torch.cuda.device(dev):
                _lib.check(lib.dcnr_gather_rows(idx.data_ptr(), B, n, len(live),
                                                _lib.ptr_array([src[k] for k in live]),
                                                _lib.ptr_array([dst[k] for k in live]), rb,
                                                _lib.stream_ptr(dev)), "dcnr_gather_rows")
        return tuple(dst[:4]), dst[4]
    out.train, out.rows_train = gather(tr)
    out.val, out.rows_val = gather(va)
    return out
