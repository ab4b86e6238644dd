"""A fitted preprocessing applied to rows it was not fitted on: what the
reference's service does on every request (``preprocess_for_ranking``,
main.py:215-230) and what scoring or fine-tuning on later reviews needs, on the
device.

``IdMap`` is a raw-id dictionary: an open-addressing hash table of int64 keys on
the device (dcnr_id_map_build / dcnr_id_map_lookup) with a numpy twin
(``lookup_host``).  ``Preprocessor`` is the fitted state of ``prepare_data`` (or
of the reference's ``artifacts`` dict): ``transform`` encodes new rows with one
native call (dcnr_rows_transform) and one read of its pinned count words;
``transform_host`` is the numpy yardstick of the same contract (DESIGN.md
section 9).  Both take ``prepare_data``'s column arguments.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib
from .prepare import REQ_BAD_DATA, _derived_arg, _filter_arg, _host, _is_missing

RESERVED_ID = -(1 << 63)     # an empty slot of the table: no legal id
REQ_OVERFLOW = 1             # DCNR_REQ_OVERFLOW
N_COUNTS = 5                 # DCNR_ROWS_TRANSFORM_COUNTS
INF_MESSAGE = "Input X contains infinity or a value too large for dtype('float64')."


class RowsTransformArgs(ctypes.Structure):
    """dcnr_rows_transform_args."""
    _fields_ = [
        ("user", ctypes.c_void_p), ("item", ctypes.c_void_p), ("target", ctypes.c_void_p),
        ("cat_key", ctypes.c_void_p), ("raw", ctypes.c_void_p),
        ("M", ctypes.c_int64), ("n_cat", ctypes.c_int32), ("n_raw", ctypes.c_int32),
        ("filter_col", ctypes.c_int32), ("filter_lo", ctypes.c_double), ("filter_hi", ctypes.c_double),
        ("n_derived", ctypes.c_int32), ("derived", ctypes.c_void_p),
        ("fill_nan", ctypes.c_int32), ("drop_unknown", ctypes.c_int32),
        ("user_table", ctypes.c_void_p), ("user_capacity", ctypes.c_int64), ("n_users", ctypes.c_int64),
        ("item_table", ctypes.c_void_p), ("item_capacity", ctypes.c_int64), ("n_items", ctypes.c_int64),
        ("cat_keys", ctypes.c_void_p), ("cat_offsets", ctypes.c_void_p),
        ("fit", ctypes.c_void_p),
        ("row", ctypes.c_void_p), ("collab", ctypes.c_void_p), ("cat", ctypes.c_void_p),
        ("num", ctypes.c_void_p), ("y", ctypes.c_void_p), ("unknown_bits", ctypes.c_void_p),
        ("counts", ctypes.c_void_p), ("host_counts", ctypes.c_void_p),
    ]


def _pow2_at_least(n: int) -> int:
    c = 1
    while c < n:
        c <<= 1
    return c


# ----------------------------------------------------------------------- IdMap
class IdMap:
    """A dictionary from distinct raw int64 ids to their positions in ``ids``.

    ``IdMap(prep.user_ids)`` numbers users as ``user_id_mapping`` does.  On a
    HIP device the ids live in an open-addressing hash table (capacity a power
    of two, at least ``2 * n``); ``device="cpu"`` keeps only the numpy side.
    -2**63 is reserved (it marks an empty slot): in ``ids`` it raises
    ``ValueError``, as a duplicate id does; as a query it is unknown.
    ``capacity=`` (a power of two >= n + 1) is for tests of a nearly full table.
    """

    def __init__(self, ids, device="cuda", capacity: Optional[int] = None):
        self.device = torch.device(device)
        t = ids if isinstance(ids, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(ids).astype(np.int64, copy=False).reshape(-1)))
        if t.dtype != torch.int64 or t.dim() != 1:
            t = t.to(torch.int64).reshape(-1)
        n = int(t.numel())
        cap = _pow2_at_least(max(2 * n, 1)) if capacity is None else int(capacity)
        if cap < n + 1 or cap & (cap - 1):
            raise ValueError(f"IdMap: capacity {cap} is not a power of two >= n + 1 = {n + 1}")
        self.capacity = cap
        self._n = n
        self._sorted = None
        if self.device.type != "cuda":
            self.ids = t.cpu()
            self._table = None
            s, _ = self._host_index()
            if n and (int(s[0]) == RESERVED_ID or bool((s[1:] == s[:-1]).any())):
                raise ValueError("IdMap: a duplicate id, or the reserved id -2**63")
            return
        lib = _lib.load()
        self.ids = t.to(self.device).contiguous()
        with torch.cuda.device(self.device):
            self._table = torch.empty((cap, 2), dtype=torch.int64, device=self.device)
            status = torch.zeros(1, dtype=torch.int32, device=self.device)
            pin = torch.zeros(1, dtype=torch.int32).pin_memory()
            _lib.check(lib.dcnr_id_map_build(self.ids.data_ptr() if n else None, n, self._table.data_ptr(), cap,
                                             status.data_ptr(), pin.data_ptr(), _lib.stream_ptr(self.device)),
                       "dcnr_id_map_build")
            torch.cuda.current_stream(self.device).synchronize()
        st = int(pin[0])
        if st & REQ_BAD_DATA:
            raise ValueError("IdMap: a duplicate id, or the reserved id -2**63")
        if st & REQ_OVERFLOW:
            raise RuntimeError("IdMap: the table is full")

    def __len__(self) -> int:
        return self._n

    def _host_index(self):
        if self._sorted is None:
            h = self.ids.cpu().numpy()
            order = np.argsort(h, kind="stable")
            self._sorted = (h[order], order.astype(np.int64))
        return self._sorted

    def lookup_host(self, raw, default: int = -1) -> np.ndarray:
        """int64 [M] in numpy: sorted ids and ``searchsorted``."""
        q = _host(raw).astype(np.int64, copy=False).reshape(-1)
        s, order = self._host_index()
        out = np.full(q.size, default, dtype=np.int64)
        if s.size and q.size:
            pos = np.minimum(np.searchsorted(s, q), s.size - 1)
            hit = (s[pos] == q) & (q != RESERVED_ID)
            out[hit] = order[pos[hit]]
        return out

    def lookup(self, raw, default: int = -1) -> torch.Tensor:
        """int64 device tensor [M]: the index of every query, ``default`` for an
        unknown id.  A device tensor is read where it is."""
        if self._table is None:
            raise RuntimeError("IdMap.lookup runs on the HIP device; lookup_host is the numpy path")
        q = raw if isinstance(raw, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(raw).astype(np.int64, copy=False).reshape(-1)))
        q = q.to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        M = int(q.numel())
        out = torch.empty(M, dtype=torch.int64, device=self.device)
        if M:
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().dcnr_id_map_lookup(self._table.data_ptr(), self.capacity, q.data_ptr(), M,
                                                          int(default), out.data_ptr(),
                                                          _lib.stream_ptr(self.device)), "dcnr_id_map_lookup")
        return out

    def _build_table(self, cap: int):
        """A fresh table of ``cap`` slots from ``ids`` (dcnr_id_map_build)."""
        n = self._n
        with torch.cuda.device(self.device):
            table = torch.empty((cap, 2), dtype=torch.int64, device=self.device)
            status = torch.zeros(1, dtype=torch.int32, device=self.device)
            pin = torch.zeros(1, dtype=torch.int32).pin_memory()
            _lib.check(_lib.load().dcnr_id_map_build(self.ids.data_ptr() if n else None, n, table.data_ptr(), cap,
                                                     status.data_ptr(), pin.data_ptr(),
                                                     _lib.stream_ptr(self.device)), "dcnr_id_map_build")
            torch.cuda.current_stream(self.device).synchronize()
        if int(pin[0]):
            raise RuntimeError(f"IdMap: rebuilding the table failed (status {int(pin[0])})")
        self._table, self.capacity = table, cap

    def insert_host(self, raw):
        """``insert`` in numpy (the yardstick, and the path of ``device="cpu"``):
        ``(indices int64 [M], new_ids int64 [n_new])``.  The distinct unknown ids
        are numbered ``len(self), len(self) + 1, ...`` in the order of their
        first appearance, as ``enumerate(df[col].unique())`` would have numbered
        them at fit time (train.py:42-43).  A device map's table is rebuilt from
        the grown ``ids``."""
        q = _host(raw).astype(np.int64, copy=False).reshape(-1)
        if (q == RESERVED_ID).any():
            raise ValueError("IdMap.insert: the reserved id -2**63")
        out = self.lookup_host(q, -1)
        unknown = np.flatnonzero(out < 0)
        uniq, first, inv = np.unique(q[unknown], return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")           # the distinct new ids by first appearance
        rank = np.empty(order.size, dtype=np.int64)
        rank[order] = np.arange(order.size, dtype=np.int64)
        out[unknown] = self._n + rank[inv.reshape(-1)]
        new_ids = uniq[order].astype(np.int64)
        if new_ids.size:
            self.ids = torch.cat([self.ids, torch.from_numpy(new_ids).to(self.ids.device)])
            self._n += int(new_ids.size)
            self._sorted = None
            if self._table is not None:
                self._build_table(max(self.capacity, _pow2_at_least(2 * self._n)))
        return out, new_ids

    def insert(self, raw, capacity: Optional[int] = None):
        """Admit the ids of ``raw`` the map does not hold (dcnr_id_map_insert):
        ``(indices, new_ids)``, device int64 ``[M]`` and ``[n_new]``.  ``raw`` is
        any batch -- known ids, new ones, duplicates; the distinct new ids get
        ``len(self), len(self) + 1, ...`` in the order of their first appearance
        and are appended to ``ids`` in that order.  The table keeps capacity
        >= 2 (n + M): a larger one is built from ``ids`` first (``capacity=``, a
        power of two above n, overrides that for tests of a nearly full table).
        One read of the pinned count words.  ``ValueError`` for the reserved id
        -2**63, with the map unchanged.  ``device="cpu"``: ``insert_host``."""
        if self._table is None:
            out, new = self.insert_host(raw)
            return torch.from_numpy(out), torch.from_numpy(new)
        q = raw if isinstance(raw, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(raw).astype(np.int64, copy=False).reshape(-1)))
        q = q.to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        M, n = int(q.numel()), self._n
        cap = max(self.capacity, _pow2_at_least(2 * (n + M))) if capacity is None else int(capacity)
        if cap < n + 1 or cap & (cap - 1):
            raise ValueError(f"IdMap.insert: capacity {cap} is not a power of two >= n + 1 = {n + 1}")
        if cap != self.capacity:
            self._build_table(cap)
        lib = _lib.load()
        with torch.cuda.device(self.device):
            nb = int(lib.dcnr_id_map_insert_workspace_size(M))
            if nb == 0:
                raise RuntimeError(f"IdMap.insert: the device call does not take M={M}: DCNR_UNSUPPORTED_SHAPE")
            new = lambda k, dt: torch.empty(k, dtype=dt, device=self.device)
            out, new_ids, ws = new(M, torch.int64), new(M, torch.int64), new(nb, torch.uint8)
            counts = new(2, torch.int32)
            pin = torch.zeros(2, dtype=torch.int32).pin_memory()
            p = lambda t: t.data_ptr() if t.numel() else None
            _lib.check(lib.dcnr_id_map_insert(self._table.data_ptr(), self.capacity, n, p(q), M, p(out), p(new_ids),
                                              counts.data_ptr(), pin.data_ptr(), p(ws), nb,
                                              _lib.stream_ptr(self.device)), "dcnr_id_map_insert")
            torch.cuda.current_stream(self.device).synchronize()   # the one host wait
        n_new, status = int(pin[0]), int(pin[1])
        if status & REQ_BAD_DATA:
            raise ValueError("IdMap.insert: the reserved id -2**63")
        if status & REQ_OVERFLOW:
            self._build_table(self.capacity)     # the table is unusable: back to the ids it had
            raise RuntimeError("IdMap.insert: the table is full")
        new_ids = new_ids[:n_new].clone()
        if n_new:
            self.ids = torch.cat([self.ids, new_ids])
            self._n += n_new
            self._sorted = None
        return out, new_ids


# ----------------------------------------------------------------- Transformed
class Transformed:
    """``transform``'s result.  ``collab`` int64 [n, 2], ``cat`` int64 [n, n_cat],
    ``num`` fp32 [n, n_num], ``y`` fp32 [n] or None; ``tensors`` those four in
    ``evaluate`` / ``fit`` order; ``rows`` int32 [n] the input positions kept;
    ``unknown_bits`` int64 [n] (bit 0 the user, bit 1 the hotel, bit 2 + c
    category c: the fallback was used; all zero under ``"drop"``).  Host counts:
    ``n``, ``n_filtered`` (rows the filter removed) and, over the rows that passed
    it, ``n_unknown_users``, ``n_unknown_items`` and ``n_unknown_cat[c]`` (an
    unseen or missing key).  Under ``"admit"`` bits 0 and 1 mean "admitted by
    this call", the two counts are the rows that carry such an id, and
    ``new_user_ids`` / ``new_item_ids`` (numpy int64, empty otherwise) are the
    admitted ids in the order of their new indices."""

    def __init__(self, collab, cat, num, y, rows, unknown_bits, n, n_filtered, n_unknown_users, n_unknown_items,
                 n_unknown_cat, new_user_ids=None, new_item_ids=None):
        self.collab, self.cat, self.num, self.y = collab, cat, num, y
        empty = np.zeros(0, dtype=np.int64)
        self.new_user_ids = empty if new_user_ids is None else new_user_ids
        self.new_item_ids = empty if new_item_ids is None else new_item_ids
        self.rows, self.unknown_bits = rows, unknown_bits
        self.n, self.n_filtered = int(n), int(n_filtered)
        self.n_unknown_users, self.n_unknown_items = int(n_unknown_users), int(n_unknown_items)
        self.n_unknown_cat = [int(v) for v in n_unknown_cat]

    @property
    def tensors(self):
        return (self.collab, self.cat, self.num, self.y)


# ---------------------------------------------------------------- Preprocessor
class Preprocessor:
    """The fitted state of ``prepare_data`` / ``prepare_data_host`` (their
    ``.preprocessor()``) or of the reference's ``artifacts`` dict
    (``from_artifacts``): ``user_ids``, ``item_ids``, per category column the
    ascending ``cat_keys`` and the ``categories`` the keys index (None: integer
    keys), ``median_``, ``scale_``, ``min_``, ``cat_names`` and the ``derived``
    and ``noise_filter`` of the fit."""

    def __init__(self, user_ids, item_ids, cat_keys, categories, median_, scale_, min_, cat_names,
                 derived=(), noise_filter=None):
        self.user_ids, self.item_ids = user_ids, item_ids
        self.cat_keys = list(cat_keys)
        self.categories = list(categories) if categories is not None else [None] * len(self.cat_keys)
        self.scale_ = np.asarray(scale_, dtype=np.float64).reshape(-1)
        self.min_ = np.asarray(min_, dtype=np.float64).reshape(-1)
        self.median_ = None if median_ is None else np.asarray(median_, dtype=np.float64).reshape(-1)
        self.cat_names = list(cat_names)
        self.derived = [(str(op), int(i), int(j)) for op, i, j in derived]
        self.noise_filter = None if noise_filter is None else tuple(noise_filter)
        self.n_cat, self.n_num = len(self.cat_keys), int(self.scale_.size)
        self.n_raw = self.n_num - len(self.derived)
        if len(self.cat_names) != self.n_cat or len(self.categories) != self.n_cat:
            raise ValueError(f"{len(self.cat_names)} cat_names for {self.n_cat} categorical columns")
        if self.min_.size != self.n_num or (self.median_ is not None and self.median_.size != self.n_num):
            raise ValueError("scale_, min_ and median_ differ in length")
        if self.n_raw < 0:
            raise ValueError(f"{len(self.derived)} derived columns for {self.n_num} numeric columns")
        self._dv = _derived_arg(self.derived, self.n_raw)
        self._cat_index = [None] * self.n_cat
        self._state = {}     # per device: id maps, category keys, the scaler
        self._host_state = None

    # ------------------------------------------------------------ construction
    @classmethod
    def from_artifacts(cls, artifacts, derived=(), median=None, noise_filter=None) -> "Preprocessor":
        """From the reference's ``artifacts`` dict (train.py:80-84): the id
        mappings' and the encoders' key order numbers the ids and categories; the
        scaler is a fitted ``MinMaxScaler`` or the dict ``artifacts()`` writes.
        ``derived`` names the derived columns among ``numerical_cols`` and
        ``median`` the medians ``fill_nan=True`` needs."""
        def keys_in_order(m, what):
            if list(m.values()) != list(range(len(m))):
                raise ValueError(f"{what}: the values are not 0 .. n - 1 in key order")
            return list(m.keys())
        user_ids = np.array(keys_in_order(artifacts["user_id_mapping"], "user_id_mapping"), dtype=np.int64)
        item_ids = np.array(keys_in_order(artifacts["item_id_mapping"], "item_id_mapping"), dtype=np.int64)
        names, cat_keys, categories = [], [], []
        for name, enc in artifacts["cat_encoders"].items():
            cats = keys_in_order(enc, f"cat_encoders[{name!r}]")
            names.append(name)
            if cats and all(isinstance(c, (int, np.integer)) and not isinstance(c, bool) for c in cats):
                keys = np.array(cats, dtype=np.int64)     # integer keys are their own categories
                if (np.diff(keys) <= 0).any():
                    raise ValueError(f"cat_encoders[{name!r}]: integer keys must ascend")
                cat_keys.append(keys)
                categories.append(None)
            else:
                cat_keys.append(np.arange(len(cats), dtype=np.int64))
                categories.append(cats)
        sc = artifacts["scaler"]
        get = (lambda k: sc[k]) if isinstance(sc, dict) else (lambda k: getattr(sc, k))
        return cls(user_ids, item_ids, cat_keys, categories, median, get("scale_"), get("min_"), names,
                   derived=derived, noise_filter=noise_filter)

    # ------------------------------------------------------------- categories
    def category_keys(self, c: int, values):
        """The fit's keys of a column's values: the index in the fitted
        categories, -1 for a missing value (None, NaN), -2 for an unseen one.
        Integer keys (and device tensors) pass through."""
        if isinstance(values, torch.Tensor):
            return values.reshape(-1)
        a = np.asarray(values)
        if a.dtype.kind in "iub":
            return a.astype(np.int64).reshape(-1)
        cats = self.categories[c]
        if cats is None:
            raise ValueError(f"category column {c} was fitted on integer keys")
        if self._cat_index[c] is None:
            self._cat_index[c] = {v: k for k, v in enumerate(cats)}
        index = self._cat_index[c]
        a = a.reshape(-1)
        if a.dtype.kind == "O":
            vals = a.tolist()
            return np.fromiter((-1 if _is_missing(v) else index.get(v, -2) for v in vals), dtype=np.int64,
                               count=len(vals))
        miss = np.isnan(a) if a.dtype.kind == "f" else np.zeros(a.size, dtype=bool)
        uniq, inv = np.unique(a[~miss], return_inverse=True)
        code = np.fromiter((index.get(v, -2) for v in uniq.tolist()), dtype=np.int64, count=uniq.size)
        keys = np.full(a.size, -1, dtype=np.int64)
        keys[~miss] = code[inv.reshape(-1)]
        return keys

    def _key_columns(self, cat, M):
        if cat is None:
            cols = []
        elif isinstance(cat, torch.Tensor):
            cat = cat.reshape(M, 1) if cat.dim() == 1 else cat
            cols = [cat[:, c] for c in range(cat.shape[1])]
        else:
            cols = list(cat)
        if len(cols) != self.n_cat:
            raise ValueError(f"{len(cols)} categorical columns; the fit has {self.n_cat}")
        return [self.category_keys(c, col) for c, col in enumerate(cols)]

    # ---------------------------------------------------------------- options
    @staticmethod
    def _policy(unknown) -> bool:
        if unknown not in ("reference", "drop", "admit"):
            raise ValueError(f"unknown={unknown!r} is neither 'reference' nor 'drop' nor 'admit'")
        return unknown == "drop"

    def _filter(self, noise_filter):
        if isinstance(noise_filter, str):
            if noise_filter != "fitted":
                raise ValueError(f"noise_filter={noise_filter!r}: 'fitted', a (column, lo, hi) or None")
            noise_filter = self.noise_filter
        return _filter_arg(noise_filter, self.n_raw)

    def _check_fill(self, fill_nan):
        if fill_nan and self.median_ is None and self.n_num:
            raise ValueError("fill_nan=True needs the fit's medians (from_artifacts(..., median=))")

    # -------------------------------------------------------------- admission
    @staticmethod
    def _check_reserved(*raws):
        for r in raws:
            if r is not None and bool((r == RESERVED_ID).any()):
                raise ValueError("admit: the reserved id -2**63")

    def _admit(self, which, raw, key):
        """Insert ``raw`` into the ``which`` ("users" / "items") map of every
        state this preprocessing holds -- first into the device state ``key``
        (None: the host state), whose numbering the others then repeat from the
        new ids in order -- and grow ``user_ids`` / ``item_ids``.  Returns
        (the indices of ``raw`` where the first insert ran, the new ids in numpy)."""
        k = 0 if which == "users" else 1
        if key is None:
            primary = self._host_fit()[k]
            idx, new = primary.insert_host(raw)
        else:
            primary = self._state[key][which]
            idx, new = primary.insert(raw)
            new = new.cpu().numpy()
        if new.size:
            for st in self._state.values():
                if st[which] is not primary:
                    st[which].insert(new)
            if self._host_state is not None and self._host_state[k] is not primary:
                self._host_state[k].insert_host(new)
            attr = "user_ids" if k == 0 else "item_ids"
            old = getattr(self, attr)
            if isinstance(old, torch.Tensor):
                grown = torch.cat([old.reshape(-1), torch.from_numpy(new).to(device=old.device, dtype=old.dtype)])
            else:
                grown = np.concatenate([np.asarray(old).reshape(-1), new.astype(np.asarray(old).dtype, copy=False)])
            setattr(self, attr, grown)
        return idx, new

    def admit(self, users=None, items=None):
        """Admit raw user and hotel ids the fit has not seen: each id map of
        every device state held, and of the host state, gets the distinct new
        ids numbered on from its length in the order of their first appearance
        (``IdMap.insert``), and ``user_ids`` / ``item_ids`` grow by them, so
        mappings built from those afterwards include the new ids.  Known ids
        and duplicates are fine.  Returns ``(new_user_ids, new_item_ids)``,
        numpy int64.  ``ValueError`` for the reserved id -2**63, with nothing
        changed."""
        as_ids = lambda r: None if r is None else (
            r.reshape(-1).to(torch.int64) if isinstance(r, torch.Tensor) else
            np.asarray(r).astype(np.int64, copy=False).reshape(-1))
        users, items = as_ids(users), as_ids(items)
        self._check_reserved(users, items)
        key = next(iter(self._state), None)
        out = []
        for which, raw in (("users", users), ("items", items)):
            out.append(np.zeros(0, dtype=np.int64) if raw is None else self._admit(which, raw, key)[1])
        return tuple(out)

    # ------------------------------------------------------------------ numpy
    def _host_fit(self):
        if self._host_state is None:
            self._host_state = (IdMap(_host(self.user_ids), device="cpu"), IdMap(_host(self.item_ids), device="cpu"),
                                [_host(k).astype(np.int64).reshape(-1) for k in self.cat_keys])
        return self._host_state

    def transform_host(self, user, item, target, cat, num, *, unknown="reference", fill_nan=True,
                       noise_filter=None) -> Transformed:
        """The contract in numpy (the yardstick of ``transform``)."""
        drop = self._policy(unknown)
        self._check_fill(fill_nan)
        fcol, lo, hi = self._filter(noise_filter)
        user = _host(user).astype(np.int64).reshape(-1)
        item = _host(item).astype(np.int64).reshape(-1)
        M = user.size
        raw = _host(num).astype(np.float64) if num is not None else np.zeros((M, 0))
        raw = raw.reshape(M, 1) if raw.ndim == 1 else raw
        keys = [_host(k).astype(np.int64).reshape(-1) for k in self._key_columns(cat, M)]
        tgt = None if target is None else _host(target).reshape(-1)
        if raw.ndim != 2 or raw.shape[1] != self.n_raw:
            raise ValueError(f"num must be [M, {self.n_raw}]")
        if any(a.shape[0] != M for a in [item, raw] + keys + ([] if tgt is None else [tgt])):
            raise ValueError("Size mismatch between columns")
        umap, imap, cat_keys = self._host_fit()
        with np.errstate(all="ignore"):
            passed = np.ones(M, dtype=bool) if fcol < 0 else (raw[:, fcol] >= hi) | (raw[:, fcol] <= lo)
            extra = []
            for op, i, j in self._dv:
                if op == 0:
                    v = raw[:, i] / raw[:, j]
                    v[~np.isfinite(v)] = 0.0
                else:
                    v = raw[:, i] - raw[:, j]
                extra.append(v)
            x = np.column_stack([raw] + extra) if extra else raw.copy()
            bits = np.zeros(M, dtype=np.uint64)
            u = umap.lookup_host(user, -1)
            bits[u < 0] |= np.uint64(1)
            u[u < 0] = len(umap) // 2
            h = imap.lookup_host(item, -1)
            bits[h < 0] |= np.uint64(2)
            h[h < 0] = 0
            codes = []
            for c, k in enumerate(keys):
                present = cat_keys[c]
                pos = np.searchsorted(present, k)
                at = np.minimum(pos, max(present.size - 1, 0))
                known = (k >= 0) & (pos < present.size)
                if present.size:
                    known &= present[at] == k
                bits[~known] |= np.uint64(1) << np.uint64(2 + c)
                codes.append(np.where(known, pos, 0).astype(np.int64))
            bits[~passed] = 0
            kept = passed & (bits == 0) if drop else passed
            rows = np.flatnonzero(kept).astype(np.int32)
            n = rows.size
            x = x[kept]
            if fill_nan:
                for c in range(self.n_num):
                    x[np.isnan(x[:, c]), c] = self.median_[c]
            if np.isinf(x).any():
                raise ValueError(INF_MESSAGE)
            xs = x * self.scale_
            xs = xs + self.min_
        count = lambda b: int(np.count_nonzero(bits & np.uint64(1) << np.uint64(b)))
        new_u = new_h = None
        if unknown == "admit":
            self._check_reserved(user[kept], item[kept])
            fu, fh = kept & (bits & np.uint64(1) != 0), kept & (bits & np.uint64(2) != 0)
            u[fu], new_u = self._admit("users", user[fu], None)
            h[fh], new_h = self._admit("items", item[fh], None)
        return Transformed(np.stack([u, h], axis=1)[kept].reshape(n, 2),
                           np.stack(codes, axis=1)[kept] if codes else np.zeros((n, 0), np.int64),
                           xs.astype(np.float32).reshape(n, self.n_num),
                           None if tgt is None else (tgt[kept] != 0).astype(np.float32),
                           rows, bits[kept].view(np.int64), n, M - int(passed.sum()), count(0), count(1),
                           [count(2 + c) for c in range(self.n_cat)], new_u, new_h)

    # ----------------------------------------------------------------- device
    @staticmethod
    def _device_key(dev):
        return (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())

    def _device_fit(self, dev):
        key = self._device_key(dev)
        st = self._state.get(key)
        if st is None:
            keys = [_host(k).astype(np.int64).reshape(-1) for k in self.cat_keys]
            off = np.zeros(self.n_cat + 1, dtype=np.int64)
            off[1:] = np.cumsum([k.size for k in keys])
            flat = np.concatenate(keys) if keys else np.zeros(0, np.int64)
            med = self.median_ if self.median_ is not None else np.full(self.n_num, np.nan)
            fit = np.stack([med, self.scale_, self.min_]) if self.n_num else np.zeros((3, 0))
            st = dict(users=IdMap(self.user_ids, device=dev), items=IdMap(self.item_ids, device=dev),
                      cat_keys=torch.from_numpy(flat).to(dev), cat_offsets=off,
                      fit=torch.from_numpy(np.ascontiguousarray(fit, dtype=np.float64)).to(dev))
            self._state[key] = st
        return st

    def transform(self, user, item, target, cat, num, *, unknown="reference", fill_nan=True, noise_filter=None,
                  device="cuda") -> Transformed:
        """New rows through the fitted preprocessing on the device: the row
        filter (``noise_filter="fitted"``, a ``(column, lo, hi)`` or None), the
        fit's derived columns, the NaN fill with ``median_`` (``fill_nan``), the
        id and category lookups, the unknown policy (``"reference"``: the
        service's fallbacks, main.py:217-225; ``"drop"``: such rows are left out),
        the scaler and the target.  Device inputs are used where they are; nothing
        but the count words travels to the host.  Raises ``ValueError`` for a kept
        +-inf, as ``prepare_data`` does."""
        drop = self._policy(unknown)
        self._check_fill(fill_nan)
        fcol, lo, hi = self._filter(noise_filter)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("transform runs on the HIP device; transform_host is the numpy path")
        lib = _lib.load()
        on = lambda t, dt: torch.as_tensor(t).to(device=dev, dtype=dt).contiguous()
        user, item = on(user, torch.int64).reshape(-1), on(item, torch.int64).reshape(-1)
        M = int(user.numel())
        two_d = lambda t: t.reshape(M, 1) if t.dim() == 1 else t
        if isinstance(cat, torch.Tensor):      # a key table: used where it is
            cat_key = two_d(on(cat, torch.int64))
            if cat_key.dim() != 2 or int(cat_key.shape[1]) != self.n_cat:
                raise ValueError(f"cat must be [M, {self.n_cat}]")
        else:
            keys = self._key_columns(cat, M)
            cat_key = torch.stack([on(k, torch.int64).reshape(-1) for k in keys], dim=1).contiguous() if keys \
                else torch.zeros((M, 0), dtype=torch.int64, device=dev)
        raw = two_d(on(num, torch.float64)) if num is not None else \
            torch.zeros((M, 0), dtype=torch.float64, device=dev)
        if raw.dim() != 2 or int(raw.shape[1]) != self.n_raw:
            raise ValueError(f"num must be [M, {self.n_raw}]")
        if target is not None:
            target = torch.as_tensor(target).to(dev).reshape(-1)
            target = (target != 0).to(torch.uint8) if target.dtype != torch.uint8 else target.contiguous()
        if any(int(t.shape[0]) != M for t in (item, cat_key, raw) + (() if target is None else (target,))):
            raise ValueError("Size mismatch between columns")
        n_cat, n_raw, n_num, dv = self.n_cat, self.n_raw, self.n_num, self._dv
        st = self._device_fit(dev)
        with torch.cuda.device(dev):
            nb = int(lib.dcnr_rows_transform_workspace_size(M, n_cat, n_raw, len(dv)))
            if nb == 0:
                raise RuntimeError(f"transform: the device call does not take this shape "
                                   f"(M={M}, n_cat={n_cat}, n_num={n_num}): DCNR_UNSUPPORTED_SHAPE")
            new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
            ws = new(nb, torch.uint8)
            row, collab, cats = new(M, torch.int32), new((M, 2), torch.int64), new((M, n_cat), torch.int64)
            num_out, bits = new((M, n_num), torch.float32), new(M, torch.int64)
            y = new(M, torch.float32) if target is not None else None
            counts = new(N_COUNTS + n_cat, torch.int32)
            pin = torch.zeros(N_COUNTS + n_cat, dtype=torch.int32).pin_memory()
            p = lambda t: t.data_ptr() if t is not None and t.numel() else None
            off = st["cat_offsets"]
            a = RowsTransformArgs(p(user), p(item), p(target), p(cat_key), p(raw), M, n_cat, n_raw, fcol, lo, hi,
                                  len(dv), dv.ctypes.data if len(dv) else None, int(bool(fill_nan)), int(drop),
                                  st["users"]._table.data_ptr(), st["users"].capacity, len(st["users"]),
                                  st["items"]._table.data_ptr(), st["items"].capacity, len(st["items"]),
                                  p(st["cat_keys"]), off.ctypes.data if n_cat else None, p(st["fit"]),
                                  p(row), p(collab), p(cats), p(num_out), p(y), p(bits),
                                  counts.data_ptr(), pin.data_ptr())
            _lib.check(lib.dcnr_rows_transform(ctypes.byref(a), p(ws), nb, _lib.stream_ptr(dev)),
                       "dcnr_rows_transform")
            torch.cuda.current_stream(dev).synchronize()   # the one host wait
        c = pin.numpy().copy()
        n, n_filtered, n_uu, n_ui, status = (int(v) for v in c[:N_COUNTS])
        if status & REQ_BAD_DATA:
            raise ValueError(INF_MESSAGE)
        new_u = new_h = None
        if unknown == "admit" and (n_uu or n_ui):
            key = self._device_key(dev)
            kept = row[:n].to(torch.int64)
            ku, kh = user[kept], item[kept]
            fu, fh = (bits[:n] & 1) != 0, (bits[:n] & 2) != 0
            self._check_reserved(ku[fu], kh[fh])
            if n_uu:
                idx, new_u = self._admit("users", ku[fu], key)
                collab[:n, 0][fu] = idx
            if n_ui:
                idx, new_h = self._admit("items", kh[fh], key)
                collab[:n, 1][fh] = idx
        return Transformed(collab[:n], cats[:n], num_out[:n], None if y is None else y[:n], row[:n], bits[:n],
                           n, n_filtered, n_uu, n_ui, c[N_COUNTS:], new_u, new_h)
