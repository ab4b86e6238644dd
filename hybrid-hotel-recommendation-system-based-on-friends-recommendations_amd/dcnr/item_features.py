"""The hotel feature tables of the /recommendations request path, derived from
``main_df``'s rows on the host and the device.

The reference scores a candidate hotel from that hotel's first ``main_df`` row
(``main_df[isin(candidates)].drop_duplicates(subset=['item_id'])``,
main.py:315), encoded and scaled by ``preprocess_for_ranking``
(main.py:215-230): a scan of the whole table per request.  ``ItemFeatures``
holds one entry per ``main_df`` row -- hotel row, the row's ``main_df`` number,
the caller's encoded categorical codes and the raw numeric columns -- with the
scaler's ``scale_`` / ``min_``, and gives for every hotel h:

  first_row[h]  the ``main_df`` number of h's first row, -1 if it has none
  item_cat[h]   that row's codes (int64); zeros without a row
  item_num[h]   float32(x * scale_ + min_) of that row's values, the product
                and the sum each rounded to float64 as MinMaxScaler.transform
                rounds them; zeros without a row

The host copies (numpy) answer ``item_cat_host``, ``item_num_host`` and
``first_rows_host``: the yardstick of the tests and a host fallback.  The device
copies come from dcnr_item_features_build over the resident columns;
``RankingPipeline(model, item_features=feat)`` scores from them.  Hotel rows
are dense; the encoders stay with the caller.
"""
from __future__ import annotations

import threading
import time

import numpy as np
import torch

from . import _lib

MAX_ITEMS = 1 << 29
MAX_WIDTH = 64
REQ_BAD_DATA = 2   # DCNR_REQ_BAD_DATA


class FeatureColumns:
    """One state of the columns and the scaler (never written once made) and the
    tables numpy derives from it, made on first use."""

    def __init__(self, item, row, cat, num, scale, mn, n_items):
        self.item, self.row, self.cat, self.num = item, row, cat, num
        self.scale, self.min, self.n_items = scale, mn, n_items
        self._tables = None
        self._lock = threading.Lock()

    def tables(self):
        """(first_row int32 [n_items], item_cat int64 [n_items, n_cat], item_num fp32 [n_items, n_num])."""
        with self._lock:
            if self._tables is None:
                hotels, at = np.unique(self.item, return_index=True)   # first occurrence
                first = np.full(self.n_items, -1, np.int32)
                first[hotels] = self.row[at]
                cat = np.zeros((self.n_items, self.cat.shape[1]), np.int64)
                cat[hotels] = self.cat[at]
                num = np.zeros((self.n_items, self.num.shape[1]), np.float32)
                with np.errstate(all="ignore"):
                    x = self.num[at] * self.scale   # MinMaxScaler.transform: X *= scale_; X += min_
                    x += self.min
                    num[hotels] = x.astype(np.float32)
                self._tables = (first, cat, num)
            return self._tables


class FeatureGeneration:
    """The device tensors of one state of an ``ItemFeatures`` on one device;
    never written after they are published.

    item_cat     int64 [n_items, n_cat]
    item_num     fp32 [n_items, n_num]
    first_row    int32 [n_items]: ``main_df`` numbers, -1 for a hotel without a row
    n_with_row   the hotels that have a row
    review_item, review_row (int32 [M]), review_cat (int32 [M, n_cat]),
    review_num (float64 [M, n_num]), scaler_scale, scaler_min (float64 [n_num]):
    the resident columns the tables were built from
    host         the ``FeatureColumns`` of the same state
    """

    def __init__(self, host, cols, scaler, first_row, item_cat, item_num, n_with_row):
        self.host = host
        self.review_item, self.review_row, self.review_cat, self.review_num = cols
        self.scaler_scale, self.scaler_min = scaler
        self.first_row, self.item_cat, self.item_num = first_row, item_cat, item_num
        self.n_with_row, self.n_items = n_with_row, host.n_items
        self.n_reviews = int(self.review_item.numel())


def _matrix(a, rows, width, dtype, what):
    """``a`` as a contiguous [rows, width] array of ``dtype`` (rows None: as many as it
    holds); None stands for no columns.  A wrong width is a ValueError."""
    if a is None:
        a = np.zeros((rows or 0, 0), dtype)
    a = np.asarray(a)
    if a.size == 0 and not rows and a.ndim <= 2:   # an empty batch, whatever its shape
        a = np.zeros((0, width), dtype)
    if a.ndim != 2 or a.shape[1] != width or (rows is not None and a.shape[0] != rows):
        raise ValueError(f"{what}: expected [{'m' if rows is None else rows}, {width}], got "
                         f"{list(a.shape)}")
    if dtype == np.int32:
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{what}: integer codes expected")
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError(f"{what}: a code does not fit 32 bits")
    return np.ascontiguousarray(a.astype(dtype))


class ItemFeatures:
    """Built from host arrays in row space; ``append`` adds the next rows of
    ``main_df``, ``remove`` takes rows out, ``set_values`` edits numeric values
    of rows, ``set_scaler`` takes a refitted scaler.

    review_item [M]          hotel row of each ``main_df`` row, in [0, n_items)
    review_cat [M, n_cat]    its encoded categorical codes (None: no such column)
    review_num [M, n_num]    its raw numeric columns (float64; anything allowed)
    scaler_scale, scaler_min [n_num]   MinMaxScaler's ``scale_`` and ``min_``, finite
    n_items                  rows of the tables
    review_row, next_review_row   (keyword only) the rows' ``main_df`` numbers,
                             strictly ascending, and the number the next appended
                             row gets: for tables that rows were removed from.
                             Default: 0..M-1 and M

    ``review_row`` and ``next_review_row`` follow ``InteractionStore`` and
    ``CitySets``: a removed row's number is never given again.  A caller drives
    the three objects with the same batches.
    """

    def __init__(self, review_item, review_cat, review_num, scaler_scale, scaler_min, n_items: int, *,
                 review_row=None, next_review_row: int | None = None):
        item = np.asarray(review_item, dtype=np.int64).reshape(-1).copy()
        M = item.size
        scale, mn = self._scaler_arg("ItemFeatures", scaler_scale, scaler_min, None)
        n_num = scale.size
        cat = None if review_cat is None else np.asarray(review_cat)
        n_cat = 0 if cat is None else (cat.shape[1] if cat.ndim == 2 else -1)
        if n_cat < 0:
            raise ValueError("ItemFeatures: review_cat must be [M, n_cat] (or None)")
        if n_cat > MAX_WIDTH or n_num > MAX_WIDTH:
            raise ValueError(f"ItemFeatures: more than {MAX_WIDTH} columns")
        cat = _matrix(cat, M, n_cat, np.int32, "ItemFeatures: review_cat")
        num = _matrix(review_num, M, n_num, np.float64, "ItemFeatures: review_num")
        row = np.arange(M, dtype=np.int64) if review_row is None else \
            np.asarray(review_row, dtype=np.int64).reshape(-1).copy()
        if row.size != M:
            raise ValueError("ItemFeatures: review_row must have one entry per review")
        if M and (row[0] < 0 or (np.diff(row) <= 0).any()):
            raise ValueError("ItemFeatures: review_row must be non-negative and strictly ascending")
        n_items = int(n_items)
        if not 1 <= n_items <= MAX_ITEMS:
            raise ValueError(f"ItemFeatures: n_items={n_items} outside [1, 2^29]")
        if M and (item.min() < 0 or item.max() >= n_items):
            raise ValueError(f"ItemFeatures: review_item outside [0, {n_items})")
        nxt = (int(row[-1]) + 1 if M else 0) if next_review_row is None else int(next_review_row)
        if M and nxt <= row[-1]:
            raise ValueError("ItemFeatures: next_review_row must lie behind every review_row")
        if max(M, nxt) >= 2 ** 31 - 1:
            raise ValueError("ItemFeatures: 2^31 - 1 or more reviews")
        self.n_items, self.n_cat, self.n_num = n_items, n_cat, n_num
        self.next_review_row = nxt
        self._cols = FeatureColumns(item, row, cat, num, scale, mn, n_items)
        self._dev, self._prev = {}, {}   # per device: the newest generation, the one before
        self.last_update = None          # timings and upload size of the last call that changed something
        self._dev_lock = threading.Lock()

    @staticmethod
    def _scaler_arg(what, scale, mn, n_num):
        scale = np.asarray(scale, dtype=np.float64).reshape(-1).copy()
        mn = np.asarray(mn, dtype=np.float64).reshape(-1).copy()
        if scale.size != mn.size or (n_num is not None and scale.size != n_num):
            raise ValueError(f"{what}: scaler_scale and scaler_min must have one entry per numeric "
                             "column")
        if not (np.isfinite(scale).all() and np.isfinite(mn).all()):
            raise ValueError(f"{what}: scaler_scale and scaler_min must be finite")
        return scale, mn

    # ------------------------------------------------------------------ host
    review_item = property(lambda self: self._cols.item)
    review_row = property(lambda self: self._cols.row)
    review_cat = property(lambda self: self._cols.cat)
    review_num = property(lambda self: self._cols.num)
    scaler_scale = property(lambda self: self._cols.scale)
    scaler_min = property(lambda self: self._cols.min)
    n_reviews = property(lambda self: self._cols.item.size)

    def first_rows_host(self) -> np.ndarray:
        """int32 [n_items]: the ``main_df`` number of each hotel's first row, -1: none."""
        return self._cols.tables()[0]

    def item_cat_host(self) -> np.ndarray:
        """int64 [n_items, n_cat]: each hotel's codes, from its first row."""
        return self._cols.tables()[1]

    def item_num_host(self) -> np.ndarray:
        """fp32 [n_items, n_num]: each hotel's scaled values, from its first row."""
        return self._cols.tables()[2]

    def _positions(self, what, rows):
        """The positions of the ``main_df`` numbers ``rows`` (ascending, distinct)."""
        old = self._cols
        at = np.searchsorted(old.row, rows)
        there = at < old.row.size
        there[there] = old.row[at[there]] == rows[there]
        if not there.all():
            raise ValueError(f"{what}: no review at main_df row {rows[~there][0]} "
                             f"({int((~there).sum())} such in the batch)")
        return at

    # ------------------------------------------- append, remove, set_values
    def append(self, review_item=(), review_cat=None, review_num=None) -> None:
        """The next rows of ``main_df``, in place: their ``review_row`` values
        are ``next_review_row .. next_review_row + m - 1`` in argument order.

        Afterwards every host array and every device tensor equals those of
        an ``ItemFeatures`` built from the concatenated rows.  On each device
        the object was uploaded to only the batch travels: the new rows are
        copied behind the resident columns and dcnr_item_features_build derives
        the next generation's tables from them.  Everything is validated, and
        every new array made, before anything is published: a failed append
        leaves the object as it was, on the host and on the devices; the
        generation before stays alive for calls that still read it (see
        ``on``).  An empty batch is a no-op.  ``last_update`` keeps the seconds
        of the host and the device part and the bytes uploaded per device."""
        item = np.asarray(review_item, dtype=np.int64).reshape(-1)
        m, old = item.size, self._cols
        cat = _matrix(review_cat, m, self.n_cat, np.int32, "ItemFeatures.append: review_cat")
        num = _matrix(review_num, m, self.n_num, np.float64, "ItemFeatures.append: review_num")
        if m and (item.min() < 0 or item.max() >= self.n_items):
            raise ValueError(f"ItemFeatures.append: review_item outside [0, {self.n_items})")
        if max(old.item.size + m, self.next_review_row + m) >= 2 ** 31 - 1:
            raise ValueError("ItemFeatures.append: 2^31 - 1 or more reviews")
        if m == 0:
            return
        t_start = time.perf_counter()
        row = self.next_review_row + np.arange(m, dtype=np.int64)
        cols = FeatureColumns(np.concatenate([old.item, item]), np.concatenate([old.row, row]),
                              np.concatenate([old.cat, cat]), np.concatenate([old.num, num]),
                              old.scale, old.min, self.n_items)

        def device(dev, gen, up):
            new = (torch.cat([gen.review_item, up(item.astype(np.int32))]),
                   torch.cat([gen.review_row, up(row.astype(np.int32))]),
                   torch.cat([gen.review_cat, up(cat)]), torch.cat([gen.review_num, up(num)]))
            return new, (gen.scaler_scale, gen.scaler_min)
        self._advance("append", cols, device, m * (8 + 4 * self.n_cat + 8 * self.n_num), t_start)
        self.next_review_row += m

    def remove(self, review_row=()) -> None:
        """Rows of ``main_df`` taken out, named by their ``main_df`` number.  A
        number the object does not hold, or one given twice, raises
        ``ValueError`` and changes nothing.  The surviving rows keep their
        numbers and ``next_review_row`` stays; a hotel whose first row went is
        served from its next one, a hotel whose only row went has no features.
        On each device only the removed positions travel; the columns are
        compacted there and the tables derived anew.  Validation, generations
        and ``last_update`` as for ``append``; an empty batch is a no-op."""
        rows = np.asarray(review_row, dtype=np.int64).reshape(-1)
        if rows.size == 0:
            return
        t_start = time.perf_counter()
        old = self._cols
        rows = np.sort(rows)
        if (np.diff(rows) == 0).any():
            raise ValueError(f"ItemFeatures.remove: main_df row {rows[1:][np.diff(rows) == 0][0]} is "
                             "given more than once")
        at = self._positions("ItemFeatures.remove", rows)
        cols = FeatureColumns(np.delete(old.item, at), np.delete(old.row, at),
                              np.delete(old.cat, at, axis=0), np.delete(old.num, at, axis=0),
                              old.scale, old.min, self.n_items)

        def device(dev, gen, up):
            keep = torch.ones(gen.n_reviews, dtype=torch.bool, device=dev)
            keep[up(at)] = False
            new = tuple(t[keep] for t in (gen.review_item, gen.review_row, gen.review_cat,
                                          gen.review_num))
            return new, (gen.scaler_scale, gen.scaler_min)
        self._advance("remove", cols, device, 8 * at.size, t_start)

    def set_values(self, review_row=(), review_num=None, columns=None) -> None:
        """Edited numeric values of rows named by their ``main_df`` number:
        ``review_num`` [k, n_num], or [k, len(columns)] for the columns named
        (indices into the numeric columns, distinct).  Of a row given more
        than once the last entry counts.  A number the object does not hold,
        a wrong width or a bad column raises ``ValueError`` and changes
        nothing.  On each device only the positions and the values travel.
        Validation, generations and ``last_update`` as for ``append``; an empty
        batch is a no-op."""
        rows = np.asarray(review_row, dtype=np.int64).reshape(-1)
        k = rows.size
        if columns is None:
            col = np.arange(self.n_num, dtype=np.int64)
        else:
            col = np.asarray(columns, dtype=np.int64).reshape(-1)
            if col.size and (col.min() < 0 or col.max() >= self.n_num):
                raise ValueError(f"ItemFeatures.set_values: column outside [0, {self.n_num})")
            if np.unique(col).size != col.size:
                raise ValueError("ItemFeatures.set_values: a column is named more than once")
        vals = _matrix(review_num, k, col.size, np.float64, "ItemFeatures.set_values: review_num")
        if k == 0 or col.size == 0:
            return
        t_start = time.perf_counter()
        old = self._cols
        # the last entry of a repeated row: the first of the reversed batch
        rows, last = np.unique(rows[::-1], return_index=True)
        vals = np.ascontiguousarray(vals[::-1][last])
        at = self._positions("ItemFeatures.set_values", rows)
        num = old.num.copy()
        num[at[:, None], col[None, :]] = vals
        cols = FeatureColumns(old.item, old.row, old.cat, num, old.scale, old.min, self.n_items)

        def device(dev, gen, up):
            d_num = gen.review_num.clone()
            d_num[up(at)[:, None], up(col)[None, :]] = up(vals)   # (distinct positions: one writer each)
            return (gen.review_item, gen.review_row, gen.review_cat, d_num), \
                (gen.scaler_scale, gen.scaler_min)
        nbytes = 8 * at.size * (1 + col.size) + (0 if columns is None else 8 * col.size)
        self._advance("set_values", cols, device, nbytes, t_start)

    def set_scaler(self, scaler_scale, scaler_min) -> None:
        """A refitted scaler: the columns stay where they are, on the host and
        on the devices; the tables are derived anew.  Non-finite values or a
        wrong width raise ``ValueError`` and change nothing."""
        scale, mn = self._scaler_arg("ItemFeatures.set_scaler", scaler_scale, scaler_min, self.n_num)
        t_start = time.perf_counter()
        old = self._cols
        cols = FeatureColumns(old.item, old.row, old.cat, old.num, scale, mn, self.n_items)

        def device(dev, gen, up):
            return (gen.review_item, gen.review_row, gen.review_cat, gen.review_num), (up(scale), up(mn))
        self._advance("set_scaler", cols, device, 16 * self.n_num, t_start)

    def _advance(self, op, cols, device, upload_bytes, t_start) -> None:
        """The next state: every device's next generation made (``device`` gives
        its columns and scaler), then all of it published together."""
        t_host = time.perf_counter()
        with self._dev_lock:
            gens = {}
            for key, gen in self._dev.items():
                dev = torch.device(*key)
                with torch.cuda.device(dev):
                    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                    new, scaler = device(dev, gen, up)
                    gens[key] = self._build(dev, cols, new, scaler)
            self._publish(gens)
            self._cols = cols
            self.last_update = dict(op=op, host_s=t_host - t_start,
                                    device_s=time.perf_counter() - t_host,
                                    upload_bytes=upload_bytes, devices=len(gens))

    def _publish(self, gens) -> None:
        """The next generation of every device (under the lock); an older one
        is dropped only when no kernel launched against it can still run."""
        if self._prev:
            for key in self._prev:
                torch.cuda.synchronize(torch.device(*key))
        self._prev = dict(self._dev)
        self._dev.update(gens)

    # ---------------------------------------------------------------- device
    def _build(self, device, host, cols, scaler) -> FeatureGeneration:
        """One generation from the resident columns: dcnr_item_features_build and
        one readback of the two count words."""
        lib = _lib.load()
        d_item, d_row, d_cat, d_num = cols
        M, n, K, F = int(d_item.numel()), self.n_items, self.n_cat, self.n_num
        nb = int(lib.dcnr_item_features_workspace_size(M, n, K, F))
        if nb == 0:
            raise RuntimeError("ItemFeatures: the device build does not take this shape")
        ws = torch.empty(nb, dtype=torch.uint8, device=device)
        first_row = torch.empty(n, dtype=torch.int32, device=device)
        item_cat = torch.empty((n, K), dtype=torch.int64, device=device)
        item_num = torch.empty((n, F), dtype=torch.float32, device=device)
        counts = torch.empty(2, dtype=torch.int32, device=device)
        pin = torch.empty(2, dtype=torch.int32, pin_memory=True)
        p = lambda t: t.data_ptr() if t.numel() else None
        _lib.check(lib.dcnr_item_features_build(
            p(d_item), p(d_row), p(d_cat), p(d_num), p(scaler[0]), p(scaler[1]), M, n, K, F,
            first_row.data_ptr(), p(item_cat), p(item_num), counts.data_ptr(), pin.data_ptr(),
            ws.data_ptr(), nb, _lib.stream_ptr(device)), "dcnr_item_features_build")
        # published only once written: the one readback of a build
        torch.cuda.current_stream(device).synchronize()
        n_with_row, st = (int(v) for v in pin.numpy())
        if st & REQ_BAD_DATA:
            raise RuntimeError("ItemFeatures: the device rejected validated input")
        return FeatureGeneration(host, cols, scaler, first_row, item_cat, item_num, n_with_row)

    def on(self, device) -> FeatureGeneration:
        """The newest generation on ``device``: uploaded and built on a
        device's first call, advanced there by every ``append``, ``remove``,
        ``set_values`` and ``set_scaler`` since.  The tensors of a generation
        are never written after they are published; whoever launches a kernel
        against one keeps it until the kernel has finished
        (``RankingPipeline`` keeps it with its answers).  The object itself
        holds the generation before the newest and synchronizes the device
        before it lets go of an older one.  Serialise the calls that change the
        object against the calls that read it."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ItemFeatures.on: the device copies live on the HIP device only")
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        with self._dev_lock:
            gen = self._dev.get(key)
            if gen is None:
                c = self._cols
                dev = torch.device(*key)
                with torch.cuda.device(dev):
                    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                    gen = self._dev[key] = self._build(
                        dev, c, (up(c.item.astype(np.int32)), up(c.row.astype(np.int32)), up(c.cat),
                                 up(c.num)), (up(c.scale), up(c.min)))
        return gen
