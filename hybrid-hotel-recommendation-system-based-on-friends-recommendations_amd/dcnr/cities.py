"""The city and popularity row sets of the /recommendations request path
(main.py:204-210), derived from ``main_df``'s rows on the host and the device.

The reference filters a request's candidates by the target city's hotels
(main.py:209-210) and, when fewer than 20 were found, fills up from the
hotels of the city's 100 most reviewed rows (main.py:204-208): two scans and a
sort over the whole table per request.  ``CitySets`` holds one entry per
``main_df`` row -- hotel row, dense city code, ``user_reviews_count`` and the
row's ``main_df`` number -- and gives, for every city c:

  city(c)      the distinct hotel rows over the rows of city c, ascending
  top_rows(c)  the first ``top`` rows of city c by popularity descending, NaN
               last, equal values (-0.0 equals +0.0) by ascending ``main_df``
               row: ``sort_values(ascending=False, kind='stable').head(top)``
  popular(c)   the distinct hotel rows of top_rows(c), ascending

The reference sorts with pandas' default kind, which leaves the order of equal
values open; where the tie group at the cut names one hotel only, both give
the same popular set.

The host copies (numpy) answer ``city_rows_host``, ``popular_rows_host`` and
``top_rows_host``: the one-request overflow path of ``RankingPipeline`` and the
yardstick of the tests.  The device copies come from dcnr_city_sets_build over
the resident columns: one CSR of 2C + 1 sets that ``recommend_many`` /
``recommend_users`` (``city_sets=``, ``cities=``) join behind the registered
sets.  City codes and hotel rows are dense; the raw-value dictionaries stay
with the caller.
"""
from __future__ import annotations

import threading
import time

import numpy as np
import torch

from . import _lib

MAX_ITEMS = 1 << 29
MAX_CITIES = 1 << 16
MAX_TOP = 256
REQ_OVERFLOW, REQ_BAD_DATA = 1, 2   # DCNR_REQ_*


def served_order(key: np.ndarray, row: np.ndarray) -> np.ndarray:
    """The order top_rows(c) is cut from: key descending, NaN last, ties by ascending row."""
    nan = np.isnan(key)
    return np.lexsort((row, np.where(nan, 0.0, -key), nan))


class CityColumns:
    """One state of the four columns (never written once made) and the sets
    numpy derives from it; the by-city index is made on first use."""

    def __init__(self, item, city, key, row, n_items, n_cities, top):
        self.item, self.city, self.key, self.row = item, city, key, row
        self.n_items, self.n_cities, self.top = n_items, n_cities, top
        self._index = None
        self._lock = threading.Lock()

    def _of_city(self, c: int) -> np.ndarray:
        """The positions of city c's rows, ascending (-1: none)."""
        if not -1 <= c < self.n_cities:
            raise ValueError(f"CitySets: city {c} outside [-1, {self.n_cities})")
        if c < 0:
            return np.zeros(0, np.int64)
        with self._lock:
            if self._index is None:
                off = np.zeros(self.n_cities + 1, np.int64)
                np.cumsum(np.bincount(self.city, minlength=self.n_cities), out=off[1:])
                self._index = (np.argsort(self.city, kind="stable"), off)
            order, off = self._index
        return order[off[c]:off[c + 1]]

    def _top(self, c: int) -> np.ndarray:
        idx = self._of_city(int(c))
        return idx[served_order(self.key[idx], self.row[idx])[:self.top]]

    def city_rows(self, c: int) -> np.ndarray:
        return np.unique(self.item[self._of_city(int(c))])

    def top_rows(self, c: int) -> np.ndarray:
        return self.row[self._top(c)]

    def popular_rows(self, c: int) -> np.ndarray:
        return np.unique(self.item[self._top(c)])


class CityGeneration:
    """The device tensors of one state of a ``CitySets`` on one device; never
    written after they are published.

    set_rows      int64: the CSR's rows; sets 0..C-1 are city(c), C..2C-1
                  popular(c), set 2C is empty (the unknown city)
    set_offsets   int64 [2C + 2] on the device; ``host_offsets``: its host copy
    top_rows      int32 [C, top]: ``main_df`` numbers in served order, -1 behind
                  a city's last
    review_item, review_city (int32), review_popularity (float64), review_row
    (int32): the resident columns the sets were built from
    host          the ``CityColumns`` of the same state
    """

    def __init__(self, host, cols, set_rows, set_offsets, host_offsets, top_rows):
        self.host = host
        self.review_item, self.review_city, self.review_popularity, self.review_row = cols
        self.set_rows, self.set_offsets, self.host_offsets, self.top_rows = (
            set_rows, set_offsets, host_offsets, top_rows)
        self.n_cities, self.top, self.n_items = host.n_cities, host.top, host.n_items
        self.n_reviews = int(self.review_item.numel())

    def set_of(self, s: int) -> torch.Tensor:
        return self.set_rows[int(self.host_offsets[s]):int(self.host_offsets[s + 1])]


class CitySets:
    """Built from host arrays in row space; ``append`` adds the next rows of
    ``main_df``, ``remove`` takes rows out.

    review_item [M]        hotel row of each ``main_df`` row, in [0, n_items)
    review_city [M]        its dense city code, in [0, n_cities)
    review_popularity [M]  its user_reviews_count (float64; NaN, +-inf allowed)
    n_items                rows of the index the hotel rows point into
    n_cities               C; default: the largest code named + 1 (at least 1)
    top                    rows of top_rows(c), main.py:206's 100; at most 256
    review_row, next_review_row   (keyword only) the rows' ``main_df`` numbers,
                           strictly ascending, and the number the next appended
                           row gets: for tables that rows were removed from.
                           Default: 0..M-1 and M

    ``review_row`` and ``next_review_row`` follow ``InteractionStore``: a
    removed row's number is never given again.  A caller drives both objects
    with the same batches.
    """

    def __init__(self, review_item, review_city, review_popularity, n_items: int,
                 n_cities: int | None = None, top: int = 100, *, review_row=None,
                 next_review_row: int | None = None):
        item = np.asarray(review_item, dtype=np.int64).reshape(-1).copy()
        city = np.asarray(review_city, dtype=np.int64).reshape(-1).copy()
        key = np.asarray(review_popularity, dtype=np.float64).reshape(-1).copy()
        if not (item.size == city.size == key.size):
            raise ValueError("CitySets: review_item, review_city and review_popularity must have "
                             "one entry per review")
        M = item.size
        row = np.arange(M, dtype=np.int64) if review_row is None else \
            np.asarray(review_row, dtype=np.int64).reshape(-1).copy()
        if row.size != M:
            raise ValueError("CitySets: review_row must have one entry per review")
        if M and (row[0] < 0 or (np.diff(row) <= 0).any()):
            raise ValueError("CitySets: review_row must be non-negative and strictly ascending")
        n_items, top = int(n_items), int(top)
        if not 1 <= n_items <= MAX_ITEMS:
            raise ValueError(f"CitySets: n_items={n_items} outside [1, 2^29]")
        if not 1 <= top <= MAX_TOP:
            raise ValueError(f"CitySets: top={top} outside [1, {MAX_TOP}]")
        C = int(n_cities) if n_cities is not None else max(1, int(city.max()) + 1 if M else 1)
        if not 1 <= C <= MAX_CITIES:
            raise ValueError(f"CitySets: n_cities={C} outside [1, {MAX_CITIES}]")
        if M and (item.min() < 0 or item.max() >= n_items):
            raise ValueError(f"CitySets: review_item outside [0, {n_items})")
        if M and (city.min() < 0 or city.max() >= C):
            raise ValueError(f"CitySets: review_city outside [0, {C})")
        nxt = (int(row[-1]) + 1 if M else 0) if next_review_row is None else int(next_review_row)
        if M and nxt <= row[-1]:
            raise ValueError("CitySets: next_review_row must lie behind every review_row")
        if max(M, nxt) >= 2 ** 31 - 1:
            raise ValueError("CitySets: 2^31 - 1 or more reviews")
        self.n_items, self.n_cities, self.top = n_items, C, top
        self.next_review_row = nxt
        self._cols = CityColumns(item, city, key, row, n_items, C, top)
        self._dev, self._prev = {}, {}   # per device: the newest generation, the one before
        self.last_update = None          # timings and upload size of the last append / remove that changed something
        self._dev_lock = threading.Lock()

    # ------------------------------------------------------------------ host
    review_item = property(lambda self: self._cols.item)
    review_city = property(lambda self: self._cols.city)
    review_popularity = property(lambda self: self._cols.key)
    review_row = property(lambda self: self._cols.row)
    n_reviews = property(lambda self: self._cols.item.size)

    def city_rows_host(self, c: int) -> np.ndarray:
        """city(c): the hotels of city c (main.py:209), ascending; -1: empty."""
        return self._cols.city_rows(c)

    def popular_rows_host(self, c: int) -> np.ndarray:
        """popular(c): the hotels of the city's ``top`` most reviewed rows
        (main.py:205-207), ascending and distinct; -1: empty."""
        return self._cols.popular_rows(c)

    def top_rows_host(self, c: int) -> np.ndarray:
        """top_rows(c): the ``main_df`` numbers of those rows in served order."""
        return self._cols.top_rows(c)

    # ------------------------------------------------------- append, remove
    def append(self, review_item=(), review_city=(), review_popularity=()) -> None:
        """The next rows of ``main_df``, in place: their ``review_row`` values
        are ``next_review_row .. next_review_row + m - 1`` in argument order.

        Afterwards every host array and every device tensor equals those of a
        ``CitySets`` built from the concatenated rows.  On each device the
        object was uploaded to only the batch travels: the new rows are
        copied behind the resident columns and dcnr_city_sets_build derives
        the next generation's sets from them.  Everything is validated, and
        every new array made, before anything is published: a failed append
        leaves the object as it was, on the host and on the devices; the
        generation before stays alive for calls that still read it (see
        ``on``).  An empty batch is a no-op.  ``last_update`` keeps the seconds
        of the host and the device part and the bytes uploaded per device.
        ``n_items``, ``n_cities`` and ``top`` are fixed; build a new object to
        change them.
        """
        item = np.asarray(review_item, dtype=np.int64).reshape(-1)
        city = np.asarray(review_city, dtype=np.int64).reshape(-1)
        key = np.asarray(review_popularity, dtype=np.float64).reshape(-1)
        if not (item.size == city.size == key.size):
            raise ValueError("CitySets.append: review_item, review_city and review_popularity "
                             "must have one entry per review")
        m, old = item.size, self._cols
        if m and (item.min() < 0 or item.max() >= self.n_items):
            raise ValueError(f"CitySets.append: review_item outside [0, {self.n_items})")
        if m and (city.min() < 0 or city.max() >= self.n_cities):
            raise ValueError(f"CitySets.append: review_city outside [0, {self.n_cities})")
        if max(old.item.size + m, self.next_review_row + m) >= 2 ** 31 - 1:
            raise ValueError("CitySets.append: 2^31 - 1 or more reviews")
        if m == 0:
            return
        t_start = time.perf_counter()
        row = self.next_review_row + np.arange(m, dtype=np.int64)
        cols = CityColumns(np.concatenate([old.item, item]), np.concatenate([old.city, city]),
                           np.concatenate([old.key, key]), np.concatenate([old.row, row]),
                           self.n_items, self.n_cities, self.top)
        t_host = time.perf_counter()
        with self._dev_lock:
            gens = {k: self._device_append(k, g, cols, item, city, key, row)
                    for k, g in self._dev.items()}
            self._publish(gens)
            self._cols = cols
            self.next_review_row += m
            self.last_update = dict(op="append", host_s=t_host - t_start,
                                    device_s=time.perf_counter() - t_host, upload_bytes=20 * m,
                                    devices=len(gens))

    def remove(self, review_row=()) -> None:
        """Rows of ``main_df`` taken out, named by their ``main_df`` number.  A
        number the object does not hold, or one given twice, raises
        ``ValueError`` and changes nothing.  The surviving rows keep their
        numbers and ``next_review_row`` stays.  Afterwards every host array and
        device tensor equals those of a ``CitySets`` built from the surviving
        rows (with their ``review_row`` values).  On each device only the
        removed positions travel; the columns are compacted there and the sets
        derived anew.  Validation, generations and ``last_update`` as for
        ``append``; an empty batch is a no-op."""
        rows = np.asarray(review_row, dtype=np.int64).reshape(-1)
        if rows.size == 0:
            return
        t_start = time.perf_counter()
        old = self._cols
        rows = np.sort(rows)
        if (np.diff(rows) == 0).any():
            raise ValueError(f"CitySets.remove: main_df row {rows[1:][np.diff(rows) == 0][0]} is "
                             "given more than once")
        at = np.searchsorted(old.row, rows)
        there = at < old.row.size
        there[there] = old.row[at[there]] == rows[there]
        if not there.all():
            raise ValueError(f"CitySets.remove: no review at main_df row {rows[~there][0]} "
                             f"({int((~there).sum())} such in the batch)")
        cols = CityColumns(np.delete(old.item, at), np.delete(old.city, at), np.delete(old.key, at),
                           np.delete(old.row, at), self.n_items, self.n_cities, self.top)
        t_host = time.perf_counter()
        with self._dev_lock:
            gens = {k: self._device_remove(k, g, cols, at) for k, g in self._dev.items()}
            self._publish(gens)
            self._cols = cols
            self.last_update = dict(op="remove", host_s=t_host - t_start,
                                    device_s=time.perf_counter() - t_host, upload_bytes=8 * at.size,
                                    devices=len(gens))

    def _publish(self, gens) -> None:
        """The next generation of every device (under the lock); an older one
        is dropped only when no kernel launched against it can still run."""
        if self._prev:
            for key in self._prev:
                torch.cuda.synchronize(torch.device(*key))
        self._prev = dict(self._dev)
        self._dev.update(gens)

    # ---------------------------------------------------------------- device
    def _device_append(self, key, gen, cols, item, city, pop, row):
        device = torch.device(*key)
        with torch.cuda.device(device):
            up = lambda a, dt: torch.from_numpy(a.astype(dt)).to(device)
            new = (torch.cat([gen.review_item, up(item, np.int32)]),
                   torch.cat([gen.review_city, up(city, np.int32)]),
                   torch.cat([gen.review_popularity, up(pop, np.float64)]),
                   torch.cat([gen.review_row, up(row, np.int32)]))
            return self._build(device, cols, new)

    def _device_remove(self, key, gen, cols, at):
        device = torch.device(*key)
        with torch.cuda.device(device):
            keep = torch.ones(gen.n_reviews, dtype=torch.bool, device=device)
            keep[torch.from_numpy(at).to(device)] = False
            new = tuple(t[keep] for t in (gen.review_item, gen.review_city, gen.review_popularity,
                                          gen.review_row))
            return self._build(device, cols, new)

    def _build(self, device, host, cols) -> CityGeneration:
        """One generation from the resident columns: dcnr_city_sets_build, one
        readback of the 2C + 2 offsets (and the status word); a ``cap`` that
        proves too small is the one the offsets report, once."""
        lib = _lib.load()
        d_item, d_city, d_key, d_row = cols
        M, C, top = int(d_item.numel()), self.n_cities, self.top
        nb = int(lib.dcnr_city_sets_workspace_size(M, self.n_items, C, top))
        if nb == 0:
            raise RuntimeError("CitySets: the device build does not take this shape")
        ws = torch.empty(nb, dtype=torch.uint8, device=device)
        set_offsets = torch.empty(2 * C + 2, dtype=torch.int64, device=device)
        top_rows = torch.empty((C, top), dtype=torch.int32, device=device)
        status = torch.empty(1, dtype=torch.int32, device=device)
        pin = torch.empty(2 * C + 3, dtype=torch.int64, pin_memory=True)
        host_off = pin.numpy()
        p = lambda t: t.data_ptr() if t.numel() else None
        # each hotel in one city, and every city's popular set full: the usual need
        cap = max(1, min(M, self.n_items) + min(M, C * top))
        stream = _lib.stream_ptr(device)
        for attempt in range(2):
            set_rows = torch.empty(cap, dtype=torch.int64, device=device)
            _lib.check(lib.dcnr_city_sets_build(
                p(d_item), p(d_city), p(d_key), p(d_row), M, self.n_items, C, top,
                set_offsets.data_ptr(), set_rows.data_ptr(), cap, top_rows.data_ptr(),
                status.data_ptr(), pin.data_ptr(), pin.data_ptr() + 8 * (2 * C + 2), ws.data_ptr(),
                nb, stream), "dcnr_city_sets_build")
            # published only once written: the one readback of a build
            torch.cuda.current_stream(device).synchronize()
            st = int(host_off[2 * C + 2]) & 0xFFFFFFFF
            if st & REQ_BAD_DATA:
                raise RuntimeError("CitySets: the device rejected validated input")
            if not st & REQ_OVERFLOW:
                break
            if attempt:
                raise RuntimeError("CitySets: the set rows overflowed the size the offsets reported")
            cap = int(host_off[2 * C + 1])
        offsets = host_off[:2 * C + 2].copy()
        return CityGeneration(host, cols, set_rows[:int(offsets[-1])], set_offsets, offsets, top_rows)

    def on(self, device) -> CityGeneration:
        """The newest generation on ``device``: uploaded and built on a
        device's first call, advanced there by every ``append`` and ``remove``
        since.  The tensors of a generation are never written after they are
        published; whoever launches a kernel against one keeps it until the
        kernel has finished (``RankingPipeline`` keeps it with its answers).
        The object itself holds the generation before the newest and
        synchronizes the device before it lets go of an older one.  Serialise
        ``append`` / ``remove`` against the calls that read the object."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("CitySets.on: the device copies live on the HIP device only")
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        with self._dev_lock:
            gen = self._dev.get(key)
            if gen is None:
                c = self._cols
                with torch.cuda.device(device):
                    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(device)
                    gen = self._dev[key] = self._build(
                        torch.device(*key), c, (up(c.item, np.int32), up(c.city, np.int32),
                                                up(c.key, np.float64), up(c.row, np.int32)))
        return gen
