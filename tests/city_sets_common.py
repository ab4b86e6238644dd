"""What the CitySets tests share: the numpy model of the city / popular sets
(main.py:205-209 in row space), the pandas restatement the model is held to, a
table generator with the awkward cases planted, and append / remove sequences
in the manner of store_append_common.py.

The model.  Per ``main_df`` row: hotel row, city code, popularity key
(user_reviews_count) and the row's number.  city(c) = the distinct hotels of
city c; top_rows(c) = the first ``top`` rows of city c in the order np.lexsort
over (row, -key with NaN mapped last, isnan) gives; popular(c) = the distinct
hotels of top_rows(c).
"""
import numpy as np
import pandas as pd

OVERFLOW, BAD_DATA = 1, 2   # DCNR_REQ_*


# ------------------------------------------------------------------ the model
def model(item, city, key, row, C, top):
    """(set_offsets [2C + 2], set_rows, top_rows [C, top]) as dcnr_city_sets_build
    lays them out: sets 0..C-1 city(c), C..2C-1 popular(c), set 2C empty;
    top_rows holds ``main_df`` numbers, -1 behind a city's last."""
    item, city, row = (np.asarray(a, np.int64) for a in (item, city, row))
    key = np.asarray(key, np.float64)
    M = item.size
    nan = np.isnan(key)
    order = np.lexsort((row, np.where(nan, 0.0, -key), nan, city))   # city, then the served order
    start = np.zeros(C + 1, np.int64)
    np.cumsum(np.bincount(city, minlength=C), out=start[1:])
    rank = np.arange(M) - start[city[order]]
    sel = order[rank < top]
    top_rows = np.full((C, top), -1, np.int64)
    top_rows[city[sel], rank[rank < top]] = row[sel]
    W = max(int(item.max()) + 1 if M else 1, 1)
    pairs = lambda idx: np.unique(city[idx] * W + item[idx])
    c_pairs, p_pairs = pairs(np.arange(M)), pairs(sel)
    lens = np.concatenate([np.bincount(c_pairs // W, minlength=C), np.bincount(p_pairs // W, minlength=C)])
    off = np.zeros(2 * C + 2, np.int64)
    np.cumsum(lens, out=off[1:2 * C + 1])
    off[2 * C + 1] = off[2 * C]
    return off, np.concatenate([c_pairs % W, p_pairs % W]), top_rows.astype(np.int32)


def model_sets(item, city, key, row, C, top):
    """The same per city: (city(c), top_rows(c), popular(c)) for c in [0, C)."""
    off, rows, top_rows = model(item, city, key, row, C, top)
    return [(rows[off[c]:off[c + 1]], top_rows[c][top_rows[c] >= 0].astype(np.int64),
             rows[off[C + c]:off[C + c + 1]]) for c in range(C)]


# -------------------------------------------- main.py:205-209 with pandas
def pandas_sets(item, city, key, row, c, top, kind=None):
    """(city hotels, the popular rows' numbers in served order, popular hotels)
    of city c by the reference's operations; kind=None: its default sort."""
    df = pd.DataFrame({"item_id": item, "city": city, "user_reviews_count": key}, index=row)
    sub = df[df["city"] == c]
    kw = {} if kind is None else dict(kind=kind)
    head = sub.sort_values(by="user_reviews_count", ascending=False, **kw).head(top)
    return (sorted(set(sub["item_id"].unique().tolist())), head.index.to_numpy(),
            sorted(set(head["item_id"].tolist())))


def cut_is_decided(item, key, row, top):
    """Of one city's rows: True if every sort kind gives the same popular set --
    the tie group at the cut does not straddle it, or names one hotel only."""
    if key.size <= top:
        return True
    nan = np.isnan(key)
    o = np.lexsort((row, np.where(nan, 0.0, -key), nan))
    same = lambda a, b: a == b or (np.isnan(a) and np.isnan(b))
    if not same(key[o[top - 1]], key[o[top]]):
        return True
    k = key[o[top]]
    group = nan if np.isnan(k) else key == k
    return np.unique(item[group]).size == 1


# ------------------------------------------------------------ generated tables
SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2e-308, -1.5, -1e300,
                    1e300, 1.0, 3.0])


def table(M, C, n_items, seed, top=100):
    """(item, city, key): cities of every size (some empty, some short of
    ``top``, some far above), hotels that appear in two cities, and keys of four
    kinds by city: distinct values, small integers (ties across the cut),
    all equal, and a mix with NaN, +-inf, +-0.0, denormals and negatives.  At
    least half of the cities draw distinct keys."""
    rng = np.random.default_rng(seed)
    w = rng.random(C) ** 3 + 1e-3
    w[rng.random(C) < 0.15] = 0.0             # empty cities
    if w.sum() == 0:
        w[0] = 1.0
    city = rng.choice(C, M, p=w / w.sum())
    home = rng.integers(0, C, n_items)         # most hotels live in one city ...
    pool = [np.flatnonzero(home == c) for c in range(C)]
    item = np.array([rng.choice(pool[c]) if pool[c].size and rng.random() < 0.9
                     else rng.integers(0, n_items) for c in city], np.int64).reshape(-1)
    kind = np.where(np.arange(C) % 2 == 0, 0, 1 + (np.arange(C) // 2) % 3)
    key = np.empty(M, np.float64)
    k0 = rng.permutation(M).astype(np.float64) * 0.5          # distinct
    k1 = rng.integers(0, 8, M).astype(np.float64)             # ties
    k3 = SPECIAL[rng.integers(0, SPECIAL.size, M)]
    for kd, src in ((0, k0), (1, k1), (2, np.full(M, 7.0)), (3, k3)):
        m = kind[city] == kd
        key[m] = src[m]
    return item, city.astype(np.int64), key


def f7_city_sets(f):
    """``CitySets`` of a fixture's main_df, as INTEGRATION.md builds one: (the
    object, city name -> code)."""
    import dcnr
    cat = f.main_df["city"].astype("category")
    code = {name: i for i, name in enumerate(cat.cat.categories)}
    cs = dcnr.CitySets(f.main_df["item_id"].map(f.item_map).to_numpy(), cat.cat.codes.to_numpy(),
                       f.main_df["user_reviews_count"].to_numpy(), n_items=f.n_items,
                       n_cities=len(code))
    return cs, code


# ------------------------------------------------- append / remove sequences
N_ITEMS, C, TOP = 40, 7, 5
ARRAYS = ["review_item", "review_city", "review_popularity", "review_row"]
COUNTS = ["n_reviews", "next_review_row", "n_items", "n_cities", "top"]


def snapshot(cs):
    s = {k: getattr(cs, k).copy() for k in ARRAYS}
    s.update({k: getattr(cs, k) for k in COUNTS})
    return s


def assert_same(got, want, what=""):
    """Every host array (values as bits, dtype, shape) and count of two objects / snapshots."""
    g = got if isinstance(got, dict) else snapshot(got)
    w = want if isinstance(want, dict) else snapshot(want)
    for k in COUNTS:
        assert g[k] == w[k], f"{what}: {k} {g[k]} != {w[k]}"
    for k in ARRAYS:
        assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape, f"{what}: {k}"
        assert g[k].tobytes() == w[k].tobytes(), f"{what}: {k}"


class State:
    """The rows a sequence has reached, kept with plain numpy."""

    def __init__(self, item, city, key):
        self.item, self.city = np.asarray(item, np.int64), np.asarray(city, np.int64)
        self.key = np.asarray(key, np.float64)
        self.row = np.arange(self.item.size, dtype=np.int64)
        self.next = self.item.size

    def apply(self, step):
        if step[0] == "append":
            _, item, city, key = step
            m = len(item)
            self.item = np.concatenate([self.item, np.asarray(item, np.int64)])
            self.city = np.concatenate([self.city, np.asarray(city, np.int64)])
            self.key = np.concatenate([self.key, np.asarray(key, np.float64)])
            self.row = np.concatenate([self.row, self.next + np.arange(m, dtype=np.int64)])
            self.next += m
        else:
            keep = ~np.isin(self.row, np.asarray(step[1], np.int64))
            self.item, self.city, self.key, self.row = (a[keep] for a in (self.item, self.city,
                                                                          self.key, self.row))

    def fresh(self):
        import dcnr
        return dcnr.CitySets(self.item, self.city, self.key, n_items=N_ITEMS, n_cities=C, top=TOP,
                             review_row=self.row, next_review_row=self.next)


def do(cs, step):
    if step[0] == "append":
        cs.append(step[1], step[2], step[3])
    else:
        cs.remove(step[1])


def base_table():
    """200 rows over 7 cities with top = 5: city 5 holds two rows, city 6 none;
    hotel 39 appears once, in city 0; city 1's keys are all equal; city 2's
    hold the special values."""
    rng = np.random.default_rng(11)
    M = 200
    city = rng.integers(0, 5, M)
    item = (city * 7 + rng.integers(0, 7, M)) % 38
    key = rng.integers(0, 6, M).astype(np.float64)
    key[city == 1] = 3.0
    m2 = np.flatnonzero(city == 2)
    key[m2] = SPECIAL[rng.integers(0, SPECIAL.size, m2.size)]
    city[[17, 150]], item[[17, 150]], key[[17, 150]] = 5, [3, 38], [2.0, np.nan]
    first0 = int(np.flatnonzero(city == 0)[0])
    item[first0], key[first0] = 39, 100.0     # the only row of (city 0, hotel 39), and city 0's best
    return item, city, key


def sequences():
    """(name, State at the start, steps).  A step is ("append", item, city, key)
    or ("remove", main_df rows)."""
    item, city, key = base_table()
    M = item.size
    of = lambda c: np.flatnonzero(city == c)
    # city 3's served order at the start: removing its best row moves the sixth up
    nan = np.isnan(key)
    o3 = of(3)[np.lexsort((of(3), np.where(nan[of(3)], 0.0, -key[of(3)]), nan[of(3)]))]
    st = lambda a=None, b=None: State(item[a:b], city[a:b], key[a:b])
    ap = lambda a, b: ("append", item[a:b], city[a:b], key[a:b])
    seqs = [
        ("all_at_once", State([], [], []), [ap(0, M)]),
        ("batches", st(0, 120), [ap(120, 121), ap(121, 180), ap(180, M)]),
        ("first_and_last_of_a_city", st(), [("remove", [of(4)[0]]), ("remove", [of(4)[-1]]),
                                            ("remove", [of(0)[-1], of(0)[0]])]),
        ("all_of_a_city", st(), [("remove", of(5)), ("remove", of(1))]),
        ("inside_top_rows", st(), [("remove", [o3[0]]), ("remove", [o3[2], o3[1]]),
                                   ("remove", o3[3:9])]),
        ("only_row_of_a_pair", st(), [("remove", [of(0)[0]])]),
        ("first_and_last_row", st(), [("remove", [0, M - 1]), ("append", [5], [6], [1.0]),
                                      ("remove", [M])]),
        ("mixed", st(0, 150), [("remove", np.arange(10, 150, 7)), ap(150, 180),
                               ("remove", [150, 179, 3]), ap(180, M),
                               ("append", [39, 39, 0], [6, 6, 6], [np.nan, -0.0, 0.0])]),
        ("everything", st(0, 30), [("remove", np.arange(30)), ap(30, 60)]),
    ]
    return seqs


def refused(cs):
    """Calls that must raise ValueError and leave the object as it was."""
    return [lambda: cs.remove([10 ** 6]), lambda: cs.remove([-1]), lambda: cs.remove([3, 4, 3]),
            lambda: cs.remove([cs.next_review_row]),
            lambda: cs.append([1, N_ITEMS], [0, 0], [1.0, 1.0]),
            lambda: cs.append([1, -1], [0, 0], [1.0, 1.0]),
            lambda: cs.append([1, 2], [0, C], [1.0, 1.0]),
            lambda: cs.append([1, 2], [0, -1], [1.0, 1.0]),
            lambda: cs.append([1, 2], [0, 1], [1.0])]
