"""What the ItemFeatures tests share: the numpy model of the feature tables
(main.py:315 and 215-230 in row space), a base table, step sequences in the
manner of city_sets_common.py, the refused calls, the F7 recipe and the
rounding witness.

The model.  Per ``main_df`` row: hotel row, the row's number, the encoded codes
and the raw numeric columns.  A hotel's first row is its first occurrence in
the columns (``np.unique(return_index=True)``); its numeric features are
``x * scale + min`` in float64 -- two operations, as MinMaxScaler.transform's
``X *= scale_; X += min_`` -- cast to float32.
"""
from fractions import Fraction

import numpy as np

BAD_DATA = 2   # DCNR_REQ_BAD_DATA


# ------------------------------------------------------------------ the model
def model(item, row, cat, num, scale, mn, n_items):
    """(first_row int32 [n_items], item_cat int64 [n_items, n_cat], item_num fp32
    [n_items, n_num], the number of hotels with a row)."""
    item, row = np.asarray(item, np.int64), np.asarray(row, np.int64)
    cat, num = np.asarray(cat, np.int64), np.asarray(num, np.float64)
    hotels, at = np.unique(item, return_index=True)
    first = np.full(n_items, -1, np.int32)
    first[hotels] = row[at]
    item_cat = np.zeros((n_items, cat.shape[1]), np.int64)
    item_cat[hotels] = cat[at]
    item_num = np.zeros((n_items, num.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        item_num[hotels] = (num[at] * np.asarray(scale, np.float64) +
                            np.asarray(mn, np.float64)).astype(np.float32)
    return first, item_cat, item_num, hotels.size


# ------------------------------------------------------- the rounding witness
def witness_column():
    """(x [20000], scale, min): a column on which the fused x * scale + min (one
    rounding to float64) and MinMaxScaler's two roundings end in different
    float32 values for some entries."""
    rng = np.random.default_rng(0)
    x = rng.integers(0, 10 ** 6, 20000) / 10 ** 5 + 100000.0
    scale = 1.0 / (x.max() - x.min())      # MinMaxScaler.fit, feature_range (0, 1)
    return x, scale, 0.0 - x.min() * scale


def fused_f32(x, scale, mn):
    """float32(fma(x, scale, min)) per entry: the exact rational x * scale + min
    rounded once to float64 (``float(Fraction)`` rounds correctly, to nearest
    even), as an fma rounds it, then to float32."""
    s, m = Fraction(float(scale)), Fraction(float(mn))
    return np.array([np.float32(float(Fraction(float(v)) * s + m)) for v in x], np.float32)


# ------------------------------------------------------------ generated tables
N_ITEMS, N_CAT, N_NUM = 90, 2, 4
SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2e-308, 1e-40, -1e-40,
                    -1.5, 1e300, -1e300, 3.0])
ARRAYS = ["review_item", "review_row", "review_cat", "review_num", "scaler_scale", "scaler_min"]
COUNTS = ["n_reviews", "next_review_row", "n_items", "n_cat", "n_num"]
TABLES = ["first_rows_host", "item_cat_host", "item_num_host"]
SCALE, MIN = np.array([0.25, 1.0 / 3.0, 1e-3, 2.0]), np.array([-0.5, 0.1, 0.0, -7.0])


def random_rows(m, seed, n_items=N_ITEMS, n_cat=N_CAT, n_num=N_NUM):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, n_items, m), rng.integers(0, 50, (m, n_cat)),
            rng.random((m, n_num)) * 20 - 5)


def base_table():
    """1500 rows over 90 hotels: hotels 0 and 89 have no row, hotel 88 has one
    (row 700), hotel 1's first row is the table's last; a few special values."""
    item, cat, num = random_rows(1500, 31)
    item = 2 + item % 86
    item[700] = 88
    item[item == 1] = 2
    item[1499] = 1
    num[::97, 1] = SPECIAL[np.arange(num[::97].shape[0]) % SPECIAL.size]
    return item, cat, num


def snapshot(ft):
    s = {k: getattr(ft, k).copy() for k in ARRAYS}
    s.update({k: getattr(ft, k)().copy() for k in TABLES})
    s.update({k: getattr(ft, k) for k in COUNTS})
    return s


def assert_same(got, want, what=""):
    """Every host array and table (values as bits, dtype, shape) and count of two objects / snapshots."""
    g = got if isinstance(got, dict) else snapshot(got)
    w = want if isinstance(want, dict) else snapshot(want)
    for k in COUNTS:
        assert g[k] == w[k], f"{what}: {k} {g[k]} != {w[k]}"
    for k in ARRAYS + TABLES:
        assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape, f"{what}: {k}"
        assert g[k].tobytes() == w[k].tobytes(), f"{what}: {k}"


def assert_model(ft, st, what=""):
    first, cat, num, _ = model(st.item, st.row, st.cat, st.num, st.scale, st.min, st.n_items)
    for got, want in ((ft.first_rows_host(), first), (ft.item_cat_host(), cat), (ft.item_num_host(), num)):
        assert got.dtype == want.dtype and got.shape == want.shape, what
        assert got.tobytes() == want.tobytes(), what


class State:
    """The rows a sequence has reached, kept with plain numpy."""

    def __init__(self, item, cat, num, scale=SCALE, mn=MIN, n_items=N_ITEMS):
        self.item = np.asarray(item, np.int64)
        self.cat, self.num = np.asarray(cat, np.int64), np.asarray(num, np.float64).copy()   # [M, width]
        self.scale, self.min, self.n_items = np.asarray(scale, np.float64), np.asarray(mn, np.float64), n_items
        self.row = np.arange(self.item.size, dtype=np.int64)
        self.next = self.item.size

    def apply(self, step):
        op = step[0]
        if op == "append":
            _, item, cat, num = step
            m = len(item)
            self.item = np.concatenate([self.item, np.asarray(item, np.int64)])
            self.cat = np.concatenate([self.cat, np.asarray(cat, np.int64)])
            self.num = np.concatenate([self.num, np.asarray(num, np.float64)])
            self.row = np.concatenate([self.row, self.next + np.arange(m, dtype=np.int64)])
            self.next += m
        elif op == "remove":
            keep = ~np.isin(self.row, np.asarray(step[1], np.int64))
            self.item, self.cat, self.num, self.row = (a[keep] for a in (self.item, self.cat,
                                                                         self.num, self.row))
        elif op == "set_values":
            _, rows, vals, columns = step
            cols = np.arange(self.num.shape[1]) if columns is None else np.asarray(columns)
            vals = np.asarray(vals, np.float64).reshape(len(rows), -1)
            for r, v in zip(rows, vals):      # in order: the last entry of a repeated row counts
                self.num[np.searchsorted(self.row, r), cols] = v
        else:
            self.scale, self.min = np.asarray(step[1], np.float64), np.asarray(step[2], np.float64)

    def fresh(self):
        import dcnr
        return dcnr.ItemFeatures(self.item, self.cat, self.num, self.scale, self.min,
                                 n_items=self.n_items, review_row=self.row, next_review_row=self.next)


def do(ft, step):
    op = step[0]
    if op == "append":
        ft.append(step[1], step[2], step[3])
    elif op == "remove":
        ft.remove(step[1])
    elif op == "set_values":
        ft.set_values(step[1], step[2], columns=step[3])
    else:
        ft.set_scaler(step[1], step[2])


def upload_bytes(step, n_cat=N_CAT, n_num=N_NUM):
    """What the step sends to a device: the batch, whatever the table's length."""
    op = step[0]
    if op == "append":
        return len(step[1]) * (8 + 4 * n_cat + 8 * n_num)
    if op == "remove":
        return 8 * len(step[1])
    if op == "set_values":
        k, w = np.unique(step[1]).size, n_num if step[3] is None else len(step[3])
        return 8 * k * (1 + w) + (0 if step[3] is None else 8 * w)
    return 16 * n_num


def sequences():
    """(name, State at the start, steps).  A step is ("append", item, cat, num),
    ("remove", main_df rows), ("set_values", rows, values, columns or None) or
    ("set_scaler", scale, min)."""
    item, cat, num = base_table()
    M = item.size
    firsts = np.unique(item, return_index=True)[1]          # every hotel's first row
    others = np.setdiff1d(np.arange(M), firsts)
    st = lambda a=None, b=None: State(item[a:b], cat[a:b], num[a:b])
    ap = lambda a, b: ("append", item[a:b], cat[a:b], num[a:b])
    rng = np.random.default_rng(5)
    v = lambda k, w=N_NUM: rng.random((k, w)) * 9 - 3
    return [
        ("all_at_once", State([], np.zeros((0, N_CAT)), np.zeros((0, N_NUM))), [ap(0, M)]),
        ("batches", st(0, 900), [ap(900, 901), ap(901, 1300), ap(1300, M)]),
        ("first_ever_row", st(), [("append", [0, 89, 0], cat[:3], num[:3]),
                                  ("append", [5], cat[:1], [[np.nan, -0.0, np.inf, 1.0]])]),
        ("first_rows", st(), [("remove", firsts[:10]), ("remove", firsts[10:]),
                              ("remove", [int(others[0])])]),
        ("only_row", st(), [("remove", [700]), ("remove", [1499]), ("append", [88], cat[:1], num[:1])]),
        ("edits", st(), [("set_values", firsts[:7], v(7), None),
                         ("set_values", others[:9], v(9), None),
                         ("set_values", [int(firsts[3]), 700, int(firsts[3])], v(3, 2), [3, 0]),
                         ("set_values", [1499], [[np.nan]], [1])]),
        ("scaler", st(), [("set_scaler", SCALE * 3, MIN - 1), ("remove", firsts[:5]),
                          ("set_scaler", [0.0, -1.0, 1e-300, 1e300], [0.0, 5e-324, -0.0, 1.0])]),
        ("mixed", st(0, 1000), [("remove", np.arange(0, 1000, 7)), ap(1000, 1200),
                                ("set_values", [1, 1001, 1199], v(3), None),
                                ("remove", [1000, 1199, 3]), ap(1200, M),
                                ("set_scaler", SCALE[::-1], MIN[::-1]),
                                ("set_values", [M - 1, 2], v(2, 1), [2])]),
        ("everything", st(0, 30), [("remove", np.arange(30)), ap(30, 60)]),
    ]


def refused(ft):
    """Calls that must raise ValueError and leave the object as it was."""
    c, x = np.zeros((2, N_CAT), np.int64), np.zeros((2, N_NUM))
    return [lambda: ft.remove([10 ** 6]), lambda: ft.remove([-1]), lambda: ft.remove([3, 4, 3]),
            lambda: ft.remove([ft.next_review_row]),
            lambda: ft.append([1, N_ITEMS], c, x), lambda: ft.append([1, -1], c, x),
            lambda: ft.append([1, 2], c[:, :1], x), lambda: ft.append([1, 2], c, x[:, :3]),
            lambda: ft.append([1, 2], c, x[:1]), lambda: ft.append([1], c, x),
            lambda: ft.set_values([10 ** 6], x[:1]), lambda: ft.set_values([3, ft.next_review_row], x),
            lambda: ft.set_values([3, 4], x[:, :3]), lambda: ft.set_values([3, 4], x, columns=[0, 1]),
            lambda: ft.set_values([3], x[:1, :2], columns=[0, N_NUM]),
            lambda: ft.set_values([3], x[:1, :2], columns=[1, 1]),
            lambda: ft.set_values([3], x[:1, :1], columns=[-1]),
            lambda: ft.set_scaler(SCALE[:3], MIN[:3]), lambda: ft.set_scaler(SCALE, MIN[:3]),
            lambda: ft.set_scaler(SCALE * np.nan, MIN), lambda: ft.set_scaler(SCALE, MIN + np.inf)]


# --------------------------------------------------------------- the F7 recipe
def f7_columns(f, main_df=None):
    """The fixture's main_df as the columns ``ItemFeatures`` takes, encoded as
    f7_common.load() encodes them: (item, cat, num, scale, min, main_df numbers)."""
    import json
    import os

    import f7_common
    art = json.load(open(os.path.join(f7_common.DIR, "artifacts.json")))
    df = f.main_df if main_df is None else main_df
    item = df["item_id"].map(f.item_map).to_numpy()
    cat = np.stack([df[c].map(lambda v, enc=enc: enc.get(str(v), 0)).to_numpy(np.int64)
                    for c, enc in art["cat_encoders"].items()], 1)
    num = df[art["numerical_cols"]].to_numpy(np.float64)
    return item, cat, num, np.array(art["scaler_scale"]), np.array(art["scaler_min"]), df.index.to_numpy()


def f7_item_features(f):
    import dcnr
    item, cat, num, scale, mn, _ = f7_columns(f)
    return dcnr.ItemFeatures(item, cat, num, scale, mn, n_items=f.n_items)


def f7_tables(f, main_df):
    """f7_common.load()'s pandas recipe for item_cat / item_num on another main_df;
    a hotel without a row keeps zeros."""
    import json
    import os

    import f7_common
    art = json.load(open(os.path.join(f7_common.DIR, "artifacts.json")))
    first = main_df.drop_duplicates(subset=["item_id"]).set_index("item_id")
    item_cat = np.zeros((f.n_items, len(art["cat_encoders"])), np.int64)
    item_num = np.zeros((f.n_items, f.n_num), np.float32)
    mn, sc = np.array(art["scaler_min"]), np.array(art["scaler_scale"])
    for h, r in f.item_map.items():
        if h not in first.index:
            continue
        row = first.loc[h]
        item_cat[r] = [enc.get(str(row[c]), 0) for c, enc in art["cat_encoders"].items()]
        x = row[art["numerical_cols"]].to_numpy(np.float64)
        item_num[r] = (x * sc + mn).astype(np.float32)
    return item_cat, item_num
