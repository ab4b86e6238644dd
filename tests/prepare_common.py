"""Cases shared by test_prepare_cpu.py and test_prepare_gpu.py: the golden frame
of tests/golden/prepare (the reference's own outputs), random frames, and the
data edge cases of the contract.  A case is a dict of the
arguments ``dcnr.prepare_data`` and ``dcnr.prepare_data_host`` share."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prepare", "prepare_golden.npz")
EPS = np.finfo(np.float64).eps
DERIVED_NAMES = {0: "ratio", 1: "diff"}


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_case(g=None):
    g = g if g is not None else load_golden()
    values = lambda a: np.array([None if v == "" else v for v in a.tolist()], dtype=object)
    col, lo, hi = g["filter"]
    return dict(user=g["user"], item=g["item"], target=g["target"],
                cat=[values(g["city"]), values(g["kind"])], num=g["raw"],
                cat_names=[str(c) for c in g["cat_names"]], noise_filter=(int(col), float(lo), float(hi)),
                derived=[(DERIVED_NAMES[int(op)], int(i), int(j)) for op, i, j in g["derived"]])


def call(fn, case, **kw):
    c = dict(case)
    return fn(c.pop("user"), c.pop("item"), c.pop("target"), c.pop("cat"), c.pop("num"), **c, **kw)


def same(a, b):
    """Equal values; NaN equals NaN and -0.0 equals 0.0 (the one freedom the
    contract leaves); dtypes and shapes equal."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and \
        (np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b))


def to_np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def assert_same_prepared(a, b, what=""):
    """Two results of prepare_data / prepare_data_host agree in every field."""
    assert a.model_dims == b.model_dims, what
    for k in ("median_", "data_min_", "data_max_", "scale_", "min_", "user_ids", "item_ids", "rows",
              "rows_train", "rows_val"):
        assert same(to_np(getattr(a, k)), to_np(getattr(b, k))), f"{what}: {k}"
    assert len(a.cat_keys) == len(b.cat_keys)
    for c, (x, y) in enumerate(zip(a.cat_keys, b.cat_keys)):
        assert same(to_np(x), to_np(y)), f"{what}: cat_keys[{c}]"
    for name in ("full", "train", "val"):
        for k, x, y in zip(("collab", "cat", "num", "y"), getattr(a, name), getattr(b, name)):
            assert same(to_np(x), to_np(y)), f"{what}: {name} {k}"
    assert a.n_after_filter == b.n_after_filter, what


def assert_matches_golden(p, g):
    """A result on golden_case() against the reference's outputs."""
    names = [str(c) for c in g["cat_names"]]
    assert p.model_dims == (int(g["n_users"]), int(g["n_items"]),
                            {n: int(d) for n, d in zip(names, g["cat_dims"])}, int(g["n_num"]))
    for split in ("train", "val"):
        for k, t in zip(("collab", "cat", "num", "y"), getattr(p, split)):
            assert same(to_np(t), g[f"{split}_{k}"]), f"{split} {k}"
    assert list(p.user_id_mapping.keys()) == g["user_ids"].tolist()
    assert list(p.user_id_mapping.values()) == list(range(int(g["n_users"])))
    assert list(p.item_id_mapping.keys()) == g["item_ids"].tolist()
    enc = p.cat_encoders
    assert list(enc[names[0]].keys()) == g["city_categories"].tolist()
    assert list(enc[names[1]].keys()) == g["kind_categories"].tolist()
    assert list(enc[names[1]].values()) == list(range(len(g["kind_categories"])))
    for k, ref in (("scale_", "scale"), ("min_", "min"), ("data_min_", "data_min"), ("data_max_", "data_max")):
        assert same(getattr(p, k), g[ref]), k
    art = p.artifacts()
    assert art["categorical_cols"] == names and art["user_id_mapping"] is p.user_id_mapping
    assert same(art["scaler"]["scale_"], g["scale"])


# ------------------------------------------------------------------ random frames
def random_case(seed, M, n_cat=2, n_raw=8, n_derived=3, n_users=None, n_items=None, nan=0.05, missing=0.05,
                use_filter=True, wide_ids=True):
    rng = np.random.default_rng(seed)
    n_users = n_users or max(1, M // 3)
    n_items = n_items or max(1, M // 7)
    user = rng.integers(0, n_users, M).astype(np.int64)
    item = rng.integers(0, n_items, M).astype(np.int64)
    if wide_ids:   # negative ids, ids above 2^40, ids that agree in their low 32 bits
        user = (user - n_users // 2) * ((1 << 32) + 0) + (user % 3)
        item = item + (1 << 41) * (item % 2)
    raw = np.round(rng.normal(5.0, 3.0, (M, n_raw)), 1)
    if n_raw:
        raw[:, 0] = rng.integers(1, 11, M)       # the filter column: ratings
        raw[rng.random((M, n_raw)) < nan] = np.nan
        raw[rng.random((M, n_raw)) < 0.03] = 0.0
    cat = [rng.integers(0, 3 + 4 * c, M).astype(np.int64) for c in range(n_cat)]
    for k in cat:
        k[rng.random(M) < missing] = -1
        k *= 1 + (seed % 2) * 1000003    # keys need not be dense
        k[k < 0] = -1
    derived = []
    for d in range(n_derived):
        i, j = rng.integers(0, n_raw, 2)
        derived.append(("ratio" if d % 3 != 2 else "diff", int(i), int(j)))
    return dict(user=user, item=item, target=rng.integers(0, 2, M), cat=cat, num=raw,
                noise_filter=(0, 4.0, 8.0) if use_filter and n_raw else None, derived=derived)


def plain_case(M, columns, n_cat=1, user=None, item=None, cat=None, **kw):
    """A frame with the given numeric columns (a list of length-M arrays), no
    filter, distinct users unless given."""
    raw = np.stack([np.asarray(c, dtype=np.float64) for c in columns], axis=1) if columns else \
        np.zeros((M, 0))
    return dict(user=np.arange(M, dtype=np.int64) if user is None else np.asarray(user, np.int64),
                item=(np.arange(M, dtype=np.int64) % 5) if item is None else np.asarray(item, np.int64),
                target=np.arange(M) % 2,
                cat=[np.arange(M, dtype=np.int64) % 3 for _ in range(n_cat)] if cat is None else cat,
                num=raw, **kw)


def edge_columns(M=101):
    """Numeric columns that exercise the median and the scaler rules, each of M
    (odd) values; returns (names, columns)."""
    rng = np.random.default_rng(5)
    base = rng.normal(0.0, 1.0, M)
    cols, names = [], []

    def add(name, c):
        names.append(name)
        cols.append(np.asarray(c, dtype=np.float64))
    add("all_nan", np.full(M, np.nan))
    add("constant", np.full(M, 2.5))
    c = np.full(M, 1.0); c[::2] = 1.0 + 5 * EPS
    add("range_5eps", c)            # scale_ must be 1.0
    c = np.full(M, 1.0); c[::2] = 1.0 + 20 * EPS
    add("range_20eps", c)           # scale_ must not
    # an even count (one NaN) whose two middle values differ in the last bit
    c = np.concatenate([np.full(M // 2, 0.1), [np.nan], np.full(M // 2, np.nextafter(0.1, 1.0))])
    add("last_bit", c)
    c = np.concatenate([np.full(M // 2, 1.7e308), [np.nan], np.full(M // 2, 1.7e308)])
    add("overflow_sum", c)          # (a + b) / 2 is inf: where scikit-learn then raises
    c = base.copy(); c[3] = -0.0; c[4] = 0.0
    add("minus_zero", c)
    c = np.abs(base) * 1e-310       # subnormals
    add("subnormal", c)
    c = base.copy(); c[::3] = np.nan
    add("third_nan", c)
    c = np.zeros(M); c[0] = -0.0; c[5:9] = np.nan
    add("zeros", c)
    return names, cols
