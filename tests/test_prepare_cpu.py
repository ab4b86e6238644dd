"""``dcnr.prepare_data_host`` (the numpy yardstick of the device prepare_data)
and ``dcnr.category_keys`` on the build machine:

  1  the golden frame: the reference's own filter lines and prepare_data
     (tests/golden/make_prepare_golden.py), every output equal in value
  2  random frames and the data edge cases against a direct pandas /
     MinMaxScaler / train_test_split computation (this file's own code), where
     pandas and scikit-learn are installed
  3  category_keys against ``astype('category').cat.codes``
  4  the split and the errors without those libraries
"""
import numpy as np
import pytest

import prepare_common as pc
from dcnr import category_keys, prepare_data_host
from dcnr import prepare as prep_mod


def test_host_matches_golden():
    g = pc.load_golden()
    pc.assert_matches_golden(pc.call(prepare_data_host, pc.golden_case(g)), g)


def test_golden_fixture_is_small_data():
    import os
    assert os.path.getsize(pc.GOLDEN) < 200 * 1024
    g = pc.load_golden()
    assert g["raw"].shape == (400, 8) and g["train_num"].shape[1] == 11


# --------------------------------------------------- 2: pandas and scikit-learn
def pandas_prepare(case, test_size=0.2, random_state=42):
    """The reference's steps written with pandas, MinMaxScaler and
    train_test_split directly (not through dcnr)."""
    pd = pytest.importorskip("pandas")
    MinMaxScaler = pytest.importorskip("sklearn.preprocessing").MinMaxScaler
    train_test_split = pytest.importorskip("sklearn.model_selection").train_test_split
    raw = np.asarray(case["num"], dtype=np.float64)
    M, n_raw = raw.shape
    df = pd.DataFrame({"u": case["user"], "i": case["item"], "t": case["target"]})
    df["pos"] = np.arange(M)
    cat_names = [f"c{k}" for k in range(len(case["cat"]))]
    for name, col in zip(cat_names, case["cat"]):
        col = np.asarray(col)
        if col.dtype.kind in "iu":    # keys: negative means missing
            col = np.where(col < 0, np.nan, col.astype(np.float64))
        df[name] = col
    num_names = [f"n{k}" for k in range(n_raw)]
    for k, name in enumerate(num_names):
        df[name] = raw[:, k]
    if case.get("noise_filter") is not None:
        col, lo, hi = case["noise_filter"]
        df = df[(df[f"n{col}"] >= hi) | (df[f"n{col}"] <= lo)].copy()
    for d, (op, i, j) in enumerate(case.get("derived", ())):
        name = f"d{d}"
        if op == "ratio":
            df[name] = (df[f"n{i}"] / df[f"n{j}"]).replace([np.inf, -np.inf], 0).fillna(0)
        else:
            df[name] = df[f"n{i}"] - df[f"n{j}"]
        num_names.append(name)
    n_after = len(df)
    median = df[num_names].median() if num_names else None
    if num_names:
        df[num_names] = df[num_names].fillna(median)
    if cat_names:
        df = df.dropna(subset=cat_names).copy()
    umap = {o: k for k, o in enumerate(df["u"].unique())}
    imap = {o: k for k, o in enumerate(df["i"].unique())}
    collab = np.stack([df["u"].map(umap).values, df["i"].map(imap).values], axis=1).astype(np.int64)
    cats, keys = [], []
    for name in cat_names:
        c = df[name].astype("category")
        keys.append(np.asarray(c.cat.categories))
        cats.append(c.cat.codes.values.astype(np.int64))
    out = dict(n_after=n_after, rows=df["pos"].values, collab=collab,
               cat=np.stack(cats, axis=1) if cats else np.zeros((len(df), 0), np.int64),
               user_ids=np.array(list(umap), dtype=np.int64), item_ids=np.array(list(imap), dtype=np.int64),
               keys=keys, y=df["t"].values.astype(np.float32),
               median=median.values if num_names else np.zeros(0))
    scaler = MinMaxScaler()
    if num_names:
        out["num"] = scaler.fit_transform(df[num_names]).astype(np.float32)   # raises on inf
        out.update(scale=scaler.scale_, min=scaler.min_, data_min=scaler.data_min_, data_max=scaler.data_max_)
    else:
        out["num"] = np.zeros((len(df), 0), np.float32)
    tr, va, _, _ = train_test_split(np.arange(len(df)), out["y"], test_size=test_size,
                                    random_state=random_state)
    out["train_idx"], out["val_idx"] = tr, va
    return out


def check_against_pandas(case):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            ref = pandas_prepare(case)
        except ValueError:
            with pytest.raises(ValueError):
                pc.call(prepare_data_host, case)
            return "raises"
    p = pc.call(prepare_data_host, case)
    assert p.n_after_filter == ref["n_after"]
    assert pc.same(p.rows, ref["rows"].astype(np.int32))
    assert pc.same(p.user_ids, ref["user_ids"]) and pc.same(p.item_ids, ref["item_ids"])
    collab, cat, num, y = p.full
    assert pc.same(collab, ref["collab"]) and pc.same(cat, ref["cat"]) and pc.same(y, ref["y"])
    for c, k in enumerate(ref["keys"]):
        assert pc.same(p.cat_keys[c], k.astype(np.int64))
    assert pc.same(num, ref["num"])
    if num.shape[1]:
        assert pc.same(p.median_, ref["median"])
        for a, b in (("scale_", "scale"), ("min_", "min"), ("data_min_", "data_min"), ("data_max_", "data_max")):
            assert pc.same(getattr(p, a), ref[b]), a
    assert pc.same(p.rows_train, p.rows[ref["train_idx"]]) and pc.same(p.rows_val, p.rows[ref["val_idx"]])
    for k, t in enumerate(p.train):
        assert pc.same(t, p.full[k][ref["train_idx"]])
    for k, t in enumerate(p.val):
        assert pc.same(t, p.full[k][ref["val_idx"]])
    return "equal"


RANDOM = [dict(seed=1, M=2), dict(seed=2, M=5, use_filter=False), dict(seed=3, M=63), dict(seed=4, M=64),
          dict(seed=5, M=65), dict(seed=6, M=1003), dict(seed=7, M=4097), dict(seed=8, M=300, n_cat=0),
          dict(seed=9, M=300, n_derived=0), dict(seed=10, M=500, nan=0.5, missing=0.3),
          dict(seed=11, M=200, n_users=1), dict(seed=12, M=20000, n_users=50, n_items=7)]


@pytest.mark.parametrize("kw", RANDOM, ids=lambda kw: f"M{kw['M']}s{kw['seed']}")
def test_host_matches_pandas_random(kw):
    assert check_against_pandas(pc.random_case(**kw)) == "equal"


def test_host_matches_pandas_edge_columns():
    names, cols = pc.edge_columns()
    keep = [c for n, c in zip(names, cols) if n != "overflow_sum"]
    assert check_against_pandas(pc.plain_case(101, keep)) == "equal"
    # even counts too: drop the first row through its category
    cat = [np.where(np.arange(101) == 0, -1, np.arange(101) % 3)]
    assert check_against_pandas(pc.plain_case(101, keep, cat=cat)) == "equal"


def test_host_matches_pandas_where_it_raises():
    names, cols = pc.edge_columns()
    over = [c for n, c in zip(names, cols) if n == "overflow_sum"]
    assert check_against_pandas(pc.plain_case(101, over)) == "raises"        # the median is inf
    c = np.arange(11.0); c[4] = np.inf
    assert check_against_pandas(pc.plain_case(11, [c])) == "raises"
    c = np.array([-np.inf, np.inf, np.nan, np.nan])                            # median NaN, inf stays
    assert check_against_pandas(pc.plain_case(4, [c])) == "raises"
    case = pc.random_case(3, 40)
    case["noise_filter"] = (0, -1.0, 100.0)                                    # drops every row
    assert check_against_pandas(case) == "raises"
    assert check_against_pandas(pc.random_case(3, 1, missing=0.0, use_filter=False)) == "raises"   # n = 1


def test_median_rules():
    m = prep_mod._median
    assert m(np.array([3.0, 1.0, 2.0])) == 2.0 and m(np.array([4.0, 1.0, 2.0, 3.0])) == 2.5
    assert np.isnan(m(np.zeros(0))) and np.isnan(m(np.array([-np.inf, np.inf])))
    assert m(np.array([1.7e308, 1.7e308])) == np.inf
    a, b = 0.1, np.nextafter(0.1, 1.0)
    assert m(np.array([a, b])) == (a + b) / 2
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(0)
    for _ in range(300):
        v = rng.normal(0, 1, rng.integers(1, 40)) * 10.0 ** rng.integers(-5, 5)
        assert m(v) == pd.Series(v).median()


# ------------------------------------------------------------ 3: category_keys
def test_category_keys_as_pandas_codes():
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(1)
    words = np.array(["b", "a", "zz", "Z", "aa", "", "10", "9"], dtype=object)
    v = words[rng.integers(0, len(words), 200)]
    v[rng.random(200) < 0.2] = None
    v[7] = float("nan")
    keys, cats = category_keys(v)
    c = pd.Series(v).astype("category")
    assert pc.same(keys, c.cat.codes.values.astype(np.int64)) and cats == list(c.cat.categories)
    f = rng.integers(-3, 4, 100).astype(np.float64)
    f[::9] = np.nan
    keys, cats = category_keys(f)
    c = pd.Series(f).astype("category")
    assert pc.same(keys, c.cat.codes.values.astype(np.int64)) and cats == list(c.cat.categories)
    keys, cats = category_keys(np.array(["x", "y", "x"]))
    assert keys.tolist() == [0, 1, 0] and cats == ["x", "y"]


def test_category_keys_plain():
    keys, cats = category_keys([None, "b", "a", float("nan"), "b"])
    assert keys.tolist() == [-1, 1, 0, -1, 1] and cats == ["a", "b"] and keys.dtype == np.int64
    ints = np.array([5, -1, 3, 5, -9])
    keys, cats = category_keys(ints)
    assert keys.tolist() == ints.tolist() and cats == [3, 5]


# ------------------------------------------------- 4: the split and the errors
def test_split_indices():
    for n in (2, 5, 9, 10, 11, 15, 1003):
        tr, va = prep_mod.split_indices(n)
        perm = np.random.RandomState(42).permutation(n)
        n_test = int(np.ceil(0.2 * n))
        assert va.tolist() == perm[:n_test].tolist() and tr.tolist() == perm[n_test:].tolist()
    for n in (0, 1):
        with pytest.raises(ValueError):
            prep_mod.split_indices(n)
    sk = pytest.importorskip("sklearn.model_selection")
    for n in (2, 3, 15, 35, 1003, 4097):
        tr, va = sk.train_test_split(np.arange(n), test_size=0.2, random_state=42)
        a, b = prep_mod.split_indices(n)
        assert a.tolist() == tr.tolist() and b.tolist() == va.tolist()


def test_host_errors_and_arguments():
    case = pc.random_case(1, 50)
    with pytest.raises(ValueError):
        pc.call(prepare_data_host, dict(case, derived=[("ratio", 0, 8)]))
    with pytest.raises(ValueError):
        pc.call(prepare_data_host, dict(case, derived=[("sum", 0, 1)]))
    with pytest.raises(ValueError):
        pc.call(prepare_data_host, dict(case, noise_filter=(8, 4.0, 8.0)))
    with pytest.raises(ValueError):
        pc.call(prepare_data_host, dict(case, cat_names=["only_one"]))
    p = pc.call(prepare_data_host, dict(case, cat_names=["city", "kind"]))
    assert list(p.model_dims[2]) == ["city", "kind"] and p.model_dims[3] == 11
    assert p.artifacts()["cat_encoders"]["city"] == {int(k): i for i, k in enumerate(p.cat_keys[0])}
