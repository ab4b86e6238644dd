"""Generate tests/golden/prepare/prepare_golden.npz by running the REFERENCE's
driver lines (train.py:280-287: the noise filter and the derived columns) and
its prepare_data (train.py:36-87) on a synthetic frame of 400 rows.

Run where the reference tree is (the build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_prepare_golden.py

The driver lines sit under the reference's ``if __name__ == "__main__"``; they
are taken from its syntax tree at run time (the assignments to ``df_full`` and
the two column lists) and executed on the synthetic frame, so none of its text
is kept here.  optuna, plotly and kaleido are only imported by train.py, never
used on this path: stub modules stand in for them.

The fixture holds data only: the input columns and every output (the four
tensors per split, model_dims, the maps as lists, the scaler's arrays).
"""
from __future__ import annotations

import ast
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "prepare", "prepare_golden.npz")
M = 400


def load_reference():
    for name in ("optuna", "plotly", "kaleido"):
        sys.modules.setdefault(name, types.ModuleType(name))
    spec = importlib.util.spec_from_file_location("ref_train", os.path.join(REF, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    cwd = os.getcwd()
    os.chdir("/tmp")
    try:
        spec.loader.exec_module(mod)
    finally:
        os.chdir(cwd)
    return mod


def driver_statements():
    """From the reference's __main__ block: the statements that filter df_full
    and add its derived columns, and the two column lists."""
    with open(os.path.join(REF, "train.py")) as f:
        tree = ast.parse(f.read())
    main = [n for n in tree.body if isinstance(n, ast.If) and "__name__" in ast.dump(n.test)][-1]
    frame, lists = [], []
    for node in ast.walk(main):
        if not isinstance(node, ast.Assign) or len(node.targets) != 1:
            continue
        t = node.targets[0]
        if isinstance(t, ast.Name) and t.id == "df_full" and isinstance(node.value, ast.Subscript):
            frame.append(node)   # the noise filter
        elif isinstance(t, ast.Subscript) and isinstance(t.value, ast.Name) and t.value.id == "df_full":
            frame.append(node)   # a derived column
        elif isinstance(t, ast.Name) and t.id in ("CATEGORICAL_COLS", "NUMERICAL_COLS"):
            lists.append(node)
    frame.sort(key=lambda n: n.lineno)
    assert len(frame) == 4 and len(lists) == 2, (len(frame), len(lists))
    return frame, lists


def run(nodes, env):
    mod = ast.Module(body=list(nodes), type_ignores=[])
    exec(compile(ast.fix_missing_locations(mod), "<reference driver>", "exec"), env)


def synthetic():
    rng = np.random.default_rng(20240607)
    user = rng.integers(0, 60, M).astype(np.int64) * 1000003 - 7       # (some negative ids)
    item = rng.integers(0, 25, M).astype(np.int64) + (1 << 41)
    target = rng.integers(0, 2, M).astype(np.int64)
    cities = np.array(["Kazan", "Moscow", "Omsk", "Perm", "Sochi", "Tver"])
    types_ = np.array(["apart", "hostel", "hotel", "villa"])
    city = cities[rng.integers(0, 5, M)].astype(object)               # "Tver" only below
    kind = types_[rng.integers(0, 4, M)].astype(object)
    price = np.round(rng.uniform(800, 30000, M), 2)
    stars = rng.integers(0, 6, M).astype(np.float64)                   # stars == 0: price / 0
    reviews = np.full(M, 3.0)                                          # the constant column
    overall = rng.integers(1, 11, M).astype(np.float64)
    loc, clean, food, serv = (rng.integers(0, 11, M).astype(np.float64) for _ in range(4))
    # NaNs in several numeric columns
    for col, k in ((price, 17), (stars, 9), (overall, 12), (loc, 20), (food, 31), (serv, 8), (reviews, 5)):
        col[rng.choice(M, k, replace=False)] = np.nan
    city[rng.choice(M, 14, replace=False)] = None
    kind[rng.choice(M, 11, replace=False)] = None
    # 0 / 0 and x / 0 in rows the filter keeps
    overall[[3, 4, 5]] = [9.0, 2.0, 10.0]
    price[3], stars[3] = 0.0, 0.0
    price[4], stars[4] = 1234.5, 0.0
    clean[5], serv[5] = 0.0, 0.0
    city[[3, 4, 5]] = "Moscow"
    kind[[3, 4, 5]] = "hotel"
    # a user, an item and a category seen only in rows that are dropped
    overall[10], user[10], item[10], city[10] = 6.0, 999999999999, 77, "Tver"   # the filter drops it
    overall[11], user[11], item[11], kind[11] = 9.0, -424242, 78, None          # the category drop
    overall[12] = np.nan                                                          # a NaN rating
    raw = np.stack([price, stars, reviews, overall, loc, clean, food, serv], axis=1)
    return user, item, target, city, kind, raw


def main():
    import pandas as pd
    ref = load_reference()
    frame_nodes, list_nodes = driver_statements()
    env = {"np": np, "pd": pd}
    run(list_nodes, env)
    cat_cols, num_cols = env["CATEGORICAL_COLS"], env["NUMERICAL_COLS"]
    raw_cols = [c for c in num_cols[:8]]
    user, item, target, city, kind, raw = synthetic()
    df = pd.DataFrame({"user_id": user, "item_id": item, "was_booked": target, cat_cols[0]: city,
                       cat_cols[1]: kind})
    for c, name in enumerate(raw_cols):
        df[name] = raw[:, c]
    env["df_full"] = df
    run(frame_nodes, env)
    df = env["df_full"].copy()
    assert list(df.columns[-3:]) == num_cols[8:], (list(df.columns), num_cols)

    # ---- what the frame must contain
    after = df
    counts = after[num_cols].notna().sum()
    assert (counts < len(after)).sum() >= 4, "NaNs in several numeric columns"
    assert (counts[counts < len(after)] % 2 == 0).any() and (counts[counts < len(after)] % 2 == 1).any(), \
        "an even and an odd non-NaN count"
    assert ((raw[:, 1] == 0) & (raw[:, 0] > 0)).any() and ((raw[:, 1] == 0) & (raw[:, 0] == 0)).any()
    assert (after[num_cols[8]] == 0).any()
    assert after[cat_cols[0]].isna().any() and after[cat_cols[1]].isna().any(), "missing categories"
    live = after.dropna(subset=cat_cols)
    assert 999999999999 not in set(live["user_id"]) and -424242 not in set(live["user_id"])
    assert 77 not in set(live["item_id"]) and 78 not in set(live["item_id"])
    assert "Tver" not in set(live[cat_cols[0]]) and "Tver" in set(city.tolist())
    assert np.isnan(raw[:, 3]).any() and ((raw[:, 3] >= 5) & (raw[:, 3] <= 7)).any()
    assert len(after) < M and len(live) < len(after)
    assert live[num_cols[2]].nunique() == 1, "a constant numeric column"

    train, val, dims, art = ref.prepare_data(df.copy(), "user_id", "item_id", "was_booked", cat_cols, num_cols)
    sc = art["scaler"]
    out = dict(
        user=user, item=item, target=target, raw=raw,
        city=np.array(["" if v is None else v for v in city.tolist()]),
        kind=np.array(["" if v is None else v for v in kind.tolist()]),
        cat_names=np.array(cat_cols), num_names=np.array(num_cols),
        filter=np.array([3.0, 4.0, 8.0]),                 # (column, lo, hi) of the driver's filter
        derived=np.array([[0, 0, 1], [0, 5, 7], [1, 3, 4]], dtype=np.int32),   # ratio, ratio, diff
        n_users=np.int64(dims[0]), n_items=np.int64(dims[1]),
        cat_dims=np.array([dims[2][c] for c in cat_cols], dtype=np.int64), n_num=np.int64(dims[3]),
        user_ids=np.array(list(art["user_id_mapping"].keys()), dtype=np.int64),
        item_ids=np.array(list(art["item_id_mapping"].keys()), dtype=np.int64),
        city_categories=np.array(list(art["cat_encoders"][cat_cols[0]].keys())),
        kind_categories=np.array(list(art["cat_encoders"][cat_cols[1]].keys())),
        scale=sc.scale_, min=sc.min_, data_min=sc.data_min_, data_max=sc.data_max_,
    )
    assert list(art["user_id_mapping"].values()) == list(range(dims[0]))
    assert list(art["cat_encoders"][cat_cols[0]].values()) == list(range(dims[2][cat_cols[0]]))
    for name, split in (("train", train), ("val", val)):
        for k, t in zip(("collab", "cat", "num", "y"), split):
            out[f"{name}_{k}"] = t.numpy()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", len(after), "rows after the filter,", len(live), "survive")


if __name__ == "__main__":
    main()
