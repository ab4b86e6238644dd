"""Generate tests/golden/transform/transform_golden.npz: the REFERENCE's
``preprocess_for_ranking`` (main.py:215-230) on rows its ``prepare_data``
(train.py:36-87) was not fitted on.

Run where the reference tree is (the build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_transform_golden.py

The fit is the one of tests/golden/prepare: the frame stored in
prepare_golden.npz goes through the reference's driver lines and its
``prepare_data`` again (make_prepare_golden.py's helpers), which gives the
``artifacts`` dict.  Then 48 extra rows, 12 for each of four users, get the
driver's derived columns and go through ``preprocess_for_ranking`` one user at
a time, as the service calls it.  The extra rows hold an unseen user, unseen
hotels, an unseen city ("Ufa"), a city seen only in rows the fit dropped
("Tver"), missing categories, NaN numerics and a division by zero.

The fixture holds data only: the extra rows' input columns and the four output
arrays.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_prepare_golden as mp  # noqa: E402
from make_serving_golden import load_main  # noqa: E402

OUT = os.path.join(HERE, "transform", "transform_golden.npz")
PER_USER = 12


def extra_rows(g):
    rng = np.random.default_rng(20240611)
    known_users = g["user_ids"]
    users = [int(known_users[0]), int(known_users[7]), 31337000000001, int(known_users[-1])]   # the third: unseen
    assert users[2] not in set(g["user"].tolist())
    M = PER_USER * len(users)
    user = np.repeat(np.array(users, dtype=np.int64), PER_USER)
    item = rng.choice(g["item_ids"], M).astype(np.int64)
    item[[2, 17, 30, 41]] = [5, (1 << 41) + 999, -12, 77]          # unseen hotels (77: only in a dropped row)
    cities = np.array(["Kazan", "Moscow", "Omsk", "Perm", "Sochi"])
    kinds = np.array(["apart", "hostel", "hotel", "villa"])
    city = cities[rng.integers(0, 5, M)].astype(object)
    kind = kinds[rng.integers(0, 4, M)].astype(object)
    city[[1, 14, 29]] = "Ufa"
    city[[6, 40]] = "Tver"
    city[[9, 33]] = None
    kind[[3, 33, 44]] = None
    kind[20] = "camping"
    price = np.round(rng.uniform(800, 30000, M), 2)
    stars = rng.integers(0, 6, M).astype(np.float64)
    reviews = rng.integers(1, 40, M).astype(np.float64)
    overall = rng.integers(1, 11, M).astype(np.float64)
    loc, clean, food, serv = (rng.integers(0, 11, M).astype(np.float64) for _ in range(4))
    for col, k in ((price, 4), (stars, 3), (overall, 3), (loc, 2), (food, 5), (serv, 3)):
        col[rng.choice(M, k, replace=False)] = np.nan
    price[10], stars[10] = 0.0, 0.0          # 0 / 0
    price[11], stars[11] = 4321.0, 0.0       # x / 0
    raw = np.stack([price, stars, reviews, overall, loc, clean, food, serv], axis=1)
    return user, item, city, kind, raw


def main():
    import pandas as pd
    g = np.load(os.path.join(HERE, "prepare", "prepare_golden.npz"), allow_pickle=False)
    ref_train = mp.load_reference()
    ref_main = load_main()
    frame_nodes, list_nodes = mp.driver_statements()
    env = {"np": np, "pd": pd}
    mp.run(list_nodes, env)
    cat_cols, num_cols = env["CATEGORICAL_COLS"], env["NUMERICAL_COLS"]
    derived_nodes = [n for n in frame_nodes if not (hasattr(n.targets[0], "id") and n.targets[0].id == "df_full")]
    assert len(derived_nodes) == 3

    def frame(user, item, city, kind, raw):
        df = pd.DataFrame({"user_id": user, "item_id": item, cat_cols[0]: city, cat_cols[1]: kind})
        for c, name in enumerate(num_cols[:8]):
            df[name] = raw[:, c]
        return df

    # ---- the fit of tests/golden/prepare, once more
    none = lambda a: np.array([None if v == "" else v for v in a.tolist()], dtype=object)
    df = frame(g["user"], g["item"], none(g["city"]), none(g["kind"]), g["raw"])
    df["was_booked"] = g["target"]
    env["df_full"] = df
    mp.run(frame_nodes, env)
    _, _, dims, art = ref_train.prepare_data(env["df_full"].copy(), "user_id", "item_id", "was_booked", cat_cols,
                                             num_cols)
    assert list(art["user_id_mapping"].keys()) == g["user_ids"].tolist()
    assert np.array_equal(art["scaler"].scale_, g["scale"])

    # ---- the extra rows through the service's preprocessing
    user, item, city, kind, raw = extra_rows(g)
    env["df_full"] = frame(user, item, city, kind, raw)
    mp.run(derived_nodes, env)
    rows = env["df_full"]
    ref_main.ml_artifacts["artifacts"] = art
    parts = []
    for u in dict.fromkeys(user.tolist()):
        items_df = rows[rows["user_id"] == u]
        parts.append([t.numpy() for t in ref_main.preprocess_for_ranking(items_df, u)])
    x_user, x_item, x_cat, x_num = (np.concatenate([p[k] for p in parts]) for k in range(4))

    # ---- what the rows must contain
    assert (x_user == dims[0] // 2).sum() == PER_USER, "one unseen user"
    seen_items = set(art["item_id_mapping"])
    assert sum(int(i) not in seen_items for i in item) == 4
    assert "Ufa" not in art["cat_encoders"][cat_cols[0]] and "Tver" not in art["cat_encoders"][cat_cols[0]]
    assert np.isnan(x_num).any() and x_num.dtype == np.float32 and x_cat.dtype == np.int64

    out = dict(user=user, item=item, raw=raw,
               city=np.array(["" if v is None else v for v in city.tolist()]),
               kind=np.array(["" if v is None else v for v in kind.tolist()]),
               x_user=x_user, x_item=x_item, x_cat=x_cat, x_num=x_num)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", len(user), "rows")


if __name__ == "__main__":
    main()
