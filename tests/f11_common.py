"""F11 (tests/golden/f11_friends, written by make_friends_golden.py running the
reference service) and what the interaction-store tests share: the fixture
loaded as F7 is, a ``dcnr.InteractionStore`` from a fixture's two tables (the
way INTEGRATION.md tells a caller of the reference service to build one), a
pandas restatement of main.py:172-194 / 336-351 on row-space arrays, and
random stores with the awkward cases planted.
"""
import os

import numpy as np
import pandas as pd

import f7_common

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f11_friends")


def load():
    """The F11 fixture as f7_common.load() reads F7 (the same layout), but for
    the weights: the state_dict is stored as plain arrays (model_state.npz)."""
    import json
    import torch
    f = f7_common.F7()
    art = json.load(open(os.path.join(DIR, "artifacts.json")))
    main_df = pd.read_csv(os.path.join(DIR, "data", "hackathon_augmented_data.csv"))
    main_df.rename(columns={"guest_id": "user_id", "hotel_id": "item_id"}, inplace=True)
    main_df["price_per_star"] = (main_df["price_rub"] / main_df["stars"]).replace(
        [np.inf, -np.inf], 0).fillna(0)
    main_df["cleanliness_vs_service"] = (main_df["rating_cleanliness"] /
                                         main_df["rating_service"]).replace([np.inf, -np.inf], 0).fillna(0)
    main_df["location_premium"] = main_df["rating_overall"] - main_df["rating_location"]
    f.main_df = main_df
    f.friends = pd.read_csv(os.path.join(DIR, "data", "friendships.csv"))
    f.user_map = {int(k): v for k, v in art["user_id_mapping"].items()}
    f.item_map = {int(k): v for k, v in art["item_id_mapping"].items()}
    f.rev = {v: k for k, v in f.item_map.items()}
    f.n_users, f.n_items, f.cat_dims, f.n_num = art["model_dims"]
    f.params = dict(art["best_params"])
    with np.load(os.path.join(DIR, "model_state.npz"), allow_pickle=False) as z:
        f.state = {k: torch.from_numpy(z[k].copy()) for k in z.files}
    f.emb = np.load(os.path.join(DIR, "item_embeddings.npy"))
    first = main_df.drop_duplicates(subset=["item_id"]).set_index("item_id")
    f.item_cat = np.zeros((f.n_items, len(art["cat_encoders"])), np.int64)
    f.item_num = np.zeros((f.n_items, f.n_num), np.float32)
    mn, sc = np.array(art["scaler_min"]), np.array(art["scaler_scale"])
    for h, r in f.item_map.items():
        row = first.loc[h]
        f.item_cat[r] = [enc.get(str(row[c]), 0) for c, enc in art["cat_encoders"].items()]
        x = row[art["numerical_cols"]].to_numpy(np.float64)
        f.item_num[r] = (x * sc + mn).astype(np.float32)   # MinMaxScaler.transform, then fp32
    f.expected = json.load(open(os.path.join(DIR, "expected.json")))
    return f


def store_of(f):
    """(InteractionStore, reviewer index of each raw user id) of a fixture:
    reviewers are every id main_df or friendships_df names, in ascending order."""
    import dcnr
    ids = np.unique(np.concatenate([f.main_df["user_id"].to_numpy(),
                                    f.friends["user_id_1"].to_numpy(),
                                    f.friends["user_id_2"].to_numpy()]))
    reviewer = {int(u): i for i, u in enumerate(ids)}
    store = dcnr.InteractionStore(
        f.main_df["user_id"].map(reviewer).to_numpy(),
        f.main_df["item_id"].map(f.item_map).to_numpy(),
        f.main_df["rating_overall"].to_numpy(),
        f.friends["user_id_1"].map(reviewer).to_numpy(),
        f.friends["user_id_2"].map(reviewer).to_numpy(),
        n_items=f.n_items, n_reviewers=len(ids))
    return store, reviewer, ids


class PandasStore:
    """main.py:172-194 / 336-351 restated with the reference's pandas
    operations on row-space columns (reviewer, item, rating; friend pairs)."""

    def __init__(self, rev, item, rating, fa, fb):
        self.df = pd.DataFrame({"user_id": rev, "item_id": item, "rating_overall": rating})
        self.fr = pd.DataFrame({"user_id_1": fa, "user_id_2": fb})

    def friends(self, u):
        fr = self.fr
        return set(fr[fr["user_id_1"] == u]["user_id_2"].tolist() +
                   fr[fr["user_id_2"] == u]["user_id_1"].tolist())

    def sources(self, u, mode):
        df = self.df
        if mode == "friends":
            src = self.friends(u)
            rv = df[df["user_id"].isin(src)] if src else pd.DataFrame()
        else:
            rv = df[df["user_id"] == u]
        if rv.empty:
            return [], []
        return (sorted(rv[rv["rating_overall"] >= 8]["item_id"].unique().tolist()),
                sorted(rv[rv["rating_overall"] <= 4]["item_id"].unique().tolist()))

    def recommended_by(self, u, ranked):
        src = self.friends(u)
        rv = self.df[self.df["user_id"].isin(src)] if src else pd.DataFrame()
        by = {}
        if not rv.empty:
            by = rv[rv["rating_overall"] >= 8].groupby("item_id")["user_id"].unique().apply(
                list).to_dict()
        return [[int(x) for x in by.get(h, [])] for h in ranked]


def random_tables(U, M, E, n_items, seed, nan=True):
    """Row-space tables with planted repeats (a reviewer reviewing a hotel
    several times), self pairs, repeated and reversed pairs, ratings of
    exactly 8 and 4, NaN ratings, reviewers without reviews or friends."""
    rng = np.random.default_rng(seed)
    rev = rng.integers(0, U - U // 10, M)             # the last tenth: no reviews
    item = rng.integers(0, n_items, M)
    rating = rng.integers(1, 11, M).astype(np.float64)
    rep = rng.choice(M, M // 8, replace=False)         # repeats of earlier (reviewer, hotel) pairs
    src = rng.integers(0, M, rep.size)
    rev[rep], item[rep] = rev[src], item[src]
    if nan:
        rating[rng.choice(M, M // 20, replace=False)] = np.nan
    fa = rng.integers(U // 20, U, E)                   # the first twentieth: no friends
    fb = rng.integers(U // 20, U, E)
    a0, b0 = fa.copy(), fb.copy()
    n1, n2, n3 = E // 30, E // 10, E // 20
    fb[:n1] = fa[:n1]                                  # self pairs
    fa[n1:n2], fb[n1:n2] = b0[n2:2 * n2 - n1], a0[n2:2 * n2 - n1]   # pairs n2.. reversed
    fa[E - n3:], fb[E - n3:] = a0[n2:n2 + n3], b0[n2:n2 + n3]       # ... and repeated
    return rev, item, rating, fa, fb
