"""``dcnr.InteractionStore`` on the host: the friends, the positives and
negatives and the recommended_by lists the reference service derives from
main_df and friendships_df (main.py:172-194, 336-351).

  1  against the F11 fixture (the reference's own functions ran, recorded by
     tests/golden/make_friends_golden.py), including the planted cases
  2  against a pandas restatement of those lines on random stores with
     repeats, self / repeated / reversed pairs and NaN ratings, and on F7
  3  constructor rejections; the host counts and the per-request bounds
  4  the C ABI: the new symbols in include/dcnr.h and the binding
"""
import os
import re

import numpy as np
import pytest

import f11_common
import f7_common
from conftest import ROOT


@pytest.fixture(scope="module")
def f11():
    f = f11_common.load()
    f.store, f.reviewer, f.reviewer_ids = f11_common.store_of(f)
    return f


def test_fixture_holds_the_planted_cases(f11):
    reqs = f11.expected["recommendations"]
    main, fr = f11.main_df, f11.friends
    assert os.path.getsize(os.path.join(f11_common.DIR, "data", "hackathon_augmented_data.csv")) < 100e3
    dup = main[main["rating_overall"] >= 8].groupby(["user_id", "item_id"]).size()
    assert (dup > 1).any()                                            # a hotel reviewed twice with >= 8
    both = main.groupby(["user_id", "item_id"])["rating_overall"].agg(["min", "max"])
    assert ((both["min"] <= 4) & (both["max"] >= 8)).any()            # positive and negative
    assert (fr["user_id_1"] == fr["user_id_2"]).any()                 # (u, u)
    assert fr.duplicated().any()                                      # a repeated pair
    rev_pairs = set(zip(fr["user_id_2"], fr["user_id_1"])) & set(zip(fr["user_id_1"], fr["user_id_2"]))
    assert any(a != b for a, b in rev_pairs)                          # a reversed pair
    assert (main["rating_overall"] == 8).any() and (main["rating_overall"] == 4).any()
    # the repeated-review order case: 112 before 111 although 111 < 112
    q = reqs[0]
    assert [112, 111] in q["recommended_by"]
    assert 110 in q["friends"]                                        # the self pair
    assert any(q["friends"] and not q["positives"] and not q["negatives"] and
               q["type"] == "friends" for q in reqs)                  # friends without reviews
    assert any(not q["friends"] and q["user_id"] in f11.reviewer for q in reqs)
    assert any(q["user_id"] not in f11.reviewer for q in reqs)        # unknown user
    assert {q["type"] for q in reqs} == {"friends", "personal"}
    assert set(reqs[0]["positives"]) & set(reqs[0]["negatives"])      # a hotel in both sets


def test_host_answers_equal_the_reference_service(f11):
    st, rows_of = f11.store, f11.item_map
    n_by = 0
    for q in f11.expected["recommendations"]:
        u = f11.reviewer.get(q["user_id"], -1)
        assert [int(f11.reviewer_ids[x]) for x in st.friends_host(u)] == q["friends"], q
        pos, neg = st.sources_host(u, q["type"])
        assert pos.tolist() == sorted(rows_of[h] for h in q["positives"]), q
        assert neg.tolist() == sorted(rows_of[h] for h in q["negatives"]), q
        assert np.all(np.diff(pos) > 0) and np.all(np.diff(neg) > 0)
        by = st.recommended_by_host(u, [rows_of[h] for h in q["ranked_hotels"]])
        assert [[int(f11.reviewer_ids[x]) for x in lst] for lst in by] == q["recommended_by"], q
        n_by += sum(len(b) for b in by)
    assert n_by >= 10


def _check_against_pandas(st, ref, U, n_items, users, rng):
    for u in users:
        assert set(st.friends_host(u).tolist()) == ref.friends(u), u
        assert np.all(np.diff(st.friends_host(u)) > 0)
        for mode in ("friends", "personal"):
            pos, neg = st.sources_host(u, mode)
            want_pos, want_neg = ref.sources(u, mode)
            assert pos.tolist() == want_pos and neg.tolist() == want_neg, (u, mode)
        # a "ranked list": some positives of the friends, some other hotels
        pos, _ = st.sources_host(u, "friends")
        ranked = rng.permutation(np.concatenate([pos, rng.integers(0, n_items, 5)])).tolist()
        assert st.recommended_by_host(u, ranked) == ref.recommended_by(u, ranked), u


@pytest.mark.parametrize("seed", [0, 1])
def test_host_answers_equal_pandas_on_random_stores(seed):
    import dcnr
    U, M, E, n_items = 300, 4000, 600, 500
    rev, item, rating, fa, fb = f11_common.random_tables(U, M, E, n_items, seed)
    assert np.isnan(rating).any() and (fa == fb).any()
    st = dcnr.InteractionStore(rev, item, rating, fa, fb, n_items=n_items, n_reviewers=U)
    ref = f11_common.PandasStore(rev, item, rating, fa, fb)
    rng = np.random.default_rng(seed + 10)
    users = np.r_[rng.choice(U, 40, replace=False), fa[:5], 0, U - 1].tolist()
    _check_against_pandas(st, ref, U, n_items, users, rng)
    assert st.sources_host(-1, "friends")[0].size == 0 and st.friends_host(-1).size == 0
    assert st.recommended_by_host(-1, [1, 2]) == [[], []]
    # the counts the batched path sizes its segments by
    for u in users:
        pos, neg = st.sources_host(u, "personal")
        assert (st.n_pos[u], st.n_neg[u]) == (pos.size, neg.size)
        assert st.n_rows[u] == (rev == u).sum() and st.n_friends[u] == len(ref.friends(u))
    rv = np.array(users + [-1], np.int64)
    for mode in (0, 1):
        md = np.full(rv.size, mode, np.int32)
        n_src, staged, pos_b, neg_b, n_fr, fr_rows, by_b = st.bounds(rv, md)
        for j, u in enumerate(rv):
            pos, neg = st.sources_host(u, mode)
            who = st.friends_host(u) if mode == 0 else np.array([u] if u >= 0 else [], np.int64)
            assert n_src[j] == who.size and staged[j] == sum((rev == w).sum() for w in who)
            assert pos_b[j] >= pos.size and (pos_b[j] > 0) == (pos.size > 0)
            assert neg_b[j] >= neg.size and (neg_b[j] > 0) == (neg.size > 0)
            fr = st.friends_host(u)
            assert n_fr[j] == fr.size and fr_rows[j] == sum((rev == w).sum() for w in fr)
            assert by_b[j] >= sum(len(b) for b in st.recommended_by_host(
                u, st.sources_host(u, 0)[0]))


def test_host_answers_equal_pandas_on_f7():
    f = f7_common.load()
    st, reviewer, ids = f11_common.store_of(f)
    rev = f.main_df["user_id"].map(reviewer).to_numpy()
    item = f.main_df["item_id"].map(f.item_map).to_numpy()
    ref = f11_common.PandasStore(rev, item, f.main_df["rating_overall"].to_numpy(),
                                 f.friends["user_id_1"].map(reviewer).to_numpy(),
                                 f.friends["user_id_2"].map(reviewer).to_numpy())
    _check_against_pandas(st, ref, len(ids), f.n_items, list(range(len(ids))),
                          np.random.default_rng(3))
    # ... and F7's own restatement of the caller's steps
    for q in f.expected["recommendations"]:
        want = f7_common.request_rows(f, q)
        pos, neg = st.sources_host(reviewer.get(q["user_id"], -1), q["type"])
        assert pos.tolist() == sorted(want["pos"]) and neg.tolist() == want["excluded"], q


def test_constructor_rejections():
    import dcnr
    ok = dict(review_reviewer=[0, 1], review_item=[3, 4], review_rating=[9, 2], friend_a=[0],
              friend_b=[1], n_items=5)
    dcnr.InteractionStore(**ok)
    for bad in (dict(review_item=[3, 5]), dict(review_item=[-1, 4]), dict(review_reviewer=[0, -1]),
                dict(review_reviewer=[0, 2], n_reviewers=2), dict(friend_a=[7], n_reviewers=3),
                dict(review_rating=[9]), dict(review_item=[3]), dict(friend_b=[1, 0]),
                dict(n_items=0)):
        with pytest.raises(ValueError):
            dcnr.InteractionStore(**{**ok, **bad})
    empty = dcnr.InteractionStore([], [], [], [], [], n_items=5, n_reviewers=3)
    assert empty.friends_host(1).size == 0 and empty.sources_host(1, "personal")[0].size == 0
    with pytest.raises(ValueError):
        empty.sources_host(1, "friendz")


def test_new_symbols_are_declared_and_bound():
    from dcnr import _lib
    txt = open(os.path.join(ROOT, "include", "dcnr.h")).read()
    declared = set(re.findall(r"\b(dcnr_[a-z0-9_]+)\s*\(", txt))
    for s in ("dcnr_requests_sources", "dcnr_requests_recommended_by"):
        assert s in declared and s in _lib.exported_symbols()
        assert hasattr(_lib.load(), s)
    assert "dcnr_interactions" in txt and _lib.load().dcnr_abi_version() == 4
