"""InteractionStore.append on the host (no device): after any sequence of
appends the store is indistinguishable from one built from the concatenated
tables, it answers as the reference's pandas operations do, and a refused
append changes nothing."""
import numpy as np
import pytest

import store_append_common as sac
from f11_common import PandasStore

SEEDS = [0, 1, 2]
NAMES = [s[0] for s in sac.sequences(0)]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", NAMES)
def test_append_equals_rebuilt(name, seed):
    _, init, batches = next(s for s in sac.sequences(seed) if s[0] == name)
    store = sac.build(init)
    for i, b in enumerate(batches):
        sac.append(store, b)
        # ... after every append, not only the last
        sac.assert_same(store, sac.build(sac.concatenated(init, batches[:i + 1])), f"{name}[{i}]")
    assert store.n_items == sac.N_ITEMS


def test_sequences_plant_their_cases():
    """The sequences hold what their names promise (so the test above tests it)."""
    seqs = {s[0]: s for s in sac.sequences(0)}
    _, init, (b,) = seqs["existing_friends"]
    before = sac.build(init)
    assert b[3].size and (b[3] == b[4]).any()
    fr = lambda u: set(before.friends_host(int(u)).tolist())
    assert all(int(y) in fr(x) for x, y in zip(b[3], b[4]))
    _, init, (b,) = seqs["fresh_reviewer"]
    before = sac.build(init)
    x = int(b[0][0])
    assert before.n_rows[x] == 0 and before.n_friends[x] == 0
    _, init, (b,) = seqs["friend_with_positives"]
    before = sac.build(init)
    a0, b0 = int(b[3][0]), int(b[4][0])
    assert b0 not in fr(a0) and before.n_friends[a0] and before.n_friends[b0]
    assert ((b[0] == b0) & (b[2] >= 8)).sum() >= 2
    _, init, batches = seqs["mixed"]
    rating = np.concatenate([x[2] for x in batches])
    assert (rating == 8).any() and (rating == 4).any() and np.isnan(rating).any()
    assert min(x[0].size for x in batches) == 1


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", ["mixed", "grow", "friend_with_positives"])
def test_reference_semantics_after_appends(name, seed):
    _, init, batches = next(s for s in sac.sequences(seed) if s[0] == name)
    store = sac.build(init)
    for b in batches:
        sac.append(store, b)
    rev, item, rating, fa, fb, n = sac.concatenated(init, batches)
    ref = PandasStore(rev, item, rating, fa, fb)
    hotels = list(range(sac.N_ITEMS))
    assert store.n_reviewers == n
    for u in range(n):
        assert set(store.friends_host(u).tolist()) == ref.friends(u)
        for mode in ("friends", "personal"):
            pos, neg = store.sources_host(u, mode)
            want = ref.sources(u, mode)
            assert (pos.tolist(), neg.tolist()) == (want[0], want[1]), (u, mode)
        assert store.recommended_by_host(u, hotels) == ref.recommended_by(u, hotels), u


def test_empty_batch_is_a_noop():
    _, init, _ = sac.sequences(0)[-1]
    store = sac.build(init)
    before = sac.snapshot(store)
    arrays = {k: getattr(store, k) for k in sac.ARRAYS}
    store.append()
    store.append([], [], [], [], [], n_reviewers=store.n_reviewers)
    sac.assert_same(store, before)
    assert all(getattr(store, k) is a for k, a in arrays.items())


BAD = [
    ("reviews_lengths", dict(review_reviewer=[1, 2], review_item=[1], review_rating=[5.0, 5.0])),
    ("rating_length", dict(review_reviewer=[1], review_item=[1], review_rating=[])),
    ("pair_lengths", dict(friend_a=[1, 2], friend_b=[1])),
    ("reviewer_negative", dict(review_reviewer=[-1], review_item=[1], review_rating=[5.0])),
    ("reviewer_beyond_U", dict(review_reviewer=[sac.U], review_item=[1], review_rating=[5.0])),
    ("reviewer_beyond_new_U", dict(review_reviewer=[sac.U + 2], review_item=[1], review_rating=[5.0],
                                   n_reviewers=sac.U + 2)),
    ("friend_a_beyond_U", dict(friend_a=[sac.U], friend_b=[0])),
    ("friend_b_negative", dict(friend_a=[0], friend_b=[-3])),
    ("item_beyond", dict(review_reviewer=[1], review_item=[sac.N_ITEMS], review_rating=[5.0])),
    ("item_negative", dict(review_reviewer=[1], review_item=[-1], review_rating=[5.0])),
    ("U_shrinks", dict(n_reviewers=sac.U - 1)),
    ("U_shrinks_with_rows", dict(review_reviewer=[1], review_item=[1], review_rating=[5.0],
                                 n_reviewers=sac.U - 1)),
    ("too_many_reviewers", dict(n_reviewers=2 ** 31 - 1)),
    # a good review next to a bad pair: nothing of the batch may land
    ("half_good", dict(review_reviewer=[1], review_item=[1], review_rating=[9.0],
                       friend_a=[0], friend_b=[sac.U])),
]


@pytest.mark.parametrize("what,kw", BAD, ids=[b[0] for b in BAD])
def test_bad_append_raises_and_changes_nothing(what, kw):
    _, init, _ = sac.sequences(0)[-1]
    store = sac.build(init)
    before = sac.snapshot(store)
    with pytest.raises(ValueError, match="InteractionStore.append"):
        store.append(**kw)
    sac.assert_same(store, before, what)
    # ... and the store still takes a good batch
    store.append(review_reviewer=[1], review_item=[1], review_rating=[9.0])
    assert store.n_reviews == before["n_reviews"] + 1


def test_too_many_reviews_is_refused():
    """The totals stay below 2^31 - 1: checked from the counts, before any array is made."""
    _, init, _ = sac.sequences(0)[-1]
    store = sac.build(init)
    before = sac.snapshot(store)
    store.n_reviews = 2 ** 31 - 2   # (as if that many were held)
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        store.append(review_reviewer=[1], review_item=[1], review_rating=[9.0])
    store.n_reviews = before["n_reviews"]
    sac.assert_same(store, before)
