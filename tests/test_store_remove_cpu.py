"""InteractionStore.remove and set_rating on the host (no device): after every
step of any sequence the store is indistinguishable from one built from the
tables without the removed rows / with the rating column edited (``review_row``
mapped through the surviving rows' numbers), it answers as the reference's
pandas operations do on those tables, and a refused call changes nothing."""
import numpy as np
import pytest

import store_remove_common as src
from f11_common import PandasStore

SEEDS = [0, 1]
NAMES = [s[0] for s in src.sequences(0)]
U, M, E = src.U, src.M, src.E


def start(name, seed=0):
    _, init, steps = next(s for s in src.sequences(seed) if s[0] == name)
    return src.Tables(*init), src.build(init), steps


def advance(t, store, step):
    t.apply(step)
    src.apply(store, step)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", NAMES)
def test_steps_equal_rebuilt(name, seed):
    t, store, steps = start(name, seed)
    for i, s in enumerate(steps):
        advance(t, store, s)
        live, rows = t.live()
        src.assert_same_mapped(store, src.build(live), rows, f"{name}[{i}]")
        # the row numbers: stable, never given twice
        assert store.next_review_row == t.rev.size
        assert store.n_reviews == rows.size == store.review_row.size
        np.testing.assert_array_equal(np.sort(store.review_row), rows)
    assert store.n_items == src.N_ITEMS and store.n_reviewers == U


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", NAMES)
def test_reference_semantics_after_each_step(name, seed):
    t, store, steps = start(name, seed)
    hotels = list(range(src.N_ITEMS))
    for i, s in enumerate(steps):
        advance(t, store, s)
        ref = PandasStore(*t.live()[0][:5])
        for u in range(U):
            assert set(store.friends_host(u).tolist()) == ref.friends(u), (i, u)
            for mode in ("friends", "personal"):
                pos, neg = store.sources_host(u, mode)
                want = ref.sources(u, mode)
                assert (pos.tolist(), neg.tolist()) == (want[0], want[1]), (i, u, mode)
            assert store.recommended_by_host(u, hotels) == ref.recommended_by(u, hotels), (i, u)


# ------------------------------------------------------------ the planted cases
def _personal(store, r):
    pos, neg = store.sources_host(r, "personal")
    return set(pos.tolist()), set(neg.tolist())


def test_plants_one_of_several_positives():
    t, store, steps = start("one_of_several_positives")
    row = int(steps[0][1]["review_row"][0])
    r, h = int(t.rev[row]), int(t.item[row])
    same = t.alive & (t.rev == r) & (t.item == h) & (t.rating >= 8)
    assert same.sum() >= 2 and steps[0][1]["review_row"].size == 1
    assert sum(len(p) >= 2 for p, _ in src.by_pair(t).values()) >= 16
    n_pos, n_rows = store.n_pos[r], store.n_rows[r]
    advance(t, store, steps[0])
    assert (store.n_pos[r], store.n_rows[r]) == (n_pos, n_rows - 1)
    advance(t, store, steps[1])
    assert store.n_pos[r] == n_pos - 1 and h not in _personal(store, r)[0]


def test_plants_the_only_positive():
    t, store, steps = start("only_positive")
    row = int(steps[0][1]["review_row"][0])
    r, h = int(t.rev[row]), int(t.item[row])
    assert ((t.rev == r) & (t.item == h) & (t.rating >= 8)).sum() == 1
    n_pos = store.n_pos[r]
    assert h in _personal(store, r)[0]
    advance(t, store, steps[0])
    assert store.n_pos[r] == n_pos - 1 and h not in _personal(store, r)[0]


def test_plants_a_pair_both_positive_and_negative():
    t, store, steps = start("positive_and_negative")
    row = int(steps[0][1]["review_row"][0])
    r, h = int(t.rev[row]), int(t.item[row])
    assert h in _personal(store, r)[0] and h in _personal(store, r)[1]
    advance(t, store, steps[0])
    assert h not in _personal(store, r)[0] and h in _personal(store, r)[1]
    advance(t, store, steps[1])
    assert h not in _personal(store, r)[1]


def test_plants_a_reviewers_last_review():
    t, store, steps = start("last_review")
    r = int(steps[1][1]["review_reviewer"][0])
    assert store.n_rows[r] >= 2 and store.n_friends[r] > 0
    advance(t, store, steps[0])
    assert store.n_rows[r] == 1
    advance(t, store, steps[1])
    assert (store.n_rows[r], store.n_pos[r], store.n_neg[r]) == (0, 0, 0)
    assert store.review_offsets[r] == store.review_offsets[r + 1]


def test_plants_the_first_and_last_reviewer_and_row():
    t, store, steps = start("ends")
    (_, kw), = steps
    last = U - U // 10 - 1
    assert {0, last} <= set(kw["review_reviewer"].tolist())
    assert {0, M - 1} <= set(kw["review_row"].tolist())
    assert store.n_rows[0] > 0 and store.n_rows[last] > 0 and store.n_rows[last + 1:].sum() == 0
    assert store.n_friends[U - 1] > 0 and set(kw["friend_a"].tolist()) == {U - 1}
    advance(t, store, steps[0])
    assert store.n_rows[0] == 0 and store.n_friends[U - 1] == 0
    assert store.review_row.min() > 0 and store.review_row.max() < M - 1


def test_plants_the_pairs():
    t, store, steps = start("pairs")
    rows = lambda a, b: int(((t.fa == a) & (t.fb == b)).sum())
    # both directions in the table; the batch repeats the pair (and a review)
    kw = steps[0][1]
    a, b = int(kw["friend_a"][0]), int(kw["friend_b"][0])
    assert a != b and rows(a, b) >= 1 and rows(b, a) >= 1
    assert kw["friend_a"].size == 3 and kw["review_row"].size == 2
    assert kw["review_row"][0] == kw["review_row"][1]
    n = store.n_reviews
    advance(t, store, steps[0])
    assert store.n_reviews == n - 1
    assert b not in store.friends_host(a) and a not in store.friends_host(b)
    assert rows(a, b) == rows(b, a) == 0
    # repeated rows of one pair, named the other way round
    kw = steps[1][1]
    a, b = int(kw["friend_a"][0]), int(kw["friend_b"][0])
    assert a != b and rows(b, a) >= 2
    assert sum(rows(x, y) >= 2 for x, y in set(zip(t.fa.tolist(), t.fb.tolist()))) > 10
    advance(t, store, steps[1])
    assert b not in store.friends_host(a) and a not in store.friends_host(b)
    # a self pair next to a pair that does not exist
    kw = steps[2][1]
    u, (x, y) = int(kw["friend_a"][0]), (int(kw["friend_a"][1]), int(kw["friend_b"][1]))
    assert kw["friend_b"][0] == u and u in store.friends_host(u)
    assert y not in store.friends_host(x) and x not in store.friends_host(y)
    n = store.friend_rows.size
    advance(t, store, steps[2])
    assert u not in store.friends_host(u) and store.friend_rows.size == n - 1
    # the pair that does not exist alone: nothing changes, not even the arrays
    before = src.snapshot(store)
    arrays = {k: getattr(store, k) for k in src.ARRAYS}
    advance(t, store, steps[3])
    src.assert_same_mapped(store, before, np.arange(store.next_review_row))
    assert all(getattr(store, k) is v for k, v in arrays.items())


def test_plants_unfriending_with_that_friends_reviews():
    t, store, steps = start("unfriend_with_reviews")
    (_, kw), = steps
    a, b = int(kw["friend_a"][0]), int(kw["friend_b"][0])
    assert b in store.friends_host(a) and store.n_pos[b] >= 1 and store.n_friends[a] >= 2
    assert set(kw["review_reviewer"].tolist()) == {b} and kw["review_row"].size == store.n_rows[b]
    want = store.friends_pos[a] - store.n_pos[b]   # (a's other friends and a itself: as they were)
    advance(t, store, steps[0])
    assert store.n_rows[b] == 0 and b not in store.friends_host(a)
    assert store.friends_pos[a] == want


def test_plants_ratings_across_both_thresholds():
    t, store, steps = start("ratings")
    kw = steps[0][1]
    moves = list(zip(t.rating[kw["review_row"]].tolist(), kw["review_rating"].tolist()))
    same = lambda x, y: x == y or (x != x and y != y)
    for want in ((8, 7), (7, 8), (4, 5), (5, 4), (np.nan, 9), (9, np.nan), (9, 3)):
        assert any(same(m[0], want[0]) and same(m[1], want[1]) for m in moves), want
    advance(t, store, steps[0])
    # 10 -> 9.5 leaves every class: nothing changes, not even the arrays
    held = store.review_class
    advance(t, store, steps[1])
    assert store.review_class is held
    # a review given twice in one batch: the last rating counts
    kw = steps[2][1]
    assert kw["review_row"][0] == kw["review_row"][-1] and kw["review_rating"][-1] == 2.0
    advance(t, store, steps[2])
    at = np.flatnonzero(store.review_row == kw["review_row"][0])[0]
    assert store.review_class[at] == 2
    advance(t, store, steps[3])
    src.assert_same_mapped(store, start("ratings")[1], np.arange(M))


def test_plants_appending_after_removing():
    t, store, steps = start("append_after_remove")
    advance(t, store, steps[0])
    gone = set(steps[0][1]["review_row"].tolist())
    assert store.next_review_row == M and store.n_reviews == M - len(gone)
    advance(t, store, steps[1])
    assert store.next_review_row == M + 3 and store.n_reviews == M - len(gone) + 3
    assert np.unique(store.review_row).size == store.n_reviews
    assert {M, M + 1, M + 2} <= set(store.review_row.tolist())
    assert not gone & set(store.review_row.tolist())
    advance(t, store, steps[2])      # an appended row goes again
    advance(t, store, steps[3])
    assert store.next_review_row == M + 4 and M + 1 not in store.review_row
    assert store.review_row.max() == M + 3


def test_plants_removing_everything():
    t, store, steps = start("everything")
    advance(t, store, steps[0])
    z = np.zeros(0, np.int64)
    src.assert_same_mapped(store, src.build((z, z, z.astype(np.float64), z, z, U)), z)
    assert store.n_reviews == 0 and store.friend_rows.size == 0 and store.n_reviewers == U
    assert store.next_review_row == M
    for k in ("n_rows", "n_pos", "n_neg", "n_friends", "friends_rows", "friends_pos", "friends_neg"):
        assert not getattr(store, k).any(), k


def test_plants_reviews_and_pairs_in_one_call():
    t, store, steps = start("mixed")
    removes = [kw for op, kw in steps if op == "remove"]
    assert len(removes) == 3 and min(kw["review_row"].size for kw in removes) == 1
    assert all(kw["review_row"].size and kw["friend_a"].size for kw in removes)
    ratings = np.concatenate([kw["review_rating"] for op, kw in steps if op == "set_rating"])
    assert (ratings == 8).any() and (ratings == 4).any() and np.isnan(ratings).any()


# ------------------------------------------------------------------- refusals
def test_empty_batch_is_a_noop():
    t, store, _ = start("mixed")
    before = src.snapshot(store)
    arrays = {k: getattr(store, k) for k in src.ARRAYS}
    store.remove()
    store.remove([], [], [], [])
    store.set_rating([], [], [])
    src.assert_same_mapped(store, before, np.arange(M))
    assert all(getattr(store, k) is a for k, a in arrays.items())
    assert store.last_remove is None


def _held(store):
    """A (reviewer, row) the store holds and a row that reviewer does not have."""
    r = int(np.argmax(store.n_rows > 0))
    row = int(store.review_row[store.review_offsets[r]])
    other = int(store.review_row[store.review_offsets[r + 1]])
    return r, row, other


BAD_REMOVE = [
    ("unknown_row", lambda r, row, other: dict(review_reviewer=[r], review_row=[other])),
    ("row_beyond", lambda r, row, other: dict(review_reviewer=[r], review_row=[M])),
    ("row_negative", lambda r, row, other: dict(review_reviewer=[r], review_row=[-1])),
    ("review_lengths", lambda r, row, other: dict(review_reviewer=[r, r], review_row=[row])),
    ("pair_lengths", lambda r, row, other: dict(friend_a=[1, 2], friend_b=[1])),
    ("reviewer_negative", lambda r, row, other: dict(review_reviewer=[-1], review_row=[row])),
    ("reviewer_beyond_U", lambda r, row, other: dict(review_reviewer=[U], review_row=[row])),
    ("friend_a_beyond_U", lambda r, row, other: dict(friend_a=[U], friend_b=[0])),
    ("friend_b_negative", lambda r, row, other: dict(friend_a=[0], friend_b=[-3])),
    # a good review and a good pair next to an unknown one: nothing of the batch may go
    ("half_good", lambda r, row, other: dict(review_reviewer=[r, r], review_row=[row, other],
                                             friend_a=[10], friend_b=[11])),
]


@pytest.mark.parametrize("what,make", BAD_REMOVE, ids=[b[0] for b in BAD_REMOVE])
def test_bad_remove_raises_and_changes_nothing(what, make):
    t, store, _ = start("mixed")
    before = src.snapshot(store)
    with pytest.raises(ValueError, match="InteractionStore.remove"):
        store.remove(**make(*_held(store)))
    src.assert_same_mapped(store, before, np.arange(M), what)
    assert store.next_review_row == M
    # ... and the store still takes a good batch; the same row twice is then unknown
    r, row, _ = _held(store)
    store.remove([r], [row])
    assert store.n_reviews == M - 1
    with pytest.raises(ValueError, match="InteractionStore.remove"):
        store.remove([r], [row])


BAD_RATING = [
    ("unknown_row", lambda r, row, other: dict(review_reviewer=[r], review_row=[other],
                                               review_rating=[9.0])),
    ("rating_length", lambda r, row, other: dict(review_reviewer=[r], review_row=[row],
                                                 review_rating=[])),
    ("row_length", lambda r, row, other: dict(review_reviewer=[r], review_row=[row, row],
                                              review_rating=[1.0])),
    ("reviewer_beyond_U", lambda r, row, other: dict(review_reviewer=[U], review_row=[row],
                                                     review_rating=[1.0])),
    ("reviewer_negative", lambda r, row, other: dict(review_reviewer=[-2], review_row=[row],
                                                     review_rating=[1.0])),
    ("half_good", lambda r, row, other: dict(review_reviewer=[r, r], review_row=[row, other],
                                             review_rating=[1.0, 1.0])),
]


@pytest.mark.parametrize("what,make", BAD_RATING, ids=[b[0] for b in BAD_RATING])
def test_bad_set_rating_raises_and_changes_nothing(what, make):
    t, store, _ = start("mixed")
    before = src.snapshot(store)
    with pytest.raises(ValueError, match="InteractionStore.set_rating"):
        store.set_rating(**make(*_held(store)))
    src.assert_same_mapped(store, before, np.arange(M), what)


def test_append_counts_the_rows_ever_seen_against_the_int32_limit():
    """review_row is an int32 payload: next_review_row, not only n_reviews, stays below 2^31 - 1."""
    t, store, _ = start("mixed")
    r, row, _ = _held(store)
    store.remove([r], [row])
    before = src.snapshot(store)
    store.next_review_row = 2 ** 31 - 2   # (as if that many rows had been seen)
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        store.append(review_reviewer=[1], review_item=[1], review_rating=[9.0])
    store.next_review_row = M
    src.assert_same_mapped(store, before, np.arange(M))
