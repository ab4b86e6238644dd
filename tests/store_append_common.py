"""What the InteractionStore.append tests share: the attributes a store is
compared by, and the append sequences (a prefix of f11_common.random_tables,
then batches) with the awkward cases planted.  A sequence is (name, init,
batches): init = (rev, item, rating, fa, fb, U) builds the store, each batch =
(rev, item, rating, fa, fb, n_reviewers or None) is one append.
"""
import numpy as np

from f11_common import random_tables

U, M, E, N_ITEMS = 60, 900, 300, 40

ARRAYS = ["review_offsets", "review_item", "review_class", "review_row", "friend_offsets",
          "friend_rows", "n_rows", "n_pos", "n_neg", "n_friends", "friends_rows", "friends_pos",
          "friends_neg"]
COUNTS = ["n_reviewers", "n_reviews"]
TENSORS = ["friend_offsets", "friend_rows", "review_offsets", "review_items", "review_rows"]

_I = np.zeros(0, np.int64)
_F = np.zeros(0, np.float64)


def snapshot(store):
    s = {k: getattr(store, k).copy() for k in ARRAYS}
    s.update({k: getattr(store, k) for k in COUNTS})
    return s


def assert_same(got, want, what=""):
    """Every host array (values, dtype, shape) and count of two stores / snapshots."""
    g = got if isinstance(got, dict) else snapshot(got)
    w = want if isinstance(want, dict) else snapshot(want)
    for k in COUNTS:
        assert g[k] == w[k], f"{what}: {k} {g[k]} != {w[k]}"
    for k in ARRAYS:
        assert g[k].dtype == w[k].dtype, f"{what}: {k} dtype {g[k].dtype} != {w[k].dtype}"
        assert g[k].shape == w[k].shape, f"{what}: {k} shape {g[k].shape} != {w[k].shape}"
        np.testing.assert_array_equal(g[k], w[k], err_msg=f"{what}: {k}")


def build(init):
    import dcnr
    rev, item, rating, fa, fb, n = init
    return dcnr.InteractionStore(rev, item, rating, fa, fb, n_items=N_ITEMS, n_reviewers=n)


def append(store, batch):
    rev, item, rating, fa, fb, n = batch
    store.append(review_reviewer=rev, review_item=item, review_rating=rating, friend_a=fa,
                 friend_b=fb, n_reviewers=n)


def concatenated(init, batches):
    """The init of the store the appends must be indistinguishable from."""
    parts = [init] + list(batches)
    n = init[5]
    for b in batches:
        n = n if b[5] is None else b[5]
    return tuple(np.concatenate([np.asarray(p[i]) for p in parts]) for i in range(5)) + (n,)


def _reviews(rev, item, rating, n=None):
    return (np.asarray(rev, np.int64), np.asarray(item, np.int64), np.asarray(rating, np.float64),
            _I, _I, n)


def _pairs(fa, fb, n=None):
    return (_I, _I, _F, np.asarray(fa, np.int64), np.asarray(fb, np.int64), n)


def _both(rev, item, rating, fa, fb, n=None):
    return _reviews(rev, item, rating)[:3] + _pairs(fa, fb)[3:5] + (n,)


def sequences(seed):
    rev, item, rating, fa, fb = random_tables(U, M, E, N_ITEMS, seed)
    full = (rev, item, rating, fa, fb, U)
    r = lambda a, b: _reviews(rev[a:b], item[a:b], rating[a:b])
    p = lambda a, b: _pairs(fa[a:b], fb[a:b])
    friends = {(int(a), int(b)) for a, b in zip(fa, fb)} | {(int(b), int(a)) for a, b in zip(fa, fb)}
    # two reviewers with friends and reviews who are not friends yet
    a0, b0 = next((a, b) for a in range(10, 40) for b in range(a + 1, 50) if (a, b) not in friends)
    seqs = []
    seqs.append(("all_at_once", (_I, _I, _F, _I, _I, U), [full[:5] + (None,)]))
    seqs.append(("reviews_only", (rev[:500], item[:500], rating[:500], fa, fb, U),
                 [r(500, 700), r(700, M)]))
    seqs.append(("friends_only", (rev, item, rating, fa[:150], fb[:150], U),
                 [p(150, 220), p(220, E)]))
    # pairs that all exist: as they are, reversed, and the self pairs (the table's first E // 30)
    seqs.append(("existing_friends", full,
                 [_pairs(np.concatenate([fa[:50], fb[50:100], fa[:E // 30]]),
                         np.concatenate([fb[:50], fa[50:100], fb[:E // 30]]))]))
    seqs.append(("one_review", (rev[:M - 1], item[:M - 1], rating[:M - 1], fa, fb, U), [r(M - 1, M)]))
    seqs.append(("ends", full,
                 [_reviews([U - 1, 0, U - 1, 0], [3, 5, 3, 39], [9.0, 8.0, 2.0, 4.0]),
                  _both([0], [0], [10.0], [0, U - 1], [U - 1, U - 1])]))
    # reviewer U - 3 has no review (random_tables) and, here, no friend before the batch
    x = U - 3
    keep = (fa != x) & (fb != x)
    seqs.append(("fresh_reviewer", (rev, item, rating, fa[keep], fb[keep], U),
                 [_both([x, x, x], [7, 7, 11], [8.0, 9.0, 1.0], [x, 20], [5, x])]))
    seqs.append(("grow", full,
                 [_both([U, U + 6, 3, U + 6, U + 2], [1, 2, 3, 2, 39], [9.0, 8.0, 4.0, 10.0, np.nan],
                        [U + 1, U + 6, U + 2, 3], [3, U + 6, U + 3, U + 1], n=U + 7),
                  _both([U + 6, 0], [5, 5], [3.0, 8.0], [U + 5], [0])]))
    # a new friendship (a0, b0) together with new positive reviews by b0 (and by a0)
    seqs.append(("friend_with_positives", full,
                 [_both([b0, b0, a0, b0, b0], [0, 39, 17, 0, 21], [9.0, 8.0, 10.0, 4.0, np.nan],
                        [a0], [b0])]))
    m0, e0 = M * 6 // 10, E // 2
    cut_m = [m0, m0 + 100, m0 + 101, M]
    cut_e = [e0, e0 + 90, e0 + 90, E]
    seqs.append(("mixed", (rev[:m0], item[:m0], rating[:m0], fa[:e0], fb[:e0], U),
                 [r(cut_m[i], cut_m[i + 1])[:3] + p(cut_e[i], cut_e[i + 1])[3:5] + (None,)
                  for i in range(3)]))
    return seqs
