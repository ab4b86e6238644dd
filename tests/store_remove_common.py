"""What the InteractionStore.remove / set_rating tests share: a model of the
two tables a store follows (every main_df row ever seen with a live mask, so
row numbers stay; the friendship rows), the comparison with a store rebuilt
from the live tables (``review_row`` mapped through the surviving rows'
numbers), and the step sequences over f11_common.random_tables with the awkward
cases planted.  A sequence is (name, init, steps): init = (rev, item, rating,
fa, fb, U) builds the store, each step = (method name, keyword arguments).
"""
import numpy as np

from f11_common import random_tables
from store_append_common import ARRAYS, COUNTS, N_ITEMS, TENSORS, U, M, E, build, snapshot  # noqa: F401

_I = np.zeros(0, np.int64)


class Tables:
    """main_df (row numbers stable: removed rows stay, dead) and friendships_df."""

    def __init__(self, rev, item, rating, fa, fb, n):
        self.rev, self.item = np.array(rev, np.int64), np.array(item, np.int64)
        self.rating = np.array(rating, np.float64)
        self.alive = np.ones(self.rev.size, bool)
        self.fa, self.fb, self.n = np.array(fa, np.int64), np.array(fb, np.int64), n

    def apply(self, step):
        op, kw = step
        g = lambda k, dt=np.int64: np.asarray(kw.get(k, ()), dt).reshape(-1)
        if op == "append":
            self.rev = np.r_[self.rev, g("review_reviewer")]
            self.item = np.r_[self.item, g("review_item")]
            self.rating = np.r_[self.rating, g("review_rating", np.float64)]
            self.alive = np.r_[self.alive, np.ones(self.rev.size - self.alive.size, bool)]
            self.fa, self.fb = np.r_[self.fa, g("friend_a")], np.r_[self.fb, g("friend_b")]
        elif op == "remove":       # df.drop(rows); every row {a, b} of friendships_df
            assert (self.rev[g("review_row")] == g("review_reviewer")).all()
            assert self.alive[g("review_row")].all()
            self.alive[g("review_row")] = False
            for a, b in zip(g("friend_a"), g("friend_b")):
                keep = ~(((self.fa == a) & (self.fb == b)) | ((self.fa == b) & (self.fb == a)))
                self.fa, self.fb = self.fa[keep], self.fb[keep]
        else:                      # df.loc[row, 'rating_overall'] = x, in argument order
            assert op == "set_rating"
            assert (self.rev[g("review_row")] == g("review_reviewer")).all()
            assert self.alive[g("review_row")].all()
            for r, x in zip(g("review_row"), g("review_rating", np.float64)):
                self.rating[r] = x

    def live(self):
        """(the init of the store the steps must be indistinguishable from, the
        original row number of each of its main_df rows)"""
        rows = np.flatnonzero(self.alive)
        return (self.rev[rows], self.item[rows], self.rating[rows], self.fa, self.fb, self.n), rows

    def rows_of(self, r):
        return np.flatnonzero(self.alive & (self.rev == r))

    def friends_of(self, u):
        return set(self.fb[self.fa == u].tolist()) | set(self.fa[self.fb == u].tolist())


def apply(store, step):
    getattr(store, step[0])(**step[1])


def assert_same_mapped(store, rebuilt, rows, what=""):
    """Every host array and count of ``store`` equals ``rebuilt``'s, the
    rebuilt store's review_row mapped through the surviving rows ``rows``."""
    g, w = snapshot(store), dict(rebuilt) if isinstance(rebuilt, dict) else snapshot(rebuilt)
    w["review_row"] = rows[w["review_row"]].astype(np.int64)
    for k in COUNTS:
        assert g[k] == w[k], f"{what}: {k} {g[k]} != {w[k]}"
    for k in ARRAYS:
        assert g[k].dtype == w[k].dtype, f"{what}: {k} dtype {g[k].dtype} != {w[k].dtype}"
        assert g[k].shape == w[k].shape, f"{what}: {k} shape {g[k].shape} != {w[k].shape}"
        np.testing.assert_array_equal(g[k], w[k], err_msg=f"{what}: {k}")


def rm(t, rows=(), fa=(), fb=()):
    rows = np.asarray(rows, np.int64).reshape(-1)
    return ("remove", dict(review_reviewer=t.rev[rows], review_row=rows,
                           friend_a=np.asarray(fa, np.int64), friend_b=np.asarray(fb, np.int64)))


def rate(t, rows, ratings):
    rows = np.asarray(rows, np.int64).reshape(-1)
    return ("set_rating", dict(review_reviewer=t.rev[rows], review_row=rows,
                               review_rating=np.asarray(ratings, np.float64)))


def by_pair(t):
    """(reviewer, hotel) -> (rows rated >= 8, rows rated <= 4) of the live table."""
    out = {}
    for r in np.flatnonzero(t.alive):
        p, n = out.setdefault((int(t.rev[r]), int(t.item[r])), ([], []))
        if t.rating[r] >= 8:
            p.append(int(r))
        if t.rating[r] <= 4:
            n.append(int(r))
    return out


def sequences(seed):
    rev, item, rating, fa, fb = random_tables(U, M, E, N_ITEMS, seed)
    init = (rev, item, rating, fa, fb, U)
    t = Tables(*init)      # (the table as built: the steps below name its rows)
    pairs = by_pair(t)
    n1, n2 = E // 30, E // 10
    seqs = []
    # one of several >= 8 reviews of a (reviewer, hotel): n_pos stays; then the others: it drops
    sev = next(p for p, _ in pairs.values() if len(p) >= 2)
    seqs.append(("one_of_several_positives", [rm(t, sev[:1]), rm(t, sev[1:])]))
    only = next(p for p, n in pairs.values() if len(p) == 1 and not n)
    seqs.append(("only_positive", [rm(t, only)]))
    both = next((p, n) for p, n in pairs.values() if p and n)
    seqs.append(("positive_and_negative", [rm(t, both[0]), rm(t, both[1])]))
    # a reviewer (with friends) down to one review, then that one
    few = min(range(U // 20, U - U // 10), key=lambda r: (t.rows_of(r).size < 2, t.rows_of(r).size))
    seqs.append(("last_review", [rm(t, t.rows_of(few)[:-1]), rm(t, t.rows_of(few)[-1:])]))
    # the first reviewer (all it has), the last with reviews, the last (its
    # friends); the first and the last main_df row
    last = U - U // 10 - 1
    ends = np.unique(np.r_[0, M - 1, t.rows_of(0), t.rows_of(last)[-1:]])
    fr = sorted(t.friends_of(U - 1))
    seqs.append(("ends", [rm(t, ends, [U - 1] * len(fr), fr)]))
    # a pair the table gives in both directions (rows n1 .. n2 reverse later
    # rows), with repeats inside the batch; one given by repeated rows (the
    # table's tail); a self pair and a pair that does not exist
    rv = next(i for i in range(n2 - 1, n1, -1) if fa[i] != fb[i])
    rp = next(i for i in range(E - 1, E - E // 20, -1) if fa[i] != fb[i])
    absent = next((a, b) for a in range(10, 40) for b in range(a + 1, 50) if b not in t.friends_of(a))
    seqs.append(("pairs", [
        rm(t, sev[:1] * 2, [fa[rv], fb[rv], fa[rv]], [fb[rv], fa[rv], fb[rv]]),
        rm(t, (), [fb[rp]], [fa[rp]]),
        rm(t, (), [fa[0], absent[0]], [fa[0], absent[1]]),
        rm(t, (), [absent[1]], [absent[0]])]))
    # unfriending together with the removal of that friend's reviews
    a0, b0 = next((int(a), int(b)) for a, b in zip(fa, fb)
                  if a != b and (rating[t.rows_of(b)] >= 8).sum() >= 2 and len(t.friends_of(a)) >= 2)
    seqs.append(("unfriend_with_reviews", [rm(t, t.rows_of(b0), [a0], [b0])]))
    # ratings across both thresholds, there and back; 9 -> 10 changes nothing
    row_at = lambda x, k=0: int(np.flatnonzero(np.isnan(rating) if x != x else rating == x)[k])
    rows = [row_at(8.0), row_at(7.0), row_at(4.0), row_at(5.0), row_at(np.nan), row_at(9.0),
            row_at(9.0, 1), row_at(9.0, 2)]
    to = [7.0, 8.0, 5.0, 4.0, 9.0, np.nan, 3.0, 10.0]
    seqs.append(("ratings", [rate(t, rows, to), rate(t, rows[-1:], [9.5]),
                             rate(t, rows + rows[:1], to + [2.0]), rate(t, rows, rating[rows])]))
    # removing, appending (rows numbered on from next_review_row), removing an appended row
    old = next(r for r in range(M - 2) if rev[r] != few)
    seqs.append(("append_after_remove", [
        rm(t, np.unique(np.r_[t.rows_of(few), M - 1, M - 2])),
        ("append", dict(review_reviewer=[few, 0, U - 1], review_item=[3, 3, 39],
                        review_rating=[9.0, 2.0, 8.0], friend_a=[few], friend_b=[0])),
        ("remove", dict(review_reviewer=[0, rev[old]], review_row=[M + 1, old], friend_a=[0],
                        friend_b=[few])),
        ("append", dict(review_reviewer=[0], review_item=[7], review_rating=[10.0])),
        ("set_rating", dict(review_reviewer=[U - 1, 0], review_row=[M + 2, M + 3],
                            review_rating=[1.0, np.nan]))]))
    # everything, then a first review and a first pair again
    seqs.append(("everything", [
        rm(t, np.arange(M), fa, fb),
        ("append", dict(review_reviewer=[4], review_item=[0], review_rating=[8.0],
                        friend_a=[4], friend_b=[5]))]))
    # drawn batches: reviews and pairs in one call, ratings in between
    rng = np.random.default_rng(100 + seed)
    order, cut = rng.permutation(M), [0, 1, 120, 400]
    steps = []
    for i in range(3):
        rows = np.sort(order[cut[i]:cut[i + 1]])
        e = rng.choice(E, 40, replace=False)
        steps.append(rm(t, rows, fa[e], fb[e]))
        edit = order[cut[i + 1]:cut[i + 1] + 60]
        steps.append(rate(t, edit, rng.choice([1.0, 4.0, 5.0, 7.0, 8.0, 10.0, np.nan], edit.size)))
    seqs.append(("mixed", steps))
    return [(name, init, steps) for name, steps in seqs]
