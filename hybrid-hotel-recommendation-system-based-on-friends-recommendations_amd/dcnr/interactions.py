"""The reviews and the friend graph as the /recommendations request path reads
them (main.py:172-194 and 336-351), in row space, on the host and the device.

The reference answers a request from two DataFrames: ``friendships_df``
(get_friends_for_user, main.py:172-178) and ``main_df`` (the source reviews of
_generate_candidates, main.py:187-194; the ``recommended_by`` lists, main.py:
336-351), each with several ``isin`` scans over the whole table per request.
``InteractionStore`` holds the same facts as two CSRs over the reviewers:

  friends   friends(u) = {b : (u, b)} | {a : (a, u)}: distinct, symmetric; u
            itself only where a (u, u) pair exists
  reviews   the reviews of a reviewer in ``main_df`` row order: hotel row, two
            class bits (rating_overall >= 8, <= 4; a NaN rating is neither)
            and the review's ``main_df`` row

The host copies (numpy) answer ``friends_host``, ``sources_host`` and
``recommended_by_host``: the overflow path of
``RankingPipeline.recommend_users`` and the yardstick of its tests.  The device
copies are what dcnr_requests_sources / dcnr_requests_recommended_by read.
Reviewer indices are dense, [0, U); hotel rows are the index's rows; the raw-id
dictionaries stay with the caller, as the joblib pickles do in main.py.
"""
from __future__ import annotations

import ctypes
import threading
import time
from typing import List, Tuple

import numpy as np
import torch

from . import _lib

FRIENDS, PERSONAL = 0, 1      # DCNR_MODE_*
POS_BIT, NEG_BIT = 1, 2       # class bits of review_items
MAX_ITEMS = 1 << 29           # hotel row * 4 + class bits in an int32


def mode_code(mode) -> int:
    """'friends' / 'personal' (main.py: any type but 'friends' is personal) -> DCNR_MODE_*."""
    if isinstance(mode, (int, np.integer)):
        if mode not in (FRIENDS, PERSONAL):
            raise ValueError(f"mode {mode}: 0 (friends) or 1 (personal)")
        return int(mode)
    if mode not in ("friends", "personal"):
        raise ValueError(f"mode {mode!r}: 'friends' or 'personal'")
    return FRIENDS if mode == "friends" else PERSONAL


def _csr(owner: np.ndarray, n: int) -> np.ndarray:
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(owner, minlength=n), out=off[1:])
    return off


class InteractionStore:
    """Built from host arrays in row space; ``append`` adds further reviews,
    friendships and reviewers in place, ``remove`` takes reviews and
    friendships out, ``set_rating`` edits ratings (the reviewers stay).

    review_reviewer [M]  dense reviewer index of each ``main_df`` row, in [0, U)
    review_item [M]      its hotel row, in [0, n_items)
    review_rating [M]    its rating_overall (the array order is main_df's)
    friend_a, friend_b [E]  reviewer indices of each friendship row; pairs may
                         repeat, appear in both directions, or be (u, u)
    n_items              rows of the index the hotel rows point into
    n_reviewers          U; default: the largest index named + 1
    """

    def __init__(self, review_reviewer, review_item, review_rating, friend_a, friend_b,
                 n_items: int, n_reviewers: int | None = None):
        rev = np.asarray(review_reviewer, dtype=np.int64).reshape(-1)
        item = np.asarray(review_item, dtype=np.int64).reshape(-1)
        rating = np.asarray(review_rating, dtype=np.float64).reshape(-1)
        fa = np.asarray(friend_a, dtype=np.int64).reshape(-1)
        fb = np.asarray(friend_b, dtype=np.int64).reshape(-1)
        if not (rev.size == item.size == rating.size):
            raise ValueError("InteractionStore: review_reviewer, review_item and review_rating "
                             "must have one entry per review")
        if fa.size != fb.size:
            raise ValueError("InteractionStore: friend_a and friend_b must have one entry per pair")
        n_items = int(n_items)
        if not 1 <= n_items <= MAX_ITEMS:
            raise ValueError(f"InteractionStore: n_items={n_items} outside [1, 2^29]")
        named = [a.max() + 1 for a in (rev, fa, fb) if a.size]
        U = int(n_reviewers) if n_reviewers is not None else int(max(named, default=0))
        for a, what in ((rev, "review_reviewer"), (fa, "friend_a"), (fb, "friend_b")):
            if a.size and (a.min() < 0 or a.max() >= U):
                raise ValueError(f"InteractionStore: {what} outside [0, {U})")
        if item.size and (item.min() < 0 or item.max() >= n_items):
            raise ValueError(f"InteractionStore: review_item outside [0, {n_items})")
        if max(rev.size, 2 * fa.size, U) >= 2 ** 31 - 1:
            raise ValueError("InteractionStore: 2^31 - 1 or more reviews, friend rows or reviewers")
        self.n_reviewers, self.n_items, self.n_reviews = U, n_items, rev.size
        self.next_review_row = rev.size   # main_df rows ever seen: n_reviews until one is removed
        # reviews by reviewer, main_df order kept inside a reviewer
        order = np.argsort(rev, kind="stable")
        cls = (rating >= 8).astype(np.int64) * POS_BIT + (rating <= 4).astype(np.int64) * NEG_BIT
        self.review_offsets = _csr(rev, U)
        self.review_item = item[order]
        self.review_class = cls[order].astype(np.int8)
        self.review_row = order.astype(np.int64)
        # friends: both directions, distinct
        pairs = np.unique(np.stack([np.concatenate([fa, fb]), np.concatenate([fb, fa])], 1), axis=0) \
            if fa.size else np.zeros((0, 2), np.int64)
        self.friend_offsets = _csr(pairs[:, 0], U)
        self.friend_rows = np.ascontiguousarray(pairs[:, 1])
        # per reviewer: review rows, distinct positives, distinct negatives ...
        srt_rev = rev[order]
        self.n_rows = np.diff(self.review_offsets)
        self.n_pos = self._distinct(srt_rev, self.review_item, self.review_class & POS_BIT)
        self.n_neg = self._distinct(srt_rev, self.review_item, self.review_class & NEG_BIT)
        # ... and the same summed over the reviewer's friends: a request's bounds
        owner = pairs[:, 0]
        fsum = lambda x: np.bincount(owner, weights=x[self.friend_rows],
                                     minlength=U).astype(np.int64)
        self.n_friends = np.diff(self.friend_offsets)
        self.friends_rows, self.friends_pos, self.friends_neg = (
            fsum(self.n_rows), fsum(self.n_pos), fsum(self.n_neg))
        self._dev, self._prev = {}, {}   # per device: the newest generation, the one before
        self.last_append = None          # timings and upload size of the last append that changed something
        self.last_remove = None          # ... of the last remove that did
        self._dev_lock = threading.Lock()

    def _distinct(self, srt_rev, items, flag) -> np.ndarray:
        m = flag != 0
        if not m.any():
            return np.zeros(self.n_reviewers, np.int64)
        pairs = np.unique(srt_rev[m] * self.n_items + items[m])
        return np.bincount(pairs // self.n_items, minlength=self.n_reviewers).astype(np.int64)

    # ------------------------------------------------------------------ host
    def friends_host(self, u: int) -> np.ndarray:
        """friends(u), ascending (get_friends_for_user, main.py:172-178); -1: none."""
        if u < 0:
            return np.zeros(0, np.int64)
        return self.friend_rows[self.friend_offsets[u]:self.friend_offsets[u + 1]]

    def _reviews_of(self, who) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(item, class, main_df row, reviewer) of the reviews of the reviewers ``who``."""
        who = np.asarray(who, np.int64).reshape(-1)
        if who.size == 0:
            z = np.zeros(0, np.int64)
            return z, z.astype(np.int8), z, z
        lo, hi = self.review_offsets[who], self.review_offsets[who + 1]
        idx = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)]) if who.size > 1 else \
            np.arange(lo[0], hi[0])
        return (self.review_item[idx], self.review_class[idx], self.review_row[idx],
                np.repeat(who, hi - lo))

    def sources_host(self, u: int, mode) -> Tuple[np.ndarray, np.ndarray]:
        """(positives, negatives) of a request, each ascending and distinct
        (main.py:187-194): the hotel rows the sources -- the friends, or the
        reviewer alone -- rated >= 8 / <= 4."""
        if u < 0:
            who = np.zeros(0, np.int64)
        elif mode_code(mode) == FRIENDS:
            who = self.friends_host(u)
        else:
            who = np.array([u], np.int64)
        item, cls, _, _ = self._reviews_of(who)
        return np.unique(item[(cls & POS_BIT) != 0]), np.unique(item[(cls & NEG_BIT) != 0])

    def recommended_by_host(self, u: int, ranked_rows) -> List[List[int]]:
        """For each hotel row of ``ranked_rows``: the distinct friends of u with
        a >= 8 review of it, in the order of their first such review's main_df
        row (groupby('item_id')['user_id'].unique(), main.py:336-351).  The
        friends are used whatever the request's mode was."""
        rows = [int(h) for h in (ranked_rows.tolist() if hasattr(ranked_rows, "tolist")
                                 else ranked_rows)]
        item, cls, row, who = self._reviews_of(self.friends_host(u))
        keep = (cls & POS_BIT) != 0
        item, row, who = item[keep], row[keep], who[keep]
        by: dict = {}
        for j in np.argsort(row, kind="stable"):
            lst = by.setdefault(int(item[j]), [])
            if int(who[j]) not in lst:
                lst.append(int(who[j]))
        return [list(by.get(h, [])) for h in rows]

    def bounds(self, reviewers: np.ndarray, modes: np.ndarray):
        """Per request, from the host counts alone: (sources, staged review
        rows, bound of the distinct positives, of the distinct negatives,
        friends, the friends' review rows, bound of the recommended_by
        entries).  A bound is at least the count and zero iff the count is."""
        known = reviewers >= 0
        u = np.where(known, reviewers, 0)
        pick = lambda own, fr: np.where(known, np.where(modes == PERSONAL, own[u], fr[u]), 0)
        nf = np.where(known, self.n_friends[u], 0)
        return (pick(np.ones_like(self.n_rows), self.n_friends), pick(self.n_rows, self.friends_rows),
                pick(self.n_pos, self.friends_pos), pick(self.n_neg, self.friends_neg),
                nf, np.where(known, self.friends_rows[u], 0), np.where(known, self.friends_pos[u], 0))

    # ---------------------------------------------------------------- append
    def append(self, review_reviewer=(), review_item=(), review_rating=(), friend_a=(),
               friend_b=(), n_reviewers: int | None = None) -> None:
        """Further rows of ``main_df`` and ``friendships_df``, in place.

        The arguments mean what they mean in the constructor: the reviews are
        the next rows of ``main_df`` (their ``review_row`` values are
        ``next_review_row .. next_review_row + m - 1``, in argument order;
        ``next_review_row`` is ``n_reviews`` as long as nothing was removed, and
        rows that ``remove`` took out are not given again), the pairs are
        further rows of ``friendships_df``.  ``n_reviewers`` may grow U (never
        shrink it; default: unchanged), and the batch may name the new
        reviewers.  Afterwards every host array and count, and every device
        tensor, equals those of a store built from the concatenated inputs
        with the final ``n_reviewers``: a reviewer's new reviews stand behind
        the old ones in batch order, a pair adds both directions (one entry
        for (u, u)) at their ascending places, and entries that exist already,
        or repeat inside the batch, are dropped.

        The host work is that of the batch and of the touched reviewers' own
        segments (plus the memory moves of the insertions): no sort of the old
        reviews, no ``np.unique`` over the old pairs.  On each device the store
        was uploaded to, dcnr_csr_insert writes the new CSRs from the old ones
        and the uploaded batch; the host copies are not uploaded again.
        Everything is validated, and every new array made, before anything
        changes: a failed append leaves the store as it was, on the host and on
        the devices.  An empty batch is a no-op.  ``last_append`` keeps the
        seconds of the host and the device part and the bytes uploaded per
        device (tools/bench_store_append.py reports them).

        Removing a review and unfriending: ``remove``; a changed rating:
        ``set_rating``.  Out of scope: changing ``n_items``, shrinking U, and
        stores sharded over several ranks.  For those, build a new store.
        """
        rev = np.asarray(review_reviewer, dtype=np.int64).reshape(-1)
        item = np.asarray(review_item, dtype=np.int64).reshape(-1)
        rating = np.asarray(review_rating, dtype=np.float64).reshape(-1)
        fa = np.asarray(friend_a, dtype=np.int64).reshape(-1)
        fb = np.asarray(friend_b, dtype=np.int64).reshape(-1)
        if not (rev.size == item.size == rating.size):
            raise ValueError("InteractionStore.append: review_reviewer, review_item and "
                             "review_rating must have one entry per review")
        if fa.size != fb.size:
            raise ValueError("InteractionStore.append: friend_a and friend_b must have one entry "
                             "per pair")
        U0, M0, E0 = self.n_reviewers, self.n_reviews, self.friend_rows.size
        U = U0 if n_reviewers is None else int(n_reviewers)
        if U < U0:
            raise ValueError(f"InteractionStore.append: n_reviewers={U} below the store's {U0}")
        for a, what in ((rev, "review_reviewer"), (fa, "friend_a"), (fb, "friend_b")):
            if a.size and (a.min() < 0 or a.max() >= U):
                raise ValueError(f"InteractionStore.append: {what} outside [0, {U})")
        if item.size and (item.min() < 0 or item.max() >= self.n_items):
            raise ValueError(f"InteractionStore.append: review_item outside [0, {self.n_items})")
        if max(M0 + rev.size, self.next_review_row + rev.size, E0 + 2 * fa.size, U) >= 2 ** 31 - 1:
            raise ValueError("InteractionStore.append: 2^31 - 1 or more reviews, friend rows or "
                             "reviewers")
        if rev.size == 0 and fa.size == 0 and U == U0:
            return
        t_start = time.perf_counter()
        grow = lambda a: np.concatenate([a, np.zeros(U - U0, a.dtype)]) if U > U0 else a.copy()
        ext = lambda off: np.concatenate([off, np.full(U - U0, off[-1], np.int64)])

        # ---- reviews: behind the reviewer's old ones, in batch order
        r_off = ext(self.review_offsets)
        order = np.argsort(rev, kind="stable")
        srt = rev[order]
        r_own, r_first, r_cnt = np.unique(srt, return_index=True, return_counts=True)
        r_pre = np.concatenate([[0], np.cumsum(r_cnt)]).astype(np.int64)
        cls = ((rating >= 8).astype(np.int64) * POS_BIT + (rating <= 4).astype(np.int64) * NEG_BIT)[order]
        r_at = r_off[srt + 1]                        # old index each one is inserted in front of
        r_pos = r_off[srt + 1] - r_off[srt] + np.arange(srt.size) - np.repeat(r_first, r_cnt)
        n_item, n_class = item[order], cls.astype(np.int8)
        n_row = self.next_review_row + order.astype(np.int64)
        review_item = np.insert(self.review_item, r_at, n_item)
        review_class = np.insert(self.review_class, r_at, n_class)
        review_row = np.insert(self.review_row, r_at, n_row)
        n_rows = grow(self.n_rows)
        n_rows[r_own] += r_cnt
        review_offsets = self._shifted(r_off, r_own, r_pre)
        n_pos, n_neg = grow(self.n_pos), grow(self.n_neg)
        deltas = [r_cnt]   # of n_rows, n_pos, n_neg at the touched reviewers
        if r_own.size:
            deltas += self._recount(review_offsets, review_item, review_class, r_own, n_pos, n_neg)

        # ---- friends: both directions, distinct, without those that exist already
        f_off = ext(self.friend_offsets)
        if fa.size:
            ent = np.unique(np.stack([np.concatenate([fa, fb]), np.concatenate([fb, fa])], 1), axis=0)
            at = self._lower_bound(self.friend_rows, f_off[ent[:, 0]], f_off[ent[:, 0] + 1], ent[:, 1])
            there = at < f_off[ent[:, 0] + 1]
            there[there] = self.friend_rows[at[there]] == ent[there, 1]
            ent, f_at = ent[~there], at[~there]
        else:
            ent, f_at = np.zeros((0, 2), np.int64), np.zeros(0, np.int64)
        f_own, f_first, f_cnt = np.unique(ent[:, 0], return_index=True, return_counts=True)
        f_pre = np.concatenate([[0], np.cumsum(f_cnt)]).astype(np.int64)
        f_pos = f_at - f_off[ent[:, 0]] + np.arange(ent.shape[0]) - np.repeat(f_first, f_cnt)
        friend_rows = np.insert(self.friend_rows, f_at, ent[:, 1])
        friend_offsets = self._shifted(f_off, f_own, f_pre)
        n_friends = grow(self.n_friends)
        n_friends[f_own] += f_cnt
        # the sums over a reviewer's friends: first each touched reviewer's change,
        # to the friends it had; then a new friend's whole (new) count
        sums = []
        if r_own.size:
            fidx, of_who = self._span(f_off, r_own)
            old_friends = self.friend_rows[fidx]
        for j, (new, fsum) in enumerate(((n_rows, self.friends_rows), (n_pos, self.friends_pos),
                                         (n_neg, self.friends_neg))):
            fsum = grow(fsum)
            if r_own.size:
                np.add.at(fsum, old_friends, deltas[j][of_who])
            np.add.at(fsum, ent[:, 0], new[ent[:, 1]])
            sums.append(fsum)

        # ---- the devices, then the host: nothing is published before all of it exists
        t_host = time.perf_counter()
        with self._dev_lock:
            gens = {key: self._device_append(key, hit, U, r_own, r_pre, r_pos,
                                             [n_item * 4 + n_class, n_row], f_own, f_pre, f_pos,
                                             [ent[:, 1]])
                    for key, hit in self._dev.items()}
            self._publish(gens)
            self.n_reviewers, self.n_reviews = U, M0 + rev.size
            self.next_review_row += rev.size
            self.review_offsets, self.review_item, self.review_class, self.review_row = (
                review_offsets, review_item, review_class, review_row)
            self.friend_offsets, self.friend_rows = friend_offsets, friend_rows
            self.n_rows, self.n_pos, self.n_neg, self.n_friends = n_rows, n_pos, n_neg, n_friends
            self.friends_rows, self.friends_pos, self.friends_neg = sums
            self.last_append = dict(host_s=t_host - t_start, device_s=time.perf_counter() - t_host,
                                    upload_bytes=8 * (r_own.size + r_pre.size + r_pos.size + f_own.size +
                                                      f_pre.size + f_pos.size + 1) +
                                    4 * (2 * r_pos.size + f_pos.size + 1), devices=len(gens))

    # ---------------------------------------------------- remove, set_rating
    def remove(self, review_reviewer=(), review_row=(), friend_a=(), friend_b=()) -> None:
        """Rows of ``main_df`` and friendships taken out, in place.

        A review is named by its reviewer and its ``main_df`` row (its
        ``review_row`` value): the lookup is a binary search inside the
        reviewer's segment, where the rows ascend.  A (reviewer, row) the
        store does not hold raises ``ValueError``; a repeat inside the batch
        counts once.  The surviving reviews keep their ``review_row`` values
        and ``next_review_row`` stays, so ``append`` never gives a removed
        row's number again; ``n_reviews`` is the number of reviews held.  A
        pair (a, b) ends the friendship in both directions, whatever rows of
        ``friendships_df`` spelled it ((u, u): the self entry); a pair that is
        not there is ignored, as ``append`` ignores one that is.  U stays.

        Afterwards every host array and count, and every device tensor, equals
        those of a store built from the tables without those rows, with
        ``review_row`` mapped through the surviving rows' original numbers.
        The host work is that of the batch and of the touched reviewers' own
        segments and friend lists (plus the memory moves).  On each device the
        store was uploaded to, the removed positions go up in one upload and
        dcnr_csr_remove writes the next generation of each CSR that changes;
        the other keeps its tensors.  The generations are handled as by
        ``append`` (see ``on``).  Everything is validated, and every new array
        made, before anything changes: a refused remove leaves the store as it
        was, on the host and on the devices.  An empty batch is a no-op.
        ``last_remove`` keeps what ``last_append`` keeps.
        """
        rr, row, fa, fb = (np.asarray(a, dtype=np.int64).reshape(-1)
                           for a in (review_reviewer, review_row, friend_a, friend_b))
        if rr.size != row.size:
            raise ValueError("InteractionStore.remove: review_reviewer and review_row must have "
                             "one entry per review")
        if fa.size != fb.size:
            raise ValueError("InteractionStore.remove: friend_a and friend_b must have one entry "
                             "per pair")
        U = self.n_reviewers
        for a, what in ((rr, "review_reviewer"), (fa, "friend_a"), (fb, "friend_b")):
            if a.size and (a.min() < 0 or a.max() >= U):
                raise ValueError(f"InteractionStore.remove: {what} outside [0, {U})")
        if rr.size == 0 and fa.size == 0:
            return
        t_start = time.perf_counter()
        minus = lambda cnt: -np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)

        # ---- reviews: their positions, ascending
        r_who, r_at, _ = self._locate("remove", rr, row)
        r_own, r_cnt = np.unique(r_who, return_counts=True)
        review_item = np.delete(self.review_item, r_at)
        review_class = np.delete(self.review_class, r_at)
        review_row = np.delete(self.review_row, r_at)
        review_offsets = self._shifted(self.review_offsets, r_own, minus(r_cnt))
        n_rows, n_pos, n_neg = self.n_rows.copy(), self.n_pos.copy(), self.n_neg.copy()
        n_rows[r_own] -= r_cnt
        deltas = [-r_cnt]   # of n_rows, n_pos, n_neg at the touched reviewers
        if r_own.size:
            deltas += self._recount(review_offsets, review_item, review_class, r_own, n_pos, n_neg)

        # ---- friends: both directions of the pairs that are there
        f_off = self.friend_offsets
        if fa.size:
            ent = np.unique(np.concatenate([fa * U + fb, fb * U + fa]))   # (owner, friend) as one word
            ent = np.stack([ent // U, ent % U], 1)
            at = self._lower_bound(self.friend_rows, f_off[ent[:, 0]], f_off[ent[:, 0] + 1], ent[:, 1])
            there = at < f_off[ent[:, 0] + 1]
            there[there] = self.friend_rows[at[there]] == ent[there, 1]
            ent, f_at = ent[there], at[there]
        else:
            ent, f_at = np.zeros((0, 2), np.int64), np.zeros(0, np.int64)
        if r_at.size == 0 and f_at.size == 0:
            return
        f_own, f_cnt = np.unique(ent[:, 0], return_counts=True)
        friend_rows = np.delete(self.friend_rows, f_at)
        friend_offsets = self._shifted(f_off, f_own, minus(f_cnt))
        n_friends = self.n_friends.copy()
        n_friends[f_own] -= f_cnt
        # the sums over a reviewer's friends: first a former friend's whole (old)
        # count, then each touched reviewer's change, to the friends it keeps
        if r_own.size:
            fidx, kf_who = self._span(friend_offsets, r_own)
            kept_friends = friend_rows[fidx]
        sums = []
        for j, (old, fsum) in enumerate(((self.n_rows, self.friends_rows), (self.n_pos, self.friends_pos),
                                         (self.n_neg, self.friends_neg))):
            fsum = fsum.copy()
            np.subtract.at(fsum, ent[:, 0], old[ent[:, 1]])
            if r_own.size:
                np.add.at(fsum, kept_friends, deltas[j][kf_who])
            sums.append(fsum)

        # ---- the devices, then the host: nothing is published before all of it exists
        t_host = time.perf_counter()
        with self._dev_lock:
            gens = {key: self._device_remove(key, hit, r_at, f_at) for key, hit in self._dev.items()}
            self._publish(gens)
            self.n_reviews -= r_at.size
            self.review_offsets, self.review_item, self.review_class, self.review_row = (
                review_offsets, review_item, review_class, review_row)
            self.friend_offsets, self.friend_rows = friend_offsets, friend_rows
            self.n_rows, self.n_pos, self.n_neg, self.n_friends = n_rows, n_pos, n_neg, n_friends
            self.friends_rows, self.friends_pos, self.friends_neg = sums
            self.last_remove = dict(host_s=t_host - t_start, device_s=time.perf_counter() - t_host,
                                    upload_bytes=8 * (r_at.size + f_at.size + 1), devices=len(gens))

    def set_rating(self, review_reviewer, review_row, review_rating) -> None:
        """``rating_overall`` of reviews the store holds, edited in place.

        The reviews are named as for ``remove``; of a (reviewer, row) given
        several times the last rating counts, and one the store does not hold
        raises ``ValueError`` and changes nothing.  A review keeps its place
        and its ``review_row``: only its class bits change, so afterwards the
        store equals one built from the tables with the rating column edited.
        The host counts the distinct positives and negatives of the touched
        reviewers anew and passes the changes on to their friends' sums.  On
        each device only ``review_items`` gets a new generation, a copy with
        the changed words scattered in; the other tensors are shared with the
        generation before.  Ratings that leave every class as it is change
        nothing.
        """
        rr, row = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (review_reviewer, review_row))
        rating = np.asarray(review_rating, dtype=np.float64).reshape(-1)
        if not (rr.size == row.size == rating.size):
            raise ValueError("InteractionStore.set_rating: review_reviewer, review_row and "
                             "review_rating must have one entry per review")
        if rr.size and (rr.min() < 0 or rr.max() >= self.n_reviewers):
            raise ValueError(f"InteractionStore.set_rating: review_reviewer outside "
                             f"[0, {self.n_reviewers})")
        if rr.size == 0:
            return
        t_start = time.perf_counter()
        who, at, inverse = self._locate("set_rating", rr, row)
        last = np.empty(at.size, np.float64)
        last[inverse] = rating     # (of a repeated index the last value is assigned)
        cls = ((last >= 8).astype(np.int8) * POS_BIT + (last <= 4).astype(np.int8) * NEG_BIT)
        changed = cls != self.review_class[at]
        if not changed.any():
            return
        who, at, cls = who[changed], at[changed], cls[changed]
        review_class = self.review_class.copy()
        review_class[at] = cls
        own = np.unique(who)
        n_pos, n_neg = self.n_pos.copy(), self.n_neg.copy()
        deltas = self._recount(self.review_offsets, self.review_item, review_class, own, n_pos, n_neg)
        fidx, f_who = self._span(self.friend_offsets, own)
        sums = []
        for d, fsum in zip(deltas, (self.friends_pos, self.friends_neg)):
            fsum = fsum.copy()
            np.add.at(fsum, self.friend_rows[fidx], d[f_who])
            sums.append(fsum)
        words = (self.review_item[at] * 4 + cls).astype(np.int32)
        t_host = time.perf_counter()
        with self._dev_lock:
            gens = {key: self._device_set_items(key, hit, at, words) for key, hit in self._dev.items()}
            self._publish(gens)
            self.review_class, self.n_pos, self.n_neg = review_class, n_pos, n_neg
            self.friends_pos, self.friends_neg = sums

    def _locate(self, what, rr, row):
        """The reviews (reviewer, main_df row) of a batch, repeats once: their
        reviewers, their positions (ascending) and each batch entry's index
        into the two; ValueError for one the store does not hold."""
        if rr.size == 0:
            z = np.zeros(0, np.int64)
            return z, z, z
        N = max(self.next_review_row, 1)
        seen = (row >= 0) & (row < N)
        if not seen.all():
            raise ValueError(f"InteractionStore.{what}: reviewer {rr[~seen][0]} has no review at "
                             f"main_df row {row[~seen][0]}: the store saw rows [0, {N})")
        # (reviewer, row) as one word: both are below 2^31
        key, inverse = np.unique(rr * N + row, return_inverse=True)
        who, key = key // N, key % N
        lo, hi = self.review_offsets[who], self.review_offsets[who + 1]
        at = self._lower_bound(self.review_row, lo, hi, key)
        there = at < hi
        there[there] = self.review_row[at[there]] == key[there]
        if not there.all():
            raise ValueError(f"InteractionStore.{what}: reviewer {who[~there][0]} has no review at "
                             f"main_df row {key[~there][0]} ({int((~there).sum())} such in the batch)")
        return who, at, inverse.reshape(-1)

    @staticmethod
    def _span(off, owners):
        """Every position of the segments off[o] .. off[o + 1] of ``owners``,
        in their order, and the index into ``owners`` each belongs to."""
        lo, n = off[owners], off[owners + 1] - off[owners]
        idx = np.repeat(lo - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(int(n.sum()))
        return idx, np.repeat(np.arange(owners.size), n)

    def _recount(self, review_offsets, review_item, review_class, owners, n_pos, n_neg):
        """n_pos / n_neg of the reviewers ``owners``, counted anew from their
        segments and written in place; returns the two changes."""
        idx, who = self._span(review_offsets, owners)
        deltas = []
        for flag, out in ((POS_BIT, n_pos), (NEG_BIT, n_neg)):
            before = out[owners].copy()
            keep = (review_class[idx] & flag) != 0
            pairs = np.unique(who[keep] * self.n_items + review_item[idx][keep])
            out[owners] = np.bincount(pairs // self.n_items, minlength=owners.size)
            deltas.append(out[owners] - before)
        return deltas

    def _publish(self, gens) -> None:
        """The next generation of every device (under the lock); an older one
        is dropped only when no kernel launched against it can still run."""
        if self._prev:
            for key in self._prev:
                torch.cuda.synchronize(torch.device(*key))
        self._prev = dict(self._dev)
        self._dev.update(gens)

    def _device_remove(self, key, hit, r_at, f_at):
        """The next generation of one device's CSRs without the entries at r_at / f_at."""
        device = torch.device(*key)
        _, old = hit
        lib = _lib.load()
        d_at = torch.from_numpy(np.concatenate([r_at, f_at, np.zeros(1, np.int64)])).to(device)
        U = old["review_offsets"].numel() - 1
        new = {}
        with torch.cuda.device(device):
            stream = _lib.stream_ptr(device)
            ptrs = lambda ts: (ctypes.c_void_p * 2)(*[t.data_ptr() or None for t in ts])
            for names, off_name, m, p_at in (
                    (["review_items", "review_rows"], "review_offsets", r_at.size, d_at.data_ptr()),
                    (["friend_rows"], "friend_offsets", f_at.size, d_at.data_ptr() + 8 * r_at.size)):
                if m == 0:   # this CSR is as it was
                    new.update({k: old[k] for k in names + [off_name]})
                    continue
                M_old = old[names[0]].numel()
                new[off_name] = torch.empty(U + 1, dtype=torch.int64, device=device)
                for k in names:
                    new[k] = torch.empty(M_old - m, dtype=torch.int32, device=device)
                _lib.check(lib.dcnr_csr_remove(
                    old[off_name].data_ptr(), U, M_old, len(names), ptrs([old[k] for k in names]),
                    p_at, m, new[off_name].data_ptr(), ptrs([new[k] for k in names]), stream),
                    "dcnr_csr_remove")
            # published only once written; the uploaded positions may go once read
            torch.cuda.current_stream(device).synchronize()
        return self._describe(new, U, new["review_rows"].numel()), new

    def _device_set_items(self, key, hit, at, words):
        """The next generation of one device: review_items with ``words`` at ``at``."""
        device = torch.device(*key)
        desc, old = hit
        new = dict(old)
        with torch.cuda.device(device):
            new["review_items"] = old["review_items"].clone()
            new["review_items"][torch.from_numpy(at).to(device)] = torch.from_numpy(words).to(device)
            torch.cuda.current_stream(device).synchronize()
        return self._describe(new, desc.n_reviewers, desc.n_reviews), new

    @staticmethod
    def _shifted(off, owners, prefix) -> np.ndarray:
        """off [U + 1] with prefix[j + 1] - prefix[j] entries more in owner owners[j]."""
        add = np.zeros(off.size, np.int64)
        add[owners + 1] = np.diff(prefix)
        return off + np.cumsum(add)

    @staticmethod
    def _lower_bound(arr, lo, hi, x) -> np.ndarray:
        """Per entry: the first index in [lo, hi) of the ascending arr[lo:hi] not below x."""
        lo, hi = lo.copy(), hi.copy()
        while True:
            act = lo < hi
            if not act.any():
                return lo
            mid = (lo + hi) >> 1
            less = act.copy()
            less[act] = arr[mid[act]] < x[act]
            lo = np.where(less, mid + 1, lo)
            hi = np.where(act & ~less, mid, hi)

    def _device_append(self, key, hit, U, r_own, r_pre, r_pos, r_vals, f_own, f_pre, f_pos, f_vals):
        """The next generation of one device's CSRs: (dcnr_interactions, tensors)."""
        device = torch.device(*key)
        _, old = hit
        lib = _lib.load()
        # the whole batch in one upload: int64 words, the int32 payloads behind them
        parts = [r_own, r_pre, r_pos, f_own, f_pre, f_pos]
        words = np.concatenate([np.asarray(a, np.int64) for a in parts] +
                               [np.zeros(1, np.int64)])   # (never empty)
        vals = np.concatenate([np.asarray(a).astype(np.int32) for a in r_vals + f_vals] +
                              [np.zeros(1, np.int32)])
        d_words = torch.from_numpy(words).to(device)
        d_vals = torch.from_numpy(vals).to(device)
        at, o = [], 0
        for a in parts:
            at.append(d_words.data_ptr() + 8 * o)
            o += a.size
        new = {}
        with torch.cuda.device(device):
            stream = _lib.stream_ptr(device)
            v = d_vals.data_ptr()
            for names, off_name, (own, pre, pos), (p_own, p_pre, p_pos), n_vals in (
                    (["review_items", "review_rows"], "review_offsets", (r_own, r_pre, r_pos), at[:3], 2),
                    (["friend_rows"], "friend_offsets", (f_own, f_pre, f_pos), at[3:], 1)):
                m, M_old, U_old = pos.size, old[names[0]].numel(), old[off_name].numel() - 1
                ins = [v + 4 * m * w for w in range(n_vals)]
                v += 4 * m * n_vals
                if m == 0 and U == U_old:   # this CSR is as it was
                    new.update({k: old[k] for k in names + [off_name]})
                    continue
                new[off_name] = torch.empty(U + 1, dtype=torch.int64, device=device)
                for k in names:
                    new[k] = torch.empty(M_old + m, dtype=torch.int32, device=device) if m else old[k]
                ptrs = lambda ps: (ctypes.c_void_p * 2)(*[p or None for p in ps])
                _lib.check(lib.dcnr_csr_insert(
                    old[off_name].data_ptr(), U_old, U, M_old, n_vals,
                    ptrs([old[k].data_ptr() for k in names]), p_own, p_pre, own.size, p_pos,
                    ptrs(ins), m, new[off_name].data_ptr(),
                    ptrs([new[k].data_ptr() for k in names]), stream), "dcnr_csr_insert")
            # published only once written; the uploaded batch may go once read
            torch.cuda.current_stream(device).synchronize()
        return self._describe(new, U, new["review_rows"].numel()), new

    @staticmethod
    def _describe(t, n_reviewers, n_reviews):
        p = lambda x: x.data_ptr() if x.numel() else None
        return _lib.Interactions(n_reviewers, p(t["friend_offsets"]), p(t["friend_rows"]),
                                 t["friend_rows"].numel(), p(t["review_offsets"]),
                                 p(t["review_items"]), p(t["review_rows"]), n_reviews)

    # ---------------------------------------------------------------- device
    def on(self, device):
        """The device CSRs as (dcnr_interactions, tensors): uploaded on a
        device's first call, advanced on that device by every ``append``,
        ``remove`` and ``set_rating`` since (what follows says ``append`` for
        all three).

        Generations.  The tensors of a generation are never written after they
        are published, and ``append`` publishes the next one only once it is
        fully written.  A kernel reads the generation its descriptor points
        into, so whoever launches one keeps the tensors returned here until the
        kernel has finished (``RankingPipeline.recommend_users`` keeps them with
        its answers).  For callers that kept the descriptor alone, the store
        itself holds the generation before the newest, and it synchronizes the
        device before it lets go of an older one: memory a kernel launched
        before that ``append`` may read is not released under it.  ``append``
        and the calls that read the host counts (``bounds``) are not atomic
        with respect to each other: serialise ``append`` against
        ``recommend_users`` on the same store.
        """
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("InteractionStore.on: the device copies live on the HIP device only")
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        with self._dev_lock:
            hit = self._dev.get(key)
            if hit is None:
                up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(device)
                t = dict(friend_offsets=up(self.friend_offsets, np.int64),
                         friend_rows=up(self.friend_rows, np.int32),
                         review_offsets=up(self.review_offsets, np.int64),
                         review_items=up(self.review_item * 4 + self.review_class, np.int32),
                         review_rows=up(self.review_row, np.int32))
                # published only once written: a call on another stream may read it at once
                torch.cuda.current_stream(device).synchronize()
                hit = self._dev[key] = (self._describe(t, self.n_reviewers, self.n_reviews), t)
        return hit
