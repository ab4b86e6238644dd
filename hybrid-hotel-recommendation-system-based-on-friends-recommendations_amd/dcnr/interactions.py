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

import threading
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
    """Built once from host arrays in row space.

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
        self._dev = {}
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

    # ---------------------------------------------------------------- device
    def on(self, device):
        """The device CSRs (uploaded once per device) as (dcnr_interactions, tensors)."""
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
                p = lambda x: x.data_ptr() if x.numel() else None
                desc = _lib.Interactions(self.n_reviewers, p(t["friend_offsets"]),
                                         p(t["friend_rows"]), t["friend_rows"].numel(),
                                         p(t["review_offsets"]), p(t["review_items"]),
                                         p(t["review_rows"]), self.n_reviews)
                hit = self._dev[key] = (desc, t)
        return hit
