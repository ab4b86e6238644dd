"""Host yardsticks and shared inputs of the large-request tests
(test_large_requests_cpu.py, test_large_requests_gpu.py), in numpy:

  ref_candidates   the candidate composition of one request with no 4096 limit:
                   oracle.candidate_union, np.union1d with the fallback when the
                   union is below min_candidates, then the set filters (what
                   test_recommend_many_gpu.ref_candidates composes on the device)
  ref_rank         the stable descending rank (main.py:325)
  mmr_f64          greedy MMR (main.py:133-169) restated in float64, with every
                   round's margin between the best and the second-best value
  mmr_case         the inputs of the GPU MMR tests; the CPU test asserts that
                   with these seeds every round's margin exceeds 1e-4 and every
                   pair of scores differs by more than 1e-5, so float32 summation
                   order cannot flip a pick
  lane_cases       the requests of the GPU candidate test
"""
import numpy as np

import dcnr_oracle as orc

SV_MAX = 4096
N_ITEMS = 5000
MIN_C = 20


def ref_candidates(pos, idx, fallback, allowed, excluded, min_c=MIN_C):
    """pos [Q] (rows < 0 skipped), idx [Q, k] (column 0 dropped, rows < 0 skipped)."""
    pos = np.asarray(pos, np.int64).reshape(-1)
    idx = np.asarray(idx, np.int64).reshape(pos.size, -1) if pos.size else np.zeros((0, 1), np.int64)
    cand = orc.candidate_union(pos[pos >= 0], idx)
    if fallback is not None and cand.size < min_c:
        cand = np.union1d(cand, np.asarray(fallback, np.int64))
    if allowed is not None:
        cand = cand[np.isin(cand, np.asarray(allowed, np.int64))]
    if excluded is not None:
        cand = cand[~np.isin(cand, np.asarray(excluded, np.int64))]
    return cand.astype(np.int64)


def ref_rank(scores):
    return np.argsort(-np.asarray(scores, np.float32), kind="stable")


def mmr_f64(emb, rows, scores, lam, top_k):
    """(picks: positions into the ranked list, margins: per selection round the
    best MMR value minus the second best, inf when only one candidate is left).
    lambda is the float32 the kernels compute with, everything else float64."""
    lam = float(np.float32(lam))
    rows = np.asarray(rows, np.int64)
    s = np.asarray(scores, np.float64)
    n = rows.size
    if n == 0:
        return [], []
    e = np.asarray(emb, np.float64)
    norm = np.sqrt((e * e).sum(1))
    unit = np.where(norm[:, None] > 0, e / np.where(norm > 0, norm, 1.0)[:, None], 0.0)
    valid = rows >= 0
    cu = unit[np.where(valid, rows, 0)]
    taken = np.zeros(n, bool)
    taken[0] = True
    maxsim = np.full(n, -np.inf)
    picks, margins, last, any_sel = [0], [], 0, False
    while True:
        if rows[last] >= 0:
            maxsim = np.maximum(maxsim, cu @ unit[rows[last]])
            any_sel = True
        if len(picks) >= min(top_k, n):
            break
        val = lam * s - (1.0 - lam) * (maxsim if any_sel else 0.0)
        val = np.where(taken | ~valid, -np.inf, val)
        best = int(np.argmax(val))
        if val[best] == -np.inf:
            break
        rest = np.delete(val, best)
        second = rest.max() if rest.size else -np.inf
        margins.append(val[best] - second)
        taken[best] = True
        picks.append(best)
        last = best
    return picks, margins


# ---- the GPU MMR tests' inputs
MMR_TABLE_ROWS = 8192
MMR_N = (4097, 6000)
MMR_D = (16, 64)
MMR_LAMBDAS = (0.3, 0.7)
MMR_TOP_K = (5, 20)
# picked on the CPU so that test_large_requests_cpu's condition holds (smallest margins 2.4e-4 .. 4.8e-4)
MMR_SEEDS = {(4097, 16): 2, (4097, 64): 3, (6000, 16): 2, (6000, 64): 7}


def mmr_case(n, d):
    """(emb float32 [MMR_TABLE_ROWS, d], rows int64 [n] with some -1, scores
    float32 [n] descending, every pair more than 5e-4 apart)."""
    rng = np.random.default_rng(MMR_SEEDS[(n, d)] * 1000 + n + d)
    emb = rng.standard_normal((MMR_TABLE_ROWS, d)).astype(np.float32)
    rows = rng.permutation(MMR_TABLE_ROWS)[:n].astype(np.int64)
    rows[rng.choice(np.arange(1, n), n // 100, replace=False)] = -1
    scores = ((n - np.arange(n)) * 1e-3 + rng.uniform(-2e-4, 2e-4, n)).astype(np.float32)
    return emb, rows, scores


# ---- the GPU candidate test's requests
def lane_sets(seed=3):
    rng = np.random.default_rng(seed)
    return [np.zeros(0, np.int64),                                          # 0: empty
            np.arange(N_ITEMS),                                             # 1: every row
            np.sort(rng.choice(N_ITEMS, N_ITEMS // 2, replace=False)),      # 2: half of the rows
            np.sort(rng.choice(N_ITEMS, 100, replace=False)),               # 3: "popular"
            np.sort(rng.choice(N_ITEMS, SV_MAX + 1, replace=False)),        # 4: a fallback of 4097 rows
            np.arange(40, 45), np.arange(40, 47), np.arange(40, 48), np.arange(40, 49)]   # 5-8: 5, 7, 8, 9 rows


def lane_cases(k, table, seed=0):
    """name -> request (pos, idx [Q, k], allowed, excluded, fallback set
    indices, bad) of the large-lane candidate test; with ``table`` the
    neighbours are rows of a neighbour table (returned too), else random lists
    with some -1.  Staged sizes (positives * k + fallback rows): 4097, 8191,
    8192, 8193, about 20 000."""
    rng = np.random.default_rng(seed + 17 * k)
    sets = lane_sets()
    nbr = rng.integers(0, N_ITEMS, (N_ITEMS, k + 1)).astype(np.int32)

    def lists(pos):
        pos = np.asarray(pos, np.int64)
        if table:
            idx = np.where(pos[:, None] >= 0, nbr[np.maximum(pos, 0), :k].astype(np.int64), -1)
        else:
            idx = rng.integers(0, N_ITEMS, (pos.size, k)).astype(np.int64)
            idx[rng.random(idx.shape) < 0.03] = -1
        return pos, idx

    def some(Q, neg=True):
        pos = rng.integers(0, N_ITEMS, Q).astype(np.int64)
        if neg:
            pos[rng.choice(Q, max(1, Q // 50), replace=False)] = -1
        return lists(pos)

    # Q positives and the fallback set (by index) that brings the staged size to `staged`
    def sized(staged):
        if k == 1:
            return staged, -1
        Q = staged // k
        f = {5: 5, 7: 6, 8: 7, 9: 8}[staged - Q * k]
        return Q, f

    cases = {}
    Q, f = sized(4097)      # the union exceeds min_candidates: its fallback is ignored
    cases["s4097"] = some(Q) + (-1, -1, f, False)
    pos, idx = lists(np.full(4100, 123))
    idx[:] = idx[0]         # a positive's neighbours are the same wherever it is repeated
    cases["one_positive"] = (pos, idx, -1, -1, 3, False)                     # a union of <= k rows
    Q, f = sized(8191)
    cases["s8191"] = some(Q) + (2, 3, f, False)
    Q, f = sized(8192)
    cases["s8192_allowed_empty"] = some(Q) + (0, -1, f, False)
    Q, f = sized(8193)
    cases["s8193_all_excluded"] = some(Q) + (-1, 1, f, False)
    cases["s20000"] = some(20000 // k) + (1, 3, -1, False)
    cases["fallback_4097"] = lists(np.zeros(0, np.int64)) + (2, -1, 4, False)   # no positives
    pos, idx = some(4097 // k + 1, neg=False)
    if table:
        pos[5] = N_ITEMS + 3        # a positive outside the table
        idx[5] = -1
    else:
        idx[5, k - 1] = N_ITEMS     # a neighbour outside the table (k = 1: column 0 is dropped)
        if k == 1:
            pos[5] = N_ITEMS
    cases["bad_row"] = (pos, idx, -1, -1, -1, True)
    small = lists(rng.integers(0, N_ITEMS, 7)) + (-1, -1, 3, False)   # a small-lane neighbour in the batch
    return sets, nbr, cases, small


LANE_GROUPS = [["s4097"], ["fallback_4097"], ["one_positive", "s8191"],
               ["s8192_allowed_empty", "s8193_all_excluded", "s20000", "bad_row", "s4097"]]
