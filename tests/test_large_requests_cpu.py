"""The host half of the large request lane, and the yardsticks and inputs of
test_large_requests_gpu.py: no device needed.

  1  pack_requests marks a request large from its bound `need` = positives * k
     + fallback rows, at 4095 / 4096 / 4097, with and without a fallback set
  2  what it packed before is unchanged by the new attributes
  3  large_lane_split: the budget rule, a lambda that rounds to 1.0f
  4  the numpy yardsticks against brute-force Python on tiny inputs
  5  the inputs of the GPU MMR tests: every round's margin above 1e-4 and every
     pair of scores more than 1e-5 apart (test_serving_gpu.py's condition on
     its inputs), so the float32 kernels must make the float64 picks
"""
import itertools

import numpy as np
import pytest

import large_requests_common as lc
import request_pack_cases as rc
from dcnr.requests import SV_MAX, large_lane_split, pack_requests


def pack(pos, k, fallback=None, lam=1.0, n_rows=100000, reg=()):
    R = len(pos)
    reg_off = np.r_[0, np.cumsum([len(s) for s in reg])].astype(np.int64)
    return pack_requests(np.zeros(R, np.int64), pos, lam, 20, None, None, fallback, None, n_users=5,
                         n_rows=n_rows, k=k, reg_off=reg_off)


@pytest.mark.parametrize("k", [1, 11])
def test_lane_split_at_the_capacity_without_a_fallback(k):
    # staged lists around SV_MAX: only a bound above it is large
    qs = sorted({SV_MAX // k - 1, SV_MAX // k, SV_MAX // k + 1, (SV_MAX - 1) // k, 3})
    p = pack([np.arange(q) for q in qs], k)
    need = np.array(qs) * k
    assert p.need.tolist() == need.tolist() and not p.fallback_len.any()
    assert p.large.tolist() == np.flatnonzero(need > SV_MAX).tolist()
    assert p.large.dtype == np.int32
    if k == 1:
        assert need.tolist() == [3, 4095, 4096, 4097] and p.large.tolist() == [3]
    assert p.cap == min(SV_MAX, need.max())


def test_lane_split_at_the_capacity_with_a_fallback():
    # 4000 staged entries + a registered fallback of 95 / 96 / 97 rows; one ad-hoc set
    reg = [np.arange(95), np.arange(96), np.arange(97)]
    pos = [np.arange(4000)] * 5
    p = pack(pos, 1, fallback=[0, 1, 2, None, list(range(50, 147))], reg=reg)
    assert p.need.tolist() == [4095, 4096, 4097, 4000, 4097]
    assert p.fallback_len.tolist() == [95, 96, 97, 0, 97]
    assert p.large.tolist() == [2, 4]
    # the fallback alone lifts a request without positives past the capacity
    p = pack([np.zeros(0, np.int64), np.arange(3)], 11, fallback=[list(range(4097)), list(range(4096))])
    assert p.need.tolist() == [4097, 4129] and p.large.tolist() == [0, 1]
    p = pack([np.zeros(0, np.int64)], 11, fallback=[list(range(4096))])
    assert p.large.size == 0


@pytest.mark.parametrize("case", list(rc.cases()))
def test_packed_outputs_keep_their_fields(case):
    """The golden test pins the bytes; here: the new attributes sit beside the
    old ones and agree with them."""
    q = rc.cases()[case]
    city = None if q["cities"] is None else (rc.CITY_OFF, rc.N_CITIES, np.asarray(q["cities"], np.int64),
                                             q["in_city"])
    p = pack_requests(q["users"], q["positive_rows"], q["lambda_param"], q["top_k"], q["allowed"],
                      q["excluded"], q["fallback"], q["neighbors_within"], n_users=rc.N_USERS,
                      n_rows=rc.N_ROWS, k=rc.K, reg_off=rc.REG_OFF, city=city)
    assert not any(name.startswith("large") for name in p.arrays)
    lens = np.diff(p.pos_off)
    assert p.need.tolist() == (lens * rc.K + p.fallback_len).tolist()
    assert p.cap == int(min(SV_MAX, max(1, p.need.max())))
    assert p.large.tolist() == np.flatnonzero(p.need > SV_MAX).tolist()


def test_budget_rule():
    lens = [10, 5000, 4097, 30, 6000, 4100]
    lam = [1.0, 0.7, 1.0, 0.3, 1.0 - 2.0 ** -30, 0.5]       # request 4: rounds to 1.0f
    p = pack([np.arange(n) for n in lens], 1, lam=lam)
    assert p.large.tolist() == [1, 2, 4, 5] and p.odd.tolist() == [False] * 4 + [True, False]
    lanes, host, off = large_lane_split(p, 1 << 20)
    assert (lanes.tolist(), host.tolist(), off.tolist()) == ([1, 2, 5], [4], [0, 5000, 9097, 13197])
    assert lanes.dtype == np.int32 and off.dtype == np.int64
    # in request order while the sum of the bounds fits: 5000 + 4097 <= 9100 < 5000 + 4097 + 4100
    lanes, host, off = large_lane_split(p, 9100)
    assert (lanes.tolist(), host.tolist(), off.tolist()) == ([1, 2], [4, 5], [0, 5000, 9097])
    lanes, host, off = large_lane_split(p, 4999)            # the first does not fit, later ones may
    assert (lanes.tolist(), host.tolist(), off.tolist()) == ([2], [1, 4, 5], [0, 4097])
    lanes, host, off = large_lane_split(p, 0)
    assert (lanes.tolist(), host.tolist(), off.tolist()) == ([], [1, 2, 4, 5], [0])
    lanes, host, off = large_lane_split(pack([np.arange(5)], 11), 1 << 20)
    assert lanes.size == 0 and host.size == 0 and off.tolist() == [0]


# ---------------------------------------------------------------- yardsticks
def brute_candidates(pos, idx, fallback, allowed, excluded, min_c):
    s = set()
    for p, row in zip(pos, idx):
        if p >= 0:
            s.add(int(p))
        s.update(int(v) for v in row[1:] if v >= 0)
    if fallback is not None and len(s) < min_c:
        s |= set(int(v) for v in fallback)
    if allowed is not None:
        s &= set(int(v) for v in allowed)
    if excluded is not None:
        s -= set(int(v) for v in excluded)
    return sorted(s)


def test_ref_candidates_against_python_sets():
    rng = np.random.default_rng(0)
    for trial in range(200):
        Q, k = int(rng.integers(0, 6)), int(rng.choice([1, 3]))
        pos = rng.integers(-1, 12, Q)
        idx = rng.integers(-1, 12, (Q, k))
        pick = lambda: None if rng.random() < 0.4 else np.unique(rng.integers(0, 12, int(rng.integers(0, 8))))
        fb, al, ex = pick(), pick(), pick()
        min_c = int(rng.integers(0, 8))
        got = lc.ref_candidates(pos, idx, fb, al, ex, min_c)
        assert got.tolist() == brute_candidates(pos, idx, fb, al, ex, min_c), trial


def test_ref_rank_is_the_stable_descending_sort():
    rng = np.random.default_rng(1)
    s = (rng.integers(-4, 4, 50) / 2).astype(np.float32)
    want = [i for _, i in sorted(zip((-s).tolist(), range(50)))]   # ties: lower position first
    assert lc.ref_rank(s).tolist() == want


def brute_mmr(emb, rows, scores, lam, top_k):
    lam = float(np.float32(lam))
    def unit(v):
        nv = np.sqrt(float(np.dot(v, v)))
        return v / nv if nv > 0 else v
    n = len(rows)
    final, remaining = [0], list(range(1, n))
    while len(final) < min(top_k, n):
        sel = [unit(emb[rows[p]].astype(np.float64)) for p in final if rows[p] >= 0]
        best, best_v = -1, -np.inf
        for p in remaining:
            if rows[p] < 0:
                continue
            ms = max(float(np.dot(unit(emb[rows[p]].astype(np.float64)), s)) for s in sel) if sel else 0.0
            v = lam * float(scores[p]) - (1.0 - lam) * ms
            if v > best_v:
                best, best_v = p, v
        if best < 0:
            break
        final.append(best)
        remaining.remove(best)
    return final


def test_mmr_f64_against_the_plain_loop():
    rng = np.random.default_rng(2)
    for trial in range(30):
        n, d = int(rng.integers(1, 14)), 5
        emb = rng.standard_normal((20, d)).astype(np.float32)
        emb[3] = 0.0
        rows = rng.permutation(20)[:n]          # distinct rows: no exactly tied values
        rows[rng.random(n) < 0.2] = -1
        scores = np.sort(rng.standard_normal(n).astype(np.float32))[::-1]
        lam, tk = float(rng.choice([0.0, 0.3, 0.7])), int(rng.integers(1, 16))
        picks, margins = lc.mmr_f64(emb, rows, scores, lam, tk)
        assert picks == brute_mmr(emb, rows, scores, lam, tk), trial
        assert len(margins) == len(picks) - 1 and all(m >= 0 for m in margins)


# ------------------------------------------------ the GPU MMR tests' inputs
@pytest.mark.parametrize("n,d", list(itertools.product(lc.MMR_N, lc.MMR_D)))
def test_gpu_mmr_inputs_cannot_flip_a_pick(n, d):
    emb, rows, scores = lc.mmr_case(n, d)
    assert n > SV_MAX and rows.size == n and (rows < 0).any() and rows[0] >= 0
    assert np.min(np.diff(np.sort(scores.astype(np.float64)))) > 1e-5, "near-tied scores"
    assert (np.diff(scores) < 0).all()                      # in ranked order
    for lam, tk in itertools.product(lc.MMR_LAMBDAS, lc.MMR_TOP_K):
        picks, margins = lc.mmr_f64(emb, rows, scores, lam, tk)
        assert len(picks) == tk and len(set(picks)) == tk
        assert min(margins) > 1e-4, (lam, tk, min(margins))
        assert picks != list(range(tk)) or tk == 1          # the re-rank does change the order
