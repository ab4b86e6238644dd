"""Requests above the 4096-row capacity in the batched device pass: the large
lane (dcnr_requests_large_*, dcnr_mmr_rerank_large; csrc/serving_large.hip).

  1  candidates against the numpy yardstick, through the C entry point
  2  the large entry points on small segments equal the small lane bit for bit
  3  the rank above the capacity: exact ties, NaN and -inf logits
  4  the MMR above the capacity, single-request and batched, against the
     float64 restatement on inputs whose margins the CPU test asserts
  5  end to end: recommend_many with two large requests, recommend() barred
  6  recommend() answers lambda < 1 above the capacity
  7  the budget sends a large request the host way

Everything compared is an integer result or a logit the same kernels computed:
every comparison is an equality.  The scored batches stay below TOWER_MIN_B =
16384 rows, where a row's eval logit does not depend on the batch it is in.
"""
import itertools

import numpy as np
import pytest
import torch

import large_requests_common as lc
import test_recommend_many_gpu as rm

pytestmark = pytest.mark.gpu

SV_MAX, N_ITEMS, MIN_C = lc.SV_MAX, lc.N_ITEMS, lc.MIN_C
BAD_DATA = 2


def _t(a, dtype, dev):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def _p(t):
    return t.data_ptr() if t is not None and t.numel() else None


# ---------------------------------------------------------------- C ABI wrappers
def c_large_candidates(dev, pos, idx, k, sets, a_idx, e_idx, f_idx, lanes, min_c, n_items, nbr=None):
    """dcnr_requests_large_candidates: R requests (pos[r], idx[r] [Q_r, k]) of which
    `lanes` are large; with `nbr` the neighbours come from that table."""
    from dcnr import _lib
    lib = _lib.load()
    R, L = len(pos), len(lanes)
    d_pos, d_pos_off, pos_off = rm._csr(pos, dev)
    Q = int(pos_off[-1])
    d_idx = _t(np.concatenate([np.asarray(i, np.int64).reshape(-1, k) for i in idx] +
                              [np.zeros((0, k), np.int64)]), torch.int64, dev)
    d_nbr = None if nbr is None else _t(nbr, torch.int32, dev)
    d_sets, d_set_off, set_off = rm._csr(sets, dev)
    S = len(sets)
    ix = [_t(v, torch.int32, dev) if S else None for v in (a_idx, e_idx, f_idx)]
    flen = [int(set_off[f + 1] - set_off[f]) if f >= 0 else 0 for f in f_idx]
    stage_off = np.r_[0, np.cumsum([len(pos[r]) * k + flen[r] for r in lanes])].astype(np.int64)
    n = int(stage_off[-1])
    d_lanes, d_stage = _t(lanes, torch.int32, dev), _t(stage_off, torch.int64, dev)
    rows = torch.full((max(n, 1),), -7, dtype=torch.int64, device=dev)
    count = torch.full((L,), -7, dtype=torch.int32, device=dev)
    status = torch.full((L,), -7, dtype=torch.int32, device=dev)
    offsets = torch.full((L + 1,), -7, dtype=torch.int64, device=dev)
    h_off = torch.full((L + 1,), -7, dtype=torch.int64).pin_memory()
    h_status = torch.full((L,), -7, dtype=torch.int32).pin_memory()
    nb = int(lib.dcnr_requests_large_workspace_size(L, n))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.check(lib.dcnr_requests_large_candidates(
        _p(d_pos), d_pos_off.data_ptr(), R, Q, None if nbr is not None else _p(d_idx), _p(d_nbr),
        0 if nbr is None else nbr.shape[1], k, _p(d_sets), d_sets.numel(),
        d_set_off.data_ptr() if S else None, S, _p(ix[0]), _p(ix[1]), _p(ix[2]), min_c, n_items,
        d_lanes.data_ptr(), d_stage.data_ptr(), L, n, rows.data_ptr(), count.data_ptr(),
        status.data_ptr(), offsets.data_ptr(), h_off.data_ptr(), h_status.data_ptr(), ws.data_ptr(), nb,
        _lib.stream_ptr(dev)), "dcnr_requests_large_candidates")
    torch.cuda.current_stream(dev).synchronize()
    assert torch.equal(h_status, status.cpu()) and torch.equal(h_off, offsets.cpu())   # the pinned mirrors
    return rows.cpu().numpy(), offsets.cpu().numpy(), count.cpu().numpy(), status.cpu().numpy()


def c_large_rank_mmr(dev, table, inv, segs):
    """dcnr_requests_large_rank_mmr over segments (rows, scores, lambda, top_k)."""
    from dcnr import _lib
    lib = _lib.load()
    L = len(segs)
    off = np.zeros(L + 1, np.int64)
    np.cumsum([len(s[0]) for s in segs], out=off[1:])
    n = int(off[-1])
    rows = _t(np.concatenate([s[0] for s in segs] + [np.zeros(0, np.int64)]), torch.int64, dev)
    logits = _t(np.concatenate([s[1] for s in segs] + [np.zeros(0, np.float32)]), torch.float32, dev)
    lam = _t([s[2] for s in segs], torch.float32, dev)
    tk = _t([s[3] for s in segs], torch.int32, dev)
    d_off = _t(off, torch.int64, dev)
    out_rows = torch.full((max(n, 1),), -9, dtype=torch.int64, device=dev)
    out_logits = torch.full((max(n, 1),), -9.0, dtype=torch.float32, device=dev)
    out_count = torch.full((L,), -9, dtype=torch.int32, device=dev)
    status = torch.zeros(L, dtype=torch.int32, device=dev)
    nb = int(lib.dcnr_requests_large_workspace_size(L, n))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.check(lib.dcnr_requests_large_rank_mmr(
        _p(logits), n, _p(rows), d_off.data_ptr(), L, table.data_ptr(), inv.data_ptr(), table.shape[1],
        table.shape[0], lam.data_ptr(), tk.data_ptr(), out_rows.data_ptr(), out_logits.data_ptr(),
        out_count.data_ptr(), status.data_ptr(), ws.data_ptr(), nb, _lib.stream_ptr(dev)),
        "dcnr_requests_large_rank_mmr")
    return off, out_rows, out_logits, out_count.cpu().numpy(), status.cpu().numpy()


# ------------------------------------------------------------- 1: candidates
@pytest.mark.parametrize("table", [False, True], ids=["knn_idx", "table"])
@pytest.mark.parametrize("k", [1, 11])
@pytest.mark.parametrize("group", range(len(lc.LANE_GROUPS)), ids=["-".join(g) for g in lc.LANE_GROUPS])
def test_candidates_against_the_yardstick(dev, group, k, table):
    sets, nbr, cases, small = lc.lane_cases(k, table)
    names = lc.LANE_GROUPS[group]
    # small requests before and between the lanes: a lane's request index is not its number
    reqs = [small] + [cases[names[0]]] + [small] + [cases[nm] for nm in names[1:]]
    lanes = [1] + list(range(3, 2 + len(names)))
    pos, idx = [q[0] for q in reqs], [q[1] for q in reqs]
    a_idx, e_idx, f_idx = ([q[j] for q in reqs] for j in (2, 3, 4))
    rows, offsets, count, status = c_large_candidates(dev, pos, idx, k, sets, a_idx, e_idx, f_idx, lanes,
                                                      MIN_C, N_ITEMS, nbr if table else None)
    staged = [len(pos[r]) * k + (len(sets[f_idx[r]]) if f_idx[r] >= 0 else 0) for r in lanes]
    assert all(s > SV_MAX for s in staged), staged
    if names == ["s4097"]:
        assert staged == [4097]
    if "s8191" in names:
        assert staged[names.index("s8191")] == 8191
    pick = lambda ix, r: None if ix[r] < 0 else sets[ix[r]]
    want_count = []
    for l, r in enumerate(lanes):
        if reqs[r][5]:                       # a row outside the table: that request alone
            assert status[l] == BAD_DATA and count[l] == 0, (names[l], status[l])
            want_count.append(0)
            continue
        want = lc.ref_candidates(pos[r], idx[r], pick(f_idx, r), pick(a_idx, r), pick(e_idx, r), MIN_C)
        assert status[l] == 0 and count[l] == want.size, (names[l], status[l], count[l], want.size)
        assert rows[offsets[l]:offsets[l] + count[l]].tolist() == want.tolist(), names[l]
        want_count.append(want.size)
        union = lc.ref_candidates(pos[r], idx[r], None, None, None)
        if names[l] == "one_positive":
            assert union.size <= k and want.size > union.size        # the fallback joined
        if names[l] == "s4097" and k == 11:
            assert union.size >= MIN_C and want.tolist() == union.tolist()   # ... and here it did not
        if names[l] in ("s8192_allowed_empty", "s8193_all_excluded"):
            assert want.size == 0
        if names[l] == "fallback_4097":
            assert union.size == 0 and want.size > SV_MAX // 3
    assert offsets.tolist() == np.r_[0, np.cumsum(want_count)].tolist()


def test_candidates_offsets_that_are_no_partition(dev):
    """Staged offsets that do not rise from 0 to n_staged reject every lane; no lane
    is read outside its bound."""
    from dcnr import _lib
    lib = _lib.load()
    pos = [np.arange(10), np.arange(20)]
    d_pos, d_pos_off, _ = rm._csr(pos, dev)
    idx = _t(np.zeros((30, 1), np.int64), torch.int64, dev)
    lanes = _t([0, 1], torch.int32, dev)
    for stage in ([0, 10, 29], [0, 12, 30], [1, 10, 30], [0, 20, 10]):
        d_stage = _t(stage, torch.int64, dev)
        rows = torch.empty(30, dtype=torch.int64, device=dev)
        words = torch.full((3, 2), -7, dtype=torch.int32, device=dev)
        offsets = torch.empty(3, dtype=torch.int64, device=dev)
        nb = int(lib.dcnr_requests_large_workspace_size(2, 30))
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        _lib.check(lib.dcnr_requests_large_candidates(
            d_pos.data_ptr(), d_pos_off.data_ptr(), 2, 30, idx.data_ptr(), None, 0, 1, None, 0, None, 0,
            None, None, None, 20, 100, lanes.data_ptr(), d_stage.data_ptr(), 2, 30, rows.data_ptr(),
            words[0].data_ptr(), words[1].data_ptr(), offsets.data_ptr(), None, None, ws.data_ptr(), nb,
            _lib.stream_ptr(dev)), "dcnr_requests_large_candidates")
        status, count = words[1].cpu().tolist(), words[0].cpu().tolist()
        # ([0, 12, 30] is a partition, but not into the requests' bounds 10 and 20)
        assert status == [BAD_DATA, BAD_DATA] and count == [0, 0], stage
        assert offsets.cpu().tolist() == [0, 0, 0]


# ------------------------------------------- 2: small segments, both lanes
@pytest.mark.parametrize("k", [1, 11])
def test_small_requests_equal_the_small_lane(dev, k):
    R = 37
    sets, pos, idx, a_idx, e_idx, f_idx = rm.candidate_requests(R, k, seed=R * 16 + k)
    slots, s_count, s_status, _, _ = rm.c_candidates(dev, pos, idx, k, sets, a_idx, e_idx, f_idx, MIN_C,
                                                     N_ITEMS, SV_MAX)
    s_count, s_status, slots = s_count.cpu().numpy(), s_status.cpu().numpy(), slots.cpu().numpy()
    rows, offsets, count, status = c_large_candidates(dev, pos, idx, k, sets, a_idx, e_idx, f_idx,
                                                      list(range(R)), MIN_C, N_ITEMS)
    assert not status.any()                                  # the large lane has no capacity to exceed
    n_same = 0
    for r in range(R):
        got = rows[offsets[r]:offsets[r] + count[r]]
        if s_status[r] == 0:
            assert count[r] == s_count[r] and got.tolist() == slots[r, :s_count[r]].tolist(), r
            n_same += 1
        else:                                                # the small lane overflowed: the yardstick
            pick = lambda ix: None if ix[r] < 0 else sets[ix[r]]
            want = lc.ref_candidates(pos[r], idx[r], pick(f_idx), pick(a_idx), pick(e_idx), MIN_C)
            assert got.tolist() == want.tolist(), r
    assert n_same >= R - 8 and n_same < R


def test_small_segments_equal_the_small_lane_rank_mmr(dev):
    table, inv = rm.make_table(32, dev)
    combos = [(n, lam, tk) for n in (1, 2, 64, 65, 1023, 1024, 1025, 4096) for lam in (0.0, 0.3, 1.0)
              for tk in (1, 5, 20, n + 7)]
    segs = rm.rank_segments(combos, seed=32)
    off, s_rows, s_logits, s_count, s_status = rm.c_rank_mmr(dev, table, inv, segs, SV_MAX)
    off2, rows, logits, count, status = c_large_rank_mmr(dev, table, inv, segs)
    assert off.tolist() == off2.tolist() and not status.any() and not s_status.any()
    assert count.tolist() == s_count.tolist()
    for r, c in enumerate(count):
        o = int(off[r])
        assert torch.equal(rows[o:o + c], s_rows[o:o + c]), combos[r]
        assert torch.equal(logits[o:o + c], s_logits[o:o + c]), combos[r]


# ------------------------------------------------ 3: rank above the capacity
def tied_scores(n, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(n).astype(np.float32)
    s[n // 3:n // 3 + 700] = 0.25                            # blocks of exactly tied scores
    s[rng.choice(n, n // 4, replace=False)] = np.float32(-1.5)
    s[5], s[9] = 0.0, -0.0                                   # equal as floats: position decides
    return s


def test_rank_above_the_capacity(dev):
    table, inv = rm.make_table(16, dev)
    rng = np.random.default_rng(5)
    lens = (4097, 8193, 20000)
    segs = [(rng.integers(0, N_ITEMS, n).astype(np.int64), tied_scores(n, n), 1.0, 20) for n in lens]
    off, rows, logits, count, status = c_large_rank_mmr(dev, table, inv, segs)
    assert not status.any() and count.tolist() == list(lens)
    for r, (cand, s, _, _) in enumerate(segs):
        order = lc.ref_rank(s)
        o = int(off[r])
        assert rows[o:o + len(s)].cpu().numpy().tolist() == cand[order].tolist(), r
        assert np.array_equal(logits[o:o + len(s)].cpu().numpy().view(np.uint32), s[order].view(np.uint32)), r


def test_logits_without_a_rank_mark_their_segment_only(dev):
    table, inv = rm.make_table(16, dev)
    rng = np.random.default_rng(6)
    segs = [(rng.integers(0, N_ITEMS, n).astype(np.int64), tied_scores(n, n + 1), lam, 20)
            for n, lam in ((4097, 1.0), (4500, 1.0), (5000, 0.3), (70, 0.3))]
    segs[0][1][4000] = np.nan
    segs[2][1][0] = -np.inf
    off, rows, logits, count, status = c_large_rank_mmr(dev, table, inv, segs)
    assert status.tolist() == [BAD_DATA, 0, BAD_DATA, 0] and count.tolist() == [0, 4500, 0, 20]
    for r in (0, 2):
        assert (rows[off[r]:off[r + 1]] == -1).all() and torch.isnan(logits[off[r]:off[r + 1]]).all()
    order = lc.ref_rank(segs[1][1])
    assert rows[off[1]:off[2]].cpu().numpy().tolist() == segs[1][0][order].tolist()
    want_rows, want_s = rm.ref_rank_mmr(dev, table, inv, *segs[3])
    assert torch.equal(rows[off[3]:off[3] + 20], want_rows) and torch.equal(logits[off[3]:off[3] + 20], want_s)


# ------------------------------------------------- 4: MMR above the capacity
@pytest.mark.parametrize("d", lc.MMR_D)
def test_mmr_above_the_capacity(dev, d):
    from dcnr import serving
    combos = list(itertools.product(lc.MMR_N, lc.MMR_LAMBDAS, lc.MMR_TOP_K))
    segs, want = [], []
    for n, lam, tk in combos:
        emb, rows, scores = lc.mmr_case(n, d)
        segs.append((rows, scores, lam, tk))
        want.append(lc.mmr_f64(emb, rows, scores, lam, tk)[0])
    # (one table for both n: mmr_case draws it per (n, d), so each n gets its own call)
    for n in lc.MMR_N:
        emb = lc.mmr_case(n, d)[0]
        table = torch.from_numpy(emb).to(dev)
        inv = serving.row_inv_norms(table)
        mine = [j for j, c in enumerate(combos) if c[0] == n]
        # the single-request call (rows of -1 among the candidates)
        for j in mine:
            rows, scores, lam, tk = segs[j]
            pos = serving.mmr_positions_large(table, inv, torch.from_numpy(rows), torch.from_numpy(scores),
                                              lam, tk)
            assert pos.cpu().tolist() == want[j], combos[j]
        # the batched call: the scores are in ranked order, so its rank keeps them
        off, out_rows, out_logits, count, status = c_large_rank_mmr(dev, table, inv, [segs[j] for j in mine])
        assert not status.any()
        for l, j in enumerate(mine):
            rows, scores, lam, tk = segs[j]
            o = int(off[l])
            assert count[l] == len(want[j])
            assert out_rows[o:o + count[l]].cpu().tolist() == rows[want[j]].tolist(), combos[j]
            assert np.array_equal(out_logits[o:o + count[l]].cpu().numpy(), scores[want[j]]), combos[j]


# ------------------------------------------------------------ 5: end to end
_pipes = {}


def get_pipe(dev, precision, table):
    """test_recommend_many_gpu's synthetic pipeline, with or without a neighbour table."""
    if (precision, table) not in _pipes:
        import dcnr
        base = rm.get_pipe(dev, precision)
        _pipes[(precision, table)] = base if not table else dcnr.RankingPipeline(
            base.model, base.item_cat, base.item_num, neighbor_table=True)
    return _pipes[(precision, table)]


def large_batch(seed=8):
    """mixed_requests with two large requests spliced in at 3 and 6."""
    reqs, popular, half = rm.mixed_requests(7, seed=seed)
    rng = np.random.default_rng(4)
    big_a = dict(reqs[1], pos=rng.choice(N_ITEMS, 400, replace=False).tolist(), lam=1.0, allowed=half,
                 excluded=None)
    big_b = dict(reqs[2], pos=rng.choice(N_ITEMS, 700, replace=False).tolist(), lam=0.7, top_k=20,
                 allowed=None, excluded=reqs[2]["pos"][:3], fallback=popular)
    return reqs[:3] + [big_a] + reqs[3:5] + [big_b] + reqs[5:], [3, 6]


def barred(*a, **kw):
    raise AssertionError("recommend() called for a request the large lane answers")


def count_waits(monkeypatch, fn):
    calls = []
    real = torch.cuda.Stream.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (calls.append(1), real(self))[1])
    out = fn()
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", real)
    return out, len(calls)


@pytest.mark.parametrize("table", [False, True], ids=["scan", "table"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_recommend_many_answers_large_requests_on_the_device(dev, precision, table, monkeypatch):
    pipe = get_pipe(dev, precision, table)
    reqs, where = large_batch()
    want = [rm.run_single(pipe, q) for q in reqs]
    assert all(len(reqs[r]["pos"]) * pipe.n_neighbors > SV_MAX for r in where)
    assert want[6][0].numel() == 20 and sum(w[0].numel() for w in want) < 16384
    # (the 700-positive request's candidates: as many as 7700 staged entries of 5000 hotels give)
    monkeypatch.setattr(pipe, "recommend", barred)
    got, waits = count_waits(monkeypatch, lambda: rm.run_many(pipe, reqs))
    monkeypatch.undo()
    assert waits == 1, waits
    rm.assert_same(got, want, f"{precision} table={table}")
    assert list(got.large) == where and list(got.on_host) == []
    # the others are what they are without the large requests
    small = [q for r, q in enumerate(reqs) if r not in where]
    rm.assert_same([g for r, g in enumerate(got) if r not in where], rm.run_many(pipe, small), "others")


@pytest.mark.parametrize("mode", ["city_sets", "neighbors_within"])
def test_large_requests_with_city_sets_and_neighbors_within(dev, mode, monkeypatch):
    import dcnr
    pipe = get_pipe(dev, "bf16", False)
    rng = np.random.default_rng(21)
    city_of = rng.integers(0, 3, N_ITEMS)
    n_pos = [5, 450, 0, 12, 700]
    pos = [rng.choice(np.flatnonzero(city_of == r % 3), n, replace=False).tolist() for r, n in enumerate(n_pos)]
    users, lam, tk = [3, 9, 27, 81, 243], [1.0, 0.7, 0.3, 1.0, 1.0], [20, 20, 5, 20, 20]
    cities = [np.flatnonzero(city_of == c) for c in range(3)]
    if mode == "city_sets":       # one review row per hotel, the key decides the popular ones
        cs = dcnr.CitySets(np.arange(N_ITEMS), city_of, rng.integers(0, 1000, N_ITEMS).astype(np.float64),
                           n_items=N_ITEMS, n_cities=3)
        single = dict(allowed=[cs.city_rows_host(r % 3) for r in range(5)],
                      fallback=[cs.popular_rows_host(r % 3) for r in range(5)])
        kw = dict(city_sets=cs, cities=[r % 3 for r in range(5)])
        cs.on(dev)                # the generation is built (and waited for) before the counted call
    else:
        single = kw = dict(allowed=[cities[r % 3] for r in range(5)],
                           neighbors_within=[cities[r % 3] if r != 3 else None for r in range(5)])
    want = [pipe.recommend(users[r], pos[r], lam[r], tk[r], **{name: v[r] for name, v in single.items()})
            for r in range(5)]
    monkeypatch.setattr(pipe, "recommend", barred)
    got, waits = count_waits(monkeypatch, lambda: pipe.recommend_many(users, pos, lam, tk, **kw))
    monkeypatch.undo()
    assert waits == 1, waits
    rm.assert_same(got, want, mode)
    assert list(got.large) == [1, 4] and list(got.on_host) == []


# ------------------------------------- 6: recommend() above the capacity
def test_recommend_mmr_above_the_capacity(dev):
    pipe = get_pipe(dev, "fp32", False)
    rng = np.random.default_rng(33)
    pos = rng.choice(N_ITEMS, 1500, replace=False).tolist()
    ranked, z = pipe.recommend(17, pos, 1.0)
    print("ranked candidates:", ranked.numel())
    assert ranked.numel() > SV_MAX
    emb = pipe.index._table.cpu().numpy()
    picks, margins = lc.mmr_f64(emb, ranked.cpu().numpy(), z.cpu().numpy(), 0.7, 20)
    # The scores are the float32 logits themselves on both sides; what differs is the
    # similarity, a float32 sum of 32 products of unit-vector components (error below
    # 32 * 2^-24 = 2e-6).  A margin above 1e-5 cannot be flipped by that.
    print("smallest margin:", min(margins))
    assert min(margins) > 1e-5, min(margins)
    rows, logits = pipe.recommend(17, pos, 0.7, top_k=20)
    assert rows.tolist() == ranked[picks].tolist()
    assert torch.equal(logits, z[picks])


# -------------------------------------------------------------- 7: budget
def test_budget_sends_a_large_request_the_host_way(dev):
    pipe = get_pipe(dev, "bf16", False)
    reqs, where = large_batch()
    want = rm.run_many(pipe, reqs)
    assert list(want.large) == where and list(want.on_host) == []
    before = pipe.large_lane_budget
    try:
        pipe.large_lane_budget = 700 * pipe.n_neighbors + 100 - 1     # below request 6's bound
        got = rm.run_many(pipe, reqs)
        assert list(got.large) == [3] and list(got.on_host) == [6]
        rm.assert_same(got, want, "budget")
        pipe.large_lane_budget = 0
        got = rm.run_many(pipe, reqs)
        assert list(got.large) == [] and list(got.on_host) == where
        rm.assert_same(got, want, "no budget")
    finally:
        pipe.large_lane_budget = before
