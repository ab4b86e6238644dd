"""/recommendations from user ids (``RankingPipeline.recommend_users``,
dcnr_requests_sources, dcnr_requests_recommended_by): the reviews and the
friend graph on the device.  Every comparison is an equality: the yardsticks
are ``InteractionStore``'s host functions (tests/test_interactions_cpu.py holds
them to the reference service) and ``recommend_many`` fed with their answers.

  1  dcnr_requests_sources through the C ABI at R = 1, 7, 70
  2  recommend_users against recommend_many(sources_host), both modes, MMR on
     and off, with and without registered city sets, bf16 and fp32
  3  the recommended_by lists against recommended_by_host
  4  the F11 and F7 fixtures (the reference service's responses) in one call
  5  capacity: sizes taken from SV_MAX
  6  corrupted store data ends that request alone (every index the kernels
     form is compared with a length passed by value before use:
     store_friends / store_reviews in csrc/serving.hip)
  7  a non-default stream; two host threads on one pipeline and one store
"""
import threading

import numpy as np
import pytest
import torch

import f11_common
import f7_common
from helpers import our_model

pytestmark = pytest.mark.gpu

SV_MAX = 4096
OVERFLOW, BAD_DATA = 1, 2     # DCNR_REQ_*
N_ITEMS, U, M, E = 500, 300, 4000, 600
CFG = dict(n_users=400, n_items=N_ITEMS, cat_dims={"a": 30, "b": 250}, n_num=4,
           params=dict(emb_dim=32, hidden_dim=64, n_cross_layers=2, n_res_blocks=2, dropout=0.0))
LONER, GHOSTS = 16, 17        # a reviewer whose friends have no reviews; one who is nobody's friend
A, B, X, HOTEL = 40, 30, 50, 123     # the repeated-review order case: recommended_by = [A, B]


def tables():
    """f11_common.random_tables plus: LONER's only friends have no reviews,
    GHOSTS has no friends, and friend A of X reviews HOTEL twice with >= 8,
    friend B's >= 8 review of it between the two rows (A > B)."""
    rev, item, rating, fa, fb = f11_common.random_tables(U, M, E, N_ITEMS, seed=4)
    keep = ~np.isin(fa, (LONER, GHOSTS)) & ~np.isin(fb, (LONER, GHOSTS))
    fa, fb = np.r_[fa[keep], LONER, U - 2, X, B], np.r_[fb[keep], U - 1, LONER, A, X]
    friends_x = set(fa[fb == X]) | set(fb[fa == X]) | {X}
    rating[np.isin(rev, list(friends_x)) & (item == HOTEL)] = 6     # nobody else's opinion of it
    # (X's own 8, so that HOTEL is a candidate of X's personal requests as well)
    for row, who, val in ((1000, A, 9), (2000, B, 8), (3000, A, 10), (3500, X, 8)):
        rev[row], item[row], rating[row] = who, HOTEL, val
    return rev, item, rating, fa, fb


_cache = {}


def get_store():
    import dcnr
    if "store" not in _cache:
        _cache["store"] = dcnr.InteractionStore(*tables(), n_items=N_ITEMS, n_reviewers=U)
    return _cache["store"]


def get_pipe(dev, precision):
    import dcnr
    if precision not in _cache:
        m = our_model(CFG, precision=precision, seed=9).to(dev).eval()
        rng = np.random.default_rng(2)
        item_cat = np.stack([rng.integers(0, c, N_ITEMS) for c in CFG["cat_dims"].values()], 1)
        item_num = rng.random((N_ITEMS, 4), dtype=np.float32)
        _cache[precision] = dcnr.RankingPipeline(m, item_cat, item_num)
    return _cache[precision]


def mixed_requests(R, seed):
    """Reviewers of every kind (unknown, without friends, with friends who have
    no reviews, without reviews, the order case), both modes, MMR on and off."""
    rng = np.random.default_rng(seed)
    special = [(-1, "friends"), (LONER, "friends"), (GHOSTS, "friends"), (3, "friends"),
               (U - 1, "personal"), (X, "friends"), (X, "personal")]
    rv = [special[r][0] if r < len(special) else int(rng.integers(0, U)) for r in range(R)]
    return dict(users=rng.integers(0, CFG["n_users"], R).tolist(), rv=rv,
                modes=[special[r][1] if r < len(special) else ["friends", "personal"][(r // 2) % 2]
                       for r in range(R)],
                lam=[[1.0, 0.3][r % 2] for r in range(R)],
                top_k=[[20, 5, 1, 500][(r // 4) % 4] for r in range(R)])


def run_users(pipe, store, q, allowed=None, fallback=None, **kw):
    return pipe.recommend_users(store, q["users"], q["rv"], q["modes"], lambda_param=q["lam"],
                                top_k=q["top_k"], allowed=allowed, fallback=fallback, **kw)


def yardstick(pipe, store, q, allowed=None, fallback=None):
    """recommend_many fed with sources_host: positives, and excluded = negatives."""
    src = [store.sources_host(u, m) for u, m in zip(q["rv"], q["modes"])]
    return pipe.recommend_many(q["users"], [s[0] for s in src], lambda_param=q["lam"],
                               top_k=q["top_k"], allowed=allowed,
                               excluded=[s[1] for s in src], fallback=fallback)


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for r, ((gr, gl), (wr, wl)) in enumerate(zip(got, want)):
        assert torch.equal(gr, wr), (what, r, gr.numel(), wr.numel())
        assert torch.equal(gl, wl), (what, r)


def assert_recommended_by(res, store, q, what=""):
    """to_lists and the CSR tensors against recommended_by_host, position by position."""
    by_off, by_rev = res.by_offsets.cpu().numpy(), res.by_reviewers.cpu().numpy()
    by_cnt = res.by_count.cpu().numpy()
    assert by_off[0] == 0 and np.array_equal(np.diff(by_off), by_cnt)
    assert (by_rev[by_off[-1]:] == -1).all()
    total = 0
    for r, (rows, logits) in enumerate(res):
        want = store.recommended_by_host(q["rv"][r], rows.tolist())
        got_rows, got_logits, got_by = res.to_lists(r)
        assert got_rows == rows.tolist() and got_logits == logits.tolist(), (what, r)
        assert got_by == want, (what, r, got_by, want)
        total += sum(len(b) for b in want)
        if res.on_host[r]:
            continue
        o, n_r = int(res._seg[r]), int(res._seg[r + 1] - res._seg[r])
        assert [by_rev[by_off[o + i]:by_off[o + i + 1]].tolist() for i in range(len(want))] == want
        assert (by_cnt[o + len(want):o + n_r] == 0).all(), (what, r)    # behind the answer: nothing
    return total


# ------------------------------------------------ 1: the sources, stage level
def c_sources(dev, desc, rv, md, pos_b, neg_b, neg_lo=5, guard=9):
    """dcnr_requests_sources over sentinel-filled buffers with words to spare at
    both ends."""
    from dcnr import _lib
    lib = _lib.load()
    R = len(rv)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    pos_off = np.r_[0, np.cumsum(pos_b)].astype(np.int64)
    neg_off = (neg_lo + np.r_[0, np.cumsum(neg_b)]).astype(np.int64)
    Q, neg_hi = int(pos_off[-1]), int(neg_off[-1])
    pos = torch.full((Q + guard,), -7, dtype=torch.int64, device=dev)
    neg = torch.full((neg_hi + guard,), -7, dtype=torch.int64, device=dev)
    counts = torch.full((2 * R,), -7, dtype=torch.int32, device=dev)
    status = torch.full((R,), -7, dtype=torch.int32, device=dev)
    h_counts = torch.full((2 * R,), -7, dtype=torch.int32).pin_memory()
    h_status = torch.full((R,), -7, dtype=torch.int32).pin_memory()
    d_rv, d_md = t(rv, torch.int32), t(md, torch.int32)
    d_po, d_no = t(pos_off, torch.int64), t(neg_off, torch.int64)
    _lib.check(lib.dcnr_requests_sources(
        desc, d_rv.data_ptr(), d_md.data_ptr(), R, N_ITEMS, d_po.data_ptr(), Q, pos.data_ptr(),
        d_no.data_ptr(), neg_lo, neg_hi, neg.data_ptr(), counts.data_ptr(), status.data_ptr(),
        h_counts.data_ptr(), h_status.data_ptr(), _lib.stream_ptr(dev)), "dcnr_requests_sources")
    torch.cuda.current_stream(dev).synchronize()
    assert torch.equal(h_counts, counts.cpu()) and torch.equal(h_status, status.cpu())
    return (pos.cpu().numpy(), pos_off, neg.cpu().numpy(), neg_off,
            counts.cpu().numpy().reshape(R, 2), status.cpu().numpy())


def check_sources(store, rv, md, out, skip=()):
    pos, pos_off, neg, neg_off, counts, status = out
    for r in range(len(rv)):
        if r in skip:
            continue
        want_pos, want_neg = store.sources_host(int(rv[r]), int(md[r]))
        assert status[r] == 0 and counts[r].tolist() == [want_pos.size, want_neg.size], r
        for buf, off, want in ((pos, pos_off, want_pos), (neg, neg_off, want_neg)):
            seg = buf[off[r]:off[r + 1]]
            assert seg[:want.size].tolist() == want.tolist(), r
            assert (seg[want.size:] == (want[-1] if want.size else 0)).all(), r   # only repeats
    # words outside the segments: untouched
    assert (pos[pos_off[-1]:] == -7).all() and (neg[:neg_off[0]] == -7).all()
    assert (neg[neg_off[-1]:] == -7).all()


@pytest.mark.parametrize("R", [1, 7, 70])
def test_sources_equal_sources_host(dev, R):
    store = get_store()
    desc, _ = store.on(dev)
    q = mixed_requests(R, seed=R)
    rv = np.array(q["rv"] if R > 1 else [X], np.int64)
    md = np.array([0 if m == "friends" else 1 for m in q["modes"]], np.int32)
    _, _, pos_b, neg_b, _, _, _ = store.bounds(rv, md)
    out = c_sources(dev, desc, rv, md, pos_b, neg_b)
    check_sources(store, rv, md, out)
    if R >= 7:   # unknown, friends without reviews, no friends: empty sets
        assert out[4][:3].tolist() == [[0, 0]] * 3
        # the bound is not the count: some tail is padding
        assert (pos_b > out[4][:, 0]).any() and (pos_b >= out[4][:, 0]).all()


# --------------------------------- 2, 3: against recommend_many(sources_host)
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_recommend_users_equals_recommend_many(dev, precision):
    pipe, store = get_pipe(dev, precision), get_store()
    q = mixed_requests(40, seed=5)
    want = yardstick(pipe, store, q)
    assert sum(w[0].numel() > 0 for w in want) > 20 and any(w[0].numel() == 0 for w in want)
    res = run_users(pipe, store, q)
    assert not res.on_host.any()
    assert_same(res, want, precision)
    assert assert_recommended_by(res, store, q, precision) > 40
    # registered city sets: an allowed half and a fallback list, by index and mixed with None
    rng = np.random.default_rng(8)
    half, popular = pipe.register_sets([rng.choice(N_ITEMS, N_ITEMS // 2, replace=False),
                                        rng.choice(N_ITEMS, 100, replace=False)])
    allowed = [half if r % 3 else None for r in range(40)]
    fallback = [popular if r % 4 else None for r in range(40)]
    want = yardstick(pipe, store, q, allowed, fallback)
    res = run_users(pipe, store, q, allowed, fallback)
    assert_same(res, want, precision + " sets")
    assert_recommended_by(res, store, q, precision + " sets")
    # one mode for all; the lists left out
    q1 = dict(q, modes=["personal"] * 40)
    res = pipe.recommend_users(store, q["users"], q["rv"], "personal", q["lam"], q["top_k"],
                               recommended_by=False)
    assert_same(res, yardstick(pipe, store, q1), precision + " personal")
    assert res.by_reviewers.numel() == 0 and not res.by_count.any()
    assert res.to_lists(5)[2] == [[] for _ in res[5][0]]


def test_recommended_by_cases(dev):
    pipe, store = get_pipe(dev, "bf16"), get_store()
    # X in both modes, the whole list (lambda 1) and an MMR answer shorter than the candidates
    q = dict(users=[1, 2, 3, 4], rv=[X, X, X, -1], modes=["friends", "personal", "friends", "friends"],
             lam=[1.0, 1.0, 0.3, 1.0], top_k=[20, 20, 5, 20])
    res = run_users(pipe, store, q)
    assert_same(res, yardstick(pipe, store, q))
    assert_recommended_by(res, store, q)
    rows, _, by = res.to_lists(0)
    assert by[rows.index(HOTEL)][:2] == [A, B]        # first review rows 1000 < 2000, although A > B
    # personal mode: X's own positives lead to the candidates, X's friends to the lists
    rows_p, _, by_p = res.to_lists(1)
    assert by_p[rows_p.index(HOTEL)][:2] == [A, B] and not res.on_host.any()
    # the MMR answer: 5 positions reported of a longer segment
    assert res[2][0].numel() == 5 and res._seg[3] - res._seg[2] > 5
    assert res[3][0].numel() == 0


# ------------------------------------------------------------- 4: the fixtures
def _fixture_pipe(f, dev):
    import dcnr
    m = dcnr.DCN_RecSys(f.n_users, f.n_items, f.cat_dims, f.n_num, dict(f.params),
                        precision="fp32")
    m.load_state_dict(f.state)
    return dcnr.RankingPipeline(m.to(dev).eval(), f.item_cat, f.item_num,
                                item_embeddings=torch.from_numpy(f.emb).to(dev))


def _fixture_call(f, dev):
    """Every request of a fixture in one call; the host steps that remain with
    the caller (city sets, the id maps, main.py:217's user row) restated."""
    pipe = _fixture_pipe(f, dev)
    store, reviewer, ids = f11_common.store_of(f)
    reqs = f.expected["recommendations"]
    rows = [f7_common.request_rows(f, q) for q in reqs]
    city_sets = {}
    for q, r in zip(reqs, rows):
        if q["city"] not in city_sets:
            city_sets[q["city"]] = tuple(pipe.register_sets([r["allowed"], r["fallback"]]))
    res = pipe.recommend_users(store, [r["user_row"] for r in rows],
                               [reviewer.get(q["user_id"], -1) for q in reqs],
                               [q["type"] for q in reqs],
                               lambda_param=[q["lambda_param"] for q in reqs],
                               allowed=[city_sets[q["city"]][0] for q in reqs],
                               fallback=[city_sets[q["city"]][1] for q in reqs])
    return reqs, res, ids


def test_f11_in_one_call(dev):
    f = f11_common.load()
    reqs, res, ids = _fixture_call(f, dev)
    n_by = 0
    for r, q in enumerate(reqs):
        rows, _, by = res.to_lists(r)
        assert [f.rev[x] for x in rows] == q["ranked_hotels"], q
        assert [[int(ids[x]) for x in lst] for lst in by] == q["recommended_by"], q
        n_by += sum(len(b) for b in by)
    assert n_by >= 10 and [112, 111] in reqs[0]["recommended_by"]
    assert any(len(q["ranked_hotels"]) == 0 for q in reqs)


def test_f7_in_one_call(dev):
    f = f7_common.load()
    reqs, res, _ = _fixture_call(f, dev)
    for q, (ranked, _) in zip(reqs, res):
        assert [f.rev[x] for x in ranked.tolist()] == q["ranked_hotels"], q


# ---------------------------------------------------------------- 5: capacity
def hub_store():
    """Reviewer 0: 64 friends with 64 reviews each, SV_MAX staged rows exactly.
    Reviewer 1: 70 friends with 60 reviews each, 4200.  Reviewer 2: 400
    distinct positives of its own (x n_neighbors = 4400 staged candidates).
    Five positives and twelve negatives per friend of 0 and 1: their bounds of
    positives stay below SV_MAX / n_neighbors, and more than 1024 classed rows
    are staged and sorted.  Reviewer 3: 30 positives of its own and 64 friends
    whose 64 reviews are all positive -- a personal request of 3 sorts a few
    thousand (position, reviewer, row) entries for its recommended_by lists."""
    import dcnr
    rng = np.random.default_rng(6)
    rev, item, rating, fa, fb = [], [], [], [], []
    nxt = 4
    for hub, n_fr, n_rev, marks in ((0, 64, 64, [9] * 5 + [2] * 12), (1, 70, 60, [9] * 5 + [2] * 12),
                                    (3, 64, 64, [9] * 64)):
        for _ in range(n_fr):
            fa.append(hub)
            fb.append(nxt)
            rev += [nxt] * n_rev
            item += rng.choice(N_ITEMS, n_rev, replace=False).tolist()
            rating += rng.permutation(marks + [6] * (n_rev - len(marks))).tolist()
            nxt += 1
    for who, cnt in ((2, 400), (3, 30)):
        rev += [who] * cnt
        item += rng.choice(N_ITEMS, cnt, replace=False).tolist()
        rating += [10] * cnt
    order = rng.permutation(len(rev))
    pick = lambda a: np.asarray(a)[order]
    return dcnr.InteractionStore(pick(rev), pick(item), pick(rating), fa, fb, n_items=N_ITEMS)


def test_capacity_from_sv_max(dev):
    pipe, store = get_pipe(dev, "bf16"), hub_store()
    assert store.friends_rows[0] == SV_MAX and store.friends_rows[1] == 4200
    assert store.friends_pos[0] * pipe.n_neighbors <= SV_MAX
    assert store.n_pos[2] * pipe.n_neighbors > SV_MAX >= store.n_rows[2]
    assert store.friends_rows[3] == SV_MAX and store.friends_pos[3] == SV_MAX
    q = dict(users=[5, 6, 7, 8, 9], rv=[0, 1, 2, 0, 3],
             modes=["friends", "friends", "personal", "personal", "personal"],
             lam=[0.3, 1.0, 1.0, 1.0, 1.0], top_k=[20] * 5)
    res = run_users(pipe, store, q)
    assert res.on_host.tolist() == [False, True, True, False, False]
    assert_same(res, yardstick(pipe, store, q), "capacity")
    assert res[0][0].numel() == 20 and res[1][0].numel() > 20 and res[2][0].numel() >= 400
    assert assert_recommended_by(res, store, q, "capacity") > 1024
    o = int(res._seg[4])
    assert int(res.by_count[o:o + res[4][0].numel()].sum()) > 1024     # sorted on the device
    # with a fallback list named by every request, the spliced ones included
    fb = pipe.register_sets([np.arange(0, N_ITEMS, 5)]) * 5
    with_fb = run_users(pipe, store, q, None, fb)
    assert_same(with_fb, yardstick(pipe, store, q, None, fb), "capacity, fallback")
    assert with_fb[3][0].numel() == 100 and res[3][0].numel() == 0
    # the padding the bound costs, as the call reports it
    assert res.n_positives[0] == store.sources_host(0, "friends")[0].size
    assert res.positives_bound[0] == store.friends_pos[0] >= res.n_positives[0]
    # the raw status bits: 4200 staged rows overflow, 4096 do not
    desc, _ = store.on(dev)
    rv, md = np.array([0, 1], np.int64), np.zeros(2, np.int32)
    _, _, pos_b, neg_b, _, _, _ = store.bounds(rv, md)
    out = c_sources(dev, desc, rv, md, pos_b, neg_b)
    assert out[5].tolist() == [0, OVERFLOW] and out[4][1].tolist() == [0, 0]
    check_sources(store, rv, md, out, skip={1})
    assert (out[0][out[1][1]:out[1][2]] == -1).all() and (out[2][out[3][1]:out[3][2]] == -1).all()


# ---------------------------------------------------------- 6: corrupted data
def test_corrupted_store_ends_that_request_alone(dev):
    """A friend index >= U and a review offset past M, in device copies of the
    store.  store_friends / store_reviews (csrc/serving.hip) compare every
    offset pair and every friend index with U, M and the friend rows' length,
    passed by value, before the first access through them: the request ends
    with DCNR_REQ_BAD_DATA, nothing is read or written outside the buffers."""
    from dcnr import _lib
    lib = _lib.load()
    store = get_store()
    desc, t = store.on(dev)
    good = [u for u in range(20, 200) if store.n_friends[u] > 1 and store.n_pos[u] > 0 and
            store.sources_host(u, 0)[0].size >= 2]
    v_friend, v_off = good[:2]
    # the review offset shared by v_off and v_off + 1 is the corrupted one: the
    # two untouched requests stay away from both reviewers
    ok1, ok2 = [u for u in good[2:] if abs(u - v_off) > 1 and
                not {v_off, v_off + 1} & set(store.friends_host(u).tolist())][:2]
    fr = t["friend_rows"].clone()
    fr[int(store.friend_offsets[v_friend])] = U + 5                     # a friend index >= U
    ro = t["review_offsets"].clone()
    ro[v_off + 1] = store.n_reviews + 1000                              # a review offset past M
    bad = _lib.Interactions(U, t["friend_offsets"].data_ptr(), fr.data_ptr(), fr.numel(),
                            ro.data_ptr(), t["review_items"].data_ptr(),
                            t["review_rows"].data_ptr(), store.n_reviews)
    rv =np.array([v_friend, ok1, v_off, ok2], np.int64)
    md = np.array([0, 0, 1, 1], np.int32)
    _, _, pos_b, neg_b, _, _, by_b = store.bounds(rv, md)
    out = c_sources(dev, bad, rv, md, pos_b, neg_b)
    assert out[5].tolist() == [BAD_DATA, 0, BAD_DATA, 0]
    check_sources(store, rv, md, out, skip={0, 2})
    for r in (0, 2):
        assert out[4][r].tolist() == [0, 0]
        assert (out[0][out[1][r]:out[1][r + 1]] == -1).all()
    # the recommended_by kernel reads the same store: two positions per request
    tt = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    rvb = np.array([v_friend, ok1], np.int64)
    _, _, _, _, _, _, by_b = store.bounds(rvb, np.zeros(2, np.int32))
    ranked = [store.sources_host(int(u), 0)[0][:2] for u in rvb]
    assert all(len(x) == 2 for x in ranked)
    n, L = 4, int(by_b.sum())
    out_rows, offsets = tt(np.concatenate(ranked), torch.int64), tt([0, 2, 4], torch.int64)
    out_count, list_off = tt([2, 2], torch.int32), tt(np.r_[0, np.cumsum(by_b)], torch.int64)
    lists = torch.full((L,), -7, dtype=torch.int32, device=dev)
    by_rev = torch.full((L,), -7, dtype=torch.int32, device=dev)
    by_cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
    by_off = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    status = torch.full((2,), -7, dtype=torch.int32, device=dev)
    d_rv = tt(rvb, torch.int32)
    _lib.check(lib.dcnr_requests_recommended_by(
        bad, d_rv.data_ptr(), 2, N_ITEMS, out_rows.data_ptr(), n, offsets.data_ptr(),
        out_count.data_ptr(), list_off.data_ptr(), L, lists.data_ptr(), by_cnt.data_ptr(),
        by_off.data_ptr(), by_rev.data_ptr(), status.data_ptr(), _lib.stream_ptr(dev)),
        "dcnr_requests_recommended_by")
    want = store.recommended_by_host(int(ok1), ranked[1].tolist())
    assert status.tolist() == [BAD_DATA, 0]
    assert by_cnt.tolist() == [0, 0] + [len(b) for b in want]
    assert by_off.tolist() == np.r_[0, np.cumsum(by_cnt.tolist())].tolist()
    assert by_rev[:int(by_off[-1])].tolist() == [x for b in want for x in b]
    assert (by_rev[int(by_off[-1]):] == -1).all() and sum(map(len, want)) > 0
    assert (lists[:int(by_b[0])] == -1).all()


def test_host_validation(dev):
    import dcnr
    pipe, store = get_pipe(dev, "bf16"), get_store()
    assert len(pipe.recommend_users(store, [], [], "friends")) == 0
    with pytest.raises(ValueError):
        pipe.recommend_users(store, [0], [U], "friends")               # reviewer outside the store
    with pytest.raises(ValueError):
        pipe.recommend_users(store, [0], [-2], "friends")
    with pytest.raises(ValueError):
        pipe.recommend_users(store, [0, 1], [3], "friends")
    with pytest.raises(ValueError):
        pipe.recommend_users(store, [0], [3], "family")
    with pytest.raises(ValueError):
        pipe.recommend_users(store, [CFG["n_users"]], [3], "friends")  # user outside the table
    wide = dcnr.InteractionStore([0], [N_ITEMS], [9], [], [], n_items=N_ITEMS + 1)
    with pytest.raises(ValueError):
        pipe.recommend_users(wide, [0], [0], "personal")               # hotel rows the pipeline lacks


# ------------------------------------------------------- 7: streams, threads
def test_other_stream_and_two_threads(dev):
    pipe, store = get_pipe(dev, "bf16"), get_store()
    q_a, q_b = mixed_requests(24, seed=31), mixed_requests(17, seed=32)
    snap = lambda res: ([(r.clone(), z.clone()) for r, z in res],
                        [res.to_lists(r)[2] for r in range(len(res))])
    want_a, want_b = snap(run_users(pipe, store, q_a)), snap(run_users(pipe, store, q_b))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        x = torch.randn(2048, 2048, device=dev)
        for _ in range(8):
            x = x @ x * 1e-3
        got = snap(run_users(pipe, store, q_a))
    side.synchronize()
    assert_same(got[0], want_a[0], "side stream")
    assert got[1] == want_a[1]
    out, errors = {}, []
    start = threading.Barrier(2)

    def worker(name, q, own_stream):
        try:
            start.wait()
            for _ in range(3):
                if own_stream:
                    s = torch.cuda.Stream(dev)
                    with torch.cuda.stream(s):
                        out[name] = snap(run_users(pipe, store, q))
                    s.synchronize()
                else:
                    out[name] = snap(run_users(pipe, store, q))
        except BaseException as e:   # noqa: BLE001 -- reported by the main thread
            errors.append((name, e))

    ths = [threading.Thread(target=worker, args=("a", q_a, False)),
           threading.Thread(target=worker, args=("b", q_b, True))]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in ths), "a thread hung"
    assert not errors, errors
    torch.cuda.synchronize()
    for name, want in (("a", want_a), ("b", want_b)):
        assert_same(out[name][0], want[0], "thread " + name)
        assert out[name][1] == want[1]
