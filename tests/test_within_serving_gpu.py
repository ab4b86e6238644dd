"""Set-scoped neighbours through dcnr.RankingPipeline: ``within`` of
similar_items / similar_items_many / candidates and ``neighbors_within`` of
recommend / recommend_many / recommend_users.

A small model over 3000 hotels with 16-wide embeddings, n_neighbors = 11 and
six registered "city" sets of 5, 9, 10, 11, 200 and 1500 rows: below, at and
above the 10 neighbours a positive asks for (the short and padded returns),
one of a few waves and one of two chunks.  The brute force is torch's cosine
distance restricted to the set, compared by test_knn_paths_gpu's rule: row ids
at the positions whose distance has no neighbour within ATOL."""
import numpy as np
import pytest
import torch

import test_knn_paths_gpu as kp
import test_recommend_users_gpu as ru
from helpers import our_model

pytestmark = pytest.mark.gpu

N_ITEMS, K = 3000, 11
SIZES = (5, 9, 10, 11, 200, 1500)
CFG = dict(n_users=200, n_items=N_ITEMS, cat_dims={"a": 30, "b": 250}, n_num=4,
           params=dict(emb_dim=16, hidden_dim=64, n_cross_layers=2, n_res_blocks=2, dropout=0.0))
_cache = {}


def city_sets():
    rng = np.random.default_rng(11)
    return [np.sort(rng.choice(N_ITEMS, n, replace=False)) for n in SIZES]


def get_pipe(dev, table=False):
    import dcnr
    if table not in _cache:
        m = our_model(CFG, precision="fp32", seed=9).to(dev).eval()
        rng = np.random.default_rng(2)
        item_cat = np.stack([rng.integers(0, c, N_ITEMS) for c in CFG["cat_dims"].values()], 1)
        item_num = rng.random((N_ITEMS, 4), dtype=np.float32)
        pipe = dcnr.RankingPipeline(m, item_cat, item_num, n_neighbors=K, neighbor_table=table)
        pipe.cities = pipe.register_sets(city_sets())
        _cache[table] = pipe
    return _cache[table]


def brute_within(pipe, item, rows, n):
    """(distances, rows) of the n nearest of `rows` other than `item`, torch fp32."""
    t = pipe.index._table
    rows = np.asarray(rows, np.int64)
    rows = rows[rows != item]
    n = min(n, rows.size)
    if n == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.int64)
    sub = t[torch.from_numpy(rows).to(t.device)]
    ref_d, ref_i = kp.reference(sub, t[item:item + 1], n)
    return ref_d[0], rows[ref_i[0]]


def check_isolated(got, ref_d, ref_rows):
    assert got.shape == ref_rows.shape
    near = np.diff(ref_d) <= kp.ATOL
    iso = np.ones(ref_d.size, bool)
    iso[1:] &= ~near
    iso[:-1] &= ~near
    np.testing.assert_array_equal(got[iso], ref_rows[iso])
    return int(iso.sum()), iso.size


def test_similar_items_within(dev):
    pipe = get_pipe(dev)
    sets = city_sets()
    n_iso = n_all = 0
    for s, rows in zip(pipe.cities, sets):
        inside = int(rows[len(rows) // 2])
        outside = int(np.setdiff1d(np.arange(N_ITEMS), rows)[17])
        for item in (inside, outside):
            got = pipe.similar_items(item, 10, within=s).cpu().numpy()
            ref_d, ref_rows = brute_within(pipe, item, rows, 10)
            assert got.size == min(10, rows.size - (item == inside))   # short below 10 rows
            assert item not in got.tolist() and set(got.tolist()) <= set(rows.tolist())
            a, b = check_isolated(got, ref_d, ref_rows)
            n_iso, n_all = n_iso + a, n_all + b
            # the rows uploaded for the call instead of the registered set
            assert pipe.similar_items(item, 10, within=rows.tolist()).tolist() == got.tolist()
    assert n_iso >= 0.95 * n_all
    # without the argument: the parent path
    assert torch.equal(pipe.similar_items(7, 10), pipe.similar_items_many([7], 10)[0])


@pytest.mark.parametrize("table", [False, True])
def test_similar_items_many_within(dev, table):
    pipe = get_pipe(dev, table)
    sets = city_sets()
    c = pipe.cities
    items = [int(sets[4][3]), 5, int(sets[0][1]), 2999, int(sets[5][700]), 12, 13, int(sets[2][0]), 77]
    adhoc = np.array([900, 3, 77, 1500, 2000, 41, 1999])
    within = [c[4], c[4], c[0], None, c[5], adhoc, None, c[2], adhoc]
    got = pipe.similar_items_many(items, 10, within=within)
    assert got.shape == (9, 10) and got.dtype == torch.int64
    glob = pipe.similar_items_many(items, 10)
    for r, (item, w) in enumerate(zip(items, within)):
        if w is None:
            assert torch.equal(got[r], glob[r])
            continue
        one = pipe.similar_items(item, 10, within=w)
        assert torch.equal(got[r, :one.numel()], one) and bool((got[r, one.numel():] == -1).all())
    assert got[2, 4:].tolist() == [-1] * 6 and got[8, 6:].tolist() == [-1] * 4   # 5 - 1 and 7 - 1 rows
    # one set for every query: an index, or rows that are no list
    for w in (c[3], adhoc):
        all_ = pipe.similar_items_many(items, 10, within=w)
        for r, item in enumerate(items):
            one = pipe.similar_items(item, 10, within=w)
            assert torch.equal(all_[r, :one.numel()], one) and bool((all_[r, one.numel():] == -1).all())
    with pytest.raises(ValueError):
        pipe.similar_items_many(items, 10, within=[c[0]] * 3)
    with pytest.raises(ValueError):
        pipe.similar_items_many(items, 10, within=len(SIZES) + 50)
    with pytest.raises(ValueError):
        pipe.similar_items(3, 10, within=[1, N_ITEMS])


def test_candidates_within(dev):
    pipe, tpipe = get_pipe(dev), get_pipe(dev, True)
    sets = city_sets()
    pos = [int(sets[4][0]), 1234, int(sets[5][9]), 8, 1234]
    for s, rows in zip(pipe.cities, sets):
        d_pos = torch.tensor(pos, dtype=torch.int64, device=dev)
        i64 = lambda *a: torch.tensor(a, dtype=torch.int64, device=dev)
        _, idx = pipe.index.kneighbors_within_device(
            pipe.index._table[d_pos], K - 1, torch.from_numpy(rows).to(dev), i64(0, rows.size),
            i64(0, len(pos)), torch.zeros(1, dtype=torch.int32, device=dev), rows.size, exclude=d_pos)
        want = sorted((set(idx.cpu().numpy().reshape(-1).tolist()) | set(pos)) - {-1})
        assert set(want) - set(pos) <= set(rows.tolist())
        for p in (pipe, tpipe):
            assert p.candidates(pos, within=s).tolist() == want
            assert p.candidates(pos, within=rows).tolist() == want
    assert pipe.candidates([], within=pipe.cities[0]).numel() == 0
    assert torch.equal(pipe.candidates(pos), tpipe.candidates(pos))


def requests(pipe):
    """R = 7: None, registered sets (two requests share one), an ad-hoc row
    list, a request without positives; allowed = the same sets; a fallback on
    two; lambda 1.0 and 0.7."""
    c, sets = pipe.cities, city_sets()
    rng = np.random.default_rng(23)
    adhoc = np.sort(rng.choice(N_ITEMS, 120, replace=False)).tolist()
    popular = np.sort(rng.choice(N_ITEMS, 30, replace=False)).tolist()
    within = [None, c[5], c[4], c[5], adhoc, c[1], c[4]]
    n_pos = [3, 8, 5, 11, 4, 2, 0]
    return dict(users=rng.integers(0, CFG["n_users"], 7).tolist(),
                pos=[rng.choice(N_ITEMS, n, replace=False).tolist() for n in n_pos],
                lam=[1.0, 0.7, 1.0, 0.7, 0.7, 1.0, 0.7], within=within, allowed=list(within),
                fallback=[None, None, popular, None, None, popular, popular])


def run_many(pipe, q, **kw):
    return pipe.recommend_many(q["users"], q["pos"], lambda_param=q["lam"], top_k=8, allowed=q["allowed"],
                               fallback=q["fallback"], neighbors_within=q["within"], **kw)


def run_single(pipe, q, r):
    arg = lambda v: pipe._set_arg(v)
    return pipe.recommend(q["users"][r], q["pos"][r], lambda_param=q["lam"][r], top_k=8,
                          allowed=arg(q["allowed"][r]), fallback=arg(q["fallback"][r]),
                          neighbors_within=q["within"][r])


def test_recommend_many_neighbors_within(dev):
    pipe, tpipe = get_pipe(dev), get_pipe(dev, True)
    q = requests(pipe)
    want = [run_single(pipe, q, r) for r in range(7)]
    got = run_many(pipe, q)
    ru.assert_same(got, want, "scan")
    assert sum(w[0].numel() > 0 for w in want) >= 5
    # the scoped requests' candidates lie inside their sets (allowed = the same set), and the
    # scope matters: without it request 1 finds other rows
    plain = pipe.recommend_many(q["users"], q["pos"], lambda_param=q["lam"], top_k=8,
                                allowed=q["allowed"], fallback=q["fallback"])
    assert torch.equal(plain[0][0], got[0][0])
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(plain[1:], got[1:]))
    # the pipeline with a neighbour table: scoped requests by the scan, the rest by lookup
    ru.assert_same(run_many(tpipe, q), want, "neighbour table")
    ru.assert_same([run_single(tpipe, q, r) for r in range(7)], want, "neighbour table, single")
    # every request scoped: no global search at all
    q2 = dict(q, within=[pipe.cities[5]] + q["within"][1:], allowed=[pipe.cities[5]] + q["allowed"][1:])
    ru.assert_same(run_many(pipe, q2), [run_single(pipe, q2, r) for r in range(7)], "all scoped")
    # the sweep passes the argument through
    sweep = pipe.lambda_sweep(q["users"], q["pos"], [1.0, 0.7], top_k=8, allowed=q["allowed"],
                              fallback=q["fallback"], neighbors_within=q["within"], ks=(5, 8))
    for j, lam in enumerate((1.0, 0.7)):
        many = pipe.recommend_many(q["users"], q["pos"], lambda_param=lam, top_k=8, allowed=q["allowed"],
                                   fallback=q["fallback"], neighbors_within=q["within"])
        ru.assert_same(sweep[j][0], many, f"sweep {lam}")
    with pytest.raises(ValueError):
        pipe.recommend_many(q["users"], q["pos"], neighbors_within=[None] * 3)


def test_recommend_many_defaults_unchanged(dev):
    """Every new argument at its default: the rows and logits of the untouched recommend()."""
    pipe = get_pipe(dev)
    q = requests(pipe)
    got = pipe.recommend_many(q["users"], q["pos"], lambda_param=q["lam"], top_k=8, allowed=q["allowed"],
                              fallback=q["fallback"])
    want = [pipe.recommend(q["users"][r], q["pos"][r], lambda_param=q["lam"][r], top_k=8,
                           allowed=pipe._set_arg(q["allowed"][r]), fallback=pipe._set_arg(q["fallback"][r]))
            for r in range(7)]
    ru.assert_same(got, want)
    ru.assert_same(pipe.recommend_many(q["users"], q["pos"], lambda_param=q["lam"], top_k=8,
                                       allowed=q["allowed"], fallback=q["fallback"],
                                       neighbors_within=[None] * 7), want, "all None")


def test_recommend_users_neighbors_within(dev):
    pipe, store = ru.get_pipe(dev, "fp32"), ru.get_store()
    rng = np.random.default_rng(31)
    towns = pipe.register_sets([np.sort(rng.choice(ru.N_ITEMS, n, replace=False)) for n in (6, 40, 250)])
    R = 12
    q = ru.mixed_requests(R, seed=3)
    adhoc = np.sort(rng.choice(ru.N_ITEMS, 90, replace=False)).tolist()
    within = [[towns[0], towns[1], None, towns[2], adhoc][r % 5] for r in range(R)]
    got = pipe.recommend_users(store, q["users"], q["rv"], q["modes"], lambda_param=q["lam"], top_k=q["top_k"],
                               allowed=within, neighbors_within=within)
    src = [store.sources_host(u, m) for u, m in zip(q["rv"], q["modes"])]
    want = pipe.recommend_many(q["users"], [s[0] for s in src], lambda_param=q["lam"], top_k=q["top_k"],
                               allowed=within, excluded=[s[1] for s in src], neighbors_within=within)
    ru.assert_same(got, want)
    assert sum(w[0].numel() > 0 for w in want) >= 4
