"""The city and popular-hotel sets on the device (dcnr_city_sets_build,
``dcnr.CitySets.on``, ``recommend_many`` / ``recommend_users`` with
``cities=``).  Every comparison is an equality.

  1  the kernel through the C ABI against the numpy model of
     tests/city_sets_common.py, every output inside sentinel-guarded buffers,
     every case twice with equal bits
  2  the device generations after every step of the CPU tests' sequences
     against the upload of a freshly built object; an older generation keeps
     its values
  3  requests by city code against the same calls given the host sets
  4  the F7 fixture served through ``cities=``: the reference service's ids
"""
import numpy as np
import pytest
import torch

import city_sets_common as cc
import f11_common
import f7_common
from helpers import our_model

pytestmark = pytest.mark.gpu

GUARD, SENT = 64, -7


# ------------------------------------------------ 1: the kernel, through the C ABI
def c_build(dev, item, city, key, row, n_items, C, top, cap):
    """dcnr_city_sets_build with every output (and the workspace) inside a
    sentinel-filled buffer with GUARD words to spare at both ends.  Returns the
    outputs' interiors; asserts the guards and the host mirrors."""
    from dcnr import _lib
    lib = _lib.load()
    M = len(item)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    d_item, d_city, d_key = t(item, torch.int32), t(city, torch.int32), t(key, torch.float64)
    d_row = t(row, torch.int32) if row is not None else None
    sizes = dict(off=(2 * C + 2, torch.int64), rows=(cap, torch.int64), top=(C * top, torch.int32),
                 st=(1, torch.int32))
    bufs = {k: torch.full((n + 2 * GUARD,), SENT, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
    h_off = torch.full((2 * C + 2 + 2 * GUARD,), SENT, dtype=torch.int64).pin_memory()
    h_st = torch.full((1 + 2 * GUARD,), SENT, dtype=torch.int32).pin_memory()
    nb = int(lib.dcnr_city_sets_workspace_size(M, n_items, C, top))
    assert nb > 0
    ws = torch.full((nb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    at = lambda b: b.data_ptr() + GUARD * b.element_size()
    p = lambda x: x.data_ptr() if x is not None and x.numel() else None
    _lib.check(lib.dcnr_city_sets_build(
        p(d_item), p(d_city), p(d_key), p(d_row), M, n_items, C, top, at(bufs["off"]), at(bufs["rows"]),
        cap, at(bufs["top"]), at(bufs["st"]), at(h_off), at(h_st), at(ws), nb, _lib.stream_ptr(dev)),
        "dcnr_city_sets_build")
    torch.cuda.current_stream(dev).synchronize()
    out = {}
    for k, b in list(bufs.items()) + [("h_off", h_off), ("h_st", h_st)]:
        a = b.cpu().numpy()
        assert (a[:GUARD] == SENT).all() and (a[a.size - GUARD:] == SENT).all(), f"guard of {k}"
        out[k] = a[GUARD:a.size - GUARD]
    w = ws.cpu().numpy()
    assert (w[:GUARD] == 0xA5).all() and (w[w.size - GUARD:] == 0xA5).all(), "guard of the workspace"
    assert np.array_equal(out["h_off"], out["off"]) and np.array_equal(out["h_st"], out["st"])
    return out


def check_case(dev, item, city, key, row, n_items, C, top, cap=None, spare=3):
    """Two runs with equal bits, both equal to the model."""
    item, city = np.asarray(item, np.int64), np.asarray(city, np.int64)
    key = np.asarray(key, np.float64)
    want_off, want_rows, want_top = cc.model(item, city, key,
                                             np.arange(item.size) if row is None else row, C, top)
    total = int(want_off[-1])
    cap = total + spare if cap is None else cap
    a = c_build(dev, item, city, key, row, n_items, C, top, cap)
    b = c_build(dev, item, city, key, row, n_items, C, top, cap)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{k} differs between two runs"
    assert np.array_equal(a["off"], want_off)
    assert np.array_equal(a["top"].reshape(C, top), want_top)
    if total <= cap:
        assert a["st"][0] == 0
        assert np.array_equal(a["rows"][:total], want_rows)
    else:   # the offsets are complete, what fits is right, the status says so
        assert a["st"][0] == cc.OVERFLOW
        assert np.array_equal(a["rows"][:cap], want_rows[:cap])
    return a


def one_city(M, seed, ties=True):
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 8, M).astype(np.float64) if ties else rng.random(M)
    return rng.integers(0, 50, M), np.zeros(M, np.int64), key


def sized_cities(sizes, n_items, seed):
    rng = np.random.default_rng(seed)
    city = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    return rng.integers(0, n_items, city.size), city, rng.integers(0, 5, city.size).astype(np.float64)


def test_empty_and_single(dev):
    z = np.zeros(0, np.int64)
    out = check_case(dev, z, z, np.zeros(0), None, 10, 3, 4)
    assert (out["off"] == 0).all() and (out["top"] == -1).all()
    check_case(dev, z, z, np.zeros(0), None, 10, 3, 4, cap=0)
    check_case(dev, [0], [0], [np.nan], None, 1, 1, 1)
    check_case(dev, [4], [0], [2.0], np.array([9]), 5, 1, 1)


# 63..65: a wave; 2047..2049: the head kernels' tile; 4095..4097: a sort unit
@pytest.mark.parametrize("M", [63, 64, 65])
def test_one_city_around_a_wave(dev, M):
    check_case(dev, *one_city(M, M), None, 50, 1, 10)
    check_case(dev, *one_city(M, M, ties=False), None, 50, 1, 100)


@pytest.mark.parametrize("M", [2047, 2048, 2049, 4095, 4096, 4097])
def test_three_cities_around_the_chunks(dev, M):
    item, city, key = cc.table(M, 3, 200, seed=M)
    check_case(dev, item, city, key, None, 200, 3, 100)


# 1, 17 and 34 sort units: the sort's totals kernel sums the units in 16
# segments, of one, two and three units here; 2, 33 and 67 tiles of heads for
# the one-workgroup scan of the tile counts
@pytest.mark.parametrize("M,C", [(4096, 300), (65537, 3), (135173, 300)])
def test_more_units_than_total_segments(dev, M, C):
    item, city, key = cc.table(M, C, 200, seed=M)
    check_case(dev, item, city, key, None, 200, C, 100)


def test_one_city_holds_everything(dev):
    check_case(dev, *one_city(20000, 5), None, 50, 1, 100)
    item, _, key = one_city(20000, 6, ties=False)
    check_case(dev, item, np.full(20000, 3), key, None, 50, 5, 100)   # ... the other four empty


def test_many_cities_short_of_top(dev):
    item, city, key = cc.table(5000, 300, 400, seed=8)
    city[::20] = 1                                             # one city above `top`
    sizes = np.bincount(city, minlength=300)
    assert (sizes == 0).any() and ((sizes > 0) & (sizes < 100)).sum() > 100 and (sizes > 100).any()
    pairs = np.unique(np.stack([item, city], 1), axis=0)
    assert np.unique(pairs[:, 0]).size < pairs.shape[0]        # hotels that appear in two cities
    check_case(dev, item, city, key, None, 400, 300, 100)


def test_most_cities(dev):
    rng = np.random.default_rng(9)
    M, C = 1000, 65536
    city = rng.integers(0, C, M)
    city[:3], city[3:40] = [0, C - 1, C - 1], 12345
    check_case(dev, rng.integers(0, 77, M), city, rng.integers(0, 3, M).astype(np.float64), None, 77, C, 100)


def test_top_256(dev):
    item, city, key = sized_cities([255, 256, 257, 1, 0, 600], 300, seed=10)
    check_case(dev, item, city, key, None, 300, 6, 256)
    check_case(dev, item, city, np.arange(item.size, dtype=np.float64), None, 300, 6, 256)


@pytest.mark.parametrize("keys", ["small", "equal", "nan", "special"])
def test_keys(dev, keys):
    rng = np.random.default_rng(12)
    M, C = 3000, 4
    item, city = rng.integers(0, 500, M), rng.integers(0, C, M)
    key = dict(small=rng.integers(0, 8, M).astype(np.float64), equal=np.full(M, 2.5),
               nan=np.full(M, np.nan), special=cc.SPECIAL[rng.integers(0, cc.SPECIAL.size, M)])[keys]
    if keys == "nan":   # both signs, several payloads: every NaN is equal and last
        key = key.view(np.uint64).copy()
        key[::3] |= np.uint64(1 << 63)
        key[::5] |= np.uint64(0xABC)
        key = key.view(np.float64)
        assert np.isnan(key).all()
    check_case(dev, item, city, key, None, 500, C, 20)


def test_largest_hotel_rows(dev):
    n_items = 1 << 29
    item = np.array([0, n_items - 1, n_items - 1, 0, 5, n_items - 2, n_items - 1, 0, 1, n_items - 1])
    city = np.array([0, 0, 1, 1, 2, 2, 0, 2, 1, 2])
    out = check_case(dev, item, city, np.arange(10) % 3, None, n_items, 3, 2)
    assert out["rows"].max() == n_items - 1
    from dcnr import _lib
    lib = _lib.load()
    # the workspace follows M, C and top, not the number of hotel rows
    assert lib.dcnr_city_sets_workspace_size(10, n_items, 3, 2) < (1 << 20)
    assert lib.dcnr_city_sets_workspace_size(10, n_items + 1, 3, 2) == 0
    assert lib.dcnr_city_sets_workspace_size(10, 5, 3, 257) == 0
    assert lib.dcnr_city_sets_workspace_size(10, 5, 65537, 2) == 0
    assert lib.dcnr_city_sets_workspace_size(2 ** 31 - 1, 5, 3, 2) == 0


def test_rows_with_gaps(dev):
    item, city, key = cc.table(1500, 6, 90, seed=13)
    row = np.cumsum(np.random.default_rng(1).integers(1, 9, 1500)) + 4
    a = check_case(dev, item, city, key, row, 90, 6, 30)
    b = check_case(dev, item, city, key, None, 90, 6, 30)
    assert np.array_equal(a["rows"], b["rows"]) and not np.array_equal(a["top"], b["top"])


def test_cap_one_short(dev):
    item, city, key = cc.table(1500, 6, 90, seed=14)
    total = int(cc.model(item, city, key, np.arange(1500), 6, 30)[0][-1])
    out = check_case(dev, item, city, key, None, 90, 6, 30, cap=total - 1)
    assert out["off"][-1] == total
    # ... and short by the whole popular family: no popular row is written
    check_case(dev, item, city, key, None, 90, 6, 30, cap=int(out["off"][6]))
    check_case(dev, item, city, key, None, 90, 6, 30, cap=1)


@pytest.mark.parametrize("what", ["city", "city_negative", "item", "item_negative", "row_order",
                                  "row_negative"])
def test_bad_data(dev, what):
    item, city, key = cc.table(1500, 6, 90, seed=15)
    row = np.arange(1500) * 2
    if what == "city":
        city[700] = 6
    elif what == "city_negative":
        city[0] = -3
    elif what == "item":
        item[1499] = 90
    elif what == "item_negative":
        item[5] = -1
    elif what == "row_order":
        row[100] = row[99]
    else:
        row[0] = -1
    # no access outside the buffers (c_build asserts the guards), the bit set
    out = c_build(dev, item, city, key, row, 90, 6, 30, cap=1500 + 6 * 30)
    assert out["st"][0] & cc.BAD_DATA


def test_bad_arguments(dev):
    from dcnr import _lib
    lib = _lib.load()
    nb = int(lib.dcnr_city_sets_workspace_size(4, 10, 2, 3))
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    ts = [z(4, torch.int32), z(4, torch.int32), z(4, torch.float64), z(6, torch.int64),
          z(16, torch.int64), z(6, torch.int32), z(1, torch.int32), z(nb, torch.uint8)]
    i_, c_, k_, off, rows, top, st, ws = (t.data_ptr() for t in ts)
    s = _lib.stream_ptr(dev)
    call = lambda *a: lib.dcnr_city_sets_build(*a, s)
    good = [i_, c_, k_, None, 4, 10, 2, 3, off, rows, 16, top, st, None, None, ws, nb]
    assert call(*good) == _lib.DCNR_OK
    torch.cuda.current_stream(dev).synchronize()
    for i, v, want in ((0, None, _lib.DCNR_BAD_ARG), (8, None, _lib.DCNR_BAD_ARG),
                       (4, -1, _lib.DCNR_BAD_ARG), (10, -1, _lib.DCNR_BAD_ARG),
                       (7, 0, _lib.DCNR_UNSUPPORTED_SHAPE), (7, 257, _lib.DCNR_UNSUPPORTED_SHAPE),
                       (6, 0, _lib.DCNR_UNSUPPORTED_SHAPE), (6, 65537, _lib.DCNR_UNSUPPORTED_SHAPE),
                       (5, (1 << 29) + 1, _lib.DCNR_UNSUPPORTED_SHAPE),
                       (16, 8, _lib.DCNR_WORKSPACE_TOO_SMALL)):
        bad = list(good)
        bad[i] = v
        assert call(*bad) == want, (i, v)


# ------------------------------------------------------------ 2: generations
GEN_TENSORS = ["set_rows", "set_offsets", "top_rows", "review_item", "review_city",
               "review_popularity", "review_row"]


def assert_generation(gen, want, what):
    for k in GEN_TENSORS:
        g, w = getattr(gen, k), getattr(want, k)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        # (bits: NaN popularity values compare equal to themselves)
        assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), (what, k)
    assert np.array_equal(gen.host_offsets, want.host_offsets), what
    assert np.array_equal(gen.host_offsets, gen.set_offsets.cpu().numpy()), what


@pytest.mark.parametrize("name,st,steps", cc.sequences(), ids=[s[0] for s in cc.sequences()])
def test_generations_follow_the_host(dev, name, st, steps):
    cs = st.fresh()
    gen = cs.on(dev)
    assert_generation(gen, st.fresh().on(dev), name)
    model = cc.model(st.item, st.city, st.key, st.row, cc.C, cc.TOP)
    assert np.array_equal(gen.host_offsets, model[0])
    assert np.array_equal(gen.set_rows.cpu().numpy(), model[1])
    assert np.array_equal(gen.top_rows.cpu().numpy(), model[2])
    for i, step in enumerate(steps):
        old = gen
        kept = {k: getattr(old, k).clone() for k in GEN_TENSORS}
        cc.do(cs, step)
        st.apply(step)
        gen = cs.on(dev)
        assert gen is not old
        assert_generation(gen, st.fresh().on(dev), f"{name}[{i}]")
        for k in GEN_TENSORS:   # the generation taken before the step still holds its values
            assert getattr(old, k).cpu().numpy().tobytes() == kept[k].cpu().numpy().tobytes(), (name, i, k)
        assert cs.last_update["devices"] == 1 and cs.last_update["upload_bytes"] > 0
    cc.assert_same(cs, st.fresh(), name)


def test_refused_calls_leave_the_device(dev):
    st = cc.State(*cc.base_table())
    cs = st.fresh()
    gen = cs.on(dev)
    for call in cc.refused(cs):
        with pytest.raises(ValueError):
            call()
        assert cs.on(dev) is gen
    cs.append()
    cs.remove([])
    assert cs.on(dev) is gen


def test_cap_retry(dev):
    """Every hotel in every city: the first guess of ``cap`` is too small and
    the build runs again with the size the offsets report."""
    import dcnr
    C, n_items = 12, 5
    item, city = np.tile(np.arange(n_items), C * 3), np.repeat(np.arange(C), n_items * 3)
    key = np.arange(item.size, dtype=np.float64) % 4
    cs = dcnr.CitySets(item, city, key, n_items=n_items, n_cities=C, top=2)
    gen = cs.on(dev)
    off, rows, top = cc.model(item, city, key, np.arange(item.size), C, 2)
    assert off[-1] > min(item.size, n_items) + min(item.size, C * 2)   # the first guess
    assert np.array_equal(gen.host_offsets, off) and np.array_equal(gen.set_rows.cpu().numpy(), rows)
    assert np.array_equal(gen.top_rows.cpu().numpy(), top)


# --------------------------------------------------------------- 3: requests
N_ITEMS, U, M, E, NC = 500, 300, 4000, 600, 8
CFG = dict(n_users=400, n_items=N_ITEMS, cat_dims={"a": 30, "b": 250}, n_num=4,
           params=dict(emb_dim=32, hidden_dim=64, n_cross_layers=2, n_res_blocks=2, dropout=0.0))
EMPTY_CITY, SMALL_CITY = 6, 7     # no rows; three rows of two hotels


def planted():
    """f11_common.random_tables with a city column: a hotel's city is its row
    mod 6, but for one review in 50 (hotels that appear in two cities); city 6
    has no rows, city 7 three."""
    rev, item, rating, fa, fb = f11_common.random_tables(U, M, E, N_ITEMS, seed=21)
    rng = np.random.default_rng(22)
    city = item % 6
    odd = rng.choice(M, M // 50, replace=False)
    city[odd] = rng.integers(0, 6, odd.size)
    city[[10, 20, 30]], item[[10, 20, 30]] = SMALL_CITY, [7, 7, 9]
    pop = rng.integers(0, 40, M).astype(np.float64)
    pop[rng.choice(M, 50, replace=False)] = np.nan
    return rev, item, rating, fa, fb, city, pop


_cache = {}


def setup(dev):
    import dcnr
    if "pipe" not in _cache:
        m = our_model(CFG, precision="fp32", seed=9).to(dev).eval()
        rng = np.random.default_rng(2)
        item_cat = np.stack([rng.integers(0, c, N_ITEMS) for c in CFG["cat_dims"].values()], 1)
        _cache["parts"] = (m, item_cat, rng.random((N_ITEMS, 4), dtype=np.float32))
        _cache["pipe"] = dcnr.RankingPipeline(*_cache["parts"])
        _cache["tables"] = planted()
    return _cache["pipe"], _cache["tables"]


def assert_answers(got, want, what):
    assert len(got) == len(want)
    for r, ((gr, gl), (wr, wl)) in enumerate(zip(got, want)):
        assert torch.equal(gr, wr), (what, r, gr.tolist(), wr.tolist())
        assert torch.equal(gl, wl), (what, r)


def requests(R, seed):
    rng = np.random.default_rng(seed)
    cities = rng.integers(0, 6, R)
    cities[:4] = [-1, EMPTY_CITY, SMALL_CITY, 2]
    rv = rng.integers(0, U, R)
    rv[0], rv[3] = 5, -1          # an unknown reviewer in a known city: the fallback fills the answer
    lam = np.where(np.arange(R) % 2 == 0, 1.0, 0.4)
    lam[5] = 1.0 - 1e-12          # rounds to 1.0f from below: answered on the host path
    return dict(users=rng.integers(0, CFG["n_users"], R), rv=rv, cities=cities, lam=lam,
                modes=["friends" if r % 3 else "personal" for r in range(R)],
                top_k=[[20, 5, 500][r % 3] for r in range(R)])


def check_requests(dev, pipe, store, cs, q, what):
    R = len(q["cities"])
    city_rows = [cs.city_rows_host(int(c)) for c in q["cities"]]
    pop_rows = [cs.popular_rows_host(int(c)) for c in q["cities"]]
    src = [store.sources_host(int(u), m) for u, m in zip(q["rv"], q["modes"])]
    for in_city in (False, True):
        within = city_rows if in_city else None
        kw = dict(lambda_param=q["lam"], top_k=q["top_k"])
        # recommend_many
        got = pipe.recommend_many(q["users"], [s[0] for s in src], excluded=[s[1] for s in src],
                                  city_sets=cs, cities=q["cities"], neighbors_in_city=in_city, **kw)
        want = pipe.recommend_many(q["users"], [s[0] for s in src], excluded=[s[1] for s in src],
                                   allowed=city_rows, fallback=pop_rows, neighbors_within=within, **kw)
        assert_answers(got, want, (what, "many", in_city))
        # recommend_users
        got_u = pipe.recommend_users(store, q["users"], q["rv"], q["modes"], city_sets=cs,
                                     cities=q["cities"], neighbors_in_city=in_city, **kw)
        want_u = pipe.recommend_users(store, q["users"], q["rv"], q["modes"], allowed=city_rows,
                                      fallback=pop_rows, neighbors_within=within, **kw)
        assert_answers(got_u, want_u, (what, "users", in_city))
        assert_answers(got_u, got, (what, "users against many", in_city))
        assert got_u._city_held is cs.on(dev)
        assert np.array_equal(got_u.on_host, want_u.on_host) and got_u.on_host[5] and \
            not got_u.on_host[:5].any()
        # the unknown city, the city without rows; the fallback alone fills request 3
        assert got[0][0].numel() == 0 and got[1][0].numel() == 0
        assert src[3][0].size == 0 and got[3][0].numel() > 0
        assert set(got[3][0].tolist()) <= set(pop_rows[3].tolist())
        assert set(got[2][0].tolist()) <= set(city_rows[2].tolist())
        assert sum(g[0].numel() > 0 for g in got) > R // 2
    return got


def test_requests_by_city(dev):
    import dcnr
    pipe, (rev, item, rating, fa, fb, city, pop) = setup(dev)
    store = dcnr.InteractionStore(rev, item, rating, fa, fb, n_items=N_ITEMS, n_reviewers=U)
    cs = dcnr.CitySets(item, city, pop, n_items=N_ITEMS, n_cities=NC)
    q = requests(24, seed=3)
    before = check_requests(dev, pipe, store, cs, q, "start")
    # registered sets in front of the generation's: the indices shift, the answers stay
    pipe2 = dcnr.RankingPipeline(*_cache["parts"])
    reg = pipe2.register_sets([[1, 2, 3], np.arange(100, 140)])
    for _ in range(2):   # (the second call finds the joined rows made by the first)
        again = pipe2.recommend_many(q["users"], [()] * 24, city_sets=cs, cities=q["cities"],
                                     excluded=[reg[1]] * 24, lambda_param=q["lam"], top_k=q["top_k"])
        want = pipe.recommend_many(q["users"], [()] * 24, excluded=[np.arange(100, 140)] * 24,
                                   allowed=[cs.city_rows_host(int(c)) for c in q["cities"]],
                                   fallback=[cs.popular_rows_host(int(c)) for c in q["cities"]],
                                   lambda_param=q["lam"], top_k=q["top_k"])
        assert_answers(again, want, "registered")
        assert sum(g[0].numel() > 0 for g in again) > 12
    # an append that gives SMALL_CITY a new hotel with the city's largest key, and
    # city 2 more rows than `top` keeps; a remove that takes hotel 9 out of SMALL_CITY
    c2 = np.flatnonzero(city == 2)
    new_item = np.r_[11, np.full(120, int(item[c2[0]]))]
    new_city = np.r_[SMALL_CITY, np.full(120, 2)]
    new_pop = np.r_[1e9, np.full(120, 1e6)]
    old_city, old_pop = cs.city_rows_host(SMALL_CITY).tolist(), cs.popular_rows_host(2).tolist()
    for obj, args in ((cs, (new_item, new_city, new_pop)),
                      (store, (np.zeros(121, np.int64), new_item, np.full(121, 9.0)))):
        obj.append(*args)
    assert cs.city_rows_host(SMALL_CITY).tolist() == [7, 9, 11] != old_city
    assert cs.popular_rows_host(2).tolist() == [int(item[c2[0]])] != old_pop
    after = check_requests(dev, pipe, store, cs, q, "appended")
    assert after[2][0].tolist() != before[2][0].tolist() or after[3][0].tolist() != before[3][0].tolist()
    cs.remove([30])
    store.remove([int(rev[30])], [30])
    assert cs.city_rows_host(SMALL_CITY).tolist() == [7, 11]
    check_requests(dev, pipe, store, cs, q, "removed")


def test_request_arguments(dev):
    import dcnr
    pipe, (rev, item, rating, fa, fb, city, pop) = setup(dev)
    cs = dcnr.CitySets(item, city, pop, n_items=N_ITEMS, n_cities=NC)
    for kw in (dict(cities=[0]), dict(city_sets=cs, cities=[0], allowed=[[1]]),
               dict(city_sets=cs, cities=[0], fallback=[[1]]), dict(city_sets=cs, cities=[NC]),
               dict(city_sets=cs, cities=[-2]), dict(city_sets=cs, cities=[0, 1]),
               dict(city_sets=cs, cities=[0], neighbors_in_city=True, neighbors_within=[[1]]),
               dict(neighbors_in_city=True)):
        with pytest.raises(ValueError):
            pipe.recommend_many([0], [[1]], **kw)
    # neighbors_within stays free without the flag
    a = pipe.recommend_many([0], [[1, 2]], city_sets=cs, cities=[1], neighbors_within=[[1, 7, 13, 19]])
    b = pipe.recommend_many([0], [[1, 2]], allowed=[cs.city_rows_host(1)],
                            fallback=[cs.popular_rows_host(1)], neighbors_within=[[1, 7, 13, 19]])
    assert_answers(a, b, "free neighbors_within")


# ----------------------------------------------------------- 4: F7 end to end
def test_f7_served_by_city_code(dev):
    import dcnr
    f = f7_common.load()
    m = dcnr.DCN_RecSys(f.n_users, f.n_items, f.cat_dims, f.n_num, dict(f.params), precision="fp32")
    m.load_state_dict(f.state)
    pipe = dcnr.RankingPipeline(m.to(dev).eval(), f.item_cat, f.item_num,
                                item_embeddings=torch.from_numpy(f.emb).to(dev))
    cs, code = cc.f7_city_sets(f)
    reqs = f.expected["recommendations"]
    rows = [f7_common.request_rows(f, req) for req in reqs]
    got = pipe.recommend_many([r["user_row"] for r in rows], [r["pos"] for r in rows],
                              lambda_param=[req["lambda_param"] for req in reqs],
                              excluded=[r["excluded"] for r in rows], city_sets=cs,
                              cities=[code.get(req["city"], -1) for req in reqs])
    for req, (ranked, _) in zip(reqs, got):
        assert [f.rev[x] for x in ranked.tolist()] == req["ranked_hotels"], req
    assert any(len(req["ranked_hotels"]) == 0 for req in reqs)
