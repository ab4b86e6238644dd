"""The hotel feature tables on the device (dcnr_item_features_build,
``dcnr.ItemFeatures.on``, ``RankingPipeline(item_features=...)``).  Every
comparison is an equality of bytes.

  1  the kernel through the C ABI against the numpy model of
     tests/item_features_common.py, every output and the workspace inside
     sentinel-guarded buffers, every case twice with equal bytes; bad data, bad
     arguments
  2  the device generations after every step of the CPU tests' sequences
     against the upload of a freshly built object; an older generation keeps
     its bytes; only the batch travels
  3  a pipeline on ``item_features=`` against one built from the host tables,
     at the start and after an append, a remove and an edit
  4  the F7 fixture served with ``item_features=``: the reference service's ids,
     and after every hotel's first row is removed the answers of a pipeline on
     the tables pandas derives from the rest
"""
import numpy as np
import pytest
import torch

import city_sets_common as cc
import f11_common
import f7_common
import item_features_common as ic
from helpers import our_model

pytestmark = pytest.mark.gpu

GUARD, SENT = 64, -7


# ------------------------------------------------ 1: the kernel, through the C ABI
def c_build(dev, item, row, cat, num, scale, mn, n_items, shift=0):
    """dcnr_item_features_build with every output (and the workspace) inside a
    sentinel-filled buffer with GUARD words to spare at both ends.  ``shift``:
    the review_item / review_row columns start that many words into their
    allocation (off the 16-byte alignment the four-row loads need).  Returns the
    outputs' interiors; asserts the guards and the host mirror."""
    from dcnr import _lib
    lib = _lib.load()
    M, n_cat, n_num = len(item), cat.shape[1], num.shape[1]

    def t(a, dt, lead=0):
        a = torch.as_tensor(np.ascontiguousarray(a), dtype=dt).reshape(-1)
        return torch.cat([torch.zeros(lead, dtype=dt), a]).to(dev)[lead:]
    d_item = t(item, torch.int32, shift)
    d_row = t(row, torch.int32, shift) if row is not None else None
    d_cat, d_num = t(cat, torch.int32), t(num, torch.float64)
    d_scale, d_min = t(scale, torch.float64), t(mn, torch.float64)
    sizes = dict(first=(n_items, torch.int32), cat=(n_items * n_cat, torch.int64),
                 num=(n_items * n_num, torch.int32), counts=(2, torch.int32))   # (num: float32 as bits)
    bufs = {k: torch.full((n + 2 * GUARD,), SENT, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
    h_counts = torch.full((2 + 2 * GUARD,), SENT, dtype=torch.int32).pin_memory()
    nb = int(lib.dcnr_item_features_workspace_size(M, n_items, n_cat, n_num))
    assert nb > 0
    ws = torch.full((nb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    at = lambda b: b.data_ptr() + GUARD * b.element_size()
    p = lambda x: x.data_ptr() if x is not None and x.numel() else None
    _lib.check(lib.dcnr_item_features_build(
        p(d_item), p(d_row), p(d_cat), p(d_num), p(d_scale), p(d_min), M, n_items, n_cat, n_num,
        at(bufs["first"]), at(bufs["cat"]), at(bufs["num"]), at(bufs["counts"]), at(h_counts), at(ws), nb,
        _lib.stream_ptr(dev)), "dcnr_item_features_build")
    torch.cuda.current_stream(dev).synchronize()
    out = {}
    for k, b in list(bufs.items()) + [("h_counts", h_counts)]:
        a = b.cpu().numpy()
        assert (a[:GUARD] == SENT).all() and (a[a.size - GUARD:] == SENT).all(), f"guard of {k}"
        out[k] = a[GUARD:a.size - GUARD]
    w = ws.cpu().numpy()
    assert (w[:GUARD] == 0xA5).all() and (w[w.size - GUARD:] == 0xA5).all(), "guard of the workspace"
    assert np.array_equal(out["h_counts"], out["counts"])
    out["num"] = out["num"].view(np.float32)
    return out


def check_case(dev, item, cat, num, scale, mn, n_items, row=None, shifts=(0, 1)):
    """Two runs with equal bytes, both equal to the model; then once more with the
    columns off their alignment (the one-row-per-lane scan)."""
    item = np.asarray(item, np.int64)
    M = item.size
    cat = np.zeros((M, 0), np.int64) if cat is None else np.asarray(cat, np.int64)     # [M, n_cat]
    num = np.zeros((M, 0)) if num is None else np.asarray(num, np.float64)               # [M, n_num]
    assert cat.shape[:1] == num.shape[:1] == (M,) and cat.ndim == num.ndim == 2
    scale, mn = np.asarray(scale, np.float64).reshape(-1), np.asarray(mn, np.float64).reshape(-1)
    first, w_cat, w_num, n_with = ic.model(item, np.arange(M) if row is None else row, cat, num, scale,
                                           mn, n_items)
    for shift in shifts:
        a = c_build(dev, item, row, cat, num, scale, mn, n_items, shift)
        b = c_build(dev, item, row, cat, num, scale, mn, n_items, shift)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), f"{k} differs between two runs"
        assert a["counts"].tolist() == [n_with, 0], shift
        assert a["first"].tobytes() == first.tobytes(), shift
        assert a["cat"].tobytes() == w_cat.tobytes(), shift
        bad = np.flatnonzero(a["num"].view(np.uint32) != w_num.reshape(-1).view(np.uint32))
        assert bad.size == 0, (shift, bad[:5], a["num"][bad[:5]], w_num.reshape(-1)[bad[:5]])
    return a


def rows_of(M, n_items, seed, n_cat=2, n_num=3):
    item, cat, num = ic.random_rows(M, seed, n_items, n_cat, n_num)
    rng = np.random.default_rng(seed + 1)
    return item, cat, num, rng.random(n_num) + 0.5, rng.random(n_num) - 0.5


def test_empty_and_single(dev):
    z = np.zeros(0, np.int64)
    out = check_case(dev, z, np.zeros((0, 2)), np.zeros((0, 3)), [1.0, 2.0, 3.0], [0.5, 0.5, 0.5], 10)
    assert (out["first"] == -1).all() and not out["cat"].any() and not out["num"].view(np.uint32).any()
    check_case(dev, [0], [[7, 8]], [[1.5, -2.0, np.nan]], [1.0, 2.0, 3.0], [0.5, 0.5, 0.5], 1)
    check_case(dev, [4], [[7, 8]], [[1.5, -2.0, 0.0]], [1.0, 2.0, 3.0], [0.5, 0.5, 0.5], 5,
               row=np.array([9]))


# 63..65: a wave; 1023..1025, 1027: a workgroup's step of the four-row scan and
# its M % 4 tail; 255..257: a workgroup's step of the one-row scan
@pytest.mark.parametrize("M", [2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027])
def test_around_the_steps(dev, M):
    item, cat, num, scale, mn = rows_of(M, 40, seed=M)
    check_case(dev, item, cat, num, scale, mn, 40)


def test_past_the_grids(dev):
    """More rows than one sweep of the scan's grid takes (2048 workgroups of 1024
    rows) and more hotels than one sweep of the gather's (2048 of 256)."""
    M, n_items = 2048 * 1024 + 1029, 2048 * 256 + 300
    rng = np.random.default_rng(3)
    item = rng.integers(1, n_items - 2, M)
    item[-1] = n_items - 2          # its only row: the table's last
    check_case(dev, item, None, rng.random((M, 1)), [2.0], [-1.0], n_items, shifts=(0,))
    check_case(dev, item[:600000], None, rng.random((600000, 1)), [2.0], [-1.0], n_items, shifts=(1,))


def test_one_hotel_table(dev):
    item, cat, num, scale, mn = rows_of(300, 1, seed=4)
    check_case(dev, item, cat, num, scale, mn, 1)


def test_hotels_without_rows_at_both_ends(dev):
    item, cat, num, scale, mn = rows_of(3000, 60, seed=5)
    out = check_case(dev, 20 + item % 25, cat, num, scale, mn, 70)
    assert (out["first"][:20] == -1).all() and (out["first"][45:] == -1).all()
    assert out["counts"][0] == 25


def test_one_hotel_holds_everything(dev):
    _, cat, num, scale, mn = rows_of(20000, 9, seed=6)
    out = check_case(dev, np.full(20000, 7), cat, num, scale, mn, 9)
    assert out["first"].tolist() == [-1] * 7 + [0, -1]


def test_reversed_by_hotel(dev):
    """Every hotel's rows in one run, the hotels descending: a hotel's first row
    lies as far back as its number is small."""
    item = np.repeat(np.arange(400)[::-1], 50)
    _, cat, num, scale, mn = rows_of(item.size, 400, seed=7)
    out = check_case(dev, item, cat, num, scale, mn, 400)
    assert out["first"].tolist() == (50 * np.arange(400)[::-1]).tolist()
    # ... and every hotel's only row, the hotels descending
    check_case(dev, np.arange(5000)[::-1], cat[:5000], num[:5000], scale, mn, 5000)


@pytest.mark.parametrize("n_cat,n_num", [(0, 3), (2, 0), (0, 0), (64, 64), (1, 1), (11, 2), (33, 17)])
def test_widths(dev, n_cat, n_num):
    item, cat, num, scale, mn = rows_of(700, 130, seed=8 + n_cat, n_cat=n_cat, n_num=n_num)
    check_case(dev, item, cat, num, scale, mn, 131)


def test_rows_with_gaps(dev):
    item, cat, num, scale, mn = rows_of(1500, 90, seed=13)
    row = np.cumsum(np.random.default_rng(1).integers(1, 9, 1500)) + 4
    a = check_case(dev, item, cat, num, scale, mn, 90, row=row)
    b = check_case(dev, item, cat, num, scale, mn, 90)
    assert a["num"].tobytes() == b["num"].tobytes() and not np.array_equal(a["first"], b["first"])
    assert np.array_equal(a["first"], row[b["first"]])
    big = np.arange(1500) * 1431655 + 7           # up to 2^31 - 1's neighbourhood
    assert big[-1] > 2 ** 31 - 2 ** 22
    check_case(dev, item, cat, num, scale, mn, 90, row=big)


def test_values_pass_as_numpy_passes_them(dev):
    """NaN of both signs with payloads (quiet ones: what a float64 operation
    returns for a signalling NaN is the platform's), +-inf, -0.0, denormals of
    both formats, values that overflow and underflow float32."""
    M = 4000
    item, cat, _, _, _ = rows_of(M, 1000, seed=14)
    rng = np.random.default_rng(15)
    bits = np.full(M, 0x7FF8000000000000, np.uint64)
    bits[::2] |= np.uint64(1 << 63)
    bits |= rng.integers(1, 1 << 51, M).astype(np.uint64)
    nan = bits.view(np.float64)
    assert np.isnan(nan).all()
    special = ic.SPECIAL[rng.integers(0, ic.SPECIAL.size, M)]
    tiny = rng.random(M) * 1e-38 * np.where(rng.random(M) < 0.5, 1, -1)   # float32 denormals
    edge = np.float64(np.finfo(np.float32).max) * (1 + (rng.random(M) - 0.5) * 1e-7)   # around the overflow
    num = np.stack([nan, special, tiny, edge, rng.random(M) * 5e-324 * 4], 1)
    # scales and offsets that make no NaN of their own (0 * inf, inf - inf): those carry
    # the sign of the platform's default NaN
    scale, mn = np.array([1.5, 2.0, 1.0, 1.0, 0.5]), np.array([1.0, 3.0, 0.0, 0.0, 0.0])
    out = check_case(dev, item, cat, num, scale, mn, 1000)
    got = out["num"].reshape(1000, 5)
    have = out["first"] >= 0
    assert np.isnan(got[have, 0]).all() and np.signbit(got[have, 0]).any() and \
        not np.signbit(got[have, 0]).all()
    assert np.isinf(got[have, 3]).any() and np.isfinite(got[have, 3]).any()
    assert ((got[have, 2] != 0) & (np.abs(got[have, 2]) < np.finfo(np.float32).tiny)).any()
    # -0.0 survives a scale and an offset of -0.0
    z = check_case(dev, [0, 1], None, [[-0.0], [0.0]], [3.0], [-0.0], 2)
    assert np.signbit(z["num"]).tolist() == [True, False]


def test_witness_column_is_not_fused(dev):
    """MinMaxScaler's two float64 roundings, not an fma's one: on this column the
    two end in different float32 values for some entries (asserted by exact
    arithmetic in the CPU test), so a build that contracts x * scale + min fails
    here."""
    x, scale, mn = ic.witness_column()
    out = check_case(dev, np.arange(x.size), None, x[:, None], [scale], [mn], x.size)
    fused = ic.fused_f32(x, scale, mn)
    assert (out["num"].view(np.uint32) != fused.view(np.uint32)).sum() >= 1


@pytest.mark.parametrize("what", ["item", "item_negative", "item_first", "row_order", "row_negative",
                                  "row_last"])
@pytest.mark.parametrize("shift", [0, 1])
def test_bad_data(dev, what, shift):
    item, cat, num, scale, mn = rows_of(1501, 90, seed=16)
    row = np.arange(1501) * 2
    if what == "item":
        item[1500] = 90
    elif what == "item_negative":
        item[5] = -2 ** 31
    elif what == "item_first":
        item[0] = 2 ** 31 - 1
    elif what == "row_order":
        row[100] = row[99]
    elif what == "row_last":
        row[1500] = row[1499] - 1
    else:
        row[0] = -1
    # no access outside the buffers (c_build asserts the guards), the bit set
    out = c_build(dev, item, row, cat, num, scale, mn, 90, shift)
    assert out["counts"][1] == ic.BAD_DATA
    if what.startswith("item"):   # such a row names no hotel: the tables are the other rows'
        ok = (item >= 0) & (item < 90)
        first, w_cat, w_num, n_with = ic.model(item[ok], row[ok], cat[ok], num[ok], scale, mn, 90)
        assert out["counts"][0] == n_with and out["first"].tobytes() == first.tobytes()
        assert out["cat"].tobytes() == w_cat.tobytes() and out["num"].tobytes() == w_num.tobytes()


def test_bad_arguments(dev):
    from dcnr import _lib
    lib = _lib.load()
    nb = int(lib.dcnr_item_features_workspace_size(4, 10, 2, 3))
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    ts = [z(4, torch.int32), z(8, torch.int32), z(12, torch.float64), z(3, torch.float64),
          z(3, torch.float64), z(10, torch.int32), z(20, torch.int64), z(30, torch.float32),
          z(2, torch.int32), z(nb, torch.uint8)]
    i_, c_, x_, sc, mn, first, cat, num, counts, ws = (t.data_ptr() for t in ts)
    s = _lib.stream_ptr(dev)
    call = lambda *a: lib.dcnr_item_features_build(*a, s)
    good = [i_, None, c_, x_, sc, mn, 4, 10, 2, 3, first, cat, num, counts, None, ws, nb]
    assert call(*good) == _lib.DCNR_OK
    torch.cuda.current_stream(dev).synchronize()
    B, U, W = _lib.DCNR_BAD_ARG, _lib.DCNR_UNSUPPORTED_SHAPE, _lib.DCNR_WORKSPACE_TOO_SMALL
    for i, v, want in ((0, None, B), (2, None, B), (3, None, B), (4, None, B), (5, None, B),
                       (10, None, B), (11, None, B), (12, None, B), (13, None, B), (15, None, B),
                       (6, -1, B), (7, -1, B), (8, -1, B), (9, -1, B),
                       (8, 65, U), (9, 65, U), (7, (1 << 29) + 1, U), (6, 2 ** 31 - 1, U),
                       (16, 8, W), (16, 4 * 10 - 1, W)):
        bad = list(good)
        bad[i] = v
        assert call(*bad) == want, (i, v)
    assert b"dcnr_item_features_build" in lib.dcnr_last_error()
    # a width of 0 takes no pointers; no rows take no columns and no workspace
    assert call(i_, None, None, x_, sc, mn, 4, 10, 0, 3, first, None, num, counts, None, ws, nb) == 0
    assert call(i_, None, c_, None, None, None, 4, 10, 2, 0, first, cat, None, counts, None, ws, nb) == 0
    assert call(None, None, None, None, sc, mn, 0, 10, 2, 3, first, cat, num, counts, None, None, 0) == 0
    torch.cuda.current_stream(dev).synchronize()
    assert ts[5].tolist() == [-1] * 10 and ts[8].tolist() == [0, 0]


# ------------------------------------------------------------ 2: generations
GEN_TENSORS = ["item_cat", "item_num", "first_row", "review_item", "review_row", "review_cat",
               "review_num", "scaler_scale", "scaler_min"]


def bits(t):
    return t.cpu().numpy().tobytes()


def assert_generation(gen, want, what):
    for k in GEN_TENSORS:
        g, w = getattr(gen, k), getattr(want, k)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        assert bits(g) == bits(w), (what, k)
    assert gen.n_with_row == want.n_with_row and gen.n_reviews == want.n_reviews, what


def assert_generation_is_host(gen, ft, what):
    assert bits(gen.item_cat) == ft.item_cat_host().tobytes(), what
    assert bits(gen.item_num) == ft.item_num_host().tobytes(), what
    assert bits(gen.first_row) == ft.first_rows_host().tobytes(), what
    assert gen.n_with_row == int((ft.first_rows_host() >= 0).sum()), what
    assert gen.item_cat.dtype == torch.int64 and gen.item_num.dtype == torch.float32 and \
        gen.first_row.dtype == torch.int32


@pytest.mark.parametrize("name,st,steps", ic.sequences(), ids=[s[0] for s in ic.sequences()])
def test_generations_follow_the_host(dev, name, st, steps):
    ft = st.fresh()
    gen = ft.on(dev)
    assert ft.on(dev) is gen
    assert_generation(gen, st.fresh().on(dev), name)
    assert_generation_is_host(gen, ft, name)
    for i, step in enumerate(steps):
        old = gen
        kept = {k: getattr(old, k).clone() for k in GEN_TENSORS}
        ic.do(ft, step)
        st.apply(step)
        gen = ft.on(dev)
        assert gen is not old
        assert_generation(gen, st.fresh().on(dev), f"{name}[{i}]")
        assert_generation_is_host(gen, ft, f"{name}[{i}]")
        for k in GEN_TENSORS:   # the generation taken before the step still holds its bytes
            assert bits(getattr(old, k)) == bits(kept[k]), (name, i, k)
        assert ft.last_update["devices"] == 1 and ft.last_update["op"] == step[0]
        assert ft.last_update["upload_bytes"] == ic.upload_bytes(step)   # the batch, not the table
    ic.assert_same(ft, st.fresh(), name)


def test_upload_does_not_grow_with_the_table(dev):
    item, cat, num = ic.base_table()
    sizes = []
    for reps in (1, 8):
        ft = ic.State(np.tile(item, reps), np.tile(cat, (reps, 1)), np.tile(num, (reps, 1))).fresh()
        ft.on(dev)
        per = []
        for step in (("append", item[:5], cat[:5], num[:5]), ("remove", [3, 4]),
                     ("set_values", [7, 8, 9], num[:3, :2], [0, 2]), ("set_scaler", ic.SCALE, ic.MIN)):
            ic.do(ft, step)
            per.append(ft.last_update["upload_bytes"])
            assert per[-1] == ic.upload_bytes(step) and ft.last_update["devices"] == 1
        sizes.append(per)
    assert sizes[0] == sizes[1]


def test_refused_calls_leave_the_device(dev):
    st = ic.State(*ic.base_table())
    ft = st.fresh()
    gen = ft.on(dev)
    for call in ic.refused(ft):
        with pytest.raises(ValueError):
            call()
        assert ft.on(dev) is gen
    ft.append()
    ft.remove([])
    ft.set_values([], np.zeros((0, ic.N_NUM)))
    assert ft.on(dev) is gen


# --------------------------------------------------------------- 3: the pipeline
N_ITEMS, U, M, E = 500, 300, 4000, 600
CFG = dict(n_users=400, n_items=N_ITEMS, cat_dims={"a": 30, "b": 250}, n_num=4,
           params=dict(emb_dim=32, hidden_dim=64, n_cross_layers=2, n_res_blocks=2, dropout=0.0))
LATE = 499        # a hotel that gets its first review after start-up
_cache = {}


def setup(dev):
    import dcnr
    if "model" not in _cache:
        _cache["model"] = our_model(CFG, precision="fp32", seed=9).to(dev).eval()
        rev, item, rating, fa, fb = f11_common.random_tables(U, M, E, N_ITEMS, seed=21)
        item[item == LATE] = LATE - 1
        rng = np.random.default_rng(23)
        cat = np.stack([rng.integers(0, c, M) for c in CFG["cat_dims"].values()], 1)
        num = rng.random((M, 4)) * 10
        _cache["tables"] = (rev, item, rating, fa, fb, cat, num)
        _cache["store"] = dcnr.InteractionStore(rev, item, rating, fa, fb, n_items=N_ITEMS, n_reviewers=U)
    return _cache["model"], _cache["tables"], _cache["store"]


def assert_answers(got, want, what):
    assert len(got) == len(want)
    for r, ((gr, gl), (wr, wl)) in enumerate(zip(got, want)):
        assert torch.equal(gr, wr), (what, r, gr.tolist(), wr.tolist())
        assert bits(gl) == bits(wl), (what, r)


def requests(R, seed):
    rng = np.random.default_rng(seed)
    lam = np.where(np.arange(R) % 2 == 0, 1.0, 0.4)
    lam[5] = 1.0 - 1e-12          # rounds to 1.0f from below: answered on the host path
    pos = [rng.integers(0, N_ITEMS, rng.integers(1, 6)).tolist() + [LATE] for _ in range(R)]
    pos[1] = []
    return dict(users=rng.integers(0, CFG["n_users"], R), rv=rng.integers(0, U, R), pos=pos, lam=lam,
                modes=["friends" if r % 3 else "personal" for r in range(R)],
                top_k=[[20, 5, 500][r % 3] for r in range(R)])


def check_pipeline(dev, model, store, ft, pipe, q, what):
    """Every entry point of ``pipe`` (on ``item_features=ft``) against a pipeline
    built from the host tables of the same state.  Returns recommend_many's answers."""
    import dcnr
    gen = ft.on(dev)
    ref = dcnr.RankingPipeline(model, ft.item_cat_host(), ft.item_num_host())
    assert pipe.item_cat is gen.item_cat and pipe.item_num is gen.item_num
    rows = torch.tensor([3, LATE, 0, 77], device=dev)
    for g, w in zip(pipe.ranking_batch(5, rows), ref.ranking_batch(5, rows)):
        assert bits(g) == bits(w), what
    assert bits(pipe.score(5, rows)) == bits(ref.score(5, rows)), what
    for r in (0, 3):
        g = pipe.recommend(int(q["users"][r]), q["pos"][r], float(q["lam"][r]))
        w = ref.recommend(int(q["users"][r]), q["pos"][r], float(q["lam"][r]))
        assert_answers([g], [w], (what, "recommend", r))
    kw = dict(lambda_param=q["lam"], top_k=q["top_k"])
    got = pipe.recommend_many(q["users"], q["pos"], **kw)
    assert_answers(got, ref.recommend_many(q["users"], q["pos"], **kw), (what, "many"))
    assert got._features_held is gen and sum(g[0].numel() > 0 for g in got) > len(got) // 2
    assert any(LATE in g[0].tolist() for g in got)
    # one generation per call, taken once: request 5 goes through recommend() inside the
    # batched call and scores from the generation the call started with
    taken, on = [], ft.on
    ft.on = lambda device: (taken.append(device), on(device))[1]
    try:
        got_u = pipe.recommend_users(store, q["users"], q["rv"], q["modes"], **kw)
        again = pipe.recommend_many(q["users"], q["pos"], **kw)
    finally:
        del ft.on
    assert len(taken) == 2 and again._features_held is gen
    assert_answers(again, got, (what, "many again"))
    want_u = ref.recommend_users(store, q["users"], q["rv"], q["modes"], **kw)
    assert_answers(got_u, want_u, (what, "users"))
    assert got_u._features_held is gen and got_u.on_host[5] and not got_u.on_host[:5].any()
    sweep = pipe.lambda_sweep(q["users"], q["pos"], [1.0, 0.5, 0.1], top_k=10, ks=(5, 10))
    want_s = ref.lambda_sweep(q["users"], q["pos"], [1.0, 0.5, 0.1], top_k=10, ks=(5, 10))
    assert sweep._features_held is gen and sweep.skipped == want_s.skipped == []
    for (ga, gm), (wa, wm) in zip(sweep, want_s):
        assert_answers(ga, wa, (what, "sweep"))
        assert repr(gm) == repr(wm)
    return got


def test_pipeline_follows_the_features(dev):
    import dcnr
    model, (rev, item, rating, fa, fb, cat, num), store = setup(dev)
    scale, mn = np.array([0.1, 0.2, 0.05, 0.1]), np.array([0.0, -1.0, 0.5, 0.0])
    ft = dcnr.ItemFeatures(item, cat, num, scale, mn, n_items=N_ITEMS)
    pipe = dcnr.RankingPipeline(model, item_features=ft)
    q = requests(12, seed=3)
    keep = lambda ans: [(r.clone(), l.clone()) for r, l in ans]
    first = check_pipeline(dev, model, store, ft, pipe, q, "start")
    held, kept = first._features_held, keep(first)
    assert ft.first_rows_host()[LATE] == -1 and not ft.item_num_host()[LATE].any()
    # a hotel's first ever row
    ft.append([LATE, 3], [[7, 11], [1, 2]], [[9.0, 8.0, 7.0, 6.0], [1.0, 1.0, 1.0, 1.0]])
    assert ft.first_rows_host()[LATE] == M
    second = check_pipeline(dev, model, store, ft, pipe, q, "appended")
    assert any(bits(a[1]) != bits(b[1]) for a, b in zip(first, second))
    # the first rows of a third of the hotels
    firsts = ft.first_rows_host()
    ft.remove(firsts[firsts >= 0][::3])
    third = check_pipeline(dev, model, store, ft, pipe, q, "removed")
    assert any(bits(a[1]) != bits(b[1]) for a, b in zip(second, third))
    # edits of first rows (what the ranker sees changes) and of others (it does not)
    firsts = ft.first_rows_host()
    ft.set_values(firsts[firsts >= 0][:200], np.full((200, 2), 3.0), columns=[0, 3])
    fourth = check_pipeline(dev, model, store, ft, pipe, q, "edited")
    assert any(bits(a[1]) != bits(b[1]) for a, b in zip(third, fourth))
    others = np.setdiff1d(ft.review_row, firsts)[:50]
    ft.set_values(others, np.zeros((50, 4)))
    fifth = check_pipeline(dev, model, store, ft, pipe, q, "edited elsewhere")
    assert_answers(fifth, fourth, "an edit of rows that are no hotel's first")
    ft.set_scaler(scale * 2, mn)
    check_pipeline(dev, model, store, ft, pipe, q, "rescaled")
    # the answers of the first call, and the generation they hold, are as they were
    assert_answers(first, kept, "answers of an earlier call")
    assert first._features_held is held and held is not ft.on(dev)
    assert bits(held.item_num) != bits(ft.on(dev).item_num)


def test_pipeline_arguments(dev):
    import dcnr
    model, (rev, item, rating, fa, fb, cat, num), _ = setup(dev)
    ft = dcnr.ItemFeatures(item, cat, num, np.ones(4), np.zeros(4), n_items=N_ITEMS)
    a, b = ft.item_cat_host(), ft.item_num_host()
    for args, kw in (((a, b), dict(item_features=ft)), ((a,), dict(item_features=ft)), ((), {}),
                     ((a,), {}), ((), dict(item_num=b)),
                     ((), dict(item_features=dcnr.ItemFeatures(item, cat[:, :1], num, np.ones(4),
                                                               np.zeros(4), n_items=N_ITEMS))),
                     ((), dict(item_features=dcnr.ItemFeatures(item, cat, num[:, :3], np.ones(3),
                                                               np.zeros(3), n_items=N_ITEMS)))):
        with pytest.raises(ValueError):
            dcnr.RankingPipeline(model, *args, **kw)
    # from arrays: plain tensors and a plain list, as before
    pipe = dcnr.RankingPipeline(model, a, b)
    assert pipe.item_cat.dtype == torch.int64 and bits(pipe.item_num) == b.tobytes()
    assert type(pipe.recommend_many([0], [[1, 2]])) is list


# ----------------------------------------------------------- 4: F7 end to end
def test_f7_served_from_item_features(dev):
    import dcnr
    f = f7_common.load()
    m = dcnr.DCN_RecSys(f.n_users, f.n_items, f.cat_dims, f.n_num, dict(f.params), precision="fp32")
    m.load_state_dict(f.state)
    m = m.to(dev).eval()
    emb = torch.from_numpy(f.emb).to(dev)
    ft = ic.f7_item_features(f)
    pipe = dcnr.RankingPipeline(m, item_features=ft, item_embeddings=emb)
    cs, code = cc.f7_city_sets(f)
    store, reviewer, _ = f11_common.store_of(f)
    reqs = f.expected["recommendations"]
    rows = [f7_common.request_rows(f, req) for req in reqs]
    got = pipe.recommend_many([r["user_row"] for r in rows], [r["pos"] for r in rows],
                              lambda_param=[req["lambda_param"] for req in reqs],
                              excluded=[r["excluded"] for r in rows], city_sets=cs,
                              cities=[code.get(req["city"], -1) for req in reqs])
    for req, (ranked, _) in zip(reqs, got):
        assert [f.rev[x] for x in ranked.tolist()] == req["ranked_hotels"], req
    assert any(len(req["ranked_hotels"]) > 0 for req in reqs)

    def serve(p):
        return p.recommend_users(store, [r["user_row"] for r in rows],
                                 [reviewer.get(q["user_id"], -1) for q in reqs],
                                 [q["type"] for q in reqs],
                                 lambda_param=[q["lambda_param"] for q in reqs], city_sets=cs,
                                 cities=[code.get(q["city"], -1) for q in reqs])
    before = serve(pipe)
    for req, (ranked, _) in zip(reqs, before):
        assert [f.rev[x] for x in ranked.tolist()] == req["ranked_hotels"], req
    kept = [(r.clone(), l.clone()) for r, l in before]
    # every hotel's first review is withdrawn: the three objects take the same batch
    firsts = f.main_df.drop_duplicates(subset=["item_id"]).index.to_numpy()
    store.remove(f.main_df.loc[firsts, "user_id"].map(reviewer).to_numpy(), firsts)
    cs.remove(firsts)
    ft.remove(firsts)
    want_cat, want_num = ic.f7_tables(f, f.main_df.drop(firsts))
    assert bits(ft.on(dev).item_cat) == want_cat.tobytes()
    assert bits(ft.on(dev).item_num) == want_num.tobytes()
    ref = dcnr.RankingPipeline(m, want_cat, want_num, item_embeddings=emb)
    after, want = serve(pipe), serve(ref)
    assert_answers(after, want, "first rows removed")
    assert sum(a[0].numel() > 0 for a in after) >= 1
    assert any(bits(a[1]) != bits(b[1]) for a, b in zip(after, before) if a[0].numel())
    assert_answers(before, kept, "answers of the call before the removal")
    # the main_df numbers for the response's city / price_rub / stars (main.py:334-335)
    ranked = after[[a[0].numel() > 0 for a in after].index(True)][0]
    nums = ft.on(dev).first_row[ranked].cpu().numpy()
    rest = f.main_df.drop(firsts)
    assert [f.item_map[h] for h in rest.loc[nums, "item_id"]] == ranked.tolist()
    assert nums.tolist() == [rest.index[rest["item_id"] == f.rev[x]][0] for x in ranked.tolist()]
