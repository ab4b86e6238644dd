"""InteractionStore.remove / set_rating on the device (dcnr_csr_remove,
csrc/serving.hip).  Every comparison is an equality.

  1  the kernel through the C ABI against np.delete and the offsets formula
  2  the device generations after each step against a rebuilt store's upload
  3  the F11 fixture served from a store the extras were removed from
  4  a random store, its heavy reviewer brought back under SV_MAX review rows
"""
import ctypes

import numpy as np
import pytest
import torch

import f11_common
import f7_common
import store_remove_common as src
import test_store_append_gpu as tsa   # (its guarded buffers, pipeline and answer comparison)
from helpers import our_model

pytestmark = pytest.mark.gpu

SV_MAX = 4096
SENTINEL = tsa.SENTINEL


# ------------------------------------------------------ 1: the kernel, directly
def model(old_off, old_vals, removed):
    """The contract of dcnr_csr_remove: (new_off, [new payloads])."""
    new_off = old_off - np.searchsorted(removed, old_off, side="left")   # #{removed < old_off[o]}
    return new_off.astype(np.int64), [np.delete(v, removed) for v in old_vals]


def make_case(rng, lens, removed, n_payloads):
    lens = np.asarray(lens, np.int64)
    old_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    old_vals = [rng.integers(0, 2 ** 31 - 1, int(old_off[-1])).astype(np.int32)
                for _ in range(n_payloads)]
    removed = np.asarray(removed, np.int64).reshape(-1)
    # what the host promises: strictly ascending, inside the old payloads
    assert (np.diff(removed) > 0).all()
    assert removed.size == 0 or (removed[0] >= 0 and removed[-1] < old_off[-1])
    return dict(old_off=old_off, old_vals=old_vals, removed=removed)


def run_remove(dev, c, guard=4, old_guard=4, expect=0, **override):
    """One call over guarded buffers; returns (status, new_off, new payloads) and
    asserts the guards and the old generation untouched."""
    from dcnr import _lib
    lib = _lib.load()
    U, M_old, m, P = c["old_off"].size - 1, int(c["old_off"][-1]), c["removed"].size, len(c["old_vals"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_old_off, d_removed = up(c["old_off"]), up(c["removed"])
    olds = [tsa.guarded(dev, M_old, torch.int32, old_guard, v) for v in c["old_vals"]]
    off_buf, new_off = tsa.guarded(dev, U + 1, torch.int64, 2)
    news = [tsa.guarded(dev, M_old - m, torch.int32, guard) for _ in range(P)]
    keep = [d_old_off.clone(), d_removed.clone()] + [b.clone() for b, _ in olds]
    arr = lambda ts: (ctypes.c_void_p * 2)(*[(t.data_ptr() if t.numel() else None) for t in ts])
    args = dict(old_offsets=d_old_off.data_ptr(), U=U, M_old=M_old, P=P,
                old=arr([v for _, v in olds]), removed=d_removed.data_ptr() or None, m=m,
                new_off=new_off.data_ptr(), new=arr([v for _, v in news]))
    args.update(override)
    st = lib.dcnr_csr_remove(*[args[k] for k in ("old_offsets", "U", "M_old", "P", "old", "removed",
                                                  "m", "new_off", "new")], _lib.stream_ptr(dev))
    torch.cuda.current_stream(dev).synchronize()
    assert st == expect, (st, lib.dcnr_last_error())
    # old generation, the removed list and every guard word: as they were
    assert torch.equal(d_old_off, keep[0]) and torch.equal(d_removed, keep[1])
    for (b, _), k in zip(olds, keep[2:]):
        assert torch.equal(b, k)
    assert (off_buf[:2] == SENTINEL).all() and (off_buf[2 + U + 1:] == SENTINEL).all()
    for b, _ in news:
        assert (b[:guard] == SENTINEL).all() and (b[guard + M_old - m:] == SENTINEL).all()
    return st, new_off.cpu().numpy(), [v.cpu().numpy() for _, v in news]


def check_case(dev, c, what, twice=False, **kw):
    want_off, want = model(c["old_off"], c["old_vals"], c["removed"])
    for _ in range(2 if twice else 1):   # the same bits on every run
        _, off, vals = run_remove(dev, c, **kw)
        np.testing.assert_array_equal(off, want_off, err_msg=str(what))
        for w in range(len(want)):
            np.testing.assert_array_equal(vals[w], want[w], err_msg=f"{what} payload {w}")


def one_owner(M_old):
    """Three owners, the middle one holding everything."""
    return [0, M_old, 0]


@pytest.mark.parametrize("U", [1, 2, 65, 1000])
def test_kernel_equals_np_delete(dev, U):
    """Owner counts with empty segments; one entry, some, a whole owner and
    every entry removed; both payload counts."""
    rng = np.random.default_rng(U)
    n = 0
    for contents in ("one", "drawn"):
        lens = tsa.old_lens(rng, U, contents)
        lens[0] += 5 * (lens.sum() == 0)
        off =np.concatenate([[0], np.cumsum(lens)])
        M_old = int(off[-1])
        o = int(np.argmax(lens))          # an owner that holds something
        sets = {"one": [int(rng.integers(0, M_old))],
                "some": np.sort(rng.choice(M_old, min(M_old, 40), replace=False)),
                "whole_owner": np.arange(off[o], off[o + 1]),
                "all": np.arange(M_old)}
        for which, removed in sets.items():
            for P in (1, 2):
                check_case(dev, make_case(rng, lens, removed, P), (U, contents, which, P),
                           twice=(n % 4 == 0))
                n += 1
    assert n == 2 * 4 * 2


def test_kernel_single_removal_at_the_chunk_edges(dev):
    from dcnr import _lib
    C = _lib.CSR_INSERT_CHUNK
    rng = np.random.default_rng(1)
    M_old = 3 * C + 5
    for at in (0, M_old - 1, C - 1, C, C + 1):
        for P in (1, 2):
            check_case(dev, make_case(rng, one_owner(M_old), [at], P), (at, P))


def test_kernel_shifted_copies_of_every_residue_and_length(dev):
    """1 .. 4 removals in front of untouched chunks (copy shifts of every
    residue mod 4) with the old and the new total at k * CHUNK + 0 .. 8: the
    old array ends inside the second 16-byte source word."""
    from dcnr import _lib
    C = _lib.CSR_INSERT_CHUNK
    rng = np.random.default_rng(2)
    for k in (1, 2):
        for n_rem in (1, 2, 3, 4):
            for j in range(0, 9 + n_rem):      # M_old = kC + j, M_new = kC + j - n_rem: both cover 0 .. 8
                M_old = k * C + j
                if M_old - n_rem < 1:
                    continue
                removed = np.sort(rng.choice(min(M_old, 50), n_rem, replace=False))
                c = make_case(rng, [7, M_old - 7], removed, 2)
                check_case(dev, c, (k, n_rem, j))


def test_kernel_runs_and_many_removals(dev):
    from dcnr import _lib
    C = _lib.CSR_INSERT_CHUNK
    rng = np.random.default_rng(3)
    M_old = 3 * C + 3
    lens = [100, C - 100, 0, 0, C + 3, C]
    # a run of removed positions across a chunk boundary (of the old and of the new array)
    check_case(dev, make_case(rng, lens, np.arange(C - 5, C + 7), 2), "run over a boundary")
    check_case(dev, make_case(rng, lens, np.r_[3, np.arange(2 * C - 6, 2 * C + 9)], 1), "run, shifted")
    # many removals in one chunk, the chunks around it untouched
    many = C + np.sort(rng.choice(C, 1000, replace=False))
    check_case(dev, make_case(rng, lens, many, 2), "many in one chunk", twice=True)
    # many everywhere
    check_case(dev, make_case(rng, lens, np.sort(rng.choice(M_old, 5000, replace=False)), 2),
               "many everywhere")
    # all but the last entry, all but the first
    check_case(dev, make_case(rng, lens, np.arange(M_old - 1), 2), "all but the last")
    check_case(dev, make_case(rng, lens, np.arange(1, M_old), 1), "all but the first")


def test_kernel_unaligned_payloads(dev):
    """Payload pointers off 16-byte alignment: the copy goes word by word."""
    from dcnr import _lib
    C = _lib.CSR_INSERT_CHUNK
    rng = np.random.default_rng(4)
    for total in (C - 1, C, 2 * C + 1):
        for removed in ([5], np.sort(rng.choice(total, 37, replace=False))):
            c = make_case(rng, one_owner(total), removed, 2)
            check_case(dev, c, (total, "unaligned new"), guard=5)
            check_case(dev, c, (total, "unaligned old"), old_guard=3)
            check_case(dev, c, (total, "unaligned both"), guard=7, old_guard=1)


def test_kernel_several_chunks_per_workgroup(dev):
    """More chunks than workgroups (the grid is capped): each takes a range."""
    from dcnr import _lib
    C = _lib.CSR_INSERT_CHUNK
    rng = np.random.default_rng(6)
    U, M_old = 1000, 2049 * C + 3
    cuts = np.sort(rng.integers(0, M_old, U - 1))
    lens = np.diff(np.concatenate([[0], cuts, [M_old]]))
    removed = np.unique(np.r_[rng.integers(0, M_old, 40), np.arange(700 * C - 3, 700 * C + 4)])
    check_case(dev, make_case(rng, lens, removed, 1), "2049 chunks")


def test_kernel_several_offset_chunks(dev):
    """More than CHUNK + 1 owners: the offsets take several chunks."""
    from dcnr import _lib
    C = _lib.CSR_INSERT_CHUNK
    rng = np.random.default_rng(8)
    lens = rng.choice([0, 1, 2], 2 * C + 5)
    M_old = int(lens.sum())
    check_case(dev, make_case(rng, lens, np.sort(rng.choice(M_old, 300, replace=False)), 2),
               "2 * CHUNK + 5 owners", twice=True)
    check_case(dev, make_case(rng, lens, np.arange(M_old), 1), "all of them, offsets only")


def test_kernel_without_removals_and_bad_arguments(dev):
    from dcnr import _lib
    rng = np.random.default_rng(7)
    lens = rng.choice([1, 2, 63], 65)
    # m = 0: nothing is launched, nothing written
    _, off, vals = run_remove(dev, make_case(rng, lens, [], 2))
    assert (off == SENTINEL).all() and all((v == SENTINEL).all() for v in vals)
    # DCNR_BAD_ARG before any launch: the outputs keep the sentinel
    c = make_case(rng, lens, [3, 9, 70], 2)
    M_old = int(c["old_off"][-1])
    null2 = (ctypes.c_void_p * 2)(None, None)
    for override in (dict(old_offsets=None), dict(new_off=None), dict(removed=None), dict(U=-1),
                     dict(M_old=-1), dict(P=0), dict(P=3), dict(m=-1), dict(m=M_old + 1),
                     dict(M_old=2), dict(old=None), dict(new=None), dict(old=null2),
                     dict(new=null2)):
        st, off, vals = run_remove(dev, c, expect=_lib.DCNR_BAD_ARG, **override)
        assert (off == SENTINEL).all() and all((v == SENTINEL).all() for v in vals), override
    check_case(dev, c, "the good call")
    # every entry removed: the payload pointers may be NULL
    c = make_case(rng, lens, np.arange(M_old), 2)
    _, off, _ = run_remove(dev, c, old=None, new=None)
    np.testing.assert_array_equal(off, np.zeros(66, np.int64))


# -------------------------------------------------- 2: the device generations
def rebuilt_generation(dev, t):
    """(descriptor, tensors) of a store built from the live tables, its rows mapped."""
    live, rows = t.live()
    rebuilt = src.build(live)
    desc, want = rebuilt.on(dev)
    want = dict(want)
    want["review_rows"] = torch.from_numpy(rows.astype(np.int32)).to(dev)[want["review_rows"].long()]
    return rebuilt, desc, want


@pytest.mark.parametrize("name", [s[0] for s in src.sequences(0)])
def test_device_generations_equal_rebuilt(dev, name):
    _, init, steps = next(s for s in src.sequences(0) if s[0] == name)
    t, store = src.Tables(*init), src.build(init)
    store.on(dev)
    for i, s in enumerate(steps):
        held = store.on(dev)[1]
        clones = {k: v.clone() for k, v in held.items()}
        t.apply(s)
        src.apply(store, s)
        rebuilt, want_desc, want = rebuilt_generation(dev, t)
        src.assert_same_mapped(store, rebuilt, t.live()[1], f"{name}[{i}]")
        desc, got = store.on(dev)
        tsa.same_generation(got, want, f"{name}[{i}]")
        assert (desc.n_reviewers, desc.n_reviews, desc.n_friend_rows) == (
            want_desc.n_reviewers, want_desc.n_reviews, want_desc.n_friend_rows)
        for k in ("friend_offsets", "friend_rows", "review_offsets", "review_items", "review_rows"):
            assert getattr(desc, k) == (got[k].data_ptr() or None), k
        # the generation from before the call: its contents as they were
        tsa.same_generation(held, clones, f"{name}[{i}] held")
        # a CSR the step does not touch keeps its tensors
        op, kw = s
        if op == "set_rating" or (op == "remove" and not len(kw["friend_a"])):
            assert got["friend_rows"] is held["friend_rows"]
            assert got["friend_offsets"] is held["friend_offsets"]
        if op == "set_rating":
            assert got["review_rows"] is held["review_rows"]
            assert got["review_offsets"] is held["review_offsets"]
        if op == "remove" and not len(kw["review_row"]):
            assert got["review_items"] is held["review_items"]
    # a refused call leaves the device as it was
    desc, got = store.on(dev)
    with pytest.raises(ValueError):
        store.remove(review_reviewer=[0], review_row=[store.next_review_row])
    with pytest.raises(ValueError):
        store.set_rating([0], [store.next_review_row], [9.0])
    assert store.on(dev)[0] is desc and store.on(dev)[1] is got


# ------------------------------------------------------------ 3: F11, end to end
def _f11_with_extras(f, dev):
    """The fixture's tables with extra reviews interleaved into main_df order
    and extra friendships, uploaded: the store, the extras as a remove batch,
    and some fixture reviews with their ratings."""
    import dcnr
    full, reviewer, ids = f11_common.store_of(f)
    rev = f.main_df["user_id"].map(reviewer).to_numpy()
    item = f.main_df["item_id"].map(f.item_map).to_numpy()
    rating = f.main_df["rating_overall"].to_numpy().astype(np.float64)
    fa = f.friends["user_id_1"].map(reviewer).to_numpy()
    fb = f.friends["user_id_2"].map(reviewer).to_numpy()
    rng = np.random.default_rng(5)
    x_rev, x_item, x_rating, x_fa, x_fb = [], [], [], [], []
    for q in f.expected["recommendations"]:
        u = reviewer.get(q["user_id"], -1)
        if u < 0 or not q["ranked_hotels"]:
            continue
        friends = full.friends_host(u)
        # the best hotel rated 1 by a source of the request: it leaves the answer ...
        who = int(friends[0]) if q["type"] == "friends" and friends.size else u
        x_rev += [who, who]
        x_item += [f.item_map[q["ranked_hotels"][0]], f.item_map[q["ranked_hotels"][-1]]]
        x_rating += [1.0, 10.0]
        # ... and a stranger with positives becomes a friend
        strangers = [s for s in np.flatnonzero(full.n_pos > 0) if s not in friends and s != u]
        x_fa.append(u)
        x_fb.append(int(strangers[int(rng.integers(0, len(strangers)))]))
    n_x, M = len(x_rev), rev.size
    at = np.sort(rng.integers(0, M + 1, n_x))          # fixture row each extra stands in front of
    x_rows = at + np.arange(n_x)                        # the extras' rows in the longer table
    ins = lambda a, x: np.insert(a, at, np.asarray(x, a.dtype))
    store = dcnr.InteractionStore(ins(rev, x_rev), ins(item, x_item), ins(rating, x_rating),
                                  np.r_[fa, x_fa], np.r_[fb, x_fb], n_items=f.n_items,
                                  n_reviewers=len(ids))
    store.on(dev)
    fixture_rows = np.delete(np.arange(M + n_x), x_rows)
    assert (np.asarray(x_rev) == ins(rev, x_rev)[x_rows]).all()
    extras = dict(review_reviewer=np.asarray(x_rev), review_row=x_rows, friend_a=x_fa, friend_b=x_fb)
    # fixture reviews of the requests' sources, to be edited and set back
    asking = [reviewer[q["user_id"]] for q in f.expected["recommendations"] if q["user_id"] in reviewer]
    sources = np.unique(np.concatenate([full.friends_host(u) for u in asking] + [asking]))
    some = np.flatnonzero(np.isin(rev, sources) & ((rating >= 8) | (rating <= 4)))[:12]
    assert some.size == 12
    edits =(rev[some], fixture_rows[some], rating[some])
    return store, extras, edits, full, fixture_rows, reviewer, ids


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_f11_served_after_the_extras_are_removed(dev, precision):
    f = f11_common.load()
    pipe = tsa._fixture_pipe(f, dev, precision)
    store, extras, edits, full, fixture_rows, reviewer, ids = _f11_with_extras(f, dev)
    reqs = f.expected["recommendations"]
    rows = [f7_common.request_rows(f, q) for q in reqs]
    city_sets = {}
    for q, r in zip(reqs, rows):
        if q["city"] not in city_sets:
            city_sets[q["city"]] = tuple(pipe.register_sets([r["allowed"], r["fallback"]]))
    call = lambda s: pipe.recommend_users(      # (raises if the device rejects validated input)
        s, [r["user_row"] for r in rows], [reviewer.get(q["user_id"], -1) for q in reqs],
        [q["type"] for q in reqs], lambda_param=[q["lambda_param"] for q in reqs],
        allowed=[city_sets[q["city"]][0] for q in reqs],
        fallback=[city_sets[q["city"]][1] for q in reqs])
    lists = lambda res: [res.to_lists(r)[::2] for r in range(len(reqs))]
    want = call(full)
    # the extras change answers (so that their removal is seen to undo it)
    assert sum(a != b for a, b in zip(lists(call(store)), lists(want))) >= 4
    # ratings pushed over the thresholds and set back
    who, row, rating = edits
    asked = [(reviewer.get(q["user_id"], -1), q["type"]) for q in reqs]
    sources = lambda: [[x.tolist() for x in store.sources_host(u, mode)] for u, mode in asked]
    before = sources()
    store.set_rating(who, row, np.where(rating >= 8, 2.0, 9.0))
    assert sources() != before
    call(store)
    store.set_rating(who, row, rating)
    assert sources() == before
    store.remove(**extras)
    src.assert_same_mapped(store, full, fixture_rows, "the fixture's store")
    res = call(store)
    tsa._answers_equal(res, want, precision)
    if precision == "fp32":   # what the reference service answered (expected.json)
        n_by = 0
        for r, q in enumerate(reqs):
            ranked, _, by = res.to_lists(r)
            assert [f.rev[x] for x in ranked] == q["ranked_hotels"], q
            assert [[int(ids[x]) for x in lst] for lst in by] == q["recommended_by"], q
            n_by += sum(len(b) for b in by)
        assert n_by >= 10


# ------------------------------------------------------------ 4: a random store
def test_random_store_with_its_heavy_reviewer_brought_under_sv_max(dev):
    import dcnr
    U, M, E, N_ITEMS = 300, 6000, 2500, 200
    cfg = dict(n_users=400, n_items=N_ITEMS, cat_dims={"a": 30, "b": 250}, n_num=4,
               params=dict(emb_dim=32, hidden_dim=64, n_cross_layers=2, n_res_blocks=2, dropout=0.0))
    m = our_model(cfg, precision="bf16", seed=9).to(dev).eval()
    rng = np.random.default_rng(2)
    item_cat = np.stack([rng.integers(0, c, N_ITEMS) for c in cfg["cat_dims"].values()], 1)
    pipe = dcnr.RankingPipeline(m, item_cat, rng.random((N_ITEMS, 4), dtype=np.float32))
    rev, item, rating, fa, fb = f11_common.random_tables(U, M, E, N_ITEMS, seed=11)
    # HEAVY stands above SV_MAX review rows: its own requests, and those of its
    # friends, are answered on the host until enough of its reviews are gone
    HEAVY = 77
    n_more = SV_MAX + 10 - int((rev == HEAVY).sum())
    rev = np.r_[rev, np.full(n_more, HEAVY)]
    item = np.r_[item, rng.integers(0, N_ITEMS, n_more)]
    rating = np.r_[rating, rng.integers(1, 11, n_more).astype(np.float64)]
    t = src.Tables(rev, item, rating, fa, fb, U)
    store = dcnr.InteractionStore(rev, item, rating, fa, fb, n_items=N_ITEMS, n_reviewers=U)
    store.on(dev)
    assert store.n_rows[HEAVY] > SV_MAX
    rv = [HEAVY, HEAVY, -1, 3] + rng.integers(0, U, 36).tolist()
    modes = ["personal", "friends"] * 20
    friend = int(f11_common.PandasStore(rev, item, rating, fa, fb).friends(HEAVY).pop())
    rv[4], modes[4] = friend, "friends"
    users = rng.integers(0, cfg["n_users"], 40).tolist()
    call = lambda s: pipe.recommend_users(s, users, rv, modes, lambda_param=[1.0, 0.3] * 20,
                                          top_k=[20, 5] * 20)

    def check(what):
        live, rows = t.live()
        rebuilt = dcnr.InteractionStore(*live[:5], n_items=N_ITEMS, n_reviewers=U)
        want = dict(rebuilt.on(dev)[1])
        want["review_rows"] = torch.from_numpy(rows.astype(np.int32)).to(dev)[want["review_rows"].long()]
        tsa.same_generation(store.on(dev)[1], want, what)
        res = call(store)
        tsa._answers_equal(res, call(rebuilt), what)
        return res

    res = check("before")
    assert res.on_host[0] and res.on_host[4]
    # some of HEAVY's reviews from all over its segment, with others' and a few pairs
    gone = np.sort(np.r_[rng.choice(t.rows_of(HEAVY), 30, replace=False),
                         rng.choice(np.flatnonzero(rev != HEAVY), 200, replace=False)])
    step = src.rm(t, gone, fa[:20], fb[:20])
    t.apply(step)
    src.apply(store, step)
    assert store.n_rows[HEAVY] == SV_MAX - 20
    res = check("after")
    assert not res.on_host[0] and not res.on_host[2:4].any()
    assert sum(r[0].numel() > 0 for r in res) > 20
