"""InteractionStore.append on the device (dcnr_csr_insert, csrc/serving.hip).
Every comparison is an equality.

  1  the kernel through the C ABI against a numpy model of its contract
  2  the device generations after each append against a rebuilt store's upload
  3  the F11 fixture served from a store that was appended to
  4  a random store, with a reviewer pushed over SV_MAX review rows
"""
import ctypes

import numpy as np
import pytest
import torch

import f11_common
import f7_common
import store_append_common as sac
from helpers import our_model

pytestmark = pytest.mark.gpu

SV_MAX = 4096
SENTINEL = -7


# ------------------------------------------------------ 1: the kernel, directly
def model(old_off, old_vals, U_new, touched, prefix, ins_pos, ins_vals):
    """The contract of dcnr_csr_insert, owner by owner: (new_off, [new payloads])."""
    U_old, M_old, m = old_off.size - 1, int(old_off[-1]), ins_pos.size
    cnt = np.zeros(U_new, np.int64)
    cnt[touched] = np.diff(prefix)
    old_len = np.concatenate([np.diff(old_off), np.zeros(U_new - U_old, np.int64)])
    new_off = np.concatenate([[0], np.cumsum(old_len + cnt)]).astype(np.int64)
    start = np.concatenate([old_off[:-1], np.full(U_new - U_old, M_old, np.int64)])
    slot = {int(o): j for j, o in enumerate(touched)}
    out = [np.empty(M_old + m, np.int32) for _ in old_vals]
    for o in range(U_new):
        seg = slice(int(new_off[o]), int(new_off[o + 1]))
        old = slice(int(start[o]), int(start[o] + old_len[o]))
        if o not in slot:
            for w, v in enumerate(old_vals):
                out[w][seg] = v[old]
            continue
        j = slot[o]
        mask = np.zeros(seg.stop - seg.start, bool)
        mask[ins_pos[prefix[j]:prefix[j + 1]]] = True
        for w, v in enumerate(old_vals):
            s = np.empty(mask.size, np.int32)
            s[mask] = ins_vals[w][prefix[j]:prefix[j + 1]]
            s[~mask] = v[old]
            out[w][seg] = s
    return new_off, out


def make_case(rng, lens, added, touched, counts, place, n_payloads):
    """Old CSR with the segment lengths ``lens``; counts[j] inserts into owner
    touched[j] at the start, at the end, or at interleaved places of the new segment."""
    lens = np.asarray(lens, np.int64)
    old_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    U_new = lens.size + added
    old_vals = [rng.integers(0, 2 ** 31 - 1, int(old_off[-1])).astype(np.int32)
                for _ in range(n_payloads)]
    touched, counts = np.asarray(touched, np.int64), np.asarray(counts, np.int64)
    prefix = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pos = []
    for o, c in zip(touched, counts):
        n_old = int(lens[o]) if o < lens.size else 0
        if place == "start":
            pos.append(np.arange(c))
        elif place == "end":
            pos.append(n_old + np.arange(c))
        else:
            pos.append(np.sort(rng.choice(n_old + c, c, replace=False)))
    ins_pos = np.concatenate(pos).astype(np.int64) if pos else np.zeros(0, np.int64)
    ins_vals = [-rng.integers(1, 2 ** 31 - 1, ins_pos.size).astype(np.int32)
                for _ in range(n_payloads)]
    return dict(old_off=old_off, old_vals=old_vals, U_new=U_new, touched=touched, prefix=prefix,
                ins_pos=ins_pos, ins_vals=ins_vals)


def guarded(dev, n, dtype, guard, fill=None):
    """A device array of n elements inside a sentinel-filled buffer: (buffer, view)."""
    buf = torch.full((n + 2 * guard,), SENTINEL, dtype=dtype, device=dev)
    view = buf[guard:guard + n]
    if fill is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(fill)))
    return buf, view


def run_insert(dev, c, guard=4, old_guard=4, expect=0, **override):
    """One call over guarded buffers; returns (status, new_off, new payloads) and
    asserts the guards and the old generation untouched."""
    from dcnr import _lib
    lib = _lib.load()
    U_old, M_old, m, P = c["old_off"].size - 1, int(c["old_off"][-1]), c["ins_pos"].size, len(c["old_vals"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_old_off = up(c["old_off"])
    olds = [guarded(dev, M_old, torch.int32, old_guard, v) for v in c["old_vals"]]
    d_touched, d_prefix, d_pos = up(c["touched"]), up(c["prefix"]), up(c["ins_pos"])
    d_ins = [up(v) for v in c["ins_vals"]]
    off_buf, new_off = guarded(dev, c["U_new"] + 1, torch.int64, 2)
    news = [guarded(dev, M_old + m, torch.int32, guard) for _ in range(P)]
    keep = [d_old_off.clone()] + [b.clone() for b, _ in olds]
    arr = lambda ts: (ctypes.c_void_p * 2)(*[t.data_ptr() or None for t in ts])
    args = dict(old_offsets=d_old_off.data_ptr(), n_old=U_old, n_new=c["U_new"], M_old=M_old, P=P,
                old=arr([v for _, v in olds]), touched=d_touched.data_ptr() or None,
                prefix=d_prefix.data_ptr(), t=c["touched"].size, pos=d_pos.data_ptr() or None,
                ins=arr(d_ins), m=m, new_off=new_off.data_ptr(), new=arr([v for _, v in news]))
    args.update(override)
    st = lib.dcnr_csr_insert(*[args[k] for k in ("old_offsets", "n_old", "n_new", "M_old", "P", "old",
                                                  "touched", "prefix", "t", "pos", "ins", "m",
                                                  "new_off", "new")], _lib.stream_ptr(dev))
    torch.cuda.current_stream(dev).synchronize()
    assert st == expect, (st, _lib.load().dcnr_last_error())
    # old generation and every guard word: as they were
    assert torch.equal(d_old_off, keep[0])
    for (b, _), k in zip(olds, keep[1:]):
        assert torch.equal(b, k)
    g = 2
    assert (off_buf[:g] == SENTINEL).all() and (off_buf[g + c["U_new"] + 1:] == SENTINEL).all()
    for b, _ in news:
        assert (b[:guard] == SENTINEL).all() and (b[guard + M_old + m:] == SENTINEL).all()
    return st, new_off.cpu().numpy(), [v.cpu().numpy() for _, v in news]


def check_case(dev, c, what, twice=False, **kw):
    want_off, want = model(c["old_off"], c["old_vals"], c["U_new"], c["touched"], c["prefix"],
                           c["ins_pos"], c["ins_vals"])
    for _ in range(2 if twice else 1):   # the same bits on every run
        _, off, vals = run_insert(dev, c, **kw)
        np.testing.assert_array_equal(off, want_off, err_msg=str(what))
        for w in range(len(want)):
            np.testing.assert_array_equal(vals[w], want[w], err_msg=f"{what} payload {w}")


def old_lens(rng, U_old, contents):
    if contents == "empty":
        return np.zeros(U_old, np.int64)
    if contents == "one":
        lens = np.zeros(U_old, np.int64)
        lens[U_old // 2] = 300
        return lens
    return rng.choice([0, 1, 2, 63, 64, 65, 300], U_old)


@pytest.mark.parametrize("U_old", [1, 2, 65, 1000])
def test_kernel_equals_model(dev, U_old):
    rng = np.random.default_rng(U_old)
    n = 0
    for added in (0, 5):
        U_new = U_old + added
        for contents in ("empty", "one", "drawn"):
            lens = old_lens(rng, U_old, contents)
            sets = {"one": [U_old // 2], "all": list(range(U_new)),
                    "last_and_added": [U_old - 1] + ([U_new - 1] if added else []),
                    "some": sorted(rng.choice(U_new, min(U_new, 9), replace=False).tolist())}
            for which, touched in sets.items():
                for place in ("start", "end", "interleaved"):
                    for P in (1, 2):
                        counts = rng.integers(1, 6, len(touched)) if which != "one" else [1]
                        c = make_case(rng, lens, added, touched, counts, place, P)
                        check_case(dev, c, (U_old, added, contents, which, place, P),
                                   twice=(n % 16 == 0))
                        n += 1
    assert n == 2 * 3 * 4 * 3 * 2


def test_kernel_total_lengths_around_the_chunk(dev):
    """M_old + m one below, at and one above the workgroup's chunk, one above
    two chunks; m = 1 and a few dozen inserts; 16-byte aligned arrays and arrays
    that are not (the copy then goes word by word)."""
    from dcnr import _lib
    C = _lib.CSR_INSERT_CHUNK
    rng = np.random.default_rng(3)
    for total in (C - 1, C, C + 1, 2 * C + 1):
        for m in (1, 37):
            for place in ("end", "interleaved"):
                lens = rng.choice([0, 1, 2, 63, 64, 65], 65)   # (their sum stays below a chunk)
                lens[7] += total - m - lens.sum()     # owner 7 takes the rest
                assert lens[7] >= 0
                touched = [64] if m == 1 else sorted(rng.choice(65, 12, replace=False).tolist())
                counts = [1] if m == 1 else np.r_[np.ones(11, np.int64), m - 11]
                c = make_case(rng, lens, 0, touched, counts, place, 2)
                assert c["old_off"][-1] + c["ins_pos"].size == total
                check_case(dev, c, (total, m, place))
                check_case(dev, c, (total, m, place, "unaligned new"), guard=5)
                check_case(dev, c, (total, m, place, "unaligned old"), old_guard=3)


def test_kernel_many_touched_owners_in_one_chunk(dev):
    """More touched segments inside one workgroup's range than it stages in
    LDS: the bounds come from global memory."""
    rng = np.random.default_rng(5)
    lens = rng.choice([0, 1, 2], 3000)
    c = make_case(rng, lens, 5, list(range(3005)), np.ones(3005, np.int64), "interleaved", 2)
    check_case(dev, c, "all of 3005 owners", twice=True)


def test_kernel_several_chunks_per_workgroup(dev):
    """More chunks than workgroups (the grid is capped): each takes a range."""
    from dcnr import _lib
    C = _lib.CSR_INSERT_CHUNK
    rng = np.random.default_rng(6)
    U_old, M_old = 1000, 2049 * C + 3
    cuts = np.sort(rng.integers(0, M_old, U_old - 1))
    old_off = np.concatenate([[0], cuts, [M_old]]).astype(np.int64)
    lens = np.diff(old_off)
    touched = np.sort(rng.choice(U_old, 40, replace=False))
    c = make_case(rng, lens, 0, touched, rng.integers(1, 4, 40), "interleaved", 1)
    # (np.insert in place of the owner loop: the same contract, at this size)
    rank = np.arange(c["ins_pos"].size) - np.repeat(c["prefix"][:-1], np.diff(c["prefix"]))
    at = np.repeat(old_off[touched], np.diff(c["prefix"])) + c["ins_pos"] - rank
    want = np.insert(c["old_vals"][0], at, c["ins_vals"][0])
    add = np.zeros(U_old + 1, np.int64)
    add[touched + 1] = np.diff(c["prefix"])
    _, off, vals = run_insert(dev, c)
    np.testing.assert_array_equal(off, old_off + np.cumsum(add))
    np.testing.assert_array_equal(vals[0], want)


def test_kernel_without_inserts_and_bad_arguments(dev):
    from dcnr import _lib
    rng = np.random.default_rng(7)
    lens = rng.choice([0, 1, 2, 63], 65)
    # m = 0 with added owners: the offsets only
    c = make_case(rng, lens, 5, [], [], "end", 2)
    _, off, vals = run_insert(dev, c)
    np.testing.assert_array_equal(off, np.r_[c["old_off"], [c["old_off"][-1]] * 5])
    assert all((v == SENTINEL).all() for v in vals)
    # m = 0, the owners as they were: nothing is launched
    c0 = make_case(rng, lens, 0, [], [], "end", 1)
    _, off, vals = run_insert(dev, c0)
    assert (off == SENTINEL).all() and (vals[0] == SENTINEL).all()
    # DCNR_BAD_ARG before any launch: the outputs keep the sentinel
    c = make_case(rng, lens, 0, [3, 9], [2, 1], "interleaved", 2)
    null2 = (ctypes.c_void_p * 2)(None, None)
    for override in (dict(old_offsets=None), dict(new_off=None), dict(n_old=-1), dict(n_new=64),
                     dict(M_old=-1), dict(P=0), dict(P=3), dict(t=-1), dict(m=-1), dict(t=4),
                     dict(t=0), dict(touched=None), dict(prefix=None), dict(pos=None),
                     dict(old=None), dict(ins=None), dict(new=None), dict(old=null2),
                     dict(ins=null2), dict(new=null2)):
        st, off, vals = run_insert(dev, c, expect=_lib.DCNR_BAD_ARG, **override)
        assert (off == SENTINEL).all() and all((v == SENTINEL).all() for v in vals), override
    check_case(dev, c, "the good call")


# -------------------------------------------------- 2: the device generations
def same_generation(got, want, what):
    for k in sac.TENSORS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert torch.equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("name", [s[0] for s in sac.sequences(0)])
def test_device_generations_equal_rebuilt(dev, name):
    _, init, batches = next(s for s in sac.sequences(0) if s[0] == name)
    store = sac.build(init)
    first = store.on(dev)
    same_generation(first[1], sac.build(init).on(dev)[1], name)
    for i, b in enumerate(batches):
        held = store.on(dev)[1]
        clones = {k: v.clone() for k, v in held.items()}
        sac.append(store, b)
        rebuilt = sac.build(sac.concatenated(init, batches[:i + 1]))
        sac.assert_same(store, rebuilt, f"{name}[{i}]")
        desc, t = store.on(dev)
        want_desc, want = rebuilt.on(dev)
        same_generation(t, want, f"{name}[{i}]")
        assert (desc.n_reviewers, desc.n_reviews, desc.n_friend_rows) == (
            want_desc.n_reviewers, want_desc.n_reviews, want_desc.n_friend_rows)
        assert desc.review_items == (t["review_items"].data_ptr() or None)
        assert desc.friend_offsets == t["friend_offsets"].data_ptr()
        # the generation from before the append: its contents as they were
        same_generation(held, clones, f"{name}[{i}] held")
    # a refused append leaves the device as it was
    desc, t = store.on(dev)
    with pytest.raises(ValueError):
        store.append(review_reviewer=[0], review_item=[sac.N_ITEMS], review_rating=[9.0])
    assert store.on(dev)[0] is desc and store.on(dev)[1] is t


# ------------------------------------------------------------ 3: F11, end to end
def _fixture_pipe(f, dev, precision):
    import dcnr
    m = dcnr.DCN_RecSys(f.n_users, f.n_items, f.cat_dims, f.n_num, dict(f.params),
                        precision=precision)
    m.load_state_dict(f.state)
    return dcnr.RankingPipeline(m.to(dev).eval(), f.item_cat, f.item_num,
                                item_embeddings=torch.from_numpy(f.emb).to(dev))


def _f11_appended(f, dev):
    """The fixture's store built from the first 60 % of main_df and the first
    half of the friendships, uploaded, then the rest appended in three batches."""
    import dcnr
    full, reviewer, ids = f11_common.store_of(f)
    rev = f.main_df["user_id"].map(reviewer).to_numpy()
    item = f.main_df["item_id"].map(f.item_map).to_numpy()
    rating = f.main_df["rating_overall"].to_numpy()
    fa = f.friends["user_id_1"].map(reviewer).to_numpy()
    fb = f.friends["user_id_2"].map(reviewer).to_numpy()
    m0, e0 = rev.size * 6 // 10, fa.size // 2
    store = dcnr.InteractionStore(rev[:m0], item[:m0], rating[:m0], fa[:e0], fb[:e0],
                                  n_items=f.n_items, n_reviewers=len(ids))
    store.on(dev)
    cm = np.linspace(m0, rev.size, 4).astype(int)
    ce = np.linspace(e0, fa.size, 4).astype(int)
    for i in range(3):
        store.append(rev[cm[i]:cm[i + 1]], item[cm[i]:cm[i + 1]], rating[cm[i]:cm[i + 1]],
                     fa[ce[i]:ce[i + 1]], fb[ce[i]:ce[i + 1]])
    sac_like = lambda s: {k: getattr(s, k) for k in sac.ARRAYS + sac.COUNTS}
    for k, v in sac_like(full).items():
        np.testing.assert_array_equal(getattr(store, k), v, err_msg=k)
    return store, full, reviewer, ids


def _answers_equal(got, want, what):
    assert len(got) == len(want)
    assert got.on_host.tolist() == want.on_host.tolist(), what
    for r, ((gr, gl), (wr, wl)) in enumerate(zip(got, want)):
        assert torch.equal(gr, wr) and torch.equal(gl, wl), (what, r)
        assert got.to_lists(r) == want.to_lists(r), (what, r)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_f11_served_from_an_appended_store(dev, precision):
    f = f11_common.load()
    pipe = _fixture_pipe(f, dev, precision)
    store, full, reviewer, ids = _f11_appended(f, dev)
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
    res, want = call(store), call(full)
    _answers_equal(res, want, precision)
    if precision == "fp32":   # what the reference service answered (expected.json)
        n_by = 0
        for r, q in enumerate(reqs):
            ranked, _, by = res.to_lists(r)
            assert [f.rev[x] for x in ranked] == q["ranked_hotels"], q
            assert [[int(ids[x]) for x in lst] for lst in by] == q["recommended_by"], q
            n_by += sum(len(b) for b in by)
        assert n_by >= 10


# ------------------------------------------------------------ 4: a random store
def test_random_store_with_a_reviewer_over_sv_max(dev):
    import dcnr
    U, M, E, N_ITEMS = 300, 6000, 2500, 200
    cfg = dict(n_users=400, n_items=N_ITEMS, cat_dims={"a": 30, "b": 250}, n_num=4,
               params=dict(emb_dim=32, hidden_dim=64, n_cross_layers=2, n_res_blocks=2, dropout=0.0))
    m = our_model(cfg, precision="bf16", seed=9).to(dev).eval()
    rng = np.random.default_rng(2)
    item_cat = np.stack([rng.integers(0, c, N_ITEMS) for c in cfg["cat_dims"].values()], 1)
    pipe = dcnr.RankingPipeline(m, item_cat, rng.random((N_ITEMS, 4), dtype=np.float32))
    rev, item, rating, fa, fb = f11_common.random_tables(U, M, E, N_ITEMS, seed=11)
    # HEAVY ends above SV_MAX review rows: its own requests, and those of its
    # friends, are answered on the host
    HEAVY = 77
    n_more = SV_MAX + 10 - int((rev == HEAVY).sum())
    rev = np.r_[rev, np.full(n_more, HEAVY)]
    item = np.r_[item, rng.integers(0, N_ITEMS, n_more)]
    rating = np.r_[rating, rng.integers(1, 11, n_more).astype(np.float64)]
    M = rev.size
    m0, e0 = 3500, 1200
    store = dcnr.InteractionStore(rev[:m0], item[:m0], rating[:m0], fa[:e0], fb[:e0],
                                  n_items=N_ITEMS, n_reviewers=U)
    store.on(dev)
    assert store.n_rows[HEAVY] <= SV_MAX
    cm, ce = [m0, 4000, 6000, M], [e0, 1201, 2000, E]
    rv = [HEAVY, HEAVY, -1, 3] + rng.integers(0, U, 36).tolist()
    modes = ["personal", "friends"] * 20
    friend = int(f11_common.PandasStore(rev, item, rating, fa, fb).friends(HEAVY).pop())
    rv[4], modes[4] = friend, "friends"
    users = rng.integers(0, cfg["n_users"], 40).tolist()
    call = lambda s: pipe.recommend_users(s, users, rv, modes, lambda_param=[1.0, 0.3] * 20,
                                          top_k=[20, 5] * 20)
    for i in range(3):
        store.append(rev[cm[i]:cm[i + 1]], item[cm[i]:cm[i + 1]], rating[cm[i]:cm[i + 1]],
                     fa[ce[i]:ce[i + 1]], fb[ce[i]:ce[i + 1]])
        rebuilt = dcnr.InteractionStore(rev[:cm[i + 1]], item[:cm[i + 1]], rating[:cm[i + 1]],
                                        fa[:ce[i + 1]], fb[:ce[i + 1]], n_items=N_ITEMS,
                                        n_reviewers=U)
        same_generation(store.on(dev)[1], rebuilt.on(dev)[1], i)
        res, want = call(store), call(rebuilt)
        _answers_equal(res, want, i)
    assert store.n_rows[HEAVY] > SV_MAX
    assert res.on_host[0] and res.on_host[4] and not res.on_host[2:4].any()
    assert sum(r[0].numel() > 0 for r in res) > 20
