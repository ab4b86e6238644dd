"""A batch of /recommendations requests in one device pass
(``RankingPipeline.recommend_many``, dcnr_requests_*): every request's answer
must be exactly what the one-request path gives.

  1  the F7 fixture's requests (the reference service's responses) in ONE call
  2  the batched kernels against compositions of the one-request entry points,
     through the C ABI, on hand-made segments: torch.equal, equal counts
  3  end to end against ``recommend()`` on a synthetic pipeline, bf16 and fp32
  4  a request above the kernels' capacity is answered by ``recommend()``
  5  a non-default stream; two host threads on one pipeline

Everything compared is an integer result or a logit the same kernels computed,
so every comparison is an equality.  (That a row's eval logit does not depend
on the batch it is scored in, below TOWER_MIN_B rows: the layer-by-layer
forward never splits K and its head sums a fixed number of partials per row;
test 3 checks it.)
"""
import threading

import numpy as np
import pytest
import torch

import f7_common
from helpers import our_model

pytestmark = pytest.mark.gpu

SV_MAX = 4096
MMR_LDS_MAX = 152 * 1024      # csrc/serving.hip
OVERFLOW, BAD_DATA = 1, 2     # DCNR_REQ_*


def lds_limit(d):
    """Largest n the LDS-resident MMR holds: (n (d + 1) + n) floats <= MMR_LDS_MAX."""
    return MMR_LDS_MAX // 4 // (d + 2)


# ---------------------------------------------------------------- C ABI wrappers
def _t(a, dtype, dev):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def _csr(lists, dev):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in lists] + [np.zeros(0, np.int64)])
    return _t(flat, torch.int64, dev), _t(off, torch.int64, dev), off


def c_candidates(dev, pos, idx, k, sets, a_idx, e_idx, f_idx, min_c, n_items, cap):
    """dcnr_requests_candidates over R requests: pos[r] rows, idx[r] [Q_r, k]."""
    from dcnr import _lib
    lib = _lib.load()
    R = len(pos)
    d_pos, d_pos_off, pos_off = _csr(pos, dev)
    Q = int(pos_off[-1])
    d_idx = _t(np.concatenate([np.asarray(i, np.int64).reshape(-1, k) for i in idx] +
                              [np.zeros((0, k), np.int64)]), torch.int64, dev)
    d_sets, d_set_off, set_off = _csr(sets, dev)
    S = len(sets)
    ix = [_t(v, torch.int32, dev) if S else None for v in (a_idx, e_idx, f_idx)]
    slots = torch.full((R, cap), -7, dtype=torch.int64, device=dev)
    count = torch.full((R,), -7, dtype=torch.int32, device=dev)
    status = torch.full((R,), -7, dtype=torch.int32, device=dev)
    offsets = torch.full((R + 1,), -7, dtype=torch.int64, device=dev)
    h_off = torch.full((R + 1,), -7, dtype=torch.int64).pin_memory()
    h_status = torch.full((R,), -7, dtype=torch.int32).pin_memory()
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    _lib.check(lib.dcnr_requests_candidates(
        p(d_pos), d_pos_off.data_ptr(), R, Q, p(d_idx), k, p(d_sets), d_sets.numel(),
        d_set_off.data_ptr() if S else None, S, p(ix[0]), p(ix[1]), p(ix[2]), min_c, n_items, cap,
        slots.data_ptr(), count.data_ptr(), status.data_ptr(), offsets.data_ptr(),
        h_off.data_ptr(), h_status.data_ptr(), _lib.stream_ptr(dev)), "dcnr_requests_candidates")
    torch.cuda.current_stream(dev).synchronize()
    assert torch.equal(h_status, status.cpu())       # the pinned mirror of the status words
    return slots, count, status, offsets, h_off


def ref_union(dev, pos, idx, k):
    """dcnr_candidate_union of one request."""
    from dcnr import _lib
    lib = _lib.load()
    Q = len(pos)
    if Q == 0:
        return torch.empty(0, dtype=torch.int64, device=dev)
    p_, i_ = _t(pos, torch.int64, dev), _t(np.asarray(idx).reshape(Q, k), torch.int64, dev)
    out = torch.empty(Q * k, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.dcnr_candidate_union(p_.data_ptr(), Q, i_.data_ptr(), k, out.data_ptr(),
                                        cnt.data_ptr(), _lib.stream_ptr(dev)), "union")
    return out[:int(cnt.item())]


def ref_candidates(dev, pos, idx, k, fallback, allowed, excluded, min_c):
    """The one-request composition recommend() makes: union, torch.unique for
    the fallback, Python sets for the filters."""
    cand = ref_union(dev, pos, idx, k)
    if fallback is not None and cand.numel() < min_c:
        cand = torch.unique(torch.cat([cand, _t(fallback, torch.int64, dev)]))
    if allowed is not None or excluded is not None:
        keep = set(cand.tolist())
        if allowed is not None:
            keep &= set(int(a) for a in allowed)
        if excluded is not None:
            keep -= set(int(e) for e in excluded)
        cand = torch.tensor(sorted(keep), dtype=torch.int64, device=dev)
    return cand


# --------------------------------------------------- 2a: candidates, stage level
N_ITEMS = 5000


def candidate_requests(R, k, seed):
    """R hand-made requests cycling through every branch: staged lists of 0, 1,
    2, 64, 65, 1023, 1024, 1025, 4096 entries (k = 1) or up to 4092 and past
    SV_MAX (k = 11); rows of -1 among positives and neighbours; a positive
    repeated; allowed sets absent / empty / superset / disjoint / partial; an
    excluded set; the fallback at min_candidates - 1 rows (joins) and at
    min_candidates rows (does not)."""
    rng = np.random.default_rng(seed)
    all_rows = np.arange(N_ITEMS)
    sets = [np.zeros(0, np.int64),                                   # 0: empty
            all_rows,                                                # 1: superset
            np.arange(N_ITEMS - 40, N_ITEMS),                        # 2: a far corner
            np.sort(rng.choice(N_ITEMS, N_ITEMS // 2, replace=False)),   # 3: half of the rows
            np.sort(rng.choice(N_ITEMS, 100, replace=False)),        # 4: "popular" fallback
            np.arange(SV_MAX)]                                       # 5: a fallback of SV_MAX rows
    qs = [0, 1, 2, 64, 65, 1023, 1024, 1025, 4096] if k == 1 else [0, 1, 3, 32, 93, 372, 373, 7]
    pos, idx, a_idx, e_idx, f_idx = [], [], [], [], []
    for r in range(R):
        Q = qs[r % len(qs)]
        if r % 11 == 5:      # exactly 19 distinct rows, one repeated: the fallback joins
            p = np.r_[np.arange(100, 119), 100] if k == 1 else np.arange(100, 102)
        elif r % 11 == 6:    # exactly 20 distinct rows: it does not
            p = np.arange(200, 220) if k == 1 else np.arange(200, 202)
        elif r % 11 == 7:    # one row outside the 4096-row fallback: 4097 rows overflow
            p = np.array([4500])
        elif r % 11 == 8:    # no positives: the fallback alone, exactly SV_MAX rows
            p = np.zeros(0, np.int64)
        else:
            p = rng.integers(0, N_ITEMS if r % 3 else 300, Q)   # (r % 3 == 0: many duplicates)
            if Q > 2:
                p[rng.integers(0, Q)] = -1
                p[1] = p[0]
        i = rng.integers(0, N_ITEMS, (len(p), k))
        i[rng.random(i.shape) < 0.05] = -1
        if r % 11 == 5 and k > 1:      # 2 positives + 17 distinct neighbours = 19 rows
            i[:] = 100
            i[0, 1:10], i[1, 1:9] = np.arange(300, 309), np.arange(400, 408)
        if r % 11 == 6 and k > 1:      # ... + 18 = 20 rows
            i[:] = 200
            i[0, 1:10], i[1, 1:10] = np.arange(300, 309), np.arange(400, 409)
        if r % 11 == 7:
            i[:] = 4500
        pos.append(p.astype(np.int64))
        idx.append(i.astype(np.int64))
        a_idx.append([-1, 0, 1, 2, 3][r % 5])
        e_idx.append([-1, 3, -1, 2][r % 4])
        f_idx.append(4 if r % 11 in (5, 6) else 5 if r % 11 in (7, 8) else [-1, 4, 5][r % 3])
        if r % 11 in (5, 6):
            a_idx[-1], e_idx[-1] = -1, -1
    return sets, pos, idx, a_idx, e_idx, f_idx


@pytest.mark.parametrize("k", [1, 11])
@pytest.mark.parametrize("R", [1, 3, 37, 300])
def test_candidates_equal_single_request_composition(dev, R, k):
    sets, pos, idx, a_idx, e_idx, f_idx = candidate_requests(R, k, seed=R * 16 + k)
    min_c = 20
    slots, count, status, offsets, h_off = c_candidates(dev, pos, idx, k, sets, a_idx, e_idx, f_idx,
                                                        min_c, N_ITEMS, SV_MAX)
    count, status = count.cpu().numpy(), status.cpu().numpy()
    seen = set()
    for r in range(R):
        pick = lambda ix: None if ix[r] < 0 else sets[ix[r]]
        staged = len(pos[r]) * k
        if staged <= SV_MAX:
            want = ref_candidates(dev, pos[r], idx[r], k, pick(f_idx), pick(a_idx), pick(e_idx), min_c)
            # the union before the filters, for the overflow rule
            un = ref_candidates(dev, pos[r], idx[r], k, pick(f_idx), None, None, min_c)
        if staged > SV_MAX or un.numel() > SV_MAX:
            assert status[r] == OVERFLOW and count[r] == 0, r
            seen.add("overflow")
            continue
        assert status[r] == 0 and count[r] == want.numel(), (r, count[r], want.numel())
        assert torch.equal(slots[r, :count[r]], want), r
        if f_idx[r] == 4 and r % 11 == 5:
            assert want.numel() > min_c
            seen.add("fallback joined")
        if f_idx[r] == 4 and r % 11 == 6:
            assert want.numel() == min_c
            seen.add("fallback not needed")
    want_off = np.r_[0, np.cumsum(count)]
    assert offsets.cpu().numpy().tolist() == want_off.tolist()
    assert h_off.numpy().tolist() == want_off.tolist()      # the pinned mirror
    if R >= 37:
        assert seen == {"overflow", "fallback joined", "fallback not needed"}


def test_candidates_small_slot_and_no_sets(dev):
    """cap below the result: that request overflows, its neighbours do not;
    S = 0 with null index arrays; n_items bounds the rows by value."""
    pos = [np.arange(10), np.arange(30), np.zeros(0, np.int64)]
    idx = [np.zeros((len(p), 1), np.int64) for p in pos]
    none = [-1, -1, -1]
    slots, count, status, offsets, _ = c_candidates(dev, pos, idx, 1, [], none, none, none, 20, 100, 16)
    assert status.tolist() == [0, OVERFLOW, 0] and count.tolist() == [10, 0, 0]
    assert slots[0, :10].tolist() == list(range(10)) and offsets.tolist() == [0, 10, 10, 10]


# ------------------------------------------------- 2b: rank + MMR, stage level
def make_table(d, dev, seed=0):
    from dcnr import serving
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((N_ITEMS, d)).astype(np.float32)
    emb[N_ITEMS // 2:] = emb[:N_ITEMS // 2]      # duplicate rows: exactly equal similarities
    emb[7] = 0.0                                  # a zero-norm row
    table = torch.from_numpy(emb).to(dev)
    return table, serving.row_inv_norms(table)


def rank_segments(lengths, seed):
    """One segment per (length, lambda, top_k) combination given: candidate rows
    (some -1, duplicates of embedding rows) and scores with planted ties."""
    rng = np.random.default_rng(seed)
    segs = []
    for j, (n, lam, tk) in enumerate(lengths):
        rows = rng.integers(0, N_ITEMS, n).astype(np.int64)
        if n > 3:
            rows[rng.choice(n, max(1, n // 40), replace=False)] = -1
        if j % 5 == 4 and n:
            rows[0] = -1                             # the always-taken first has no embedding
        if j % 3 == 0:
            s = rng.integers(-6, 6, n).astype(np.float32) / 4      # runs of equal scores
        elif j % 3 == 1:
            s = np.full(n, 0.5, np.float32)                        # all equal: position decides
        else:
            s = rng.standard_normal(n).astype(np.float32)
        segs.append((rows, s, lam, tk))
    return segs


def ref_rank_mmr(dev, table, inv, rows, scores, lam, tk):
    """dcnr_rank_by_score, then dcnr_mmr_rerank when lambda < 1."""
    from dcnr import _lib
    lib = _lib.load()
    n = len(rows)
    r_, s_ = _t(rows, torch.int64, dev), _t(scores, torch.float32, dev)
    if n == 0:
        return r_, s_
    order = torch.empty(n, dtype=torch.int64, device=dev)
    _lib.check(lib.dcnr_rank_by_score(s_.data_ptr(), n, order.data_ptr(), _lib.stream_ptr(dev)), "rank")
    ranked, rs = r_[order].contiguous(), s_[order].contiguous()
    if not lam < 1.0:
        return ranked, rs
    out = torch.empty(tk, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.dcnr_mmr_rerank(table.data_ptr(), inv.data_ptr(), table.shape[1], ranked.data_ptr(),
                                   rs.data_ptr(), n, float(lam), tk, out.data_ptr(), cnt.data_ptr(),
                                   _lib.stream_ptr(dev)), "mmr")
    p = out[:int(cnt.item())]
    return ranked[p], rs[p]


def c_rank_mmr(dev, table, inv, segs, cap):
    from dcnr import _lib
    lib = _lib.load()
    R = len(segs)
    off = np.zeros(R + 1, np.int64)
    np.cumsum([len(s[0]) for s in segs], out=off[1:])
    n = int(off[-1])
    slots = np.full((R, cap), -3, np.int64)
    for r, s in enumerate(segs):
        slots[r, :len(s[0])] = s[0]
    d_slots = _t(slots, torch.int64, dev)
    logits = _t(np.concatenate([s[1] for s in segs] + [np.zeros(0, np.float32)]), torch.float32, dev)
    lam = _t([s[2] for s in segs], torch.float32, dev)
    tk = _t([s[3] for s in segs], torch.int32, dev)
    d_off = _t(off, torch.int64, dev)
    out_rows = torch.full((max(n, 1),), -9, dtype=torch.int64, device=dev)
    out_logits = torch.full((max(n, 1),), -9.0, dtype=torch.float32, device=dev)
    out_count = torch.full((R,), -9, dtype=torch.int32, device=dev)
    status = torch.zeros(R, dtype=torch.int32, device=dev)
    nb = int(lib.dcnr_requests_workspace_size(R, 0, 1, cap))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.check(lib.dcnr_requests_rank_mmr(
        logits.data_ptr() if n else out_logits.data_ptr(), n, d_slots.data_ptr(), cap,
        d_off.data_ptr(), R, table.data_ptr(), inv.data_ptr(), table.shape[1], table.shape[0],
        lam.data_ptr(), tk.data_ptr(), out_rows.data_ptr(), out_logits.data_ptr(),
        out_count.data_ptr(), status.data_ptr(), ws.data_ptr(), nb, _lib.stream_ptr(dev)),
        "dcnr_requests_rank_mmr")
    return off, out_rows, out_logits, out_count.cpu().numpy(), status.cpu().numpy()


def check_rank_mmr(dev, table, inv, segs, cap=SV_MAX):
    off, out_rows, out_logits, count, status = c_rank_mmr(dev, table, inv, segs, cap)
    assert not status.any()
    for r, (rows, s, lam, tk) in enumerate(segs):
        want_rows, want_s = ref_rank_mmr(dev, table, inv, rows, s, lam, tk)
        o = int(off[r])
        assert count[r] == want_rows.numel(), (r, len(rows), lam, tk, count[r], want_rows.numel())
        assert torch.equal(out_rows[o:o + count[r]], want_rows), (r, len(rows), lam, tk)
        assert torch.equal(out_logits[o:o + count[r]], want_s), (r, len(rows), lam, tk)


@pytest.mark.parametrize("d", [24, 32, 64])
def test_rank_mmr_every_length_and_form(dev, d):
    """Every segment length at which the sort or the MMR changes shape, and the
    LDS-resident form's limit for this d from both sides; lambda 0 / 0.3 / 1;
    top_k 1, 5, 20 and above n."""
    table, inv = make_table(d, dev)
    lim = lds_limit(d)
    lengths = [0, 1, 2, 64, 65, 1023, 1024, 1025, 4096, lim, lim + 1]
    combos = []
    for j, n in enumerate(lengths):
        for lam in (0.0, 0.3, 1.0):
            # top_k 1, 5, 20 and above n, dealt over the lengths so that each meets each lambda
            for tk in ((1, 20) if (j + int(lam * 10)) % 2 else (5, n + 7)):
                combos.append((n, lam, tk))
    check_rank_mmr(dev, table, inv, rank_segments(combos, seed=d))


@pytest.mark.parametrize("R", [1, 3, 37, 300])
def test_rank_mmr_request_counts(dev, R):
    """R = 1 .. more workgroups than the card has CUs, short mixed segments."""
    table, inv = make_table(32, dev)
    rng = np.random.default_rng(R)
    combos = [(int(rng.choice([0, 1, 2, 17, 64, 65, 130, 300])), [0.0, 0.3, 1.0][r % 3],
               [1, 5, 20, 400][r % 4]) for r in range(R)]
    check_rank_mmr(dev, table, inv, rank_segments(combos, seed=100 + R), cap=512)


# ------------------------------------------------------------------- 1: F7
def _f7_pipe(f, dev):
    import dcnr
    m = dcnr.DCN_RecSys(f.n_users, f.n_items, f.cat_dims, f.n_num, dict(f.params),
                        precision="fp32")
    m.load_state_dict(f.state)
    m = m.to(dev).eval()
    return dcnr.RankingPipeline(m, f.item_cat, f.item_num,
                                item_embeddings=torch.from_numpy(f.emb).to(dev))


def test_f7_in_one_call(dev):
    f = f7_common.load()
    pipe = _f7_pipe(f, dev)
    reqs = f.expected["recommendations"]
    rows = [f7_common.request_rows(f, q) for q in reqs]
    city_sets = {}     # city -> (index of its hotels' set, index of its popular list)
    for q, r in zip(reqs, rows):
        if q["city"] not in city_sets:
            city_sets[q["city"]] = tuple(pipe.register_sets([r["allowed"], r["fallback"]]))
    got = pipe.recommend_many([r["user_row"] for r in rows], [r["pos"] for r in rows],
                              lambda_param=[q["lambda_param"] for q in reqs],
                              allowed=[city_sets[q["city"]][0] for q in reqs],
                              excluded=[r["excluded"] for r in rows],
                              fallback=[city_sets[q["city"]][1] for q in reqs])
    assert len(got) == len(reqs)
    n_mmr = 0
    for q, (ranked, logits) in zip(reqs, got):
        ids = [f.rev[x] for x in ranked.tolist()]
        assert ids == q["ranked_hotels"], (q, ids)
        assert logits.numel() == ranked.numel()
        n_mmr += q["lambda_param"] < 1.0 and len(ids) > 1
    assert n_mmr >= 5 and any(len(q["ranked_hotels"]) == 0 for q in reqs)
    # /similar_items, the cases the service answered, one call per n
    cases = [c for c in f.expected["similar_items"] if c["status"] == 200]
    assert cases
    for n in sorted({c["n"] for c in cases}):
        cs = [c for c in cases if c["n"] == n]
        idx = pipe.similar_items_many([f.item_map[c["item_id"]] for c in cs], n).tolist()
        for c, row in zip(cs, idx):
            assert [f.rev[x] for x in row] == c["ids"], c


# ---------------------------------------------------- 3-5: synthetic pipeline
CFG = dict(n_users=900, n_items=N_ITEMS, cat_dims={"a": 30, "b": 250, "c": 1000}, n_num=4,
           params=dict(emb_dim=32, hidden_dim=64, n_cross_layers=2, n_res_blocks=2, dropout=0.0))


def synth_pipe(dev, precision):
    import dcnr
    m = our_model(CFG, precision=precision, seed=9).to(dev).eval()
    rng = np.random.default_rng(2)
    item_cat = np.stack([rng.integers(0, c, N_ITEMS) for c in CFG["cat_dims"].values()], 1)
    item_num = rng.random((N_ITEMS, 4), dtype=np.float32)
    return dcnr.RankingPipeline(m, item_cat, item_num)


_pipes = {}


def get_pipe(dev, precision):
    if precision not in _pipes:
        _pipes[precision] = synth_pipe(dev, precision)
    return _pipes[precision]


def mixed_requests(R, seed):
    """0, 1 and 32 positives; filters, fallback and MMR settings mixed."""
    rng = np.random.default_rng(seed)
    popular = np.sort(rng.choice(N_ITEMS, 100, replace=False)).tolist()
    half = np.sort(rng.choice(N_ITEMS, N_ITEMS // 2, replace=False)).tolist()
    reqs = []
    for r in range(R):
        Q = [0, 1, 32][r % 3]
        pos = rng.choice(N_ITEMS, Q, replace=False).tolist()
        if Q == 32 and r % 2:
            pos[5] = pos[4]                         # a positive repeated
        reqs.append(dict(user=int(rng.integers(0, CFG["n_users"])), pos=pos,
                         lam=[1.0, 0.7, 0.3, 0.0][r % 4], top_k=[20, 5, 1, 500][(r // 4) % 4],
                         allowed=[None, half, list(range(N_ITEMS)), []][(r // 2) % 4],
                         excluded=[None, pos[:3] + popular[:5]][(r // 3) % 2],
                         fallback=[popular, None, popular][r % 3] if r % 5 else None))
    return reqs, popular, half


def run_many(pipe, reqs, popular=None, half=None, registered=None):
    """recommend_many over reqs; with `registered` = (popular, half) set
    indices, the two shared lists go by index and the rest per call."""
    def arg(v):
        if registered and v is popular:
            return registered[0]
        if registered and v is half:
            return registered[1]
        return v
    return pipe.recommend_many([q["user"] for q in reqs], [q["pos"] for q in reqs],
                               lambda_param=[q["lam"] for q in reqs],
                               top_k=[q["top_k"] for q in reqs],
                               allowed=[arg(q["allowed"]) for q in reqs],
                               excluded=[arg(q["excluded"]) for q in reqs],
                               fallback=[arg(q["fallback"]) for q in reqs])


def run_single(pipe, q):
    return pipe.recommend(q["user"], q["pos"], lambda_param=q["lam"], top_k=q["top_k"],
                          allowed=q["allowed"], excluded=q["excluded"], fallback=q["fallback"])


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for r, ((gr, gl), (wr, wl)) in enumerate(zip(got, want)):
        assert torch.equal(gr, wr), (what, r, gr.numel(), wr.numel())
        assert torch.equal(gl, wl), (what, r)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_recommend_many_equals_recommend(dev, precision):
    pipe = get_pipe(dev, precision)
    reqs, popular, half = mixed_requests(40, seed=5)
    registered = pipe.register_sets([popular, half])
    want = [run_single(pipe, q) for q in reqs]
    got = run_many(pipe, reqs, popular, half, registered)
    assert sum(w[0].numel() for w in want) < 16384      # both sides: the layer-by-layer forward
    assert sum(w[0].numel() > 0 for w in want) > 20 and any(w[0].numel() == 0 for w in want)
    assert_same(got, want, precision)
    # per-call sets instead of registered ones: the same mechanism, the same answers
    assert_same(run_many(pipe, reqs), want, precision + " ad hoc")
    # the batched logits are the model's over the concatenated ranking batch:
    # lambda = 1 returns every candidate of every request
    full = pipe.recommend_many([q["user"] for q in reqs], [q["pos"] for q in reqs], 1.0,
                               allowed=[q["allowed"] for q in reqs],
                               excluded=[q["excluded"] for q in reqs],
                               fallback=[q["fallback"] for q in reqs])
    batch, logits = [], []
    for q, (rows, z) in zip(reqs, full):
        order = torch.argsort(rows)                  # candidates ascending, as scored
        batch.append(pipe.ranking_batch(q["user"], rows[order]))
        logits.append(z[order])
    with torch.no_grad():
        z = pipe.model(*[torch.cat([b[j] for b in batch]) for j in range(4)]).reshape(-1)
    assert torch.equal(torch.cat(logits), z)


def test_set_lists_of_none_on_a_fresh_pipeline(dev):
    """Lists whose entries are all None name no set (a batch in which nobody has
    negatives): no registered sets, S = 0, and the answers of recommend()."""
    pipe = synth_pipe(dev, "bf16")
    reqs, _, _ = mixed_requests(7, seed=12)
    nones = [None] * len(reqs)
    for q in reqs:
        q.update(allowed=None, excluded=None, fallback=None)
    want = [run_single(pipe, q) for q in reqs]
    for kw in (dict(allowed=nones), dict(excluded=nones), dict(fallback=nones),
               dict(allowed=nones, excluded=nones, fallback=nones)):
        got = pipe.recommend_many([q["user"] for q in reqs], [q["pos"] for q in reqs],
                                  lambda_param=[q["lam"] for q in reqs],
                                  top_k=[q["top_k"] for q in reqs], **kw)
        assert_same(got, want, str(sorted(kw)))
    # ... and beside one request that does name a set
    reqs[2]["excluded"] = reqs[2]["pos"][:1] + [17]
    got = run_many(pipe, reqs)
    assert_same(got, [run_single(pipe, q) for q in reqs], "one set")


def test_lambda_that_rounds_to_one(dev):
    """recommend() decides lambda < 1 on the Python double and computes with its
    float32; 1 - 2^-30 is such a lambda (MMR with lambda 1.0f, top_k items)."""
    pipe = get_pipe(dev, "bf16")
    reqs, _, _ = mixed_requests(6, seed=14)
    for q in reqs:
        q.update(lam=1.0 - 2.0 ** -30, top_k=5)
    reqs[0]["lam"] = 0.5
    want = [run_single(pipe, q) for q in reqs]
    assert any(0 < w[0].numel() <= 5 for w in want[1:])
    assert_same(run_many(pipe, reqs), want, "lambda")


def test_index_and_feature_tables_must_match(dev):
    import dcnr
    pipe = get_pipe(dev, "bf16")
    emb = pipe.index._table[:N_ITEMS - 10]
    short = dcnr.RankingPipeline(pipe.model, pipe.item_cat, pipe.item_num, item_embeddings=emb)
    with pytest.raises(ValueError):
        short.recommend_many([0], [[1]])


def test_logits_without_a_rank_mark_the_answer(dev):
    """A -inf or NaN logit has no place in the order: that request ends with
    count 0, the bad-data bit, rows -1 and logits NaN over its whole segment (the
    Python layer reads nothing back after the forward); its neighbours are
    answered.  Every position the kernel uses is checked first."""
    table, inv = make_table(32, dev)
    segs = rank_segments([(70, 1.0, 20), (70, 0.3, 20), (70, 1.0, 20), (1500, 0.3, 5), (9, 0.0, 3)],
                         seed=77)
    segs[0][1][3] = -np.inf
    segs[1][1][69] = np.nan
    segs[3][1][0] = -np.inf
    off, out_rows, out_logits, count, status = c_rank_mmr(dev, table, inv, segs, 2048)
    assert status.tolist() == [BAD_DATA, BAD_DATA, 0, BAD_DATA, 0]
    assert count.tolist() == [0, 0, 70, 0, 3]
    for r in (0, 1, 3):
        assert (out_rows[off[r]:off[r + 1]] == -1).all()
        assert torch.isnan(out_logits[off[r]:off[r + 1]]).all()
    for r in (2, 4):
        want_rows, want_s = ref_rank_mmr(dev, table, inv, *segs[r])
        assert torch.equal(out_rows[off[r]:off[r] + count[r]], want_rows)
        assert torch.equal(out_logits[off[r]:off[r] + count[r]], want_s)


def test_host_validation(dev):
    pipe = get_pipe(dev, "bf16")
    assert pipe.recommend_many([], []) == []
    with pytest.raises(ValueError):
        pipe.recommend_many([0], [[N_ITEMS]])                       # positive outside the table
    with pytest.raises(ValueError):
        pipe.recommend_many([CFG["n_users"]], [[1]])                # user outside the table
    with pytest.raises(ValueError):
        pipe.recommend_many([0], [[1]], allowed=[[-1, 3]])          # set row outside the table
    with pytest.raises(ValueError):
        pipe.register_sets([[N_ITEMS]])
    with pytest.raises(ValueError):
        pipe.recommend_many([0], [[1]], fallback=[10 ** 6])         # not a registered set
    a = pipe.register_sets([[5, 3, 3, 9]])
    b = pipe.register_sets([[1], []])
    assert b == [a[0] + 1, a[0] + 2]                                # a later call appends


def test_overflow_is_answered_by_recommend(dev):
    """400 positives x 11 neighbours > SV_MAX: that request goes through
    recommend(); the others are what they are without it."""
    from dcnr import _lib  # noqa: F401
    pipe = get_pipe(dev, "bf16")
    reqs, popular, half = mixed_requests(6, seed=8)
    rng = np.random.default_rng(4)
    big = dict(reqs[1], pos=rng.choice(N_ITEMS, 400, replace=False).tolist(), lam=1.0,
               allowed=half, excluded=None)
    assert len(big["pos"]) * pipe.n_neighbors > SV_MAX
    with_big = reqs[:3] + [big] + reqs[3:]
    got = run_many(pipe, with_big)
    assert_same(got, [run_single(pipe, q) for q in with_big], "overflow")
    assert got[3][0].numel() > 0
    assert_same(got[:3] + got[4:], run_many(pipe, reqs), "others unchanged")
    # the raw status bit, through the C entry point
    pos = [np.arange(10), np.arange(400), np.arange(5)]
    idx = [rng.integers(0, N_ITEMS, (len(p), 11)) for p in pos]
    none = [-1] * 3
    _, count, status, _, _ = c_candidates(dev, pos, idx, 11, [], none, none, none, 20, N_ITEMS, SV_MAX)
    assert status.tolist() == [0, OVERFLOW, 0] and count[1] == 0 and count[0] > 0 and count[2] > 0


def test_other_stream_and_two_threads(dev):
    pipe = get_pipe(dev, "bf16")
    reqs_a, _, _ = mixed_requests(24, seed=31)
    reqs_b, _, _ = mixed_requests(17, seed=32)
    want_a, want_b = run_many(pipe, reqs_a), run_many(pipe, reqs_b)
    torch.cuda.synchronize()
    # a non-default stream with work queued ahead of the batch
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        x = torch.randn(2048, 2048, device=dev)
        for _ in range(8):
            x = x @ x * 1e-3
        got = run_many(pipe, reqs_a)
    side.synchronize()
    assert_same(got, want_a, "side stream")
    # two host threads on one pipeline (re-entrant)
    out, errors = {}, []
    start = threading.Barrier(2)

    def worker(name, reqs, own_stream):
        try:
            start.wait()
            for _ in range(3):
                if own_stream:
                    s = torch.cuda.Stream(dev)
                    with torch.cuda.stream(s):
                        res = run_many(pipe, reqs)
                    s.synchronize()
                else:
                    res = run_many(pipe, reqs)
                out[name] = [(r.clone(), z.clone()) for r, z in res]
        except BaseException as e:   # noqa: BLE001 -- reported by the main thread
            errors.append((name, e))

    ths = [threading.Thread(target=worker, args=("a", reqs_a, False)),
           threading.Thread(target=worker, args=("b", reqs_b, True))]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in ths), "a thread hung"
    assert not errors, errors
    torch.cuda.synchronize()
    assert_same(out["a"], want_a, "thread a")
    assert_same(out["b"], want_b, "thread b")
