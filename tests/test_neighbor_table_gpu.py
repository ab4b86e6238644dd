"""The item neighbour table (dcnr_cosine_neighbor_table,
``NearestNeighbors.build_neighbor_table``) and the request path that reads it
(dcnr_candidate_union_table, dcnr_requests_candidates_table,
``RankingPipeline(neighbor_table=...)``).

  1  the table against an independent torch fp32 brute force, test_knn_paths_gpu's
     comparison rule (distances at atol 2e-6, row ids at every isolated
     position, every list sorted by (dist, row)), planted ties on their own
  2  the table against the single-query search, bit for bit
  3  ranges split at awkward places, k = N, argument errors
  4  a range across scan v4's sample boundary, with the packed copy
  5  the table forms of the candidate kernels against the list forms, C ABI
  6  end to end: a table-backed pipeline answers as a scanning one does
  7  no launch of the top-k class in a table-backed request

Shapes (d, k) of 1 and 2 and the scan each takes for a chunk of queries
(knn.hip use_v4 / use_v2; the build keeps scan v3 out): (32, 11), (64, 11),
(64, 32) scan v4; (16, 11), (48, 11) scan v2 where an ordinary batched call
takes v3; (24, 11) scan v2; (128, 11) scan v1 by width; (64, 51) scan v1 by
k > 32.  The single-query side of 2 is scan v2 or v1 in every case.

The comparison rule is test_knn_paths_gpu's, with one thing mended for lists
by the thousand: whether the LAST position of a list is isolated also depends
on the reference's (k + 1)-th distance, which a k-long reference list does not
show (two rows within 2e-6 of each other either side of the cut are as
interchangeable as two inside the list; among 5003 x k positions some are).
So the reference is taken k + 1 long and its extra column only decides that.
"""
import numpy as np
import pytest
import torch

import f7_common
import test_knn_paths_gpu as kp
import test_recommend_many_gpu as rm
import test_recommend_users_gpu as ru

pytestmark = pytest.mark.gpu

ATOL = kp.ATOL
OK, BAD_ARG, WORKSPACE_TOO_SMALL = 0, 1, 5       # dcnr_status
OVERFLOW, BAD_DATA = 1, 2                        # DCNR_REQ_*
SHAPES = [(32, 11), (64, 11), (64, 32), (16, 11), (48, 11), (24, 11), (128, 11), (64, 51)]

_built = {}


def built(dev, d, k):
    """random_case's 5003-row table (20 copies of row 5, one zero row), its
    index, the full neighbour table with distances, and the torch reference --
    computed once per shape."""
    import dcnr
    if (d, k) not in _built:
        table, _, ties = kp.random_case(dev, d, 1, k)
        nn_ = dcnr.NearestNeighbors(n_neighbors=k).fit(table)
        dist, nbr = nn_.build_neighbor_table(return_distance=True)
        assert nbr.dtype == torch.int32 and nbr.shape == (table.shape[0], k)
        assert nn_.neighbor_table_ is nbr
        zero = int((table == 0).all(1).nonzero()[0, 0])
        ref_d, ref_i = reference(table, 0, table.shape[0], k + 1)
        _built[(d, k)] = dict(table=table, nn=nn_, dist=dist, nbr=nbr, ties=ties, zero=zero,
                              ref_d=ref_d, ref_i=ref_i)
    return _built[(d, k)]


def reference(table, lo, hi, k, block=1024):
    """torch fp32 1 - tn @ tn.T top-k of rows [lo, hi), in row blocks."""
    tn = table / table.norm(dim=1, keepdim=True).clamp_min(1e-30)
    ds, is_ = [], []
    for b in range(lo, hi, block):
        d_, i_ = torch.topk((1.0 - tn[b:min(b + block, hi)] @ tn.T).clamp(0, 2), k, dim=1,
                            largest=False)
        ds.append(d_)
        is_.append(i_)
    return torch.cat(ds).cpu().numpy(), torch.cat(is_).cpu().numpy()


def check_against_reference(dist_, idx, ref_d, ref_i):
    """kp.check_against_reference for lists [Q, k] against a reference
    [Q, k + 1]: distances at atol ATOL; row ids at every position whose
    reference distance is not within ATOL of the one before or behind it (the
    (k + 1)-th included); every list ascending by (dist, row).  Returns the
    isolated share."""
    k = dist_.shape[1]
    assert ref_d.shape == (dist_.shape[0], k + 1)
    np.testing.assert_allclose(dist_, ref_d[:, :k], rtol=0, atol=ATOL)
    near = np.diff(ref_d, axis=1) <= ATOL          # [Q, k]: positions j and j + 1
    iso = ~near
    iso[:, 1:] &= ~near[:, :k - 1]
    np.testing.assert_array_equal(idx[iso], ref_i[:, :k][iso])
    d0, d1, i0, i1 = dist_[:, :-1], dist_[:, 1:], idx[:, :-1], idx[:, 1:]
    assert np.all((d0 < d1) | ((d0 == d1) & (i0 < i1)))
    return float(iso.mean())


def check_planted(dist, nbr, rows0, ties, zero, k):
    """dist / nbr: numpy lists of rows rows0 + [0 .. len).  Every copy lists the
    copies first, ascending rows, one distance <= ATOL; the zero row is at
    distance 1 from everything, ascending rows."""
    m = min(k, ties.size)
    for r in ties:
        assert nbr[r - rows0][:m].tolist() == ties[:m].tolist(), r
        assert np.all(dist[r - rows0][:m] == dist[r - rows0][0]) and dist[r - rows0][0] <= ATOL, r
    assert nbr[zero - rows0].tolist() == list(range(k))
    assert np.all(dist[zero - rows0] == 1.0)


def single_queries(nn_, table, rows, k):
    """kneighbors_device of each row alone: (dist [n, k], idx int32 [n, k])."""
    out = [nn_.kneighbors_device(table[r:r + 1], k) for r in rows]
    return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out]).to(torch.int32)


# ------------------------------------------------------------ 1: brute force
@pytest.mark.parametrize("d,k", SHAPES)
def test_table_against_brute_force(dev, d, k):
    b = built(dev, d, k)
    dist, nbr = b["dist"].cpu().numpy(), b["nbr"].cpu().numpy()
    check_planted(dist, nbr, 0, b["ties"], b["zero"], k)
    rest = np.ones(dist.shape[0], bool)
    rest[b["ties"]] = False
    rest[b["zero"]] = False
    share = check_against_reference(dist[rest], nbr[rest], b["ref_d"][rest], b["ref_i"][rest])
    print(f"d={d} k={k}: isolated share {share:.4f}")
    assert share >= 0.95


# ---------------------------------------------------- 2: single-query search
@pytest.mark.parametrize("d,k", SHAPES)
def test_table_equals_single_query_search(dev, d, k):
    b = built(dev, d, k)
    N = b["table"].shape[0]
    rows = np.unique(np.r_[np.random.default_rng(d + k).choice(N, 256, replace=False),
                           b["ties"], b["zero"], 0, N - 1])
    d1, i1 = single_queries(b["nn"], b["table"], rows.tolist(), k)
    sel = torch.from_numpy(rows).to(dev)
    assert torch.equal(b["nbr"][sel], i1)
    assert torch.equal(b["dist"][sel], d1)


# ------------------------------------------------- 3: ranges, k = N, errors
@pytest.mark.parametrize("d", [64, 16])
def test_ranges_split_at_awkward_places(dev, d):
    """One row; 15, 16 and 17 rows (either side of the width from which an
    ordinary call takes scan v3 at d = 16); one whole chunk; a chunk and a
    row; the rest up to N."""
    b = built(dev, d, 11)
    N = b["table"].shape[0]
    cuts = [0, 1, 16, 32, 49, 49 + 1024, 49 + 1024 + 1025, N]
    parts = [b["nn"].build_neighbor_table(rows=(lo, hi), return_distance=True)
             for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert [p[1].shape[0] for p in parts] == np.diff(cuts).tolist()
    assert torch.equal(torch.cat([p[1] for p in parts]), b["nbr"])
    assert torch.equal(torch.cat([p[0] for p in parts]), b["dist"])
    assert b["nn"].neighbor_table_ is b["nbr"]          # a partial build is not kept
    # no distances asked for: the same rows
    assert torch.equal(b["nn"].build_neighbor_table(rows=(4000, N)), b["nbr"][4000:])


def test_k_equals_n(dev):
    import dcnr
    table = torch.randn(11, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    nn_ = dcnr.NearestNeighbors(n_neighbors=11).fit(table)
    dist, nbr = nn_.build_neighbor_table(return_distance=True)
    d1, i1 = single_queries(nn_, table, range(11), 11)
    assert torch.equal(nbr, i1) and torch.equal(dist, d1)
    assert all(sorted(r) == list(range(11)) for r in nbr.tolist())
    with pytest.raises(ValueError):
        nn_.build_neighbor_table(k=12)
    # fit drops the kept table
    assert nn_.neighbor_table_ is nbr
    nn_.fit(table)
    assert nn_.neighbor_table_ is None


def test_argument_errors(dev):
    from dcnr import _lib
    lib = _lib.load()
    b = built(dev, 64, 11)
    t, inv, N, k = b["nn"]._table, b["nn"]._inv, b["table"].shape[0], 11
    nb = int(lib.dcnr_cosine_neighbor_table_workspace_size(N, k))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    out = torch.full((32, k), -7, dtype=torch.int32, device=dev)

    def call(lo, hi, out_=out, ws_=ws, nbytes=nb, kk=k):
        return lib.dcnr_cosine_neighbor_table(t.data_ptr(), inv.data_ptr(), None, N, 64, kk, lo, hi,
                                              out_.data_ptr() if out_ is not None else None, None,
                                              ws_.data_ptr() if ws_ is not None else None, nbytes,
                                              _lib.stream_ptr(dev))
    assert call(5, 4) == BAD_ARG and call(N - 1, N + 1) == BAD_ARG and call(-1, 3) == BAD_ARG
    assert call(0, 8, kk=0) == BAD_ARG and call(0, 8, kk=N + 1) == BAD_ARG
    assert call(0, 32, nbytes=nb - 1) == WORKSPACE_TOO_SMALL
    torch.cuda.synchronize()
    assert bool((out == -7).all())                       # nothing was written by any of them
    # an empty range: DCNR_OK without a launch (no output, no workspace needed)
    _lib.profile_enable(1)
    try:
        _lib.profile_collect()
        assert call(7, 7, out_=None, ws_=None, nbytes=0) == OK
        assert _lib.profile_collect()["knn"][1] == 0
    finally:
        _lib.profile_enable(0)
    assert call(N - 32, N) == OK
    assert torch.equal(out, b["nbr"][N - 32:])


# ---------------------------------------- 4: across the v4 sample boundary
def test_range_across_the_sample_boundary_with_packed_rows(dev):
    """N = 70001 > PACKED_MIN_ROWS (the bf16 copy is read) and > V4_S = 65536
    (rows behind the admission bound's sample); rows [65000, 66000) only."""
    import dcnr
    N, d, k, lo, hi = 70001, 64, 11, 65000, 66000
    g = torch.Generator(device=dev).manual_seed(77)
    table = torch.randn(N, d, device=dev, generator=g)
    ties = np.sort(np.r_[65005, np.random.default_rng(5).choice(np.arange(lo, hi), 20, replace=False)])
    ties = np.unique(ties)
    zero = next(r for r in range(65700, hi) if r not in ties)
    # copies in front of the range and behind it as well: they must be listed
    outside = np.array([17, 40000, 65600 - 700, 69999])
    table[torch.from_numpy(np.r_[ties, outside]).to(dev)] = table[65005].clone()
    table[zero] = 0.0
    all_ties = np.sort(np.r_[ties, outside])
    nn_ = dcnr.NearestNeighbors(n_neighbors=k).fit(table)
    assert nn_._packed is not None
    dist, nbr = nn_.build_neighbor_table(rows=(lo, hi), return_distance=True)
    assert nn_.neighbor_table_ is None
    dn, nn = dist.cpu().numpy(), nbr.cpu().numpy()
    for r in ties:
        assert nn[r - lo].tolist() == all_ties[:k].tolist(), r
        assert np.all(dn[r - lo] == dn[r - lo][0]) and dn[r - lo][0] <= ATOL, r
    assert nn[zero - lo].tolist() == list(range(k)) and np.all(dn[zero - lo] == 1.0)
    ref_d, ref_i = reference(table, lo, hi, k + 1)
    rest = np.ones(hi - lo, bool)
    rest[ties - lo] = False
    rest[zero - lo] = False
    share = check_against_reference(dn[rest], nn[rest], ref_d[rest], ref_i[rest])
    print(f"N={N}: isolated share {share:.4f}")
    assert share >= 0.95
    rows = np.unique(np.r_[np.random.default_rng(6).choice(np.arange(lo, hi), 256, replace=False),
                           ties, zero, lo, hi - 1])
    d1, i1 = single_queries(nn_, table, rows.tolist(), k)
    sel = torch.from_numpy(rows - lo).to(dev)
    assert torch.equal(nbr[sel], i1) and torch.equal(dist[sel], d1)


# ------------------------------------------- 5: candidate kernels, C ABI
def c_candidates_table(dev, pos, nbr, k, sets, a_idx, e_idx, f_idx, min_c, n_items, cap):
    """dcnr_requests_candidates_table over R requests; as rm.c_candidates."""
    from dcnr import _lib
    lib = _lib.load()
    R = len(pos)
    d_pos, d_pos_off, pos_off = rm._csr(pos, dev)
    Q = int(pos_off[-1])
    d_sets, d_set_off, _ = rm._csr(sets, dev)
    S = len(sets)
    ix = [rm._t(v, torch.int32, dev) if S else None for v in (a_idx, e_idx, f_idx)]
    slots = torch.full((R, cap), -7, dtype=torch.int64, device=dev)
    count = torch.full((R,), -7, dtype=torch.int32, device=dev)
    status = torch.full((R,), -7, dtype=torch.int32, device=dev)
    offsets = torch.full((R + 1,), -7, dtype=torch.int64, device=dev)
    h_off = torch.full((R + 1,), -7, dtype=torch.int64).pin_memory()
    h_status = torch.full((R,), -7, dtype=torch.int32).pin_memory()
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    _lib.check(lib.dcnr_requests_candidates_table(
        p(d_pos), d_pos_off.data_ptr(), R, Q, nbr.data_ptr(), nbr.shape[1], k, p(d_sets),
        d_sets.numel(), d_set_off.data_ptr() if S else None, S, p(ix[0]), p(ix[1]), p(ix[2]), min_c,
        n_items, cap, slots.data_ptr(), count.data_ptr(), status.data_ptr(), offsets.data_ptr(),
        h_off.data_ptr(), h_status.data_ptr(), _lib.stream_ptr(dev)),
        "dcnr_requests_candidates_table")
    torch.cuda.current_stream(dev).synchronize()
    assert torch.equal(h_status, status.cpu())       # the pinned mirror of the status words
    return slots, count, status, offsets, h_off


def table_requests(R, k, kt, seed):
    """rm.candidate_requests' segments (empty requests, repeated positives,
    every set form, staged lists past SV_MAX) over a made-up table: the
    positives' -1 rows replaced (a list of neighbours of row -1 has no
    counterpart in a table), the neighbours read from the table."""
    sets, pos, _, a_idx, e_idx, f_idx = rm.candidate_requests(R, k, seed)
    pos = [np.where(p < 0, 7, p) for p in pos]
    nbr = np.random.default_rng(seed).integers(0, rm.N_ITEMS, (rm.N_ITEMS, kt)).astype(np.int32)
    idx = [nbr[p][:, :k].astype(np.int64) for p in pos]
    return sets, pos, nbr, idx, a_idx, e_idx, f_idx


@pytest.mark.parametrize("k,kt", [(11, 11), (11, 16), (1, 1), (1, 3)])
@pytest.mark.parametrize("R", [1, 37])
def test_requests_candidates_table_equals_list_form(dev, R, k, kt):
    sets, pos, nbr, idx, a_idx, e_idx, f_idx = table_requests(R, k, kt, seed=R * 16 + k)
    want = rm.c_candidates(dev, pos, idx, k, sets, a_idx, e_idx, f_idx, 20, rm.N_ITEMS, rm.SV_MAX)
    got = c_candidates_table(dev, pos, rm._t(nbr, torch.int32, dev), k, sets, a_idx, e_idx, f_idx, 20,
                             rm.N_ITEMS, rm.SV_MAX)
    for g, w, what in zip(got, want, ("slots", "count", "status", "offsets", "host offsets")):
        assert torch.equal(g, w), what
    status = want[2].cpu().numpy()
    if R >= 37:
        assert (status == OVERFLOW).any() and (status == 0).sum() > R // 2
        assert any(len(p) == 0 for p in pos) and int(want[1].sum()) > 1000


def test_bad_table_entries_end_that_request_alone(dev):
    """An entry >= n_items and a negative one, each under one request's
    positive, inside the first k columns: DCNR_REQ_BAD_DATA there, every other
    request as before.  Behind column k nothing is read."""
    N, k, kt = 500, 11, 13
    rng = np.random.default_rng(8)
    nbr = rng.integers(0, N, (N, kt)).astype(np.int32)
    pos = [np.arange(10 * r, 10 * r + 3) for r in range(6)]
    none = [-1] * 6
    run = lambda t: c_candidates_table(dev, pos, rm._t(t, torch.int32, dev), k, [], none, none, none,
                                       20, N, rm.SV_MAX)
    clean = run(nbr)
    assert clean[2].tolist() == [0] * 6 and min(clean[1].tolist()) > 3
    far = nbr.copy()
    far[:, k:] = [N, -1]                       # behind column k: not part of any neighbour list
    for g, w in zip(run(far), clean):
        assert torch.equal(g, w)
    bad = far.copy()
    bad[21, 3] = N                             # request 2
    bad[42, k - 1] = -1                        # request 4
    bad[51, 0] = 2 ** 31 - 1                   # request 5: position 0 is dropped, never read as a row
    slots, count, status, offsets, _ = run(bad)
    assert status.tolist() == [0, 0, BAD_DATA, 0, BAD_DATA, 0]
    want_count = clean[1].clone()
    want_count[[2, 4]] = 0
    assert torch.equal(count, want_count)
    assert offsets.tolist() == np.r_[0, np.cumsum(want_count.cpu().numpy())].tolist()
    for r in (0, 1, 3, 5):
        assert torch.equal(slots[r], clean[0][r])
    # a positive past the table: that request alone (a negative one is skipped, as in the list form)
    pos2 = [p.copy() for p in pos]
    pos2[1][2] = N
    pos2[3][0] = -1
    s2 = c_candidates_table(dev, pos2, rm._t(nbr, torch.int32, dev), k, [], none, none, none, 20, N,
                            rm.SV_MAX)
    assert s2[2].tolist() == [0, BAD_DATA, 0, 0, 0, 0]
    idx3 = nbr[pos[3]][:, :k].astype(np.int64)
    assert torch.equal(s2[0][3, :int(s2[1][3])], rm.ref_union(dev, pos2[3][1:], idx3[1:], k))
    # kt below k: DCNR_BAD_ARG
    with pytest.raises(ValueError):
        c_candidates_table(dev, pos, rm._t(nbr[:, :k - 1], torch.int32, dev), k, [], none, none, none,
                           20, N, rm.SV_MAX)


def c_union_table(dev, pos, nbr, k):
    from dcnr import _lib
    lib = _lib.load()
    p_ = rm._t(pos, torch.int64, dev)
    out = torch.full((len(pos) * k,), -7, dtype=torch.int64, device=dev)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=dev)
    _lib.check(lib.dcnr_candidate_union_table(p_.data_ptr(), len(pos), nbr.data_ptr(), nbr.shape[1],
                                              nbr.shape[0], k, out.data_ptr(), cnt.data_ptr(),
                                              _lib.stream_ptr(dev)), "dcnr_candidate_union_table")
    return out, int(cnt.item())


@pytest.mark.parametrize("k,kt", [(11, 11), (11, 14), (1, 2)])
def test_candidate_union_table_equals_list_form(dev, k, kt):
    N = 3000
    rng = np.random.default_rng(k * 7 + kt)
    nbr = rng.integers(0, N, (N, kt)).astype(np.int32)
    d_nbr = rm._t(nbr, torch.int32, dev)
    for Q in (1, 2, 93, rm.SV_MAX // k):
        pos = rng.integers(0, N, Q)
        if Q > 2:
            pos[1] = pos[0]
        out, cnt = c_union_table(dev, pos, d_nbr, k)
        want = rm.ref_union(dev, pos, nbr[pos][:, :k].astype(np.int64), k)
        assert cnt == want.numel() and torch.equal(out[:cnt], want), Q
    # a positive past the table, a table entry past it: count -1, nothing read out of bounds
    assert c_union_table(dev, np.array([4, N, 6]), d_nbr, k)[1] == -1
    if k > 1:
        bad = nbr.copy()
        bad[5, 1] = N
        assert c_union_table(dev, np.array([4, 5, 6]), rm._t(bad, torch.int32, dev), k)[1] == -1
        assert c_union_table(dev, np.array([4, 6]), rm._t(bad, torch.int32, dev), k)[1] > 0


# ----------------------------------------------------------- 6: end to end
_twins = {}


def twin(dev, base, key):
    """A table-backed pipeline over base's model, tables and index rows."""
    import dcnr
    if key not in _twins:
        _twins[key] = dcnr.RankingPipeline(base.model, base.item_cat, base.item_num,
                                           neighbor_table=True)
        assert _twins[key]._nbr.shape == (base.n_items, base.n_neighbors)
        assert base._nbr is None
    return _twins[key]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_table_backed_pipeline_answers_as_the_scanning_one(dev, precision):
    base = rm.get_pipe(dev, precision)
    tab = twin(dev, base, ("many", precision))
    reqs, popular, half = rm.mixed_requests(40, seed=5)
    # recommend(), one request at a time (every third request: 0, 1 and 32 positives in turn)
    some = reqs[:3] + reqs[3::7]
    rm.assert_same([rm.run_single(tab, q) for q in some], [rm.run_single(base, q) for q in some],
                   precision + " recommend")
    want = rm.run_many(base, reqs)
    assert sum(w[0].numel() > 0 for w in want) > 20
    rm.assert_same(rm.run_many(tab, reqs), want, precision + " recommend_many")
    # a request above the batched kernels' capacity: recommend()'s chunked candidates
    big = np.random.default_rng(1).choice(rm.N_ITEMS, rm.SV_MAX // 11 + 30, replace=False).tolist()
    args = ([3, 4], [big, reqs[2]["pos"]])
    rm.assert_same(tab.recommend_many(*args), base.recommend_many(*args), precision + " overflow")
    assert torch.equal(tab.candidates(big), base.candidates(big))
    # /similar_items: from the table up to n = kt - 1, through the scan beyond
    rows = [0, 17, rm.N_ITEMS - 1, 17]
    for n in (1, 10, 15):
        assert torch.equal(tab.similar_items_many(rows, n), base.similar_items_many(rows, n)), n
        assert torch.equal(tab.similar_items(17, n), base.similar_items(17, n)), n
    assert tab.similar_items(17, 15).numel() == 15
    assert tab.similar_items_many([], 10).shape == (0, 10)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_table_backed_recommend_users(dev, precision):
    base = ru.get_pipe(dev, precision)
    tab = twin(dev, base, ("users", precision))
    store = ru.get_store()
    q = ru.mixed_requests(30, seed=11)
    want = ru.run_users(base, store, q)
    got = ru.run_users(tab, store, q)
    assert sum(w[0].numel() > 0 for w in want) > 15
    ru.assert_same(got, want, precision)
    assert torch.equal(got.by_offsets, want.by_offsets) and torch.equal(got.by_reviewers, want.by_reviewers)
    assert got.on_host.tolist() == want.on_host.tolist()


def _f7_pipe(f, dev, **kw):
    import dcnr
    m = dcnr.DCN_RecSys(f.n_users, f.n_items, f.cat_dims, f.n_num, dict(f.params), precision="fp32")
    m.load_state_dict(f.state)
    m = m.to(dev).eval()
    return dcnr.RankingPipeline(m, f.item_cat, f.item_num,
                                item_embeddings=torch.from_numpy(f.emb).to(dev), **kw)


def test_f7_golden_requests_with_the_table(dev):
    f = f7_common.load()
    pipe = _f7_pipe(f, dev, neighbor_table=True)
    assert pipe._nbr is not None
    n_mmr = 0
    for req in f.expected["recommendations"]:
        r = f7_common.request_rows(f, req)
        rows, _ = pipe.recommend(r["user_row"], r["pos"], lambda_param=req["lambda_param"],
                                 allowed=r["allowed"], excluded=r["excluded"], fallback=r["fallback"])
        got = [f.rev[x] for x in rows.tolist()]
        assert got == req["ranked_hotels"], (req, got)
        n_mmr += req["lambda_param"] < 1.0 and len(got) > 1
    assert n_mmr >= 5
    looked_up = 0
    for case in f.expected["similar_items"]:
        row = f.item_map.get(case["item_id"])
        if row is None:
            continue
        looked_up += case["n"] + 1 <= pipe._nbr.shape[1]
        got = [f.rev[x] for x in pipe.similar_items(row, case["n"]).tolist()]
        assert case["status"] == 200 and got == case["ids"], (case, got)
    assert looked_up > 0


def test_adopted_tables(dev):
    base = rm.get_pipe(dev, "fp32")
    import dcnr
    make = lambda t: dcnr.RankingPipeline(base.model, base.item_cat, base.item_num, neighbor_table=t)
    nbr = base.index.build_neighbor_table(16)
    assert nbr.shape == (rm.N_ITEMS, 16)
    reqs, _, _ = rm.mixed_requests(12, seed=3)
    want = rm.run_many(base, reqs)
    for t in (nbr, nbr.cpu().numpy(), 16):       # a device tensor, a host array, a k of its own
        pipe = make(t)
        assert pipe._nbr.shape == (rm.N_ITEMS, 16) and pipe._nbr.dtype == torch.int32
        rm.assert_same(rm.run_many(pipe, reqs), want)
        assert torch.equal(pipe.similar_items(5, 15), base.similar_items(5, 15))
    for wrong in (nbr[:-1], nbr[:, :10], nbr.to(torch.int64), nbr[0], 10):
        with pytest.raises(ValueError):
            make(wrong)
    base.index.neighbor_table_ = None            # (the shared pipeline as it was)


# ------------------------------------------- 7: no scan in the request path
def test_no_topk_launch_with_the_table(dev):
    from dcnr import _lib
    base = rm.get_pipe(dev, "bf16")
    tab = twin(dev, base, ("many", "bf16"))
    reqs, _, _ = rm.mixed_requests(12, seed=4)

    def knn_launches(pipe):
        _lib.profile_collect()
        rm.run_many(pipe, reqs)
        pipe.similar_items_many([1, 2, 3], 10)
        return _lib.profile_collect()["knn"][1]
    _lib.profile_enable(1)
    try:
        assert knn_launches(tab) == 0
        assert knn_launches(base) > 0
    finally:
        _lib.profile_enable(0)
