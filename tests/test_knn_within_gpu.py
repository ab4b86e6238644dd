"""The set-scoped search (dcnr_cosine_topk_within) on the device.

The defining property: for an ascending row set the answer equals
``dcnr_cosine_topk`` over the compacted table ``table[set]`` with positions
mapped back through the set -- the same rows, the distances bit for bit.  The
reference side therefore fits a second ``dcnr.NearestNeighbors`` on
``table[set]`` and queries it at most 8 queries at a time (below MFMA_MIN_Q,
so the fp32-MFMA scan, whose sums run in another order, is never taken).
``exclude`` is modelled by leaving the row out of the compacted table.

Shapes: N = 5003 (test_knn_paths_gpu.random_case: 20 exact copies of one row,
one all-zero row, query 0 = 3 x that row); every (d, k) leg of the kernel:
wave-register lists (d <= 64, k <= 32) at DV = 1, 6, 16, the LDS-buffer scan
for k > 32 (MAXV = 16) and for d > 64 (MAXV = 64, k = 11 and k = 64).
"""
import numpy as np
import pytest
import torch

import test_knn_paths_gpu as kp

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
BAD_DATA = 2   # DCNR_REQ_BAD_DATA
CASES = [(4, 3), (24, 10), (64, 32), (64, 40), (128, 11), (256, 64)]


def set_sizes(k):
    return sorted({0, 1, k - 1, k, k + 1, 63, 64, 65, 257, kp.N_RANDOM})


def csr(dev, sets):
    off = np.zeros(len(sets) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in sets])
    rows = np.concatenate([np.asarray(s, np.int64) for s in sets]) if sets else np.zeros(0, np.int64)
    return torch.from_numpy(rows).to(dev), torch.from_numpy(off).to(dev)


def within(nn, q, k, sets, seg_off, seg_set, exclude=None, out=None, max_rows=None, status=None):
    dev = q.device
    rows, off = csr(dev, sets)
    if max_rows is None:
        max_rows = max([len(s) for s in sets] + [0])
    ex = None if exclude is None else torch.as_tensor(np.asarray(exclude, np.int64)).to(dev)
    dist, idx = nn.kneighbors_within_device(
        q, k, rows, off, torch.as_tensor(np.asarray(seg_off, np.int64)).to(dev),
        torch.as_tensor(np.asarray(seg_set, np.int32)).to(dev), max_rows, exclude=ex, out=out,
        seg_status=status)
    torch.cuda.synchronize()
    return dist.cpu().numpy(), idx.cpu().numpy()


def compact_reference(table, rows, q, k):
    """dcnr_cosine_topk over table[rows] (rows ascending), at most 8 queries
    per call, positions mapped back; padded with (-1, FLT_MAX) past the set."""
    import dcnr
    Q = q.shape[0]
    idx = np.full((Q, k), -1, np.int64)
    dist = np.full((Q, k), FLT_MAX, np.float32)
    kk = min(k, len(rows))
    if kk:
        rt = torch.from_numpy(np.asarray(rows, np.int64)).to(table.device)
        sub = dcnr.NearestNeighbors(metric="cosine").fit(table[rt].contiguous())
        for s in range(0, Q, 8):
            d_, i_ = sub.kneighbors_device(q[s:s + 8], kk)
            idx[s:s + 8, :kk] = np.asarray(rows, np.int64)[i_.cpu().numpy()]
            dist[s:s + 8, :kk] = d_.cpu().numpy()
    return dist, idx


def assert_same(dist, idx, ref_d, ref_i, what=""):
    np.testing.assert_array_equal(idx, ref_i, err_msg=f"rows {what}")
    np.testing.assert_array_equal(dist.view(np.uint32), ref_d.view(np.uint32), err_msg=f"distance bits {what}")


@pytest.mark.parametrize("d,k", CASES)
def test_within_equals_compacted_table(dev, d, k):
    """Every set size around k and around the 64-row wave step, each with
    exclude = a row of the set, a row outside it and -1: one call whose
    segments are the (set, exclude) pairs, against one compacted-table search
    per pair.  Sizes below k (and k itself with a row excluded) pin the
    padding; the whole-table set has five chunks."""
    import dcnr
    table, q, ties = kp.random_case(dev, d, 8, k)
    N = kp.N_RANDOM
    nn = dcnr.NearestNeighbors(metric="cosine").fit(table)
    rng = np.random.default_rng(100 * d + k)
    # the planted ties first, so that small sets hold some of them
    pool = np.concatenate([ties, rng.permutation(np.setdiff1d(np.arange(N), ties))])
    sets, seg_set, exclude, refs = [], [], [], []
    for si, n in enumerate(set_sizes(k)):
        rows = np.sort(pool[:n])
        sets.append(rows)
        outside = np.setdiff1d(np.arange(N), rows)
        exs = [-1]
        if n:
            exs.append(int(rows[min(n - 1, 2)]))
        if outside.size:
            exs.append(int(outside[0]))
        for e in exs:
            seg_set.append(si)
            exclude.append(e)
            refs.append(rows[rows != e])
    G = len(seg_set)
    qq = q.repeat(G, 1)
    dist, idx = within(nn, qq, k, sets, np.arange(G + 1) * 8, seg_set, exclude=np.repeat(exclude, 8))
    for g in range(G):
        ref_d, ref_i = compact_reference(table, refs[g], q, k)
        assert_same(dist[8 * g:8 * g + 8], idx[8 * g:8 * g + 8], ref_d, ref_i,
                    f"(set of {len(sets[seg_set[g]])}, exclude {exclude[g]})")
        n_ok = min(k, len(refs[g]))
        assert np.all(idx[8 * g:8 * g + 8, n_ok:] == -1) and np.all(dist[8 * g:8 * g + 8, n_ok:] == FLT_MAX)


@pytest.fixture(scope="module")
def staircase(dev):
    table, q = kp.staircase_case(dev, 16, 100_003, 9, 32)
    N = table.shape[0]
    # 70 000 of the rows whose distance to query 0 descends in row order, ascending: in set
    # order every new row beats the running k-th best
    rng = np.random.default_rng(7)
    rows = np.sort(rng.choice(np.arange(512, N), 70_000, replace=False))
    ref = compact_reference(table, rows, q, 32)
    return table, q, rows, ref


@pytest.mark.parametrize("Q", [1, 8, 9])
def test_within_multi_chunk_staircase(dev, staircase, Q):
    """69 chunks of 1024 set positions; a wave sees 256 rows of a chunk, each
    better than the last, against its 64-slot list: the room == 0 compaction
    inside the scan; then merge_kernel's block over 69 lists.  Q = 9: a
    second, ragged window."""
    import dcnr
    table, q, rows, (ref_d, ref_i) = staircase
    nn = dcnr.NearestNeighbors(metric="cosine").fit(table)
    dist, idx = within(nn, q[:Q], 32, [rows], [0, Q], [0])
    assert idx[0].tolist() == rows[::-1][:32].tolist()
    assert_same(dist, idx, ref_d[:Q], ref_i[:Q])


def test_within_segments_overlay(dev):
    """G = 6: an empty segment, a skipped one, two naming one set, one naming
    an empty set, and one of 11 queries (windows of 8 + 3 that also straddle
    segment borders).  ld = k + 3 over sentinel-filled outputs."""
    import dcnr
    d, k = 24, 10
    table, q, _ = kp.random_case(dev, d, 25, k)
    nn = dcnr.NearestNeighbors(metric="cosine").fit(table)
    rng = np.random.default_rng(3)
    sets = [np.sort(rng.choice(kp.N_RANDOM, 300, replace=False)), np.zeros(0, np.int64),
            np.sort(rng.choice(kp.N_RANDOM, 1500, replace=False))]
    seg_off = [0, 0, 4, 7, 12, 14, 25]
    seg_set = [0, -1, 0, 0, 1, 2]
    idx = torch.full((25, k + 3), -7, dtype=torch.int64, device=dev)
    dist = torch.full((25, k + 3), -7.0, dtype=torch.float32, device=dev)
    status = torch.full((6,), 9, dtype=torch.int32, device=dev)
    within(nn, q, k, sets, seg_off, seg_set, out=(idx[:, :k], dist[:, :k]), status=status)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert status.tolist() == [0] * 6
    assert np.all(idx[:, k:] == -7) and np.all(dist[:, k:] == -7.0)
    assert np.all(idx[0:4] == -7) and np.all(dist[0:4] == -7.0)   # the skipped segment
    for g in (2, 3, 4, 5):
        a, b = seg_off[g], seg_off[g + 1]
        one_d, one_i = within(nn, q[a:b], k, [sets[seg_set[g]]], [0, b - a], [0])
        assert_same(dist[a:b, :k], idx[a:b, :k], one_d, one_i, f"(segment {g})")
    assert np.all(idx[12:14, :k] == -1) and np.all(dist[12:14, :k] == FLT_MAX)   # the empty set
    ref_d, ref_i = compact_reference(table, sets[2], q[14:25], k)
    assert_same(dist[14:25, :k], idx[14:25, :k], ref_d, ref_i, "(11 queries)")


@pytest.mark.parametrize("d,k", [(24, 10), (128, 11)])
def test_within_bad_device_data(dev, d, k):
    """Malformed segments -- a set index >= S, set offsets out of range, a set
    row >= N, a negative set row -- are padded and flagged; the well-formed
    segments between them are answered.  Both scan kernels."""
    import dcnr
    table, q, _ = kp.random_case(dev, d, 20, k)
    N = kp.N_RANDOM
    nn = dcnr.NearestNeighbors(metric="cosine").fit(table)
    rng = np.random.default_rng(5)
    good = np.sort(rng.choice(N, 400, replace=False))
    big = good.copy()
    big[-1] = N          # one row past the table
    neg = good.copy()
    neg[0] = -3
    rows = torch.from_numpy(np.concatenate([good, big, neg])).to(dev)
    # set 3's offsets reach past n_set_rows
    set_off = torch.tensor([0, 400, 800, 1200, 1300], dtype=torch.int64, device=dev)
    seg_off = torch.tensor([0, 4, 8, 12, 14, 17, 20], dtype=torch.int64, device=dev)
    seg_set = torch.tensor([0, 4, 1, 3, 2, 0], dtype=torch.int32, device=dev)
    status = torch.full((6,), 9, dtype=torch.int32, device=dev)
    dist, idx = nn.kneighbors_within_device(q, k, rows, set_off, seg_off, seg_set, 400, seg_status=status)
    torch.cuda.synchronize()
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    assert status.tolist() == [0, BAD_DATA, BAD_DATA, BAD_DATA, BAD_DATA, 0]
    assert np.all(idx[4:17] == -1) and np.all(dist[4:17] == FLT_MAX)
    for a, b in ((0, 4), (17, 20)):
        ref_d, ref_i = compact_reference(table, good, q[a:b], k)
        assert_same(dist[a:b], idx[a:b], ref_d, ref_i, f"(queries {a}..{b})")
    # a set longer than max_set_rows, and segment offsets that run backwards / past Q
    seg_off = torch.tensor([0, 4, 2, 8, 30], dtype=torch.int64, device=dev)
    seg_set = torch.tensor([0, 0, 0, 0], dtype=torch.int32, device=dev)
    status = torch.full((4,), 9, dtype=torch.int32, device=dev)
    dist, idx = nn.kneighbors_within_device(q, k, rows, set_off, seg_off, seg_set, 400, seg_status=status)
    torch.cuda.synchronize()
    assert status.tolist() == [0, BAD_DATA, 0, BAD_DATA]
    ref_d, ref_i = compact_reference(table, good, q[0:4], k)
    assert_same(dist[0:4].cpu().numpy(), idx[0:4].cpu().numpy(), ref_d, ref_i)
    assert np.all(idx[8:20].cpu().numpy() == -1)
    status = torch.full((1,), 9, dtype=torch.int32, device=dev)
    dist, idx = nn.kneighbors_within_device(
        q, k, rows, set_off, torch.tensor([0, 20], dtype=torch.int64, device=dev),
        torch.zeros(1, dtype=torch.int32, device=dev), 399, seg_status=status)
    torch.cuda.synchronize()
    assert status.tolist() == [BAD_DATA] and np.all(idx.cpu().numpy() == -1)


def test_within_against_sklearn_fixture(dev):
    """tests/golden/f13_knn_within.npz (make_within_golden.py): scikit-learn's
    brute-force cosine index fitted on table[set], as main.py:268-270 builds
    it.  Distances at test_knn_paths_gpu's ATOL; row ids at every position
    whose reference distance has no neighbour within it, at least 95 % of
    them."""
    import dcnr
    from conftest import golden
    g = golden("f13_knn_within.npz")
    table = torch.from_numpy(g["table"]).to(dev)
    nn = dcnr.NearestNeighbors(metric="cosine").fit(table)
    n_sets = int(g["n_sets"])
    n_iso = n_cmp = 0
    for s in range(n_sets):
        rows, q, ref_d, ref_i = g[f"set{s}"], g[f"q{s}"], g[f"dist{s}"], g[f"idx{s}"]
        k = ref_d.shape[1]
        dist, idx = nn.kneighbors(q, n_neighbors=k, within=rows)
        Q = q.shape[0]
        share = kp.check_against_reference(dist, idx, ref_d, rows[ref_i])
        n_iso += share * Q * k
        n_cmp += Q * k
    print(f"isolated share {n_iso / n_cmp:.4f}")
    assert n_iso / n_cmp >= 0.95


def test_kneighbors_within_host_call(dev):
    """kneighbors(within=): unsorted rows with duplicates are sorted and
    de-duplicated, n_neighbors above the set's size pads with (-1, inf)."""
    import dcnr
    table, q, _ = kp.random_case(dev, 24, 3, 10)
    nn = dcnr.NearestNeighbors(n_neighbors=10, metric="cosine").fit(table)
    rows = [40, 7, 7, 4000, 12, 40]
    dist, idx = nn.kneighbors(q.cpu().numpy(), within=rows)
    assert idx.shape == (3, 10) and np.all(idx[:, 4:] == -1) and np.all(np.isinf(dist[:, 4:]))
    ref_d, ref_i = compact_reference(table, np.array([7, 12, 40, 4000]), q, 4)
    assert_same(dist[:, :4], idx[:, :4], ref_d, ref_i)
    assert nn.kneighbors(q.cpu().numpy(), within=rows, return_distance=False).tolist() == idx.tolist()
    with pytest.raises(ValueError):
        nn.kneighbors(q.cpu().numpy(), within=[3, kp.N_RANDOM])
