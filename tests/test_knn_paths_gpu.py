"""Every dispatch leg of the cosine top-k (knn.hip cosine_topk) that the
other kNN tests leave out: the exact scans v1 / v2 / v3 at the reference's own
embedding widths (16, 24, 48) and past them, each with its merge_kernel
branch, on tables that (a) end every scan in a ragged tile and (b) force the
in-scan compaction of the candidate lists.

Same comparison as test_cosine_knn_small_and_ragged_tables: a torch fp32
brute force on the device, distances at atol 2e-6, row ids at every position
whose reference distance is not within 2e-6 of a neighbour's ("isolated"),
every list sorted by (distance, row).  Each case also asserts that at least
95 % of the compared positions are isolated, so the row-id check cannot
shrink to nothing.

Where the legs come from (knn.hip): use_v4 needs d % 32 == 0, so none of
these shapes takes scan v4; use_v2 needs d <= 64 and k <= 32, scan v3 on top
of that Q >= MFMA_MIN_Q = 16 and d % 16 == 0; everything else is scan v1.
plan2 gives v2 / v3 slices of rup(N / min(512, N / 256), 64) rows, plan gives
v1 min(2048 / qtiles, N / 2048) slices.  merge_kernel sees `lists` k-lists
per query: fast path 0 needs lists * k <= 6144 and at least k lists (its
select is over the lists' minima), the fast path at most 512 valid
candidates, the compact loop takes the rest.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ATOL = 2e-6
N_RANDOM = 5003   # no multiple of 16, 64 or 256: 20 slices of 256 rows (v2 / v3), 3 of 1668 (v1)
N_COPIES = 20

# d, Q, k: the leg (reasoned from use_v2 / use_v4 / plan / plan2 as above).  Where a case says
# fast path 0, 3-24 candidates per query lie under its bound (counted on the CPU), far below
# its 128 slots.  merge_kernel's compact loop is reached by the staircase cases only.
RANDOM_CASES = [
    # scan v3 (Q >= 16, d % 16 == 0), one query tile half full; 20 lists >= k: merge fast path 0
    (16, 16, 11),
    # scan v3, two query tiles (K3_QT = 32), v3's largest k; 20 lists < k: fast path 0's select
    # fails; 226-382 admitted candidates per query (counted from the bound on the CPU), under
    # the 512 of the buffer: merge fast path
    (16, 33, 32),
    # scan v3, S4 = 3, two query tiles; merge fast path 0
    (48, 40, 11),
    # scan v2 (Q < MFMA_MIN_Q), DV = 12; merge fast path 0
    (48, 15, 11),
    # scan v2 (d % 16 != 0), DV = 6, a single query (the planted ties only); merge fast path 0
    (24, 1, 11),
    # scan v2, two query tiles (K2_QT = 32); 20 lists < k, 226-428 admitted candidates per
    # query: merge fast path
    (24, 33, 32),
    # scan v2, DV = 1, the smallest d; merge fast path 0
    (4, 5, 3),
    # scan v1 scan_kernel<64> (d > 64), two query tiles (QT = 8); every block compacts its
    # 512-entry buffer in the scan (no admission bound in v1); 3 lists < k: merge fast path
    (128, 9, 11),
    # scan v1, the widest d, KMAX; in-scan compact; 192 candidates: merge fast path
    (256, 3, 64),
    # scan v1 scan_kernel<16>, because k > K2_KMAX; in-scan compact; merge fast path
    (64, 5, 40),
]

# d, N, Q, k
STAIRCASE_CASES = [
    # scan v2, 469 slices of 640 rows: a wave sees 128-192 rows of one query against its
    # 64-slot list -> wave_compact from the append loop's room == 0 branch; 15008
    # candidates, all valid for query 0: merge compact loop
    (16, 300_000, 1, 32),
    # scan v3, half a query tile: lists compacted past K2_CAP - 16 entries between row
    # tiles; merge compact loop
    (16, 300_000, 16, 32),
    # scan v2, DV = 6, two query tiles; room == 0 compaction; merge compact loop
    (24, 300_000, 33, 32),
    # scan v1 scan_kernel<64>, 10 slices of 2000 rows against the 512-entry buffer:
    # compact() with a live threshold; 640 valid candidates: merge compact loop
    (128, 20_000, 3, 64),
    # scan v1 scan_kernel<16> (k > 32), in-scan compact; 400 candidates: merge fast path
    (64, 20_000, 3, 40),
]


def random_case(dev, d, Q, k):
    """Random table with N_COPIES exact copies of row 5 at scattered rows and
    one all-zero row; query 0 is 3 * table[5].  Returns (table, q, ties)."""
    g = torch.Generator(device=dev).manual_seed(1000 + 7 * d + 3 * Q + k)
    N = N_RANDOM
    table = torch.randn(N, d, device=dev, generator=g)
    perm = torch.randperm(N, device=dev, generator=g)
    perm = perm[perm != 5]
    dup, zero = perm[:N_COPIES], perm[N_COPIES]
    table[dup] = table[5].clone()
    table[zero] = 0.0
    q = torch.cat([table[5:6] * 3.0, torch.randn(Q - 1, d, device=dev, generator=g)])
    ties = np.sort(np.concatenate([[5], dup.cpu().numpy()]))
    return table, q, ties


def staircase_case(dev, d, N, Q, k):
    """Rows at prescribed cosine distances to a unit vector qv: rows 0..511 at
    0.9 (the admission bound then admits everything after them), the middle
    descending 0.5 -> 0.1 in row order (every new row beats the running k-th
    best), the last 64 at 0.05 - 5e-4 j.  Queries: 3 qv, two table rows, then
    qv with 5 % noise (Q > 3).  Returns (table, q)."""
    g = torch.Generator(device=dev).manual_seed(2000 + 7 * d + 3 * Q + k)
    qv = torch.randn(d, device=dev, generator=g, dtype=torch.float64)
    qv /= qv.norm()
    u = torch.randn(N, d, device=dev, generator=g, dtype=torch.float64)
    u -= (u @ qv)[:, None] * qv
    u /= u.norm(dim=1, keepdim=True)
    dist = torch.empty(N, device=dev, dtype=torch.float64)
    dist[:512] = 0.9
    dist[512:N - 64] = torch.linspace(0.5, 0.1, N - 576, device=dev, dtype=torch.float64)
    dist[N - 64:] = 0.05 - 5e-4 * torch.arange(64, device=dev, dtype=torch.float64)
    c = 1.0 - dist
    s = 0.5 + 1.5 * torch.rand(N, device=dev, generator=g, dtype=torch.float64)
    table = ((c[:, None] * qv + torch.sqrt(1.0 - c * c)[:, None] * u) * s[:, None]).float()
    qs = [3.0 * qv.float()[None]]
    if Q > 1:
        qs.append(table[[N // 2, N - 10]])
    if Q > 3:
        noise = torch.randn(Q - 3, d, device=dev, generator=g) * (0.05 / d ** 0.5)
        qs.append(qv.float()[None] + noise)
    return table.contiguous(), torch.cat(qs).contiguous()


def reference(table, q, k):
    tn = table / table.norm(dim=1, keepdim=True).clamp_min(1e-30)
    qn = q / q.norm(dim=1, keepdim=True)
    ref_d, ref_i = torch.topk((1.0 - qn @ tn.T).clamp(0, 2), k, dim=1, largest=False)
    return ref_d.cpu().numpy(), ref_i.cpu().numpy()


def check_against_reference(dist_, idx, ref_d, ref_i, skip0=0):
    """The module's comparison; the first skip0 positions of query 0 (planted
    exact ties, checked by the caller) are left out of the row-id check and of
    the isolated share.  Returns the isolated share."""
    Q, k = ref_d.shape
    np.testing.assert_allclose(dist_, ref_d, rtol=0, atol=ATOL)
    n_iso = n_cmp = 0
    for r in range(Q):
        near = np.diff(ref_d[r]) <= ATOL
        iso = np.ones(k, bool)
        iso[1:] &= ~near
        iso[:-1] &= ~near
        lo = skip0 if r == 0 else 0
        np.testing.assert_array_equal(idx[r][lo:][iso[lo:]], ref_i[r][lo:][iso[lo:]])
        n_iso += int(iso[lo:].sum())
        n_cmp += k - lo
        key = list(zip(dist_[r].tolist(), idx[r].tolist()))
        assert key == sorted(key), r
    return n_iso / n_cmp if n_cmp else 1.0


def search(table, q, k):
    import dcnr
    nn_ = dcnr.NearestNeighbors(metric="cosine").fit(table)
    dist_, idx = nn_.kneighbors_device(q, k)
    return dist_.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("d,Q,k", RANDOM_CASES)
def test_knn_path_random_table(dev, d, Q, k):
    """One dispatch leg per case (RANDOM_CASES says which scan, merge_kernel
    branch and compaction each reaches) over 5003 rows: query 0's 21 rows on
    its own direction first, ascending rows, one distance; every other
    position against the torch brute force."""
    table, q, ties = random_case(dev, d, Q, k)
    dist_, idx = search(table, q, k)
    m = min(k, ties.size)
    assert idx[0][:m].tolist() == ties[:m].tolist()
    assert np.all(dist_[0][:m] == dist_[0][0]) and dist_[0][0] <= ATOL
    ref_d, ref_i = reference(table, q, k)
    share = check_against_reference(dist_, idx, ref_d, ref_i, skip0=m)
    print(f"d={d} Q={Q} k={k}: isolated share {share:.4f}")
    assert share >= 0.95


@pytest.mark.parametrize("d,N,Q,k", STAIRCASE_CASES)
def test_knn_path_staircase_compaction(dev, d, N, Q, k):
    """Distances descending in row order (STAIRCASE_CASES says which scan,
    compaction branch and merge_kernel branch each case reaches): every list
    fills and is compacted inside the scan, which random tables under the
    admission bound never do.  Query 0's answer is rows N-1, N-2, ... ."""
    table, q = staircase_case(dev, d, N, Q, k)
    dist_, idx = search(table, q, k)
    assert idx[0].tolist() == list(range(N - 1, N - 1 - k, -1))
    ref_d, ref_i = reference(table, q, k)
    share = check_against_reference(dist_, idx, ref_d, ref_i)
    print(f"d={d} N={N} Q={Q} k={k}: isolated share {share:.4f}")
    assert share >= 0.95
