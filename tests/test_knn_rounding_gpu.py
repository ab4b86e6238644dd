"""Scan v4's admission margin (knn.hip V4_EPS) and the neighbour-table update
filter that shares it, at worst-case bf16 rounding.

The tables come from knn_rounding_cases.py (its docstring has the
construction; test_knn_rounding_cpu.py checks the inputs): k "decoy" rows in
k blocks of the bound's 65536-row sample whose coarse bf16 distance to the
query q is ~0.006 under their exact one, and k "neighbour" rows behind the
sample -- the true top-k, exactly nearer than the decoys by 1e-4 or more --
whose coarse distance is ~0.006 over theirs.  Both errors are inside the true
rounding bound (2^-7 + 2^-16) * sum |x_i q_i|, so an exact search has to
return the neighbours: the oracle is a float64 brute force, never another
call into the library.

  1  the search, through bound5 + scan4's own merge (Q <= 32) and through
     bound5_merge_kernel (Q > 32), with and without the packed bf16 copy
  2  the neighbour-table build, q a row of the table
  3  the neighbour-table update: rows turned into the neighbours must enter
     q's list (the filter's one-sided margin)

On the library as it stood with V4_EPS = 0.004 (a margin of 2^-9 per factor;
bf16's unit roundoff is 2^-8) the adversarial queries of (1) and (2) returned
the decoys at distance ~1.0002 (d = 64; 1.00006 at d = 32), and the update of
(3) left q's list as it was.
"""
import numpy as np
import pytest
import torch

import knn_rounding_cases as rc
import test_knn_paths_gpu as kp
from test_neighbor_update_gpu import assert_equals_rebuild

pytestmark = pytest.mark.gpu

ATOL = kp.ATOL   # 2e-6


def fitted(dev, table, packed=True):
    import dcnr
    nn_ = dcnr.NearestNeighbors(metric="cosine").fit(torch.from_numpy(table).to(dev))
    assert nn_._packed is not None   # (N_ROWS is above PACKED_MIN_ROWS)
    if not packed:
        nn_._packed = None
    return nn_


def assert_sorted(dist_, idx):
    key = list(zip(dist_.tolist(), idx.tolist()))
    assert key == sorted(key)


def assert_list_is(dist_, idx, table, q, k, want_rows, what):
    """One returned list against the float64 brute force of q over table: the
    rows as a set (want_rows, which the brute force must give as well), the
    distances at ATOL, the order by (distance, row)."""
    bd, bi = rc.brute_force(table, q, k)
    assert sorted(bi.tolist()) == sorted(np.asarray(want_rows).tolist()), what
    print(f"{what}: rows {np.sort(idx).tolist()[:6]}..., distances {dist_[0]:.6f} .. {dist_[-1]:.6f}; "
          f"float64 {bd[0]:.6f} .. {bd[-1]:.6f}")
    assert sorted(idx.tolist()) == sorted(bi.tolist()), what
    np.testing.assert_allclose(dist_, bd, rtol=0, atol=ATOL, err_msg=what)
    assert_sorted(dist_, idx)


# ------------------------------------------------------------------- 1: the search
_queries = {}


def queries(dev, c, Q):
    """Q queries: positive multiples of q (1x, 3x, 0.5x) at batch positions 0,
    17 and Q - 1 where they exist, random ones elsewhere, and the torch fp32
    brute force of the random ones -- once per (d, k, Q)."""
    key = (c.d, c.k, Q)
    if key not in _queries:
        g = torch.Generator(device=dev).manual_seed(31 * c.d + 7 * c.k + Q)
        q = torch.randn(Q, c.d, device=dev, generator=g)
        adv = {}
        for pos, scale in ((0, 1.0), (17, 3.0), (Q - 1, 0.5)):
            if pos < Q:
                adv[pos] = scale
        for pos, scale in adv.items():
            q[pos] = torch.from_numpy(c.q * np.float32(scale)).to(dev)
        rand = np.array([i for i in range(Q) if i not in adv], np.int64)
        ref = None
        if rand.size:
            table = torch.from_numpy(c.table).to(dev)
            ref = kp.reference(table, q[torch.from_numpy(rand).to(dev)], c.k)
        _queries[key] = (q.contiguous(), adv, rand, ref)
    return _queries[key]


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "fp32rows"])
@pytest.mark.parametrize("Q", [2, 40])
@pytest.mark.parametrize("k", [1, 11, 32])
@pytest.mark.parametrize("d", [32, 64])
def test_search_returns_the_true_neighbours(dev, d, k, Q, packed):
    c = rc.build(d, k)
    q, adv, rand, ref = queries(dev, c, Q)
    nn_ = fitted(dev, c.table, packed)
    dist_, idx = nn_.kneighbors_device(q, k)
    dist_, idx = dist_.cpu().numpy(), idx.cpu().numpy()
    assert len(adv) == (2 if Q == 2 else 3)
    for pos, scale in adv.items():
        assert_list_is(dist_[pos], idx[pos], c.table, c.q, k, c.neighbours,
                       f"d={d} k={k} Q={Q} query {pos} ({scale} q)")
    if rand.size:
        share = kp.check_against_reference(dist_[rand], idx[rand], *ref)
        print(f"d={d} k={k} Q={Q}: isolated share {share:.4f}")
        assert share >= 0.95


# ------------------------------------------------------- 2: the neighbour-table build
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "fp32rows"])
@pytest.mark.parametrize("d,k", [(32, 11), (64, 11), (64, 32)])
def test_build_lists_the_true_neighbours_of_a_table_row(dev, d, k, packed):
    """q is row c.query_row: its list is itself, then the k - 1 neighbour
    rows.  A few other rows' lists against the float64 brute force as well
    (the module's comparison: distances at ATOL, rows where isolated)."""
    c = rc.build(d, k, query_row=True)
    nn_ = fitted(dev, c.table, packed)
    dist_, nbr = nn_.build_neighbor_table(k, return_distance=True)
    assert nbr.shape == (rc.N_ROWS, k)
    r = c.query_row
    dr, ir = dist_[r].cpu().numpy(), nbr[r].cpu().numpy().astype(np.int64)
    assert ir[0] == r and dr[0] <= ATOL
    assert_list_is(dr, ir, c.table, c.q, k, np.concatenate([[r], c.neighbours]), f"d={d} k={k} row {r}")
    others = np.array([0, c.decoys[0], c.neighbours[-1], 40000, rc.N_ROWS - 2])
    ref = [rc.brute_force(c.table, c.table[o], k) for o in others]
    ref_d, ref_i = np.stack([x[0] for x in ref]), np.stack([x[1] for x in ref])
    sel = torch.from_numpy(others).to(dev)
    kp.check_against_reference(dist_[sel].cpu().numpy(), nbr[sel].cpu().numpy().astype(np.int64), ref_d, ref_i)


# ------------------------------------------------------ 3: the neighbour-table update
@pytest.mark.parametrize("d,k", [(32, 11), (64, 11), (64, 32)])
def test_update_admits_rows_turned_into_true_neighbours(dev, d, k):
    """The table starts with "far" vectors in the neighbour rows: q's list is
    itself and the k - 1 decoys, its k-th distance dk a decoy's exact one.
    update_rows then plants the neighbours.  Their coarse distance to q is
    ~0.0055 above dk while their exact one is below it: the filter has to mark
    q's row all the same, and the merge then puts them in its list."""
    c = rc.build(d, k, query_row=True)
    r = c.query_row
    start = c.table.copy()
    start[c.neighbours] = c.far
    nn_ = fitted(dev, start)
    dist_, nbr = nn_.build_neighbor_table(k, return_distance=True)
    assert_list_is(dist_[r].cpu().numpy(), nbr[r].cpu().numpy().astype(np.int64), start, c.q, k,
                   np.concatenate([[r], c.decoys]), f"d={d} k={k} row {r} before the update")
    stats = nn_.update_rows(c.neighbours, c.table[c.neighbours], return_stats=True)
    print(f"d={d} k={k}: {stats}")
    assert not stats["rebuilt"] and stats["changed"] == k - 1
    assert nn_.neighbor_table_ is nbr   # in place
    got = nbr[r].cpu().numpy().astype(np.int64)
    bd, bi = rc.brute_force(c.table, c.q, k)
    assert sorted(bi.tolist()) == sorted([r] + c.neighbours.tolist())
    assert got[0] == r and sorted(got.tolist()) == sorted(bi.tolist()), (got.tolist(), bi.tolist())
    # ... and everything equal to fit + build on the new table, as after every update
    assert_equals_rebuild(nn_, torch.from_numpy(c.table).to(dev), k, "after the update")
