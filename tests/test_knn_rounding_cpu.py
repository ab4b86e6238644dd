"""The adversarial tables of knn_rounding_cases.py are what the GPU test
(test_knn_rounding_gpu.py) needs them to be: conditions on the inputs alone,
from a float64 brute force and an emulation of the scan's coarse bf16 score.
No kernel runs here.

With them met, a scan that grants the coarse score a margin of 0.004 per
side (2 * 0.004 + the bound's bin, as before the margin was derived from 2^-8
per factor) cannot return the true neighbours, and one that grants the true
bound (2^-7 + 2^-16) * sum |x_i q_i| must.
"""
import numpy as np
import pytest

import knn_rounding_cases as rc

SHAPES = [(d, k, qr) for d in (32, 64) for k in (1, 11, 32) for qr in (False, True) if not (qr and k == 1)]


def test_bf16_emulation_is_round_to_nearest_even():
    """bf16_round against hand-made ties and, where torch is present, its cast."""
    x = np.array([1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, rc.UP, rc.DOWN, -rc.UP * 0.125, 3.0e-39, 0.0],
                 np.float32)
    want = np.array([1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, 1.0, -(1 + 2.0 ** -7) * 0.125, 0, 0], np.float32)
    got = rc.bf16_round(x)
    assert np.array_equal(got[:5], want[:5])
    torch = pytest.importorskip("torch")
    v = np.random.default_rng(0).standard_normal(100_000).astype(np.float32)
    v = np.concatenate([v, x[:5], v * np.float32(1e-30), v * np.float32(1e30)])
    ref = torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(rc.bf16_round(v), ref)


@pytest.mark.parametrize("d", [32, 64])
def test_directions_are_exact_in_fp32_and_unit(d):
    q, s, q_filler, row_filler = rc.directions(d)
    a = q_filler[0]
    # the active coordinates: 12 significant bits, the same in fp32, in 3x and in 0.5x
    for v in (q[:a], s[:a]):
        for scale in (1.0, 3.0, 0.5):
            assert np.array_equal((v * scale).astype(np.float32).astype(np.float64), v * scale)
    assert np.array_equal(np.abs(q[:a]), np.abs(s[:a]))
    # filler where the other side is 0
    assert not s[q_filler].any() and not q[row_filler].any() and not s[row_filler].any()
    assert abs(np.linalg.norm(q) - 1.0) < 1e-12
    # every active magnitude sits 2^-11 (relative to its power of two) from a bf16 midpoint
    m = np.abs(q[:a])
    frac = m / 2.0 ** np.floor(np.log2(m)) - (1 + 2.0 ** -8)
    assert np.array_equal(np.abs(frac), np.full(a, 2.0 ** -11))


@pytest.mark.parametrize("d,k,query_row", SHAPES)
def test_inputs_meet_the_gpu_tests_conditions(d, k, query_row):
    c = rc.build(d, k, query_row)
    p = k - 1 if query_row else k
    table, q = c.table, c.q
    assert table.shape == (rc.N_ROWS, d) and table.dtype == np.float32 and rc.N_ROWS > rc.SAMPLE_ROWS
    # where the planted rows are
    assert c.decoys.size == p and c.neighbours.size == p
    assert np.unique(c.decoys // rc.SAMPLE_BLOCK).size == p and np.all(c.decoys < rc.SAMPLE_ROWS)
    assert np.all(c.neighbours >= rc.SAMPLE_ROWS) and np.unique(c.neighbours).size == p
    if query_row:
        assert c.query_row < rc.SAMPLE_ROWS and np.array_equal(table[c.query_row], q)
        assert c.query_row // rc.SAMPLE_BLOCK not in set((c.decoys // rc.SAMPLE_BLOCK).tolist())
    assert np.unique(table[np.concatenate([c.decoys, c.neighbours])], axis=0).shape[0] == 2 * p
    assert c.far.shape == (p, d)

    exact = rc.exact_dist(table, q)
    coarse = rc.coarse_dist(table, q)
    planted = np.zeros(rc.N_ROWS, bool)
    planted[c.decoys] = planted[c.neighbours] = True
    if query_row:
        planted[c.query_row] = True
        assert exact[c.query_row] < 1e-12
    # every other row is far, and so are the stand-ins for the update test
    assert exact[~planted].min() >= 1.05
    assert rc.exact_dist(c.far, q).min() >= 1.05
    # the neighbours are the true top-k, by a margin the suite's atol (2e-6) cannot blur
    assert exact[c.decoys].min() - exact[c.neighbours].max() >= 1e-4
    bd, bi = rc.brute_force(table, q, k)
    want = np.concatenate([[c.query_row], c.neighbours]) if query_row else c.neighbours
    assert sorted(bi.tolist()) == sorted(want.tolist())
    # aligned rounding: the coarse score misses by more than the old margin, in opposite directions
    err = coarse - exact
    assert err[c.decoys].max() <= -0.0055 and err[c.neighbours].min() >= 0.0055
    # ... and by less than the true bound for these vectors
    for r in np.concatenate([c.decoys, c.neighbours]):
        assert abs(err[r]) <= rc.TRUE_BOUND * rc.sum_abs_products(table[r], q) + 1e-6
    # the admission bound starts from the k-th smallest block minimum of the sample: a decoy's
    # (the query row's own block holds the smallest), rounded up to its bin edge
    sample = coarse[:rc.SAMPLE_ROWS].astype(np.float32).reshape(-1, rc.SAMPLE_BLOCK).min(1)
    kth = np.sort(sample)[k - 1]
    assert kth == np.float32(coarse[c.decoys].max())
    M = float(rc.bin_edge(kth))
    gap = coarse[c.neighbours] - M
    # beyond the old two-sided margin 2 * 0.004 + 5e-4 by 1e-3 ...
    assert gap.min() >= 0.0095
    assert gap.min() >= 2 * rc.OLD_EPS + 5e-4 + 1e-3
    # ... and inside the true one: a correct margin must admit them
    assert gap.max() <= 2 * rc.TRUE_BOUND
    # the update filter's one-sided test, coarse <= dk + 0.004 + 1e-5 with dk a decoy's exact
    # distance: no neighbour passes it
    assert (coarse[c.neighbours] - exact[c.decoys].max()).min() >= rc.OLD_EPS + 1e-5 + 1e-3
    # no far row comes near either bound
    assert coarse[~planted].min() >= 1.04
