"""Adversarial tables for scan v4's bf16 admission margin (knn.hip V4_EPS)
and the neighbour-table update filter that shares it.  numpy only.

The coarse score is sum_i bf16(x_i * inv_x) * bf16(q_i / |q|): each factor is
rounded to 8 significant bits, a relative error of up to 2^-8, so the coarse
cosine of two unit vectors is off by up to (2^-7 + 2^-16) * sum_i |x_i q_i|.
Random tables never come near that: the per-element errors cancel.  Here they
are aligned.

Every active coordinate of the unit vectors q (query), s (decoy) and n
(neighbour) has the magnitude 2^e * UP or 2^e * DOWN,

    UP   = 1 + 2^-8 + 2^-11    just above the bf16 midpoint: rounds to 1 + 2^-7
    DOWN = 1 + 2^-8 - 2^-11    just below it:                rounds to 1

(12 significant bits: exact in fp32, and exact again after a scale by 3 or
0.5; the 2^-11 relative distance to the midpoint is 4000 times what the fp32
normalisation x * inv can move a value).  q and s carry the same magnitude at
every active coordinate.  Where it is UP, s has q's sign -- a positive product
whose two factors both round up; where it is DOWN, s has the opposite sign --
a negative product whose two factors both round down.  Either way the coarse
cosine of (s, q) gains ~0.0068 |s_i q_i|.  n = s with its active coordinates
negated: every product changes sign, and the coarse cosine of (n, q) loses as
much.  With P_up, P_down the total 2^(2e) of the two kinds,

    cos(s, q) = P_up UP^2 - P_down DOWN^2,    cos(n, q) = -cos(s, q),

and the layouts below make that slightly negative: n is the nearer row,
exactly, while the coarse score puts s ~0.011 in front of it.

The rest of each vector's unit norm sits in "filler" coordinates where the
other side is 0 (q's filler is 0 in s and n, theirs is 0 in q), so neither
the exact nor the coarse cosine sees it and normalisation rescales nothing.
The planted rows differ only in how their filler mass is split.

Every other row is random and pushed away from q: cosine to q <= -0.05.
"""
import numpy as np

N_ROWS = 70001            # larger than scan v4's 65536-row bound sample; no multiple of 16
SAMPLE_ROWS = 65536       # knn.hip V4_S
SAMPLE_BLOCK = 512        # knn.hip B5_C: the bound takes one minimum per block of the sample
LOWBIT = 13               # knn.hip V4_LOWBIT: the bound's k-th minimum is rounded up to a 2^13-ulp bin edge
OLD_EPS = 0.004           # the margin the scan granted before it was derived from 2^-8 per factor
TRUE_BOUND = 2.0 ** -7 + 2.0 ** -16   # |coarse - exact| <= TRUE_BOUND * sum |x_i q_i| (+ fp32 accumulation)

UP = 1.0 + 2.0 ** -8 + 2.0 ** -11
DOWN = 1.0 + 2.0 ** -8 - 2.0 ** -11

# d -> [(exponent e, UP coordinates, DOWN coordinates)]: the active coordinates, then q's
# filler, then the rows' filler.  P_up - P_down = -2^-10 in both (the lone 2^-5 DOWN pair).
#   d = 64: 54 x 2^-3, 1 x 2^-5; sum |s_i q_i| = 0.851, cos(s, q) = -1.6e-4
#   d = 32: 14 x 2^-2, 4 x 2^-3, 1 x 2^-5; sum |s_i q_i| = 0.946, cos(s, q) = -6.0e-5
LAYOUT = {
    64: [(-3, 27, 27), (-5, 0, 1)],
    32: [(-2, 7, 7), (-3, 2, 2), (-5, 0, 1)],
}
Q_FILLER = {64: 3, 32: 5}    # q's filler coordinates; the rows get the rest of d


def bf16_round(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32: the
    conversion the kernels' (bf16) casts and torch's .to(bfloat16) perform."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def _inv_norm32(x):
    """fp32 1 / |row| as fit computes it (zero rows: 1), up to summation order."""
    x = np.asarray(x, np.float32)
    ss = np.sum(x * x, axis=-1, dtype=np.float32)
    return np.where(ss > 0, np.float32(1) / np.sqrt(ss, dtype=np.float32), np.float32(1)).astype(np.float32)


def coarse_dist(table, q):
    """The scan's coarse distance, emulated: fp32 x * inv and q * inv, each
    rounded to bf16, dotted in float64.  table [n, d], q [d] -> [n]."""
    table = np.atleast_2d(np.asarray(table, np.float32))
    xh = bf16_round(table * _inv_norm32(table)[:, None])
    q = np.asarray(q, np.float32)
    qh = bf16_round(q * _inv_norm32(q))
    return 1.0 - xh.astype(np.float64) @ qh.astype(np.float64)


def exact_dist(table, q):
    """Cosine distance in float64 (zero rows: 1).  table [n, d], q [d] -> [n]."""
    t = np.atleast_2d(np.asarray(table, np.float64))
    q = np.asarray(q, np.float64)
    nt = np.linalg.norm(t, axis=1)
    nt[nt == 0] = 1.0
    return np.clip(1.0 - (t @ q) / (nt * np.linalg.norm(q)), 0.0, 2.0)


def brute_force(table, q, k):
    """float64 top-k of q over the table by (distance, row): (dist [k], rows [k])."""
    d = exact_dist(table, q)
    order = np.lexsort((np.arange(d.size), d))[:k]
    return d[order], order


def bin_edge(x):
    """The upper edge of x's 2^13-ulp bin of fp32 bit patterns, as
    v4_kth_bounds rounds the k-th block minimum up."""
    u = np.asarray(x, np.float32).view(np.uint32)
    return (u | np.uint32((1 << LOWBIT) - 1)).view(np.float32).astype(np.float64)


def sum_abs_products(row, q):
    """sum_i |x_i q_i| of the normalised vectors: what scales the true bound."""
    r, q = np.asarray(row, np.float64), np.asarray(q, np.float64)
    return float(np.abs(r * q).sum() / (np.linalg.norm(r) * np.linalg.norm(q)))


def directions(d):
    """(q, s_active, q_filler, row_filler): the unit query, the decoys'
    active part (zero elsewhere) and the two sets of filler coordinates."""
    mag, up = [], []
    for e, n_up, n_down in LAYOUT[d]:
        mag += [2.0 ** e * UP] * n_up + [2.0 ** e * DOWN] * n_down
        up += [True] * n_up + [False] * n_down
    mag, up = np.array(mag), np.array(up)
    a, fq = mag.size, Q_FILLER[d]
    assert a + fq + 2 <= d
    # scatter the two kinds over the active coordinates, and the signs of q over both
    rng = np.random.default_rng(900 + d)
    perm = rng.permutation(a)
    mag, up = mag[perm], up[perm]
    sign = rng.choice([-1.0, 1.0], a)
    q = np.zeros(d)
    s = np.zeros(d)
    q[:a] = sign * mag
    s[:a] = np.where(up, sign, -sign) * mag
    q_filler = np.arange(a, a + fq)
    row_filler = np.arange(a + fq, d)
    rest = 1.0 - float(mag @ mag)
    assert rest > 0.02
    q[q_filler] = np.sqrt(rest / fq)
    return q, s, q_filler, row_filler


def _filled(active, filler, j, n):
    """active plus the rest of the unit norm on the filler coordinates, split
    by an angle that depends on j (of n): the planted rows differ in this alone."""
    v = active.copy()
    rest = 1.0 - float(active @ active)
    w = np.cos(np.linspace(0.2, 1.3, filler.size) * (1.0 + 2.0 * (j + 1) / (n + 1)))
    w = np.abs(w) + 0.05
    v[filler] = w * np.sqrt(rest / float(w @ w))
    return v


class Case:
    """table fp32 [N_ROWS, d]; q fp32 [d] (unit); decoys / neighbours: the
    planted rows (ascending); query_row: the table row that holds q, or None;
    far: fp32 [len(neighbours), d], "far" vectors to stand in the neighbour
    rows before an update plants them."""


_cache = {}


def build(d, k, query_row=False):
    """The table for width d and list length k.  query_row=False: k decoys
    and k neighbours, q outside the table.  query_row=True: q is a table row
    (in a sample block of its own), with k - 1 decoys and k - 1 neighbours, so
    that row's k nearest are itself and the neighbours.  Deterministic; cached
    (callers must not write into it)."""
    key = (d, k, bool(query_row))
    if key in _cache:
        return _cache[key]
    q, s_act, _, row_filler = directions(d)
    p = k - 1 if query_row else k
    rng = np.random.default_rng(7000 + 10 * d + k + (500 if query_row else 0))
    n_blocks = SAMPLE_ROWS // SAMPLE_BLOCK
    assert p + 1 <= n_blocks
    # every other row: a random direction orthogonal to q plus -c q, c in [0.06, 0.5], any length
    g = rng.standard_normal((N_ROWS + p, d))
    g -= (g @ q)[:, None] * q
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    c = rng.uniform(0.06, 0.5, N_ROWS + p)
    rows = (np.sqrt(1.0 - c * c)[:, None] * g - c[:, None] * q) * rng.uniform(0.5, 2.0, N_ROWS + p)[:, None]
    table = rows[:N_ROWS].astype(np.float32)
    far = rows[N_ROWS:].astype(np.float32)
    # decoys: one per sample block, at any offset in it (the last block's last rows included)
    blocks = np.sort(rng.choice(n_blocks, p + 1, replace=False))
    offs = rng.integers(0, SAMPLE_BLOCK, p + 1)
    if p:
        offs[0], offs[p - 1] = 0, SAMPLE_BLOCK - 1
    spots = blocks * SAMPLE_BLOCK + offs
    take = rng.permutation(p + 1)
    decoys = np.sort(spots[take[:p]])
    qrow = int(spots[take[p]]) if query_row else None
    # neighbours: scattered behind the sample, the table's last row among them
    tail = np.arange(SAMPLE_ROWS, N_ROWS - 1)
    neighbours = np.sort(np.concatenate([rng.choice(tail, max(p - 1, 0), replace=False), [N_ROWS - 1]])[:p]
                         if p else np.zeros(0, np.int64))
    for j, r in enumerate(decoys):
        table[r] = _filled(s_act, row_filler, j, 2 * p).astype(np.float32)
    for j, r in enumerate(neighbours):
        table[r] = _filled(-s_act, row_filler, p + j, 2 * p).astype(np.float32)
    if query_row:
        table[qrow] = q.astype(np.float32)
    case = Case()
    case.d, case.k = d, k
    case.table, case.q = table, q.astype(np.float32)
    case.decoys, case.neighbours, case.query_row, case.far = decoys, neighbours, qrow, far
    _cache[key] = case
    return case
