"""The neighbour-table update rule restated in numpy, the changed-row recipe
of the update tests, and a brute-force table -- shared by
test_neighbor_update_cpu.py (which checks the restatement against the brute
force) and test_neighbor_update_gpu.py (which uses it as the oracle of the
device's counts).

Keys are (distance, row) packed into one uint64 -- the bits of a non-negative
float32 order like its value -- so ``<`` on keys is the kernels' cless.
"""
import numpy as np

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def planted_table(N, d, seed, copies=20):
    """test_knn_paths_gpu.random_case's shape on the host: a random normal
    table, `copies` exact copies of row 5 at scattered rows, one zero row.
    Returns (table, ties ascending, zero)."""
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((N, d)).astype(np.float32)
    perm = rng.permutation(N)
    perm = perm[perm != 5]
    dup, zero = perm[:copies], int(perm[copies])
    table[dup] = table[5]
    table[zero] = 0.0
    return table, np.sort(np.r_[5, dup]), zero


def changed_set(table, ties, zero, seed, counts=(12, 12, 11), exclude=()):
    """The update tests' changed rows and their new vectors: counts[0] rows
    redrawn at random, counts[1] moved next to an unchanged row (1.5 *
    table[t] + 0.05 * noise), counts[2] jittered by 0.01 * noise, one planted
    copy redrawn, one planted copy scaled by 2.  Rows outside `exclude`,
    distinct, in the order drawn (not sorted).  Returns (rows int64 [m],
    vectors [m, d])."""
    rng = np.random.default_rng(seed)
    N, d = table.shape
    taken = set(int(x) for x in exclude) | set(int(x) for x in ties) | {int(zero)}
    free = np.array([r for r in rng.permutation(N) if int(r) not in taken])
    a, b, c = counts
    n = a + b + c
    rows, targets = free[:n], free[n:n + b]
    noise = lambda k: rng.standard_normal((k, d)).astype(np.float32)
    vec = np.concatenate([
        noise(a),
        np.float32(1.5) * table[targets] + np.float32(0.05) * noise(b),
        table[rows[a + b:]] + np.float32(0.01) * noise(c)])
    copies = [int(t) for t in ties if int(t) not in set(int(x) for x in exclude)]
    c0, c1 = copies[3], copies[11]
    rows = np.r_[rows, c0, c1].astype(np.int64)
    vec = np.concatenate([vec, noise(1), np.float32(2.0) * table[c1:c1 + 1]])
    return rows, vec.astype(np.float32)


def distances(table):
    """d(query r, row x) = clip(1 - <t_r / |t_r|, t_x / |t_x|>, 0, 2), float32
    [N, N]; a zero row is left as it is (sklearn's normalize)."""
    nrm = np.linalg.norm(table.astype(np.float64), axis=1)
    tn = (table / np.where(nrm > 0, nrm, 1.0)[:, None]).astype(np.float32)
    return np.clip(np.float32(1.0) - tn @ tn.T, 0.0, 2.0).astype(np.float32)


def keys(dist, rows):
    return (dist.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
        rows.astype(np.uint64)


def brute_table(D, k, rows=None):
    """The k smallest keys of each listed row of the distance matrix D: int64
    [n, k], ascending by (distance, row)."""
    sel = np.arange(D.shape[0]) if rows is None else np.asarray(rows)
    out = np.empty((sel.size, k), np.int64)
    cols = np.arange(D.shape[1])
    for lo in range(0, sel.size, 512):
        kk = keys(D[sel[lo:lo + 512]], np.broadcast_to(cols, (min(512, sel.size - lo), D.shape[1])))
        part = np.partition(kk, k - 1, axis=1)[:, :k]
        out[lo:lo + 512] = (np.sort(part, axis=1) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return out


def apply_rule(old_nbr, D_new, C):
    """The rule, from the table as it stood (old_nbr [N, kt]) and the new
    distances alone.  Returns (new table int64 [N, kt], branches): branches
    maps a name to a bool mask over the rows --
      changed      r in C (searched again)
      untouched    no changed row in L(r), none at or under its k-th key
      gained       no changed row in L(r), some changed row entered (merged)
      merged_hole  a changed row in L(r), the merge still filled the list
      hole         a changed row in L(r) left a hole (searched again)
      emptied      every entry of L(r) is in C (searched again)
    The rows searched again get the brute-force answer."""
    N, kt = old_nbr.shape
    C = np.asarray(C, np.int64)
    in_c = np.zeros(N, bool)
    in_c[C] = True
    L = old_nbr.astype(np.int64)
    l_in_c = in_c[L]                                              # [N, kt]
    key_l = keys(np.take_along_axis(D_new, L, axis=1), L)
    key_l[l_in_c] = PAD
    key_c = keys(D_new[:, C], np.broadcast_to(C, (N, C.size)))
    has_keep = ~l_in_c.all(1)
    # K': the key of the last entry of L(r) outside C
    last = kt - 1 - np.argmax(~l_in_c[:, ::-1], axis=1)
    k_prime = np.take_along_axis(key_l, last[:, None], axis=1)[:, 0]
    M = np.sort(np.concatenate([key_l, key_c], axis=1), axis=1)
    fills = has_keep & (M[:, kt - 1] <= k_prime) & (M[:, kt - 1] != PAD)
    merged = fills & ~in_c
    new = L.copy()
    new[merged] = (M[merged, :kt] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    again = ~merged
    new[again] = brute_table(D_new, kt, np.nonzero(again)[0])
    holds = l_in_c.any(1)
    enters = (key_c <= k_prime[:, None]).any(1)
    rest = ~in_c
    branches = dict(changed=in_c,
                    untouched=rest & ~holds & ~enters,
                    gained=rest & ~holds & enters,
                    merged_hole=rest & holds & merged,
                    hole=rest & holds & has_keep & ~merged,
                    emptied=rest & ~has_keep)
    return new, branches
