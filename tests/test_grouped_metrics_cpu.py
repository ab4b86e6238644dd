"""CPU tests of the per-group ranking metrics: the host reference of
tests/grouped_metrics_cases.py reproduces scikit-learn's per-group values
(tests/golden/f12_grouped_metrics.npz), has the closed forms its patterns
were chosen for, and the native entry points are bound as the header declares
them and refuse bad arguments on the host."""
import ctypes
import math

import numpy as np
import pytest

import grouped_metrics_cases as gm
import metrics_cases as mc
from conftest import golden

IDS = [gm.case_id(c) for c in gm.CASES]


@pytest.fixture(scope="module")
def fx():
    f = golden("f12_grouped_metrics.npz")
    assert list(f["names"]) == IDS, "regenerate f12_grouped_metrics.npz"
    return {k: f[k] for k in f.files}


@pytest.mark.parametrize("idx", range(len(gm.CASES)), ids=IDS)
def test_host_reference_reproduces_fixture(fx, idx):
    """AUC_u = U2_u / (2 P_u N_u) is sklearn's roc_auc_score of the group
    within n_u 2^-52 (the rounding bound of its n_u-term trapezoid sum), and on
    ``distinct`` scores dcg_u / ideal is sklearn's ndcg_score within
    (k + 2) 2^-52, k the number of rows the cutoff leaves (min(k, n_u): the
    terms either side sums)."""
    case = gm.CASES[idx]
    ref = gm.case_with_reference(case)[5]
    pick = gm.sampled(ref["auc_groups"])
    want = fx[f"auc_{idx}"]
    assert want.shape == pick.shape
    auc_all = np.zeros(len(ref["gids"]))
    auc_all[ref["auc_groups"]] = ref["auc_u"]
    assert np.all(np.abs(auc_all[pick] - want) <= ref["n_u"][pick] * 2.0 ** -52)
    if case[1] == "distinct":
        pick = gm.sampled(ref["ranked_groups"] & (ref["n_u"] >= 2))
        want = fx[f"ndcg_{idx}"]
        assert want.shape == (len(pick), len(gm.KS))
        for j, k in enumerate(gm.KS):
            keff = np.minimum(k, ref["n_u"][pick])
            assert np.all(np.abs(ref["ndcg_u"][pick, j] - want[:, j]) <= (keff + 2) * 2.0 ** -52)
    else:
        assert f"ndcg_{idx}" not in fx


def test_equal_scores_follow_input_position():
    """All scores equal: every AUC group has AUC_u exactly 0.5, and the rank
    is the position among the group's rows in input order."""
    n = 3 * gm.UNIT + 3
    for case in (c for c in gm.CASES if c[0] == n and c[1] == "equal"):
        z, y, g, ng, _, ref = gm.case_with_reference(case)
        assert ref["n_groups_auc"] > 0 or case[2] == "own"
        assert np.all(ref["auc_u"] == 0.5)
        if ref["n_groups_auc"]:
            assert ref["gauc"] == 0.5 and ref["auc_macro"] == 0.5
        for o in gm.sampled(ref["ranked_groups"], 32):
            rows = np.flatnonzero(g == ref["gids"][o])          # ascending input position
            first = int(np.flatnonzero(y[rows] == 1.0)[0]) + 1
            assert int(ref["first_pos_rank"][o]) == first
            for j, k in enumerate(gm.KS):
                assert int(ref["hits"][o, j]) == int((y[rows][:k] == 1.0).sum())


def test_separated_scores_are_perfect():
    """Every positive above every negative: gauc, mrr and every ndcg are 1.0."""
    z, y = mc.make_case((3 * gm.UNIT + 3, "sep_pos", 77))
    rng = np.random.default_rng(78)
    g = rng.integers(0, 1500, z.shape[0]).astype(np.int64)
    ref = gm.host_reference(z, y, g, 1500)
    assert ref["gauc"] == 1.0 and ref["auc_macro"] == 1.0 and ref["mrr"] == 1.0
    assert ref["ndcg"] == (1.0,) * len(gm.KS)
    assert ref["hit_rate"] == (1.0,) * len(gm.KS)
    assert ref["recall"][-1] == 1.0 and ref["n_groups_ranked"] > 1000


def test_one_group_is_the_global_auc():
    case = next(c for c in gm.CASES if c[2] == "one" and c[1] == "q16" and c[0] == 65)
    z, y, g, ng, _, ref = gm.case_with_reference(case)
    u2, P, N = mc.exact_u2(z, y)
    assert (int(ref["auc_u2"][0]), int(ref["n_pos"][0]), int(ref["n_u"][0])) == (u2, P, P + N)


def test_symbols_structs_and_workspace():
    from dcnr import _lib
    assert ctypes.sizeof(_lib.GroupRecordStruct) == 96
    assert ctypes.sizeof(_lib.GroupSummaryStruct) == 216
    lib = _lib.load()
    assert lib.dcnr_eval_group_metrics.argtypes[5] == ctypes.POINTER(ctypes.c_int32)
    assert len(lib.dcnr_eval_group_metrics.argtypes) == 14
    size = lib.dcnr_eval_group_metrics_workspace_size
    assert size.restype == ctypes.c_size_t
    assert size(0, 1) == 0 and size(0, 1 << 20) == 0 and size(-5, 1) == 0
    ns = (1, 2, 63, 64, 65, 2048, 4096, 4097, 1 << 20, (1 << 22) + 1, (1 << 31) - 1)
    for ng in (1, 1 << 17, (1 << 31) - 1):
        sizes = [size(n, ng) for n in ns]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
        assert sizes[8] >= 16 << 20                       # two 8-byte keys per row
        assert sizes[8] < 32 << 20                        # O(n): no per-group storage
    # the pass count decides, not the value of n_groups
    n = 1 << 20
    assert size(n, (1 << 22) + 1) == size(n, 1 << 23)
    assert size(n, 1) == size(n, 2)                                      # 3 passes: 33 key bits
    assert size(n, 3) == size(n, (1 << 11) + 1) == size(n, 1 << 12)      # 4 passes
    assert size(n, 1) < size(n, (1 << 11) + 1) < size(n, (1 << 22) + 1) < size(n, (1 << 31) - 1)
    # the header's formula
    U = min(1024, -(-n // 4096))
    A = -(-n // max(2048, -(-(-(-n // 1024)) // 256) * 256))
    for ng, p in ((1, 3), ((1 << 11) + 1, 4), ((1 << 22) + 1, 5), ((1 << 31) - 1, 6)):
        exact = 16 * n + 4 * 2048 * (p + U) + 32 + 552 * A
        assert exact <= size(n, ng) < exact + 2048


def test_bad_arguments_return_on_the_host():
    """Every DCNR_BAD_ARG case is decided before any launch: the device
    pointers are null."""
    from dcnr import _lib
    lib = _lib.load()
    out = ctypes.create_string_buffer(216)
    o = ctypes.addressof(out)
    one = ctypes.create_string_buffer(64)
    p = ctypes.addressof(one)          # stands for non-null device arrays that are never read

    def call(n=0, ng=1, ks=(), outp=o, ptrs=p):
        arr = (ctypes.c_int32 * max(1, len(ks)))(*ks)
        return lib.dcnr_eval_group_metrics(None, None, None, n, ng, arr, len(ks), ptrs, ptrs, outp,
                                           None, None, 0, None)

    B = _lib.DCNR_BAD_ARG
    assert call(n=-1) == B
    assert call(n=1 << 31) == B
    assert call(ng=0) == B
    assert call(ng=1 << 31) == B
    assert call(ng=-3) == B
    assert call(ks=(1, 2, 3, 4, 5)) == B
    assert call(ks=(0,)) == B
    assert call(ks=(5, 5)) == B
    assert call(ks=(10, 5)) == B
    assert call(ks=((1 << 20) + 1,)) == B
    assert call(outp=None) == B
    assert call(ks=(5,), ptrs=None) == B                # cutoffs without their tables
    assert call(n=10) == B                              # rows without their arrays
    assert b"dcnr_eval_group_metrics" in lib.dcnr_last_error()
    assert lib.dcnr_abi_version() == 4


def test_python_names_exported():
    import dcnr
    assert dcnr.GroupMetrics._fields[:3] == ("gauc", "auc_macro", "mrr")
    assert callable(dcnr.group_metrics) and callable(dcnr.evaluate_ranking)
    d, i = dcnr.metrics.dcg_tables(7)
    d2, i2 = gm.dcg_tables(7)
    assert d.tobytes() == d2.tobytes() and i.tobytes() == i2.tobytes()
    assert d[0] == 1.0 and math.isclose(i[1], 1.0 + 1.0 / math.log2(3.0), rel_tol=1e-15)
