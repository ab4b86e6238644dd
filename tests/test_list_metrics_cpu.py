"""Host tests of the list metrics: the reference of tests/list_metrics_cases.py
against brute force, ``dcnr.popularity_information``, and everything of
dcnr_eval_list_metrics and ``dcnr.list_metrics`` that is decided before a
launch (no GPU)."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import list_metrics_cases as lc


def count_of_counts_numerator(expo, R):
    """The device's route in Python ints: h[v] = items with count v (v <= R),
    ascending scan of v h_v (2 before_v + h_v - n_items); the few counts above
    R one item each, ascending."""
    n_items = len(expo)
    h = {}
    for c in expo:
        h[c] = h.get(c, 0) + 1
    before = total = 0
    for v in sorted(h):
        total += v * h[v] * (2 * before + h[v] - n_items)
        before += h[v]
    return total


@pytest.mark.parametrize("name", [n for n in lc.NAMES if n not in lc.BIG])
def test_reference_against_brute_force(name):
    c = lc.make_case(name)
    inv = lc.numpy_inv_norms(c["table"])
    ref = lc.host_reference(c, inv)
    expo = ref["exposure"]
    n_items, total = c["n_items"], sum(expo)
    assert total == ref["n_entries"] == int(ref["records"]["m"].sum())
    # Gini = sum_ij |c_i - c_j| / (2 n sum c), exactly
    if total and n_items <= 1000:
        e = np.array(expo, np.int64)
        mad = int(np.abs(e[:, None] - e[None, :]).sum())
        assert Fraction(mad, 2 * n_items * total) == Fraction(ref["gini_num"], n_items * total)
        assert 0.0 <= ref["gini"] < 1.0
    assert count_of_counts_numerator(expo, c["R"]) == ref["gini_num"]
    assert ref["n_distinct_items"] == n_items - expo.count(0)
    # ILD by explicit loops over the measured rows of a few lists
    T = c["table"].astype(np.float64)
    invd = inv.astype(np.float64)
    checked = 0
    for r in range(c["R"]):
        m = int(ref["records"]["m"][r])
        if m < 2 or checked >= 12:
            continue
        o = int(c["offsets"][r])
        lst = c["rows"][o:o + m]
        s = 0.0
        for i in range(m):
            for j in range(i + 1, m):
                s += float(np.dot(T[lst[i]], T[lst[j]])) * invd[lst[i]] * invd[lst[j]]
        assert abs(s - ref["records"]["pair_cos_sum"][r]) <= 1e-12 * m * m
        checked += 1


def test_closed_forms_of_the_reference():
    c = lc.make_case("identical")
    ref = lc.host_reference(c, lc.numpy_inv_norms(c["table"]))
    m, n_items = c["at"], c["n_items"]
    # m items shown R times each, the rest never: Gini = 1 - m / n_items
    assert Fraction(ref["gini_num"], n_items * ref["n_entries"]) == 1 - Fraction(m, n_items)
    assert ref["n_distinct_items"] == m
    c = lc.make_case("equal")
    ref = lc.host_reference(c, lc.numpy_inv_norms(c["table"]))
    assert ref["gini_num"] == 0 and ref["gini"] == 0.0 and ref["coverage"] == 1.0
    c = lc.make_case("broken")
    ref = lc.host_reference(c, lc.numpy_inv_norms(c["table"]))
    assert (ref["n_marked"], ref["n_bad_list"]) == (1, 7)
    c = lc.make_case("mix")
    ref = lc.host_reference(c, lc.numpy_inv_norms(c["table"]))
    # rows 0, 1, 2 share one embedding: their three cosines are 1
    r = next(r for r in range(0, c["R"], 4) if ref["records"]["m"][r] == 3)
    assert abs(ref["records"]["pair_cos_sum"][r] - 3.0) < 1e-6
    assert sorted(set(int(v) for v in ref["records"]["m"])) == lc.lengths(c["at"])[:-1]


def test_popularity_information():
    import dcnr
    p = dcnr.popularity_information([0, 1, 3, 0])
    assert p.dtype == np.float64 and p.shape == (4,)
    want = [-math.log2((c + 1) / (4 + 4)) for c in (0, 1, 3, 0)]
    assert np.allclose(p, want, rtol=1e-15, atol=0)
    assert p[0] == 3.0 and p[2] == 1.0                    # 1/8 and 4/8
    assert np.isfinite(p).all() and (p >= 0).all()
    assert (dcnr.popularity_information(np.zeros(5)) == math.log2(5)).all()
    assert np.array_equal(dcnr.popularity_information(torch.tensor([2, 0])), dcnr.popularity_information([2, 0]))
    with pytest.raises(ValueError):
        dcnr.popularity_information([1, -1])


def test_symbols_structs_and_workspace():
    from dcnr import _lib
    assert ctypes.sizeof(_lib.ListRecordStruct) == 112
    assert ctypes.sizeof(_lib.ListSummaryStruct) == 248
    syms = _lib.exported_symbols()
    assert "dcnr_eval_list_metrics" in syms and "dcnr_eval_list_metrics_workspace_size" in syms
    lib = _lib.load()
    assert len(lib.dcnr_eval_list_metrics.argtypes) == 24
    size = lib.dcnr_eval_list_metrics_workspace_size
    assert size.restype == ctypes.c_size_t
    # empty shapes and shapes the call rejects
    assert size(0, 1000) == 0 and size(-1, 1000) == 0 and size(10, 0) == 0 and size(10, -4) == 0
    assert size((1 << 22) + 1, 1000) == 0 and size(10, 1 << 31) == 0
    # the two histograms and < 400 KiB of partial sums
    for R, n_items in ((1, 1), (256, 1000), (1 << 20, 1 << 20), (1 << 22, (1 << 31) - 1)):
        s = size(R, n_items)
        assert 4 * n_items + 4 * (R + 1) <= s < 4 * n_items + 4 * (R + 1) + (400 << 10)
    assert lib.dcnr_abi_version() == _lib.ABI_VERSION == 4


def test_bad_arguments_return_on_the_host():
    """Every argument error is decided before any launch: the device pointers
    are null or stand-ins that are never read."""
    from dcnr import _lib
    lib = _lib.load()
    out = ctypes.create_string_buffer(248)
    o = ctypes.addressof(out)
    one = ctypes.create_string_buffer(64)
    p = ctypes.addressof(one)

    def call(n=10, R=2, at=20, d=64, n_items=100, ks=(), outp=o, rows=p, offsets=p, table=p, inv=p,
             rel_rows=None, n_rel=0, rel_off=None, tabs=p, ws=None, ws_bytes=0):
        arr = (ctypes.c_int32 * max(1, len(ks)))(*ks)
        return lib.dcnr_eval_list_metrics(rows, n, offsets, None, R, at, table, inv, d, n_items, None,
                                          None, rel_rows, n_rel, rel_off, arr, len(ks), tabs, tabs,
                                          outp, None, ws, ws_bytes, None)

    B, U, W = _lib.DCNR_BAD_ARG, _lib.DCNR_UNSUPPORTED_SHAPE, _lib.DCNR_WORKSPACE_TOO_SMALL
    assert call(R=-1) == B
    assert call(n=-1) == B
    assert call(n_items=0) == B
    assert call(at=0) == B
    assert call(at=129) == B
    assert call(d=0) == B
    assert call(d=257) == B
    assert call(outp=None) == B
    assert call(rows=None) == B
    assert call(offsets=None) == B
    assert call(table=None) == B
    assert call(inv=None) == B
    assert call(ks=(1, 2, 3, 4, 5)) == B
    assert call(ks=(0,)) == B
    assert call(ks=(5, 5)) == B
    assert call(ks=(10, 5)) == B
    assert call(ks=(5, 21)) == B                               # a cutoff above at
    assert call(ks=(5,), rel_off=p, tabs=None) == B            # cutoffs and sets without the tables
    assert call(rel_off=p, n_rel=3, rel_rows=None) == B        # held-out rows missing
    assert call(n_rel=-1) == B
    assert b"dcnr_eval_list_metrics" in lib.dcnr_last_error()
    assert call(R=(1 << 22) + 1) == U
    assert call(n=(1 << 30) + 1) == U
    assert call(n_items=1 << 31) == U
    need = lib.dcnr_eval_list_metrics_workspace_size(2, 100)
    assert call(ws=p, ws_bytes=need - 1) == W
    assert call(ws=None, ws_bytes=0) == W
    assert b"workspace too small" in lib.dcnr_last_error()
    assert call(ws=None, ws_bytes=need) == B                   # a size without a workspace


def test_wrapper_value_errors():
    """``dcnr.list_metrics`` raises before it asks for a device."""
    import dcnr
    rows = torch.arange(6)
    off = torch.tensor([0, 3, 6])
    table = torch.ones(10, 4)
    ok = dict(table=table, at=3, ks=(1, 3))
    for kw in (dict(ks=(3, 1)), dict(ks=(2, 2)), dict(ks=(0, 2)), dict(ks=(1, 4)), dict(at=129, ks=()),
               dict(at=0, ks=()), dict(ks=(1, 2, 3, 4, 5), at=20),
               dict(scores=torch.zeros(5)), dict(info=np.zeros(9)), dict(inv_norms=torch.ones(9)),
               dict(relevant=[{1}]), dict(relevant=[{1}, {10}]), dict(relevant=([1], [0, 1])),
               dict(relevant=([1, 2], [0, 2, 1])), dict(table=torch.ones(10))):
        with pytest.raises(ValueError):
            dcnr.list_metrics(rows, off, **{**ok, **kw})
    with pytest.raises(ValueError):
        dcnr.list_metrics(rows, off, torch.tensor([3], dtype=torch.int32), **ok)
    with pytest.raises(ValueError):
        dcnr.list_metrics(rows, torch.zeros(0, dtype=torch.int64), **ok)
    # valid arguments on host tensors: the device is asked for, not an eager stand-in
    with pytest.raises(RuntimeError, match="HIP device only"):
        dcnr.list_metrics(rows, off, **ok)
    assert dcnr.ListMetrics._fields[:3] == ("ild", "coverage", "gini")


def test_relevant_csr_sorts_and_deduplicates():
    from dcnr.metrics import relevant_csr
    rows, off = relevant_csr([[5, 1, 5], None, (), {9, 0}], 4, 10)
    assert rows.tolist() == [1, 5, 0, 9] and off.tolist() == [0, 2, 2, 2, 4]
    rows2, off2 = relevant_csr((np.array([5, 1, 5, 9, 0]), np.array([0, 3, 3, 3, 5])), 4, 10)
    assert rows2.tolist() == rows.tolist() and off2.tolist() == off.tolist()
    rows3, off3 = relevant_csr([[], []], 2, 10)
    assert rows3.size == 0 and off3.tolist() == [0, 0, 0]
