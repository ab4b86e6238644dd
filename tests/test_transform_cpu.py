"""``dcnr.Preprocessor.transform_host`` and ``dcnr.IdMap.lookup_host`` (no
device).  Every comparison is exact: integers equal, floats equal as
``prepare_common.same`` defines it.

  1  ``transform_host`` against the reference's ``preprocess_for_ranking`` on the
     fixture of tests/golden/transform
  2  identity: the fit's own input through ``transform_host`` is
     ``prepare_data_host``'s unsplit tables (the train.py side)
  3  ``from_artifacts`` transforms like ``preprocessor()``
  4  ``IdMap.lookup_host`` against a dict; the ``ValueError``s
  5  the C ABI: the new symbols in include/dcnr.h and the binding
"""
import os
import re

import numpy as np
import pytest

import prepare_common as pc
import transform_common as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_fit():
    import dcnr
    return pc.call(dcnr.prepare_data_host, pc.golden_case())


# ------------------------------------------------------------ 1: the reference
def test_transform_host_matches_reference():
    g = tc.load_golden()
    pre = golden_fit().preprocessor()
    t = pre.transform_host(*tc.golden_rows(g), unknown="reference", fill_nan=False)
    tc.assert_matches_golden(t, g)
    # what the fixture's rows hold, seen through the counts and the bits
    assert t.n_unknown_users == 12 and t.n_unknown_items == 4
    assert t.n_unknown_cat == [7, 4]          # Ufa x3, Tver x2, missing x2; missing x3, camping
    bits = t.unknown_bits
    assert (bits[t.collab[:, 0] != len(pre.user_ids) // 2] & 1 == 0).all()
    assert ((bits & 2) != 0).sum() == 4 and (t.collab[(bits & 2) != 0, 1] == 0).all()
    assert np.isnan(t.num).any()
    # the same rows with the medians filled in: no NaN left
    filled = pre.transform_host(*tc.golden_rows(g), unknown="reference", fill_nan=True)
    assert not np.isnan(filled.num).any()
    keep = ~np.isnan(t.num)
    assert pc.same(filled.num[keep], t.num[keep])


def test_category_keys_of_the_fit():
    pre = golden_fit().preprocessor()
    k = pre.category_keys(0, np.array(["Moscow", None, "Ufa", float("nan"), "Kazan"], dtype=object))
    cats = pre.categories[0]
    assert k.tolist() == [cats.index("Moscow"), -1, -2, -1, cats.index("Kazan")]
    assert pre.category_keys(0, np.array(["Moscow", "Ufa"])).tolist() == [cats.index("Moscow"), -2]
    assert pre.category_keys(1, np.array([3, -1, 7])).tolist() == [3, -1, 7]   # integer keys pass through


# -------------------------------------------------------------- 2: the identity
@pytest.mark.parametrize("case", ["golden", 41, 42, 43])
def test_identity_on_the_fit_input(case):
    import dcnr
    case = pc.golden_case() if case == "golden" else pc.random_case(case, 900 + 37 * case)
    p = pc.call(dcnr.prepare_data_host, case)
    assert p.derived == [tuple(d) for d in case["derived"]] and p.noise_filter == tuple(case["noise_filter"])
    t = p.preprocessor().transform_host(case["user"], case["item"], case["target"], case["cat"], case["num"],
                                        noise_filter="fitted", unknown="drop", fill_nan=True)
    for k, a, b in zip(("collab", "cat", "num", "y"), t.tensors, p.full):
        assert pc.same(a, b), k
    assert pc.same(t.rows, p.rows)
    assert t.n == len(p.rows) and t.n_filtered == len(case["user"]) - p.n_after_filter
    # (the counts are over the rows that passed the filter: a row the fit dropped for its
    # missing category may hold a user or hotel seen nowhere else)
    assert not t.unknown_bits.any()
    assert sum(t.n_unknown_cat) >= p.n_after_filter - t.n > 0


# ------------------------------------------------------------ 3: from_artifacts
@pytest.mark.parametrize("case", ["golden", 44])
def test_from_artifacts_transforms_like_preprocessor(case):
    import dcnr
    if case == "golden":
        fit_case, g = pc.golden_case(), tc.load_golden()
        new = tc.golden_rows(g)
    else:
        whole = pc.random_case(case, 1500, n_users=400, n_items=150)
        fit_case = dict(whole, **dict(zip(("user", "item", "target", "cat", "num"), tc.part(whole, 0, 800))))
        new = tc.part(whole, 800, 1500)
    p = pc.call(dcnr.prepare_data_host, fit_case)
    a = p.preprocessor()
    b = dcnr.Preprocessor.from_artifacts(p.artifacts(), derived=fit_case["derived"], median=p.median_,
                                         noise_filter=fit_case["noise_filter"])
    assert b.cat_names == a.cat_names and b.n_raw == a.n_raw
    for unknown in ("reference", "drop"):
        ta = a.transform_host(*new, unknown=unknown, noise_filter="fitted")
        tb = b.transform_host(*new, unknown=unknown, noise_filter="fitted")
        tc.assert_same_transformed(ta, tb, f"{case} {unknown}")
    # without the medians only fill_nan=False can run
    c = dcnr.Preprocessor.from_artifacts(p.artifacts(), derived=fit_case["derived"])
    with pytest.raises(ValueError):
        c.transform_host(*new)
    tc.assert_same_transformed(c.transform_host(*new, fill_nan=False), a.transform_host(*new, fill_nan=False))


def test_from_artifacts_takes_a_scaler_object():
    import dcnr
    p = golden_fit()
    art = dict(p.artifacts())
    art["scaler"] = type("Scaler", (), dict(scale_=p.scale_, min_=p.min_))()
    b = dcnr.Preprocessor.from_artifacts(art, derived=p.derived, median=p.median_)
    g = tc.load_golden()
    tc.assert_matches_golden(b.transform_host(*tc.golden_rows(g), fill_nan=False), g)


# ------------------------------------------------------------------- 4: IdMap
@pytest.mark.parametrize("n,multiples", [(0, False), (1, False), (2, True), (1000, False), (1000, True)])
def test_lookup_host_against_a_dict(n, multiples):
    import dcnr
    rng = np.random.default_rng(n + multiples)
    ids = tc.wide_ids(rng, n, multiples)
    m = dcnr.IdMap(ids, device="cpu")
    assert len(m) == n and m.ids.numpy().tolist() == ids.tolist()
    table = {int(v): i for i, v in enumerate(ids.tolist())}
    absent = tc.wide_ids(rng, 300, multiples) + 7
    q = np.concatenate([rng.choice(ids, 300) if n else absent[:0], absent, [tc.RESERVED, 0]]).astype(np.int64)
    for default in (-1, 12345):
        want = [table.get(int(v), default) for v in q.tolist()]
        assert m.lookup_host(q, default).tolist() == want
    assert m.lookup_host(np.zeros(0, np.int64)).shape == (0,)


def test_value_errors():
    import dcnr
    with pytest.raises(ValueError):
        dcnr.IdMap(np.array([5, 9, 5]), device="cpu")
    with pytest.raises(ValueError):
        dcnr.IdMap(np.array([5, tc.RESERVED]), device="cpu")
    with pytest.raises(ValueError):
        dcnr.IdMap(np.arange(8), device="cpu", capacity=8)       # no room for an empty slot
    with pytest.raises(ValueError):
        dcnr.IdMap(np.arange(8), device="cpu", capacity=24)      # no power of two
    g = tc.load_golden()
    pre = golden_fit().preprocessor()
    user, item, target, cat, num = tc.golden_rows(g)
    with pytest.raises(ValueError):
        pre.transform_host(user, item[:-1], target, cat, num)
    with pytest.raises(ValueError):
        pre.transform_host(user, item, np.zeros(3), cat, num)
    with pytest.raises(ValueError):
        pre.transform_host(user, item, target, [cat[0][:-1], cat[1]], num)
    with pytest.raises(ValueError):
        pre.transform_host(user, item, target, cat[:1], num)
    with pytest.raises(ValueError):
        pre.transform_host(user, item, target, cat, num[:, :5])
    with pytest.raises(ValueError):
        pre.transform_host(user, item, target, cat, num, unknown="ignore")
    with pytest.raises(ValueError):
        pre.transform_host(user, item, target, cat, num, noise_filter="fit")
    with pytest.raises(ValueError):
        pre.transform_host(user, item, target, cat, num, noise_filter=(8, 4.0, 8.0))
    bad = num.copy()
    bad[5, 2] = np.inf
    with pytest.raises(ValueError, match="infinity"):
        pre.transform_host(user, item, target, cat, bad)


# ------------------------------------------------------------------ 5: the ABI
def test_new_symbols_are_declared_and_bound():
    import dcnr
    from dcnr import _lib
    txt = open(os.path.join(ROOT, "include", "dcnr.h")).read()
    declared = set(re.findall(r"\b(dcnr_[a-z0-9_]+)\s*\(", txt))
    lib = _lib.load()
    for s in ("dcnr_id_map_build", "dcnr_id_map_lookup", "dcnr_rows_transform_workspace_size",
              "dcnr_rows_transform"):
        assert s in declared and s in _lib.exported_symbols() and hasattr(lib, s)
    assert lib.dcnr_abi_version() == 4
    assert callable(dcnr.Preprocessor.transform) and callable(dcnr.IdMap.lookup) and dcnr.Transformed
    size = lib.dcnr_rows_transform_workspace_size
    assert 4 * 1000 <= size(1000, 2, 8, 3) < 4 * 1000 + 4096
    assert size(0, 0, 0, 0) > 0 and size(10, 62, 61, 3) > 0
    assert size(10, 63, 8, 3) == 0 and size(10, 2, 62, 3) == 0 and size(-1, 2, 8, 3) == 0
    assert size(2 ** 31 - 1, 2, 8, 3) == 0
