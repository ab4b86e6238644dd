"""``dcnr.ItemFeatures`` on the host (no device): every comparison is an
equality of bytes.

  1  the host object against the numpy model of tests/item_features_common.py
     and against a freshly built object after every step of every sequence
  2  refused calls change nothing
  3  the F7 fixture: the object reproduces f7_common.load()'s tables, and after
     every hotel's first row is removed the same pandas recipe on the rest
  4  the rounding rule: the witness column on which a fused multiply-add gives
     another float32 than MinMaxScaler's two roundings
  5  the C ABI: the new symbols in include/dcnr.h and the binding
"""
import os
import re

import numpy as np
import pytest

import f7_common
import item_features_common as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------ 1: the host object, the sequences
@pytest.mark.parametrize("name,st,steps", ic.sequences(), ids=[s[0] for s in ic.sequences()])
def test_host_sequences(name, st, steps):
    ft = st.fresh()
    ic.assert_model(ft, st, name)
    for i, step in enumerate(steps):
        before = ic.snapshot(ft)
        ic.do(ft, step)
        st.apply(step)
        ic.assert_same(ft, st.fresh(), f"{name}[{i}]")
        ic.assert_model(ft, st, f"{name}[{i}]")
        assert ft.last_update["op"] == step[0] and ft.last_update["devices"] == 0
        assert ft.last_update["upload_bytes"] == ic.upload_bytes(step)
        first, was = ft.first_rows_host(), before["first_rows_host"]
        if name == "first_ever_row" and i == 0:   # hotels 0 and 89 had no features at all
            assert was[0] == was[89] == -1 and first[0] == 1500 and first[89] == 1501
            assert ft.item_num_host()[89].tobytes() != before["item_num_host"][89].tobytes()
        if name == "first_rows" and i < 2:        # every hotel named moves on to its next row
            gone = np.asarray(step[1])
            moved = np.isin(was, gone)
            assert moved.sum() == gone.size and (first[moved] != was[moved]).all()
            assert ((first[moved] > was[moved]) | (first[moved] == -1)).all()
        if name == "only_row" and i == 0:
            assert was[88] == 700 and first[88] == -1 and not ft.item_num_host()[88].any()
        if name == "edits":                       # an edit of a non-first row changes no table
            changed = ft.item_num_host().tobytes() != before["item_num_host"].tobytes()
            assert changed == (i != 1)
            assert ft.item_cat_host().tobytes() == before["item_cat_host"].tobytes()
        if name == "scaler" and i == 0:
            assert ft.item_num_host().tobytes() != before["item_num_host"].tobytes()
            assert ft.review_num is before["review_num"] or \
                ft.review_num.tobytes() == before["review_num"].tobytes()


def test_repeated_row_in_set_values_takes_the_last():
    st = ic.State(*ic.base_table())
    ft = st.fresh()
    ft.set_values([2, 9, 2, 2], [[1.0], [2.0], [3.0], [4.0]], columns=[1])
    assert ft.review_num[2, 1] == 4.0 and ft.review_num[9, 1] == 2.0


# ------------------------------------------------------------ 2: refused calls
def test_refused_calls_change_nothing():
    import dcnr
    st = ic.State(*ic.base_table())
    ft = st.fresh()
    snap = ic.snapshot(ft)
    for j, call in enumerate(ic.refused(ft)):
        with pytest.raises(ValueError):
            call()
        ic.assert_same(ft, snap, f"refused[{j}]")
    ft.append()
    ft.remove([])
    ft.set_values([], np.zeros((0, ic.N_NUM)))
    ft.set_values([], np.zeros((0, 1)), columns=[2])
    ic.assert_same(ft, snap)
    assert ft.last_update is None
    for bad in (dict(n_items=0), dict(n_items=ic.N_ITEMS - 2), dict(review_row=np.arange(1500)[::-1]),
                dict(review_row=np.arange(1499)), dict(next_review_row=5),
                dict(scaler_scale=ic.SCALE[:3]), dict(scaler_min=np.full(4, np.inf)),
                dict(review_cat=st.cat[:, 0]), dict(review_num=st.num[:, :3]),
                dict(review_cat=st.cat[:7])):
        kw = dict(review_item=st.item, review_cat=st.cat, review_num=st.num, scaler_scale=ic.SCALE,
                  scaler_min=ic.MIN, n_items=ic.N_ITEMS)
        kw.update(bad)
        with pytest.raises(ValueError):
            dcnr.ItemFeatures(**kw)
    # no categorical column, no numeric column, no row
    a = dcnr.ItemFeatures(st.item, None, st.num, ic.SCALE, ic.MIN, n_items=ic.N_ITEMS)
    assert a.item_cat_host().shape == (ic.N_ITEMS, 0) and a.n_cat == 0
    b = dcnr.ItemFeatures(st.item, st.cat, None, [], [], n_items=ic.N_ITEMS)
    assert b.item_num_host().shape == (ic.N_ITEMS, 0) and b.n_num == 0
    e = dcnr.ItemFeatures([], np.zeros((0, 2)), np.zeros((0, 4)), ic.SCALE, ic.MIN, n_items=3)
    assert (e.first_rows_host() == -1).all() and not e.item_num_host().any() and e.next_review_row == 0


# ----------------------------------------------------------- 3: the F7 fixture
def test_f7_tables_and_first_rows_removed():
    f = f7_common.load()
    assert len(f.main_df) == 499
    ft = ic.f7_item_features(f)
    assert ft.item_cat_host().tobytes() == f.item_cat.tobytes()
    assert ft.item_num_host().tobytes() == f.item_num.tobytes()
    firsts = f.main_df.drop_duplicates(subset=["item_id"]).index.to_numpy()
    assert sorted(ft.first_rows_host().tolist()) == sorted(firsts.tolist())
    ft.remove(firsts)
    rest = f.main_df.drop(firsts)
    want_cat, want_num = ic.f7_tables(f, rest)
    assert ft.item_cat_host().tobytes() == want_cat.tobytes()
    assert ft.item_num_host().tobytes() == want_num.tobytes()
    # the hotels that moved on to another row (three lost their only row: zeros, not counted)
    differ = (ft.item_num_host().view(np.uint32) != f.item_num.view(np.uint32)).any(axis=1)
    changed = int((differ & (ft.first_rows_host() >= 0)).sum())
    print("hotels whose numeric features changed:", changed, "; without a row:",
          int((ft.first_rows_host() < 0).sum()))
    assert changed >= 80
    item, cat, num, scale, mn, row = ic.f7_columns(f, rest)
    import dcnr
    ic.assert_same(ft, dcnr.ItemFeatures(item, cat, num, scale, mn, n_items=f.n_items, review_row=row,
                                         next_review_row=499))


# ---------------------------------------------------------- 4: the rounding rule
def test_witness_column_tells_fused_from_two_step():
    x, scale, mn = ic.witness_column()
    two_step = (x * scale + mn).astype(np.float32)
    fused = ic.fused_f32(x, scale, mn)
    differ = int((two_step.view(np.uint32) != fused.view(np.uint32)).sum())
    print("entries whose fused result rounds to another float32:", differ)
    assert differ >= 1
    # the host object and the model give the two-step values
    import dcnr
    ft = dcnr.ItemFeatures(np.arange(x.size), None, x[:, None], [scale], [mn], n_items=x.size)
    assert ft.item_num_host().tobytes() == two_step.tobytes()
    assert ic.model(np.arange(x.size), np.arange(x.size), np.zeros((x.size, 0)), x[:, None], [scale],
                    [mn], x.size)[2].tobytes() == two_step.tobytes()


# -------------------------------------------------------------------- 5: the ABI
def test_new_symbols_are_declared_and_bound():
    import dcnr
    from dcnr import _lib
    txt = open(os.path.join(ROOT, "include", "dcnr.h")).read()
    declared = set(re.findall(r"\b(dcnr_[a-z0-9_]+)\s*\(", txt))
    lib = _lib.load()
    for s in ("dcnr_item_features_workspace_size", "dcnr_item_features_build"):
        assert s in declared and s in _lib.exported_symbols() and hasattr(lib, s)
    assert lib.dcnr_abi_version() == 4
    assert callable(dcnr.ItemFeatures.set_values)
    size = lib.dcnr_item_features_workspace_size
    assert 4 * 1000 <= size(10, 1000, 2, 11) == size(1 << 24, 1000, 64, 0) < 4 * 1000 + 16384
    assert size(10, (1 << 29) + 1, 2, 11) == 0 and size(2 ** 31 - 1, 5, 2, 11) == 0
    assert size(10, 5, 65, 1) == 0 and size(10, 5, 1, 65) == 0 and size(-1, 5, 1, 1) == 0
