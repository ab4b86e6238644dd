"""``dcnr.CitySets`` on the host (no device): every comparison is an equality.

  1  the numpy model of tests/city_sets_common.py against the pandas
     restatement of main.py:205-209 on generated tables: with kind='stable' for
     every city, with the reference's default kind for the cities whose tie
     group at the cut names one hotel or does not straddle the cut
  2  ``CitySets`` on the F7 fixture against ``f7_common.request_rows``
  3  ``CitySets``'s host functions, ``append`` and ``remove`` against the model
     and a freshly built object, array by array; refused calls change nothing
"""
import numpy as np
import pytest

import city_sets_common as cc
import f7_common


# ------------------------------------------------ 1: the model against pandas
@pytest.mark.parametrize("M,C,n_items,top,seed", [(3000, 12, 150, 100, 1), (2500, 30, 60, 20, 2),
                                                   (600, 5, 30, 100, 3)])
def test_model_against_pandas(M, C, n_items, top, seed):
    item, city, key = cc.table(M, C, n_items, seed, top)
    row = np.arange(M)
    sets = cc.model_sets(item, city, key, row, C, top)
    nonempty = decided = above = 0
    for c in range(C):
        got_city, got_top, got_pop = sets[c]
        want_city, want_top, want_pop = cc.pandas_sets(item, city, key, row, c, top, kind="stable")
        assert got_city.tolist() == want_city, c
        assert got_top.tolist() == want_top.tolist(), c
        assert got_pop.tolist() == want_pop, c
        m = city == c
        if not m.any():
            continue
        nonempty += 1
        above += int(m.sum()) > top
        if cc.cut_is_decided(item[m], key[m], row[m], top):
            decided += 1
            assert got_pop.tolist() == cc.pandas_sets(item, city, key, row, c, top)[2], c
    # the generator's promise: the reference's own sort kind decides at least half
    assert 2 * decided >= nonempty and nonempty < C and above >= 2


# ----------------------------------------------------------- 2: the F7 fixture
def test_f7_sets_match_request_rows():
    f = f7_common.load()
    cs, code = cc.f7_city_sets(f)
    assert len(code) == 3
    sizes = []
    for name, c in code.items():
        r = f7_common.request_rows(f, dict(user_id=-1, city=name, type="personal"))
        assert cs.city_rows_host(c).tolist() == r["allowed"], name
        assert set(cs.popular_rows_host(c).tolist()) == set(r["fallback"]), name
        stable = f.main_df[f.main_df["city"] == name].sort_values(
            by="user_reviews_count", ascending=False, kind="stable").head(100)
        assert cs.top_rows_host(c).tolist() == stable.index.tolist(), name
        sizes.append(cs.popular_rows_host(c).size)
    assert sorted(sizes) == [18, 18, 19]
    assert cs.city_rows_host(-1).size == cs.popular_rows_host(-1).size == cs.top_rows_host(-1).size == 0


# ------------------------------------------- 3: the host object, the sequences
def assert_model(cs, st, what):
    sets = cc.model_sets(st.item, st.city, st.key, st.row, cc.C, cc.TOP)
    for c in range(cc.C):
        for got, want in zip((cs.city_rows_host(c), cs.top_rows_host(c), cs.popular_rows_host(c)),
                             sets[c]):
            assert got.dtype == np.int64 and got.tolist() == want.tolist(), (what, c)


@pytest.mark.parametrize("name,st,steps", cc.sequences(), ids=[s[0] for s in cc.sequences()])
def test_host_sequences(name, st, steps):
    cs = st.fresh()
    assert_model(cs, st, name)
    for i, step in enumerate(steps):
        before = (cs.city_rows_host(0).tolist(), cs.top_rows_host(3).tolist())
        cc.do(cs, step)
        st.apply(step)
        cc.assert_same(cs, st.fresh(), f"{name}[{i}]")
        assert_model(cs, st, f"{name}[{i}]")
        if name == "only_row_of_a_pair":
            assert 39 in before[0] and 39 not in cs.city_rows_host(0)
        if name == "inside_top_rows" and i == 0:
            assert cs.top_rows_host(3).tolist()[:4] == before[1][1:] and \
                len(cs.top_rows_host(3)) == cc.TOP and cs.top_rows_host(3)[4] not in before[1]
    assert cs.last_update is not None and cs.last_update["devices"] == 0


def test_refused_calls_change_nothing():
    st = cc.State(*cc.base_table())
    cs = st.fresh()
    snap = cc.snapshot(cs)
    for call in cc.refused(cs):
        with pytest.raises(ValueError):
            call()
        cc.assert_same(cs, snap)
    cs.append()
    cs.remove([])
    cc.assert_same(cs, snap)
    assert cs.last_update is None
    import dcnr
    for bad in (dict(n_items=0), dict(top=0), dict(top=257), dict(n_cities=0), dict(n_cities=65537),
                dict(review_row=np.arange(200)[::-1]), dict(next_review_row=5)):
        kw = dict(n_items=cc.N_ITEMS, n_cities=cc.C, top=cc.TOP)
        kw.update(bad)
        with pytest.raises(ValueError):
            dcnr.CitySets(st.item, st.city, st.key, **kw)
