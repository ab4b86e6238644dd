"""Admitting new users and hotels, the parts that need no device.

  1  ``IdMap.insert_host`` against a Python dict that numbers by first appearance
  2  the numbering is the reference's: a fit on P, then ``transform_host(S,
     unknown="admit")``, numbers users and hotels as a fit on P + S does
     (``prepare_data_host`` is pinned to train.py by test_prepare_cpu.py)
  3  the append route of the neighbour table is exact: the update rule of
     neighbor_update_rule.py, fed the appended rows as the changed rows of the
     grown table, gives the brute-force table through three branches only
  4  ``Preprocessor.admit``; ``DCN_RecSys.grow_`` on the host
  5  the C ABI: the new symbols declared, exported and bound; the size query
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import admit_common as ac
import neighbor_update_rule as rule
import prepare_common as pc
import transform_common as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------- 1: insert_host
def host_map(ids):
    import dcnr
    return dcnr.IdMap(np.asarray(ids, dtype=np.int64), device="cpu")


@pytest.mark.parametrize("case", ["duplicates", "all_known", "all_new", "empty", "negative", "int64_max",
                                  "empty_map"])
def test_insert_host_against_a_dict(case):
    rng = np.random.default_rng(7)
    ids = np.array([10, -3, 7, 1 << 40, 0], dtype=np.int64)
    raw = {
        "duplicates": np.array([99, 7, 99, 98, 99, 10, 98, 97, 97, 7]),
        "all_known": np.array([0, 10, 10, -3, 1 << 40]),
        "all_new": np.array([5, 4, 3, 2, 1]),
        "empty": np.zeros(0),
        "negative": np.array([-1, -(1 << 62), -3, -1, ac.RESERVED + 1, -7]),
        "int64_max": np.array([ac.INT64_MAX, 7, ac.INT64_MAX, ac.INT64_MAX - 1]),
        "empty_map": rng.integers(-50, 50, 300),
    }[case].astype(np.int64)
    if case == "empty_map":
        ids = np.zeros(0, np.int64)
    m = host_map(ids)
    table = {int(v): i for i, v in enumerate(ids.tolist())}
    want_idx, want_new = ac.dict_insert(table, raw)
    idx, new = m.insert_host(raw)
    assert idx.dtype == np.int64 and new.dtype == np.int64
    assert np.array_equal(idx, want_idx) and np.array_equal(new, want_new)
    assert len(m) == len(table) and m.ids.numpy().tolist() == list(table.keys())
    # the sorted host cache follows: every id ever inserted is found
    every = np.array(list(table.keys()), dtype=np.int64)
    assert np.array_equal(m.lookup_host(every), np.arange(every.size))
    # a second insert numbers on from there
    more = np.concatenate([raw[::-1], np.array([123456789, raw[0] if raw.size else 1])]).astype(np.int64)
    want_idx, want_new = ac.dict_insert(table, more)
    idx, new = m.insert_host(more)
    assert np.array_equal(idx, want_idx) and np.array_equal(new, want_new)
    # insert on a host map is insert_host
    idx, new = m.insert(np.array([1, 2, 1], dtype=np.int64) + (1 << 45))
    assert idx.tolist() == [len(table), len(table) + 1, len(table)] and new.tolist() == [(1 << 45) + 1, (1 << 45) + 2]


def test_insert_host_reserved_id_leaves_the_map():
    m = host_map([4, 5, 6])
    with pytest.raises(ValueError):
        m.insert_host(np.array([9, ac.RESERVED, 4], dtype=np.int64))
    assert len(m) == 3 and m.ids.tolist() == [4, 5, 6]
    assert m.lookup_host(np.array([9, 4])).tolist() == [-1, 0]


# ------------------------------------------------- 2: the reference's numbering
@pytest.mark.parametrize("use_filter", [False, True])
@pytest.mark.parametrize("seed,M,M2", [(51, 600, 400), (52, 300, 900)])
def test_admit_numbers_like_a_fit_on_all_rows(seed, M, M2, use_filter):
    import dcnr
    whole, fit_case = ac.split_case(seed, M, M2, use_filter=use_filter)
    small = pc.call(dcnr.prepare_data_host, fit_case)
    full = pc.call(dcnr.prepare_data_host, whole)
    pre = small.preprocessor()
    n_u, n_h = len(pre.user_ids), len(pre.item_ids)
    t = pre.transform_host(*tc.part(whole, M, M + M2), unknown="admit",
                           noise_filter="fitted" if use_filter else None)
    assert t.new_user_ids.size > 10 and t.new_item_ids.size > 3
    assert np.array_equal(np.concatenate([pc.to_np(small.user_ids), t.new_user_ids]), pc.to_np(full.user_ids))
    assert np.array_equal(np.concatenate([pc.to_np(small.item_ids), t.new_item_ids]), pc.to_np(full.item_ids))
    assert np.array_equal(pc.to_np(pre.user_ids), pc.to_np(full.user_ids))
    assert np.array_equal(pc.to_np(pre.item_ids), pc.to_np(full.item_ids))
    # S's kept rows carry the full fit's codes
    rows = pc.to_np(full.rows).astype(np.int64)
    later = rows >= M
    assert np.array_equal(rows[later] - M, t.rows)
    assert np.array_equal(pc.to_np(full.full[0])[later], t.collab)
    # bits 0 and 1: admitted by this call
    assert np.array_equal((t.unknown_bits & 1) != 0, t.collab[:, 0] >= n_u)
    assert np.array_equal((t.unknown_bits & 2) != 0, t.collab[:, 1] >= n_h)
    assert t.n_unknown_users == int((t.collab[:, 0] >= n_u).sum())
    # afterwards nothing of S is unknown
    again = pre.transform_host(*tc.part(whole, M, M + M2), unknown="reference",
                               noise_filter="fitted" if use_filter else None)
    assert again.n_unknown_users == 0 and again.n_unknown_items == 0
    assert np.array_equal(again.collab, t.collab)
    # "reference" and "drop" are as they were: a fresh preprocessing of P does not grow
    fresh = small.preprocessor()
    ref = fresh.transform_host(*tc.part(whole, M, M + M2), unknown="reference")
    assert len(fresh.user_ids) == n_u and ref.new_user_ids.size == 0 and ref.n_unknown_users > 0


def test_preprocessor_admit_on_the_host():
    import dcnr
    whole, fit_case = ac.split_case(53, 200, 50)
    pre = pc.call(dcnr.prepare_data_host, fit_case).preprocessor()
    users0, items0 = pc.to_np(pre.user_ids).copy(), pc.to_np(pre.item_ids).copy()
    new_u, new_h = pre.admit(users=np.array([users0[3], 1 << 55, 17 + (1 << 56), 1 << 55]),
                             items=np.array([(1 << 57) + 1]))
    assert new_u.tolist() == [1 << 55, 17 + (1 << 56)] and new_h.tolist() == [(1 << 57) + 1]
    assert pc.to_np(pre.user_ids).tolist() == users0.tolist() + new_u.tolist()
    assert pc.to_np(pre.item_ids).tolist() == items0.tolist() + new_h.tolist()
    assert pre.admit(users=new_u)[0].size == 0             # known now
    assert pre.admit()[0].size == 0 and pre.admit()[1].size == 0
    mapping = {int(v): i for i, v in enumerate(pc.to_np(pre.user_ids).tolist())}   # artifacts()-style
    assert mapping[1 << 55] == users0.size
    with pytest.raises(ValueError):
        pre.admit(users=np.array([5]), items=np.array([ac.RESERVED]))
    assert len(pre.user_ids) == users0.size + 2            # nothing changed: 5 was not admitted


# -------------------------------------------------- 3: the append route is exact
@pytest.fixture(scope="module")
def fitted():
    table, ties, zero = rule.planted_table(300, 16, seed=3)
    return table, rule.brute_table(rule.distances(table), 11)


@pytest.mark.parametrize("m", [1, 7, 64])
def test_append_through_the_update_rule_is_exact(fitted, m):
    table, old = fitted
    N, kt = old.shape
    new = ac.appended_rows(table, m, seed=100 + m)
    D = ac.grown_distances(table, new)
    start = np.concatenate([old, np.zeros((m, kt), np.int64)])     # the new rows' lists: row 0
    C = np.arange(N, N + m)
    got, branches = rule.apply_rule(start, D, C)
    want = rule.brute_table(D, kt)
    assert np.array_equal(got, want)
    for name in ("merged_hole", "hole", "emptied"):
        assert not branches[name].any(), name
    assert branches["changed"].sum() == m and (m == 1 or branches["gained"].any())
    assert (branches["changed"] | branches["untouched"] | branches["gained"]).all()
    # the planted kinds did what they are there for
    assert np.array_equal(want[N], want[5]) and N not in want[5]   # the copy ties with row 5's copies: by row
    if m >= 4:
        assert N + 3 in want[N + 2][:2] and N + 2 in want[N + 3][:2]   # nearest each other
        assert (want[N + 1] == np.arange(kt)).all()                    # the zero row: every distance 1


# ------------------------------------------------------------------ 4: grow_
def small_model(n_users=9, n_items=6):
    import dcnr
    torch.manual_seed(0)
    return dcnr.DCN_RecSys(n_users, n_items, {"a": 5}, 2,
                           dict(emb_dim=4, hidden_dim=8, n_cross_layers=1, n_res_blocks=1, dropout=0.0))


def test_grow_keeps_parameters_and_loads_into_a_fresh_model():
    model = small_model()
    pu, ph = model.user_embedding.weight, model.item_embedding.weight
    u0, h0 = pu.detach().clone(), ph.detach().clone()
    assert model.grow_(n_users=12, n_items=7) == (3, 1)
    assert model.user_embedding.weight is pu and model.item_embedding.weight is ph
    assert tuple(pu.shape) == (12, 4) and tuple(ph.shape) == (7, 4)
    assert model.user_embedding.num_embeddings == 12 and model.item_embedding.num_embeddings == 7
    assert model._dims["n_users"] == 12 and model._dims["n_items"] == 7
    assert model.desc().n_users == 12 and model.desc().n_items == 7 and model._flat is None
    assert torch.equal(pu[:9], u0) and torch.equal(ph[:6], h0)
    assert torch.equal(pu[9:], u0[9 // 2].expand(3, -1)) and torch.equal(ph[6:], h0[0:1])   # the fallback rows
    fresh = small_model(12, 7)
    fresh.load_state_dict(model.state_dict())
    assert torch.equal(fresh.user_embedding.weight, pu)


def test_grow_init_and_errors():
    model = small_model()
    rows = torch.arange(8, dtype=torch.float32).reshape(2, 4)
    model.grow_(n_items=8, init=rows)
    assert torch.equal(model.item_embedding.weight[6:], rows)
    model.grow_(n_users=10, n_items=9, init=(rows[:1] + 1, rows[1:] + 2))
    assert torch.equal(model.user_embedding.weight[9:], rows[:1] + 1)
    assert torch.equal(model.item_embedding.weight[8:], rows[1:] + 2)
    torch.manual_seed(5)
    model.grow_(n_users=13, init="normal")
    torch.manual_seed(5)
    assert torch.equal(model.user_embedding.weight[10:], torch.empty(3, 4).normal_())
    before = model.user_embedding.weight.detach().clone()
    assert model.grow_() == (0, 0) and model.grow_(n_users=13) == (0, 0)
    for bad in (dict(n_users=12), dict(n_items=3), dict(n_users=14, init="zeros"),
                dict(n_users=14, init=rows), dict(n_users=14, n_items=10, init=rows[:1])):
        with pytest.raises(ValueError):
            model.grow_(**bad)
    assert torch.equal(model.user_embedding.weight, before) and model._dims["n_users"] == 13


# -------------------------------------------------------------- 5: the C ABI
def test_new_symbols_declared_exported_and_bound():
    from dcnr import _lib
    txt = open(os.path.join(ROOT, "include", "dcnr.h")).read()
    assert re.search(r"#define DCNR_ABI_VERSION 4\b", txt)
    lib = _lib.load()
    for name in ("dcnr_id_map_insert_workspace_size", "dcnr_id_map_insert"):
        assert re.search(r"\b%s\(" % name, txt), name
        assert name in _lib.exported_symbols() and hasattr(lib, name)


def test_insert_size_query():
    from dcnr import _lib
    lib = _lib.load()
    size = lib.dcnr_id_map_insert_workspace_size
    assert size(-1) == 0 and size((1 << 31) - 1) == 0 and size(1 << 40) == 0
    assert size(0) > 0 and size(1) > 0
    assert size((1 << 31) - 2) >= 12 * ((1 << 31) - 2)
    assert size(1 << 20) >= 12 << 20 and size(1 << 20) > size(1 << 10)


def test_insert_argument_checks_launch_nothing():
    """DCNR_BAD_ARG / DCNR_UNSUPPORTED_SHAPE / DCNR_WORKSPACE_TOO_SMALL come
    before any launch, so they need no device (the pointers are never read)."""
    from dcnr import _lib
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    counts = (ctypes.c_int32 * 2)()
    cp = ctypes.addressof(counts)
    call = lambda table, cap, n, raw, M, out, new, cnt, ws, nb: lib.dcnr_id_map_insert(
        table, cap, n, raw, M, out, new, cnt, None, ws, nb, None)
    ok_args = dict(table=base, cap=16, n=3, raw=base, M=4, out=base, new=base, cnt=cp, ws=base, nb=1 << 20)
    bad = [dict(table=None), dict(table=base + 8), dict(cap=12), dict(cap=2), dict(n=-1), dict(M=-1),
           dict(raw=None), dict(out=None), dict(new=None), dict(cnt=None), dict(ws=None), dict(cap=0)]
    codes = set()
    for change in bad:
        a = dict(ok_args, **change)
        st = call(a["table"], a["cap"], a["n"], a["raw"], a["M"], a["out"], a["new"], a["cnt"], a["ws"], a["nb"])
        assert st != 0, change
        codes.add(st)
    assert len(codes) == 1                                  # DCNR_BAD_ARG, every one
    bad_arg = codes.pop()
    huge = call(base, 16, 3, base, (1 << 31) - 1, base, base, cp, base, 1 << 20)
    small = call(base, 16, 3, base, 4, base, base, cp, base, 8)
    assert len({0, bad_arg, huge, small}) == 4              # two further distinct errors
