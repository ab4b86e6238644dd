"""The item neighbour table updated in place when some embeddings change
(``NearestNeighbors.update_rows``, dcnr_cosine_neighbor_table_update /
dcnr_cosine_neighbor_table_rows, ``RankingPipeline.update_item_embeddings``).

Row r of the table is bit for bit the single-query search for table[r], so the
oracle is exact: after an update the table, the inverse norms and the packed
copy must equal (``torch.equal``) those of a fresh index fitted on the new
embeddings and built from scratch.

  1  equality with the rebuild on the build test's shapes, then a second
     update on top of the first
  2  the work was incremental: the device's counts against the rule restated
     in numpy (neighbor_update_rule.apply_rule, checked on its own in
     test_neighbor_update_cpu.py)
  3  the packed copy and more changed rows than one LDS tile of the filter
  4  edges: nothing changed, rows modified in place, a zero vector, k = N,
     nearly everything changed, bad row sets
  5  a pipeline after update_item_embeddings answers as one built fresh

Shapes (d, k) and what they take: (32, 11), (64, 11), (64, 32) the MFMA filter
(rows rounded on the fly: 5003 rows have no packed copy) and scan v4 for the
re-search; (16, 11), (24, 11) the exact filter and scan v2; (128, 11) the
exact filter and scan v1 by width; (64, 51) scan v1 by k > 32 and a merge of
more than 32 entries.
"""
import numpy as np
import pytest
import torch

import neighbor_update_rule as rule
import test_knn_paths_gpu as kp
import test_recommend_many_gpu as rm

pytestmark = pytest.mark.gpu

SHAPES = [(32, 11), (64, 11), (16, 11), (24, 11), (128, 11), (64, 32), (64, 51)]


def fresh_index(table, k, build=True):
    """An index of its own over a copy of `table` (fit keeps the tensor it is
    given), its neighbour table built."""
    import dcnr
    nn_ = dcnr.NearestNeighbors(n_neighbors=k).fit(table.clone())
    if build:
        nn_.build_neighbor_table()
    return nn_


def assert_equals_rebuild(nn_, new_table, k, what=""):
    """Everything derived from the table, against fit + build on new_table."""
    want = fresh_index(new_table, k)
    assert torch.equal(nn_._table, new_table), what
    assert torch.equal(nn_._inv, want._inv), what
    assert (nn_._packed is None) == (want._packed is None), what
    if want._packed is not None:
        assert torch.equal(nn_._packed, want._packed), what
    bad = (nn_.neighbor_table_ != want.neighbor_table_).any(1).nonzero().flatten().tolist()
    assert not bad, (what, len(bad), bad[:8])
    return want


def holders(old_nbr, rows):
    """Rows outside the changed set whose old list holds a changed row."""
    hold = np.isin(old_nbr, rows).any(1)
    hold[rows] = False
    return int(hold.sum())


_cases = {}


def case(dev, d, k):
    """random_case's 5003-row table (20 copies of row 5, a zero row), an index
    with its table updated for the recipe's changed set, the stats of that
    update and the table as it stood before -- once per shape."""
    if (d, k) not in _cases:
        table, _, ties = kp.random_case(dev, d, 1, k)
        zero = int((table == 0).all(1).nonzero()[0, 0])
        host = table.cpu().numpy()
        counts = (3, 3, 3) if k == 51 else (12, 12, 11)
        rows, vec = rule.changed_set(host, ties, zero, seed=d + k, counts=counts)
        nn_ = fresh_index(table, k)
        nbr = nn_.neighbor_table_
        old_nbr = nbr.cpu().numpy()
        stats = nn_.update_rows(rows, vec, return_stats=True)
        assert nn_.neighbor_table_ is nbr                      # in place
        new_table = table.clone()
        new_table[torch.from_numpy(rows).to(dev)] = torch.from_numpy(vec).to(dev)
        _cases[(d, k)] = dict(table=table, host=host, ties=ties, zero=zero, rows=rows, vec=vec, nn=nn_,
                              old_nbr=old_nbr, stats=stats, new_table=new_table, counts=counts)
    return _cases[(d, k)]


# --------------------------------------------------- 1: equality with the rebuild
@pytest.mark.parametrize("d,k", SHAPES)
def test_update_equals_rebuild(dev, d, k):
    c = case(dev, d, k)
    assert c["rows"].size == (11 if k == 51 else 37)
    assert not c["stats"]["rebuilt"]
    assert_equals_rebuild(c["nn"], c["new_table"], k, "first update")
    # other rows on top of the first (a copy of the index: the shared case stays as it is)
    nn2 = fresh_index(c["new_table"], k, build=False)
    nn2.neighbor_table_ = c["nn"].neighbor_table_.clone()
    rows2, vec2 = rule.changed_set(c["new_table"].cpu().numpy(), c["ties"], c["zero"], seed=1000 + d + k,
                                   counts=c["counts"], exclude=c["rows"])
    assert not np.intersect1d(rows2, c["rows"]).size
    stats2 = nn2.update_rows(torch.from_numpy(rows2), torch.from_numpy(vec2).to(dev), return_stats=True)
    assert not stats2["rebuilt"] and stats2["merged"] > 0
    newer = c["new_table"].clone()
    newer[torch.from_numpy(rows2).to(dev)] = torch.from_numpy(vec2).to(dev)
    assert_equals_rebuild(nn2, newer, k, "second update")


# ------------------------------------------------------ 2: the work was incremental
@pytest.mark.parametrize("d,k", SHAPES)
def test_update_was_incremental(dev, d, k):
    c = case(dev, d, k)
    rows, m = c["rows"], c["rows"].size
    # the rule on the host, from the table as it stood and the new distances (numpy's, not the
    # kernels' bits: an oracle for the branches and the counts, not for the lists)
    _, br = rule.apply_rule(c["old_nbr"], rule.distances(c["new_table"].cpu().numpy()), rows)
    n = {name: int(v.sum()) for name, v in br.items()}
    hold = holders(c["old_nbr"], rows)
    print(f"d={d} k={k}: rule {n}, holders {hold}, device {c['stats']}")
    assert n["merged_hole"] > 0 and n["hole"] > 0 and n["untouched"] > 0 and n["gained"] > 0
    assert n["hole"] + n["emptied"] <= hold
    s = c["stats"]
    assert s["changed"] == m and s["merged"] > 0
    assert m < s["researched"] <= m + hold
    assert s["researched"] + s["merged"] == m + s["affected"]
    # (expected: the holders, the rows gaining a changed row, and a few per cent of V4_EPS margin)
    assert hold <= s["affected"] < 5003 // 2
    # the filter marks a superset of the rows the rule touches, and not much more
    assert s["affected"] >= n["gained"] + n["merged_hole"] + n["hole"] + n["emptied"]


# ------------------------------------------------------- 3: packed copy and tiling
def test_update_with_packed_rows_and_two_filter_tiles(dev):
    """N = 40003 (above PACKED_MIN_ROWS: the filter reads the bf16 copy; not
    a multiple of 16) x 32, k = 11, m = 300 changed rows: past the filter's
    LDS tile of 256."""
    N, d, k = 40003, 32, 11
    host, ties, zero = rule.planted_table(N, d, seed=41)
    rows, vec = rule.changed_set(host, ties, zero, seed=42, counts=(100, 100, 98))
    assert rows.size == 300
    # the last row of the table and a row of the last, partial, 16-row tile among them
    rows[0], rows[1] = N - 1, N - 3
    assert np.unique(rows).size == 300
    table = torch.from_numpy(host).to(dev)
    nn_ = fresh_index(table, k)
    assert nn_._packed is not None
    old_nbr = nn_.neighbor_table_.cpu().numpy()
    stats = nn_.update_rows(rows, vec, return_stats=True)
    new_table = table.clone()
    new_table[torch.from_numpy(rows).to(dev)] = torch.from_numpy(vec).to(dev)
    assert_equals_rebuild(nn_, new_table, k)
    hold = holders(old_nbr, rows)
    print(f"N={N}: holders {hold}, device {stats}")
    assert not stats["rebuilt"] and stats["merged"] > 0
    assert 300 < stats["researched"] <= 300 + hold


# -------------------------------------------------------------------- 4: edges
def test_edges(dev):
    d, k = 32, 11
    c = case(dev, d, k)
    nn_ = fresh_index(c["table"], k)
    before = nn_.neighbor_table_.clone()
    # nothing changed
    assert nn_.update_rows([]) is None
    assert nn_.update_rows(np.zeros(0, np.int64), np.zeros((0, d), np.float32),
                           return_stats=True)["changed"] == 0
    # bad row sets: ValueError, nothing changed
    for bad in ([3, 9, 3], [5003], [-1, 4], [1.5]):
        with pytest.raises(ValueError):
            nn_.update_rows(bad, np.ones((len(bad), d), np.float32))
    with pytest.raises(ValueError):
        nn_.update_rows([3, 9], np.ones((3, d), np.float32))
    assert torch.equal(nn_._table, c["table"]) and torch.equal(nn_.neighbor_table_, before)
    # rows of the fitted table modified in place, then vectors=None; one of them a zero vector
    rows = torch.tensor([4000, 17, 2500], device=dev)
    new_table = c["table"].clone()
    new_table[rows] = torch.randn(3, d, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    new_table[2500] = 0.0
    nn_._table[rows] = new_table[rows]
    stats = nn_.update_rows(rows, return_stats=True)
    assert stats["changed"] == 3 and not stats["rebuilt"]
    assert_equals_rebuild(nn_, new_table, k, "in place")
    assert nn_.neighbor_table_[2500].tolist() == list(range(k))
    # a table of its own (wider than n_neighbors), the index's kept table left alone
    wide = fresh_index(new_table, k, build=False)
    t16 = wide.build_neighbor_table(16, rows=(0, 5003))
    wide.neighbor_table_ = None
    newer = new_table.clone()
    newer[100] = new_table[200] * 0.5
    wide.update_rows([100], newer[100:101], table=t16)
    assert wide.neighbor_table_ is None
    assert torch.equal(t16, fresh_index(newer, k, build=False).build_neighbor_table(16))
    # no table at all: the norms are refreshed, the search sees the new row
    bare = fresh_index(new_table, k, build=False)
    bare.update_rows([100], newer[100:101])
    assert torch.equal(bare._inv, fresh_index(newer, k, build=False)._inv)


def test_every_list_holds_every_row(dev):
    """N = 40, k = 40: every row is in every list; forced through the
    incremental path and through the rule's own choice (the rebuild)."""
    N, d, k = 40, 24, 40
    g = torch.Generator(device=dev).manual_seed(40)
    table = torch.randn(N, d, device=dev, generator=g)
    new_table = table.clone()
    new_table[[7, 31]] = torch.randn(2, d, device=dev, generator=g)
    for force in (False, None):
        nn_ = fresh_index(table, k)
        stats = nn_.update_rows([31, 7], new_table[[31, 7]], return_stats=True, rebuild=force)
        assert stats["rebuilt"] == (force is None)
        if force is False:
            assert stats["affected"] == N - 2 and stats["merged"] + stats["researched"] == N
        assert_equals_rebuild(nn_, new_table, k, f"rebuild={force}")


def test_widest_table_merges_more_than_a_wave(dev):
    """kt = 64, the widest table: a row that keeps its 64 entries and gains a
    changed row has more than 64 merge candidates -- the workgroup's sort, not
    the wave's."""
    d, k = 32, 64
    table, _, ties = kp.random_case(dev, d, 1, k)
    zero = int((table == 0).all(1).nonzero()[0, 0])
    rows, vec = rule.changed_set(table.cpu().numpy(), ties, zero, seed=d + k)
    nn_ = fresh_index(table, k)
    old_nbr = nn_.neighbor_table_.cpu().numpy()
    stats = nn_.update_rows(rows, vec, return_stats=True, rebuild=False)
    new_table = table.clone()
    new_table[torch.from_numpy(rows).to(dev)] = torch.from_numpy(vec).to(dev)
    assert_equals_rebuild(nn_, new_table, k)
    hold = holders(old_nbr, rows)
    # every affected row that holds no changed row was merged, with 64 + at least one candidates
    assert stats["merged"] >= stats["affected"] - hold > 0
    assert stats["researched"] <= rows.size + hold


def test_nearly_everything_changed_takes_the_rebuild(dev):
    N, d, k = 300, 32, 11
    g = torch.Generator(device=dev).manual_seed(300)
    table = torch.randn(N, d, device=dev, generator=g)
    rows = np.setdiff1d(np.arange(N), [11, 250])
    new_table = table.clone()
    new_table[torch.from_numpy(rows).to(dev)] = torch.randn(rows.size, d, device=dev, generator=g)
    nn_ = fresh_index(table, k)
    stats = nn_.update_rows(rows, new_table[torch.from_numpy(rows).to(dev)], return_stats=True)
    assert stats["rebuilt"] and stats["changed"] == 298
    assert_equals_rebuild(nn_, new_table, k)


# ------------------------------------------------------------------ 5: pipeline
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_pipeline_after_update_answers_as_a_fresh_one(dev, precision):
    import dcnr
    base = rm.get_pipe(dev, precision)                       # (its item tables; its model is left alone)
    model = rm.our_model(rm.CFG, precision=precision, seed=9).to(dev).eval()
    pipe = dcnr.RankingPipeline(model, base.item_cat, base.item_num, neighbor_table=True)
    # the index shares the model's table: the hazard update_item_embeddings exists for
    assert pipe.index._table.data_ptr() == model.item_embedding.weight.data_ptr()
    g = torch.Generator(device=dev).manual_seed(12)
    rows = np.random.default_rng(12).choice(rm.N_ITEMS, 40, replace=False)
    old = model.item_embedding.weight.detach().clone()
    vec = old[torch.from_numpy(rows).to(dev)] * 0.5 + 0.3 * torch.randn(40, old.shape[1], device=dev, generator=g)
    nbr = pipe._nbr
    stats = pipe.update_item_embeddings(rows, vec, return_stats=True)
    assert pipe._nbr is nbr and stats["changed"] == 40 and not stats["rebuilt"]
    new = old.clone()
    new[torch.from_numpy(rows).to(dev)] = vec
    assert torch.equal(model.item_embedding.weight.detach(), new)
    other = rm.our_model(rm.CFG, precision=precision, seed=9).to(dev).eval()
    with torch.no_grad():
        other.item_embedding.weight.copy_(new)
    fresh = dcnr.RankingPipeline(other, base.item_cat, base.item_num, neighbor_table=True)
    assert torch.equal(pipe._nbr, fresh._nbr)
    reqs, _, _ = rm.mixed_requests(24, seed=6)
    for q in reqs[:6]:
        q["pos"] = (q["pos"] + rows[:4].tolist())[:32] if q["pos"] else q["pos"]
    want = rm.run_many(fresh, reqs)
    assert sum(w[0].numel() > 0 for w in want) > 10
    rm.assert_same(rm.run_many(pipe, reqs), want, precision)
    some = rows[:5].tolist() + [0, rm.N_ITEMS - 1]
    assert torch.equal(pipe.similar_items_many(some, 10), fresh.similar_items_many(some, 10))
    # an index with a table of its own (item_embeddings given): the model's rows are written as well
    model2 = rm.our_model(rm.CFG, precision=precision, seed=9).to(dev).eval()
    pipe2 = dcnr.RankingPipeline(model2, base.item_cat, base.item_num, item_embeddings=old.clone(),
                                 neighbor_table=True)
    assert pipe2.index._table.data_ptr() != model2.item_embedding.weight.data_ptr()
    pipe2.update_item_embeddings(rows, vec)
    assert torch.equal(model2.item_embedding.weight.detach(), new)
    assert torch.equal(pipe2._nbr, fresh._nbr)
    rm.assert_same(rm.run_many(pipe2, reqs), want, precision + " own table")
