"""Admitting new users and hotels on the device: ``IdMap.insert``
(dcnr_id_map_insert), ``Preprocessor.transform(unknown="admit")``,
``DCN_RecSys.grow_``, ``FusedTrainer.grow``, ``NearestNeighbors.append_rows``
and ``RankingPipeline.append_items``.  Every comparison is exact.

  1  ``IdMap.insert`` against ``insert_host`` (itself against a dict in
     test_admit_cpu.py): batch sizes around the scan's tile of 1024 and its
     second level (tile 1025), one id 4096 times, nearly full tables whose
     chains wrap, ids equal in their low 32 bits, inserts in a row, two runs,
     the reserved id
  2  ``transform(unknown="admit")`` against ``transform_host``
  3  admission preserves scores, bit for bit
  4  a trainer that grows equals one born with the full tables, bit for bit
  5  ``append_rows`` equals ``fit`` + ``build_neighbor_table`` on the grown table
  6  end to end: the grown pipeline answers as one built fresh
"""
import numpy as np
import pytest
import torch

import admit_common as ac
import neighbor_update_rule as rule
import prepare_common as pc
import transform_common as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def bits(t):
    """A float tensor as integers of its width: equality bit for bit."""
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def twins(dev, ids, capacity=None):
    import dcnr
    return dcnr.IdMap(ids, device=dev, capacity=capacity), dcnr.IdMap(ids, device="cpu")


def assert_insert_matches(dm, hm, raw, capacity=None, what=""):
    n = len(dm)
    out, new = dm.insert(raw, capacity=capacity)
    want_out, want_new = hm.insert_host(raw)
    assert out.device.type == "cuda" and out.dtype == torch.int64 and new.dtype == torch.int64
    assert np.array_equal(out.cpu().numpy(), want_out), what
    assert np.array_equal(new.cpu().numpy(), want_new), what
    assert len(dm) == len(hm) == n + want_new.size
    assert np.array_equal(dm.ids.cpu().numpy(), hm.ids.numpy()), what
    assert dm.capacity > len(dm)
    return out, new


def assert_finds_everything(dm):
    got = dm.lookup(dm.ids)
    assert torch.equal(got, torch.arange(len(dm), device=got.device)), "lookup over every id ever inserted"
    assert np.array_equal(dm.lookup_host(dm.ids), np.arange(len(dm)))


# ---------------------------------------------------------------- 1: IdMap.insert
@pytest.mark.parametrize("M", [1, 1023, 1024, 1025, 4097, (1 << 20) + 1025])
def test_insert_against_insert_host(dev, M):
    rng = np.random.default_rng(M)
    ids = tc.wide_ids(rng, 1000)
    dm, hm = twins(dev, ids)
    raw = ac.mixed_batch(rng, ids, M, n_new=max(1, M // 3))     # known and new ids interleaved
    if M >= 1025:
        raw[-1] = (1 << 60) + 5                                  # a first appearance in the last tile
    _, new = assert_insert_matches(dm, hm, raw, what=f"M={M}")
    assert new.numel() >= 1 and dm.capacity >= 2 * (1000 + M)
    assert_finds_everything(dm)
    absent = torch.tensor([(1 << 61) + 1, tc.RESERVED], device=dev)
    assert dm.lookup(absent).tolist() == [-1, -1]


def test_insert_one_new_id_many_times(dev):
    ids = np.arange(50, dtype=np.int64) * 7
    dm, hm = twins(dev, ids)
    out, new = assert_insert_matches(dm, hm, np.full(4096, 12345678901, dtype=np.int64))
    assert new.tolist() == [12345678901] and (out == 50).all()
    assert_finds_everything(dm)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("cap", [8, 16])
def test_insert_into_a_nearly_full_table(dev, cap, seed):
    """n + distinct new = capacity - 1: one free slot is left, chains wrap."""
    rng = np.random.default_rng(100 * cap + seed)
    n = 3
    every = tc.wide_ids(rng, cap - 1, multiples=bool(seed % 2))
    ids, fresh = every[:n], every[n:]
    dm, hm = twins(dev, ids, capacity=cap)
    raw = np.concatenate([fresh, rng.choice(fresh, 9), rng.choice(ids, 5)])
    rng.shuffle(raw)
    assert_insert_matches(dm, hm, raw, capacity=cap, what=f"cap={cap} seed={seed}")
    assert dm.capacity == cap and len(dm) == cap - 1
    assert_finds_everything(dm)
    assert dm.lookup(every + 1).tolist() == [-1] * (cap - 1)     # absent ids: the probe ends at the free slot


def test_insert_ids_equal_in_their_low_32_bits(dev):
    rng = np.random.default_rng(5)
    ids = (np.arange(1, 301, dtype=np.int64) << 32) + 77
    dm, hm = twins(dev, ids)
    raw = ac.mixed_batch(rng, ids, 3000, n_new=700, low32=True)
    assert (raw & 0xFFFFFFFF == raw[0] & 0xFFFFFFFF).sum() >= 1500
    assert_insert_matches(dm, hm, raw)
    assert_finds_everything(dm)


def test_two_inserts_in_a_row_and_growth(dev):
    rng = np.random.default_rng(9)
    ids = tc.wide_ids(rng, 10)
    dm, hm = twins(dev, ids)
    assert dm.capacity == 32
    first = ac.mixed_batch(rng, ids, 500, n_new=200)
    assert_insert_matches(dm, hm, first, what="first")
    assert dm.capacity >= 2 * (10 + 500)                         # a larger table was built from ids first
    second = np.concatenate([first[::3], ac.mixed_batch(rng, dm.ids.cpu().numpy(), 2000, n_new=900)])
    assert_insert_matches(dm, hm, second, what="second")
    assert_finds_everything(dm)
    out, new = dm.insert(np.zeros(0, np.int64))                  # an empty batch
    assert out.numel() == 0 and new.numel() == 0
    out, new = dm.insert(torch.from_numpy(second).to(dev))       # a device tensor; everything known now
    assert new.numel() == 0 and np.array_equal(out.cpu().numpy(), hm.lookup_host(second))


def test_insert_is_the_same_on_every_run(dev):
    rng = np.random.default_rng(11)
    ids = tc.wide_ids(rng, 2000)
    raw = ac.mixed_batch(rng, ids, 50000, n_new=9000)
    runs = []
    for _ in range(2):
        dm, _ = twins(dev, ids)
        out, new = dm.insert(raw)
        runs.append((out.clone(), new.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_insert_reserved_id_changes_nothing(dev):
    rng = np.random.default_rng(13)
    ids = tc.wide_ids(rng, 100)
    dm, hm = twins(dev, ids)
    raw = ac.mixed_batch(rng, ids, 300, n_new=100)
    probe = np.concatenate([ids, raw])
    before = dm.lookup(probe).clone()
    bad = raw.copy()
    bad[-1] = tc.RESERVED                                        # found in the last row, after 299 good ones
    with pytest.raises(ValueError):
        dm.insert(bad, capacity=dm.capacity)
    assert len(dm) == 100 and torch.equal(dm.lookup(probe), before)
    assert (before[100:] < 0).any()
    assert_insert_matches(dm, hm, raw, what="after the refused call")
    assert_finds_everything(dm)


# --------------------------------------------------- 2: transform(unknown="admit")
# seed: (M, M2, users, hotels).  The first three are test_transform_gpu.py's frames (few new ids, missing
# and unseen categories among S's rows); the last one's S brings about a hundred new users and two hundred hotels
CASES = {31: (3000, 3000, 1500, 600), 33: (257, 257, 128, 51), 36: (24, 500, 12, 4), 61: (1500, 600, 1050, 1500)}


def fit_pair(dev, seed):
    import dcnr
    M, M2, n_users, n_items = CASES[seed]
    whole = pc.random_case(seed, M + M2, n_users=n_users, n_items=n_items)
    fit_case = dict(whole, **dict(zip(ac.FIVE, tc.part(whole, 0, M))))
    return (whole, pc.call(dcnr.prepare_data, fit_case, device=dev).preprocessor(),
            pc.call(dcnr.prepare_data_host, fit_case).preprocessor())


@pytest.mark.parametrize("use_filter", [False, True])
@pytest.mark.parametrize("seed", sorted(CASES))
def test_transform_admit_against_transform_host(dev, seed, use_filter):
    whole, pre_dev, pre_host = fit_pair(dev, seed)
    M, M2 = CASES[seed][:2]
    new = tc.part(whole, M, M + M2)
    n_u, n_h = len(pre_host.user_ids), len(pre_host.item_ids)
    kw = dict(fill_nan=True, noise_filter="fitted" if use_filter else None)
    want = pre_host.transform_host(*new, unknown="admit", **kw)
    got = pre_dev.transform(*new, unknown="admit", device=dev, **kw)
    tc.assert_same_transformed(got, want, f"seed {seed} {kw}")
    assert want.new_user_ids.size > 0 or use_filter
    if seed == 61 and not use_filter:
        assert want.new_user_ids.size > 100 and want.new_item_ids.size > 100
    assert np.array_equal(got.new_user_ids, want.new_user_ids)
    assert np.array_equal(got.new_item_ids, want.new_item_ids)
    assert np.array_equal(pc.to_np(pre_dev.user_ids), pc.to_np(pre_host.user_ids))
    assert np.array_equal(pc.to_np(pre_dev.item_ids), pc.to_np(pre_host.item_ids))
    assert len(pre_dev.user_ids) == n_u + want.new_user_ids.size
    collab = got.collab.cpu().numpy()
    assert np.array_equal((got.unknown_bits.cpu().numpy() & 1) != 0, collab[:, 0] >= n_u)
    assert np.array_equal((got.unknown_bits.cpu().numpy() & 2) != 0, collab[:, 1] >= n_h)
    # the same rows afterwards: no unknown user or hotel, the same codes
    again = pre_dev.transform(*new, unknown="reference", device=dev, **kw)
    assert again.n_unknown_users == 0 and again.n_unknown_items == 0
    assert torch.equal(again.collab, got.collab) and again.n_unknown_cat == got.n_unknown_cat
    # every device state and the host state follow an admit()
    pre_dev.transform_host(*tc.part(whole, 0, 5))                # (the host state now exists)
    late = np.array([(1 << 58) + 3, (1 << 58) + 1, (1 << 58) + 3])
    new_u, new_h = pre_dev.admit(users=late, items=late[:1])
    assert new_u.tolist() == [(1 << 58) + 3, (1 << 58) + 1] and new_h.tolist() == [(1 << 58) + 3]
    st = next(iter(pre_dev._state.values()))
    assert st["users"].lookup(late).tolist() == [n_u + want.new_user_ids.size + k for k in (0, 1, 0)]
    assert pre_dev._host_fit()[0].lookup_host(late).tolist() == st["users"].lookup(late).tolist()
    assert pc.to_np(pre_dev.item_ids)[-1] == (1 << 58) + 3


# ------------------------------------------------- 3: admission preserves scores
PARAMS = dict(emb_dim=8, hidden_dim=64, n_cross_layers=2, n_res_blocks=2, dropout=0.0)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_admission_preserves_scores(dev, precision):
    import dcnr
    whole, pre, _ = fit_pair(dev, 33)
    M, M2 = CASES[33][:2]
    new = tc.part(whole, M, M + M2)
    n_u, n_h = len(pre.user_ids), len(pre.item_ids)
    cat_dims = {name: int(len(k)) for name, k in zip(pre.cat_names, pre.cat_keys)}
    torch.manual_seed(3)
    model = dcnr.DCN_RecSys(n_u, n_h, cat_dims, pre.n_num, PARAMS, precision=precision).to(dev).eval()
    before = pre.transform(*new, unknown="reference", device=dev)
    assert before.n_unknown_users > 0 and before.n_unknown_items > 0
    with torch.no_grad():
        z0 = model(before.collab[:, 0], before.collab[:, 1], before.cat, before.num).clone()
    after = pre.transform(*new, unknown="admit", device=dev)
    assert int(after.collab[:, 0].max()) >= n_u and int(after.collab[:, 1].max()) >= n_h
    # before the model grows the new indices are out of range
    with torch.no_grad(), pytest.raises(IndexError):
        model(after.collab[:, 0], after.collab[:, 1], after.cat, after.num)
        model.check_index_errors()
    model.grow_(n_users=len(pre.user_ids), n_items=len(pre.item_ids), init="fallback")
    with torch.no_grad():
        z1 = model(after.collab[:, 0], after.collab[:, 1], after.cat, after.num)
        model.check_index_errors()
    assert z0.shape == z1.shape and z0.numel() > 100
    assert torch.equal(bits(z0), bits(z1))


# --------------------------------------------------------- 4: the trainer grows
N_U0, N_H0, N_U1, N_H1 = 150, 90, 197, 131
CAT_DIMS = {"a": 12, "b": 40}
N_NUM = 5


def trainer_batches(dev, seed):
    """Six batches of 64: three with ids below the old counts, three that use the new ids."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for s in range(6):
        hi_u, hi_h = (N_U0, N_H0) if s < 3 else (N_U1, N_H1)
        u, h = torch.randint(0, hi_u, (64,), generator=g), torch.randint(0, hi_h, (64,), generator=g)
        if s >= 3:
            u[:20] = torch.randint(N_U0, N_U1, (20,), generator=g)
            h[10:30] = torch.randint(N_H0, N_H1, (20,), generator=g)
        c = torch.stack([torch.randint(0, n, (64,), generator=g) for n in CAT_DIMS.values()], 1)
        x = torch.rand((64, N_NUM), generator=g)
        y = (torch.rand(64, generator=g) < 0.5).float()
        out.append(tuple(t.to(dev) for t in (u, h, c, x, y)))
    return out


@pytest.mark.parametrize("dense_table_grads", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_grown_trainer_equals_one_born_with_the_full_tables(dev, precision, dense_table_grads):
    import dcnr
    torch.manual_seed(17)
    big = dcnr.DCN_RecSys(N_U1, N_H1, CAT_DIMS, N_NUM, PARAMS, precision=precision).to(dev)
    small = dcnr.DCN_RecSys(N_U0, N_H0, CAT_DIMS, N_NUM, PARAMS, precision=precision).to(dev)
    sd = {k: v.detach().clone() for k, v in big.state_dict().items()}
    init = (sd["user_embedding.weight"][N_U0:].clone(), sd["item_embedding.weight"][N_H0:].clone())
    sd["user_embedding.weight"] = sd["user_embedding.weight"][:N_U0].clone()
    sd["item_embedding.weight"] = sd["item_embedding.weight"][:N_H0].clone()
    small.load_state_dict(sd)
    kw = dict(lr=1e-2, weight_decay=0.0, optimizer_name="AdamW", dense_table_grads=dense_table_grads)
    a, b = dcnr.FusedTrainer(big, **kw), dcnr.FusedTrainer(small, **kw)
    params_b = list(small.parameters())
    batches = trainer_batches(dev, 23)
    losses = {0: [], 1: []}
    for s, batch in enumerate(batches):
        if s == 3:
            assert b.grow(n_users=N_U1, n_items=N_H1, init=init) == (N_U1 - N_U0, N_H1 - N_H0)
            assert b.step_count == 3 and b._ws is None and b.flat.numel() == a.flat.numel()
            assert small.flat_offsets == big.flat_offsets and small.flat_emb_end == big.flat_emb_end
        for k, tr in enumerate((a, b)):
            losses[k].append(tr.step(*batch).clone())
    a.check_indices()
    b.check_indices()
    for la, lb in zip(losses[0], losses[1]):
        assert torch.equal(bits(la.reshape(1)), bits(lb.reshape(1)))
    assert all(p is q for p, q in zip(params_b, small.parameters()))       # the same Parameter objects
    names = [n for n, _ in big.named_parameters()]
    for name, off, pa, pb in zip(names, big.flat_offsets, big.param_tensors(), small.param_tensors()):
        n = pa.numel()
        assert pa.shape == pb.shape and torch.equal(bits(pa.detach()), bits(pb.detach())), name
        assert pb.data_ptr() == b.flat.data_ptr() + 4 * off                 # flat again
        for what in ("m", "v"):
            ma, mb = getattr(a, what)[off:off + n], getattr(b, what)[off:off + n]
            assert torch.equal(bits(ma), bits(mb)), (name, what)
    assert torch.equal(bits(a.m), bits(b.m)) and torch.equal(bits(a.v), bits(b.v))
    for (ka, va), (kb, vb) in zip(big.state_dict().items(), small.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka                         # the BN buffers too
    # rows no batch touched: no moments in either
    touched = torch.cat([bt[0] for bt in batches]).unique()
    idle = torch.ones(N_U1, dtype=torch.bool, device=dev)
    idle[touched] = False
    assert idle[N_U0:].any()
    d = PARAMS["emb_dim"]
    m_users = b.m[small.flat_offsets[0]:small.flat_offsets[0] + N_U1 * d].view(N_U1, d)
    assert not m_users[idle].any() and m_users[~idle].any()
    new_idle = idle[N_U0:]
    assert torch.equal(small.user_embedding.weight.detach()[N_U0:][new_idle], init[0][new_idle])


def test_grow_raises_for_a_smaller_count(dev):
    import dcnr
    torch.manual_seed(1)
    model = dcnr.DCN_RecSys(20, 10, {"a": 3}, 2, PARAMS).to(dev)
    tr = dcnr.FusedTrainer(model)
    with pytest.raises(ValueError):
        tr.grow(n_users=19)
    assert tr.grow(n_users=20) == (0, 0) and model._flat is not None


# ------------------------------------------------------------- 5: append_rows
def fresh_index(table, k):
    import dcnr
    nn_ = dcnr.NearestNeighbors(n_neighbors=k).fit(table.clone())
    nn_.build_neighbor_table()
    return nn_


def assert_equals_fresh(nn_, grown, k, what=""):
    want = fresh_index(grown, k)
    assert torch.equal(nn_._table, grown), what
    assert nn_._inv.shape == want._inv.shape and torch.equal(nn_._inv.view(torch.int32), want._inv.view(torch.int32))
    assert (nn_._packed is None) == (want._packed is None), what
    if want._packed is not None:
        assert torch.equal(nn_._packed, want._packed), what
    assert nn_.neighbor_table_.dtype == torch.int32 and nn_.neighbor_table_.shape == want.neighbor_table_.shape
    bad = (nn_.neighbor_table_ != want.neighbor_table_).any(1).nonzero().flatten().tolist()
    assert not bad, (what, len(bad), bad[:8])
    assert nn_.n_samples_fit_ == grown.shape[0]
    return want


def append_both_ways(dev, table, new, k, what, **kw):
    """The ``vectors=`` and the ``storage=`` form; returns the grown table and the last index."""
    grown = torch.cat([table, new])
    for form in ("vectors", "storage"):
        nn_ = fresh_index(table, k)
        if form == "vectors":
            out, stats = nn_.append_rows(vectors=new, return_stats=True, **kw)
        else:
            storage = grown.clone()
            out, stats = nn_.append_rows(storage=storage, return_stats=True, **kw)
            assert nn_._table.data_ptr() == storage.data_ptr()             # adopted without a copy
        assert out is nn_.neighbor_table_ and stats["changed"] == new.shape[0]
        assert_equals_fresh(nn_, grown, k, f"{what} {form}")
    return grown, nn_, stats


@pytest.mark.parametrize("m", [1, 7, 64])
def test_append_rows_small_table_and_brute_force(dev, m):
    host, _, _ = rule.planted_table(300, 16, seed=3)
    new = ac.appended_rows(host, m, seed=100 + m)
    grown, nn_, stats = append_both_ways(dev, torch.from_numpy(host).to(dev), torch.from_numpy(new).to(dev), 11,
                                         f"m={m}", rebuild=False)
    assert not stats["rebuilt"] and stats["researched"] >= m
    want = rule.brute_table(ac.grown_distances(host, new), 11)
    got = nn_.neighbor_table_.cpu().numpy().astype(np.int64)
    differ = np.flatnonzero((got != want).any(1))
    print("rows that differ from numpy's brute force:", differ.tolist(), got[differ].tolist(), want[differ].tolist())
    assert np.array_equal(got, want)


@pytest.mark.parametrize("m", [1, 64])
def test_append_rows_4099_by_64(dev, m):
    g = torch.Generator(device="cpu").manual_seed(40 + m)
    table = torch.randn(4099, 64, generator=g)
    table[torch.randperm(4099, generator=g)[:20]] = table[5].clone()
    new = torch.randn(m, 64, generator=g)
    new[0] = table[5]
    if m > 3:
        new[1] = 0.0
        new[3] = new[2] * 3 + 0.01 * new[3]
    grown, nn_, stats = append_both_ways(dev, table.to(dev), new.to(dev), 11, f"m={m}")
    assert not stats["rebuilt"]
    # a second append on top of the first, onto a table handed in by the caller
    more = torch.randn(5, 64, generator=g).to(dev)
    own = nn_.neighbor_table_.clone()
    out = nn_.append_rows(vectors=more, table=own)
    assert out.shape[0] == grown.shape[0] + 5 and nn_.neighbor_table_ is None   # (it was not the table grown)
    assert torch.equal(out, fresh_index(torch.cat([grown, more]), 11).neighbor_table_)


def test_append_rows_more_than_one_native_call(dev):
    import dcnr.knn as knn
    m = knn.UPDATE_MAX_ROWS + 1
    g = torch.Generator(device="cpu").manual_seed(77)
    table, new = torch.randn(3000, 16, generator=g).to(dev), torch.randn(m, 16, generator=g).to(dev)
    nn_ = fresh_index(table, 11)
    _, stats = nn_.append_rows(vectors=new, return_stats=True, rebuild=False)
    assert not stats["rebuilt"] and stats["researched"] >= m
    assert_equals_fresh(nn_, torch.cat([table, new]), 11, "two native calls")
    nn_ = fresh_index(table, 11)
    _, stats = nn_.append_rows(vectors=new, return_stats=True)              # the rule's own choice
    assert stats["rebuilt"] == knn.rebuild_is_cheaper(m, 11, 3000 + m)
    assert_equals_fresh(nn_, torch.cat([table, new]), 11, "the rule's choice")


@pytest.mark.parametrize("N", [32760, 33001])
def test_append_rows_keeps_the_packed_copy(dev, N):
    """d = 32 around PACKED_MIN_ROWS: a table that grows past it gets the packed
    copy a fit would make; one that has it grows it."""
    g = torch.Generator(device="cpu").manual_seed(N)
    table, new = torch.randn(N, 32, generator=g).to(dev), torch.randn(40, 32, generator=g).to(dev)
    nn_ = fresh_index(table, 11)
    assert (nn_._packed is None) == (N == 32760)
    nn_.append_rows(vectors=new)
    want = assert_equals_fresh(nn_, torch.cat([table, new]), 11, f"N={N}")
    assert want._packed is not None


def test_append_rows_arguments(dev):
    table = torch.randn(50, 16, device=dev)
    nn_ = fresh_index(table, 5)
    for bad in (dict(), dict(vectors=table[:2], storage=table), dict(storage=table[:40]),
                dict(storage=torch.randn(60, 8, device=dev)), dict(storage=torch.randn(60, 16)),
                dict(vectors=table[:2], table=torch.zeros((49, 5), dtype=torch.int32, device=dev))):
        with pytest.raises(ValueError):
            nn_.append_rows(**bad)
    assert nn_._table.shape[0] == 50 and nn_.neighbor_table_.shape[0] == 50
    out = nn_.append_rows(vectors=torch.zeros((0, 16), device=dev))
    assert out is nn_.neighbor_table_ and out.shape[0] == 50


# ---------------------------------------------------------------- 6: end to end
def test_end_to_end_admission(dev):
    """Fit on P; S arrives: transform(admit), trainer.grow, two steps,
    append_items with the ItemFeatures rebuilt for the new count -- and the
    pipeline answers as one built fresh on the same model and features."""
    import dcnr
    M, M2 = 1500, 600
    whole, fit_case = ac.split_case(61, M, M2, use_filter=False, n_items=1500)
    prep = pc.call(dcnr.prepare_data, fit_case, device=dev)
    pre = prep.preprocessor()
    n_u, n_h = len(pre.user_ids), len(pre.item_ids)
    cat_dims = {name: int(len(k)) for name, k in zip(pre.cat_names, pre.cat_keys)}
    params = dict(emb_dim=32, hidden_dim=64, n_cross_layers=2, n_res_blocks=2, dropout=0.0)
    torch.manual_seed(5)
    model = dcnr.DCN_RecSys(n_u, n_h, cat_dims, pre.n_num, params).to(dev)
    trainer = dcnr.FusedTrainer(model, lr=1e-2, weight_decay=0.0)
    full = prep.full
    trainer.step(full[0][:256, 0], full[0][:256, 1], full[1][:256], full[2][:256], full[3][:256])

    def features(rows_item, rows_cat, rows_raw, n_items):
        """ItemFeatures of main_df's rows so far (raw numeric columns; the fit's scaler)."""
        return dcnr.ItemFeatures(rows_item, rows_cat, rows_raw, pre.scale_, pre.min_, n_items=n_items)

    # main_df so far, in the fit's codes: P's kept rows
    p_rows = pc.to_np(prep.rows).astype(np.int64)
    p_item, p_cat = pc.to_np(full[0])[:, 1], pc.to_np(full[1])
    raw_all = np.nan_to_num(np.column_stack([whole["num"]] + [np.ones(len(whole["user"]))] * len(pre.derived)))
    pipe = dcnr.RankingPipeline(model, item_features=features(p_item, p_cat, raw_all[p_rows], n_h),
                                neighbor_table=True)
    store = dcnr.InteractionStore(pc.to_np(full[0])[:, 0], p_item, raw_all[p_rows, 0], [0], [1],
                                  n_items=n_h, n_reviewers=n_u)
    assert pipe.n_items == n_h and store.n_items == n_h

    # S arrives
    t = pre.transform(*tc.part(whole, M, M + M2), unknown="admit", device=dev)
    assert t.new_user_ids.size > 20 and t.new_item_ids.size > 20
    n_u1, n_h1 = len(pre.user_ids), len(pre.item_ids)
    assert trainer.grow(n_users=n_u1, n_items=n_h1) == (n_u1 - n_u, n_h1 - n_h)
    for lo in (0, 256):
        trainer.step(t.collab[lo:lo + 256, 0], t.collab[lo:lo + 256, 1], t.cat[lo:lo + 256],
                     t.num[lo:lo + 256], t.y[lo:lo + 256])
    trainer.check_indices()
    model.eval()
    s_rows = M + pc.to_np(t.rows).astype(np.int64)
    s_item, s_cat = pc.to_np(t.collab)[:, 1], pc.to_np(t.cat)
    all_item, all_cat = np.concatenate([p_item, s_item]), np.concatenate([p_cat, s_cat])
    all_raw = raw_all[np.concatenate([p_rows, s_rows])]
    # the store and the features are rebuilt from main_df's rows with the new counts
    store = dcnr.InteractionStore(np.concatenate([pc.to_np(full[0])[:, 0], pc.to_np(t.collab)[:, 0]]), all_item,
                                  all_raw[:, 0], [0], [1],
                                  n_items=n_h1, n_reviewers=n_u1)
    ft = features(all_item, all_cat, all_raw, n_h1)
    stats = pipe.append_items(item_features=ft, return_stats=True)
    assert stats["changed"] == n_h1 - n_h and pipe.n_items == pipe.n_rows == n_h1
    assert pipe.index._table.data_ptr() == model.item_embedding.weight.data_ptr()   # shared, as before
    fresh = dcnr.RankingPipeline(model, item_features=ft, neighbor_table=True)
    assert torch.equal(pipe._nbr, fresh._nbr)
    assert torch.equal(pipe.index._inv, fresh.index._inv)

    new_user, new_hotel = n_u1 - 1, n_h1 - 1
    users = [new_user, 3, new_user - 1, 7]
    pos = [[2, new_hotel, 5], [new_hotel], [1, 2, 3, n_h + 1], [4]]
    kw = dict(lambda_param=[1.0, 0.5, 1.0, 0.3], top_k=[10, 5, 20, 10])
    got, want = pipe.recommend_many(users, pos, **kw), fresh.recommend_many(users, pos, **kw)
    assert len(got) == len(want) == 4 and got[0][0].numel() > 0
    for (gr, gl), (wr, wl) in zip(got, want):
        assert torch.equal(gr, wr) and torch.equal(gl.view(torch.int32), wl.view(torch.int32))
    assert any((g[0] >= n_h).any() for g in got)                 # a new hotel is recommended
    for row in (new_hotel, n_h, 0):
        assert torch.equal(pipe.similar_items(row, 10), fresh.similar_items(row, 10))
    gu = pipe.recommend_users(store, [new_user, 3], [new_user, 3], ["personal", "personal"], top_k=10)
    wu = fresh.recommend_users(store, [new_user, 3], [new_user, 3], ["personal", "personal"], top_k=10)
    for (gr, gl), (wr, wl) in zip(gu, wu):
        assert torch.equal(gr, wr) and torch.equal(gl.view(torch.int32), wl.view(torch.int32))
