"""``dcnr.IdMap.lookup`` and ``dcnr.Preprocessor.transform`` on the device
(dcnr_id_map_build, dcnr_id_map_lookup, dcnr_rows_transform).  Every comparison
is exact: integers equal, floats equal as ``prepare_common.same`` defines it.

  1  ``IdMap.lookup`` against a Python dict, at the default capacity and in a
     nearly full table (long probe chains, wrap-around)
  2  ``transform`` against ``transform_host``, every field and every count
  3  identity: the fit's own input is ``prepare_data``'s unsplit tables
  4  the fixture of tests/golden/transform through the device path
  5  edges; bad data
  6  what comes out feeds ``dcnr.evaluate`` and ``FusedTrainer.step``
"""
import numpy as np
import pytest
import torch

import prepare_common as pc
import transform_common as tc

pytestmark = pytest.mark.gpu

QUERIES = (0, 1, 257, 70001)
# seed: (M, M2).  The fits of seeds 31-34 hold every key of both category columns, so their new
# rows meet missing keys but no unseen one; the small fit of seed 36 is there for that kind.
CASES = {31: (3000, 3000), 32: (777, 70001), 33: (257, 257), 34: (40, 1000), 36: (24, 500)}
FIVE = ("user", "item", "target", "cat", "num")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------- 1: IdMap
@pytest.mark.parametrize("tight", [False, True])
@pytest.mark.parametrize("multiples", [False, True])
@pytest.mark.parametrize("n", [1, 2, 1000, 100003])
def test_lookup_against_a_dict(dev, n, multiples, tight):
    import dcnr
    rng = np.random.default_rng(1000 * n + 2 * multiples + tight)
    ids = tc.wide_ids(rng, n, multiples)
    cap = None
    if tight:           # the smallest power of two above n: 1000 ids in 1024 slots
        cap = 1
        while cap <= n:
            cap <<= 1
    m = dcnr.IdMap(ids, device=dev, capacity=cap)
    assert len(m) == n and m.capacity == (cap or m.capacity) and m.capacity >= (n + 1 if tight else 2 * n)
    assert m.ids.device.type == "cuda" and m.ids.cpu().numpy().tolist() == ids.tolist()
    table = {int(v): i for i, v in enumerate(ids.tolist())}
    for M in QUERIES:
        absent = tc.wide_ids(rng, M - M // 2, multiples) + 7
        q = np.concatenate([rng.choice(ids, M // 2), absent]).astype(np.int64)
        rng.shuffle(q)
        if M > 1:
            q[M // 3] = tc.RESERVED
        for default in (-1, n // 2):
            want = np.array([table.get(int(v), default) for v in q.tolist()], dtype=np.int64)
            got = m.lookup(q, default)                       # a host array
            assert got.device.type == "cuda" and got.dtype == torch.int64
            assert np.array_equal(got.cpu().numpy(), want), (n, M, default)
            assert np.array_equal(m.lookup_host(q, default), want)
        got_dev = m.lookup(torch.from_numpy(q).to(dev))      # a device tensor, read where it is
        assert np.array_equal(got_dev.cpu().numpy(), m.lookup(q).cpu().numpy())
    if n > 1:   # the reverse map is a plain gather
        back = m.ids[m.lookup(ids[::-1].copy())]
        assert np.array_equal(back.cpu().numpy(), ids[::-1])


def test_idmap_value_errors(dev):
    import dcnr
    with pytest.raises(ValueError):
        dcnr.IdMap(np.array([5, 9, 5]), device=dev)
    with pytest.raises(ValueError):
        dcnr.IdMap(torch.tensor([5, tc.RESERVED], device=dev), device=dev)
    with pytest.raises(ValueError):
        dcnr.IdMap(np.arange(8), device=dev, capacity=8)
    assert dcnr.IdMap(np.zeros(0, np.int64), device=dev).lookup(np.array([3])).tolist() == [-1]


# ----------------------------------------------- 2: transform against its yardstick
@pytest.fixture(scope="module")
def fits(dev):
    """Per seed: the frame, its device and host fits on the first M rows."""
    import dcnr
    out = {}
    for seed, (M, M2) in CASES.items():
        whole = pc.random_case(seed, M + M2, n_users=M // 2, n_items=M // 5)
        fit_case = dict(whole, **dict(zip(FIVE, tc.part(whole, 0, M))))
        out[seed] = (whole, pc.call(dcnr.prepare_data, fit_case, device=dev).preprocessor(),
                     pc.call(dcnr.prepare_data_host, fit_case).preprocessor())
    return out


@pytest.mark.parametrize("use_filter", [False, True])
@pytest.mark.parametrize("fill_nan", [False, True])
@pytest.mark.parametrize("unknown", ["reference", "drop"])
@pytest.mark.parametrize("seed", sorted(CASES))
def test_transform_against_transform_host(dev, fits, seed, unknown, fill_nan, use_filter):
    whole, pre_dev, pre_host = fits[seed]
    M, M2 = CASES[seed]
    new = tc.part(whole, M, M + M2)
    kw = dict(unknown=unknown, fill_nan=fill_nan, noise_filter="fitted" if use_filter else None)
    want = pre_host.transform_host(*new, **kw)
    got = pre_dev.transform(*new, device=dev, **kw)
    tc.assert_same_transformed(got, want, f"seed {seed} {kw}")
    assert got.collab.device.type == "cuda" and got.n == got.collab.shape[0] == got.rows.shape[0]
    assert (want.n_filtered > 0) == use_filter
    if unknown == "drop":
        assert 0.25 * M2 <= got.n <= 0.75 * M2, (seed, got.n, M2)
        assert not got.unknown_bits.any().item()
    else:
        assert want.n == M2 - want.n_filtered


def test_every_kind_of_unknown_occurs(fits):
    """Over the cases above: an unknown user, an unknown hotel, an unseen category key, a missing one."""
    kinds = set()
    for seed, (M, M2) in CASES.items():
        whole, _, pre_host = fits[seed]
        new = tc.part(whole, M, M + M2)
        t = pre_host.transform_host(*new)
        keys = np.stack(new[3], axis=1)
        unk = (t.unknown_bits[:, None] >> (2 + np.arange(keys.shape[1]))) & 1 != 0
        kinds |= {"missing"} if (unk & (keys < 0)).any() else set()
        kinds |= {"category"} if (unk & (keys >= 0)).any() else set()
        kinds |= {"user"} if t.n_unknown_users else set()
        kinds |= {"hotel"} if t.n_unknown_items else set()
    assert kinds == {"user", "hotel", "category", "missing"}


# -------------------------------------------------------------- 3: the identity
@pytest.mark.parametrize("case", ["golden", 45])
def test_identity_on_the_device(dev, case):
    import dcnr
    case = pc.golden_case() if case == "golden" else pc.random_case(case, 5003)
    p = pc.call(dcnr.prepare_data, case, device=dev)
    t = p.preprocessor().transform(*[case[k] for k in FIVE], noise_filter="fitted", unknown="drop", fill_nan=True,
                                   device=dev)
    for k, a, b in zip(("collab", "cat", "num", "y"), t.tensors, p.full):
        assert pc.same(pc.to_np(a), pc.to_np(b)), k
    assert pc.same(pc.to_np(t.rows), pc.to_np(p.rows))
    assert t.n_filtered == len(case["user"]) - p.n_after_filter


# ------------------------------------------------------------ 4: the reference
def test_golden_fixture_on_the_device(dev):
    import dcnr
    g = tc.load_golden()
    p = pc.call(dcnr.prepare_data, pc.golden_case(), device=dev)
    for pre in (p.preprocessor(),
                dcnr.Preprocessor.from_artifacts(p.artifacts(), derived=p.derived, median=p.median_)):
        t = pre.transform(*tc.golden_rows(g), unknown="reference", fill_nan=False, device=dev)
        tc.assert_matches_golden(t, g)
        assert (t.n_unknown_users, t.n_unknown_items, t.n_unknown_cat) == (12, 4, [7, 4])


# ------------------------------------------------------------------- 5: edges
def small_fit(dev, n_cat=2, n_raw=8, n_derived=3, M=300, seed=51):
    import dcnr
    whole = pc.random_case(seed, 2 * M, n_cat=n_cat, n_raw=n_raw, n_derived=n_derived, n_users=M // 2,
                           n_items=M)
    fit_case = dict(whole, **dict(zip(FIVE, tc.part(whole, 0, M))))
    return (whole, pc.call(dcnr.prepare_data, fit_case, device=dev).preprocessor(),
            pc.call(dcnr.prepare_data_host, fit_case).preprocessor())


@pytest.mark.parametrize("M2", [0, 1])
def test_tiny_inputs(dev, M2):
    whole, pre_dev, pre_host = small_fit(dev)
    new = tc.part(whole, 300, 300 + M2)
    for unknown in ("reference", "drop"):
        got = pre_dev.transform(*new, unknown=unknown, device=dev)
        tc.assert_same_transformed(got, pre_host.transform_host(*new, unknown=unknown), f"M2={M2}")
        assert got.num.shape == (got.n, 11) and got.cat.shape == (got.n, 2)


@pytest.mark.parametrize("shape", [dict(n_cat=0), dict(n_raw=0, n_derived=0)])
def test_no_categories_and_no_numeric_columns(dev, shape):
    whole, pre_dev, pre_host = small_fit(dev, **shape)
    new = tc.part(whole, 300, 600)
    for unknown in ("reference", "drop"):
        got = pre_dev.transform(*new, unknown=unknown, noise_filter="fitted", device=dev)
        tc.assert_same_transformed(got, pre_host.transform_host(*new, unknown=unknown, noise_filter="fitted"),
                                   str(shape))
        assert got.n > 0


def test_all_unknown_target_none_and_device_inputs(dev):
    whole, pre_dev, pre_host = small_fit(dev)
    user, item, target, cat, num = tc.part(whole, 300, 600)
    # no row has a known user: nothing survives "drop", and nothing is wrong with that
    strangers = user * 0 + np.arange(user.size) + (1 << 50)
    got = pre_dev.transform(strangers, item, target, cat, num, unknown="drop", device=dev)
    assert got.n == 0 and got.collab.shape == (0, 2) and got.num.shape == (0, 11) and got.y.shape == (0,)
    assert got.n_unknown_users == user.size
    tc.assert_same_transformed(got, pre_host.transform_host(strangers, item, target, cat, num, unknown="drop"))
    # no target: no y
    got = pre_dev.transform(user, item, None, cat, num, device=dev)
    want = pre_host.transform_host(user, item, None, cat, num)
    assert got.y is None and got.tensors[3] is None
    tc.assert_same_transformed(got, want, "target=None")
    # device-resident columns are used where they are
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = pre_dev.transform(up(user), up(item), up(target), torch.stack([up(k) for k in cat], dim=1), up(num),
                            unknown="drop", noise_filter="fitted", device=dev)
    tc.assert_same_transformed(got, pre_host.transform_host(user, item, target, cat, num, unknown="drop",
                                                            noise_filter="fitted"), "device inputs")
    with pytest.raises(ValueError):
        pre_dev.transform(user, item[:-1], target, cat, num, device=dev)
    with pytest.raises(ValueError):
        pre_dev.transform(user, item, target, cat, num, unknown="ignore", device=dev)


def test_bad_data(dev):
    whole, pre_dev, pre_host = small_fit(dev)
    user, item, target, cat, num = tc.part(whole, 300, 600)
    num = num.copy()
    dropped = int(np.flatnonzero((num[:, 0] > 4.0) & (num[:, 0] < 8.0))[0])   # a row the filter removes
    num[dropped, 3] = -np.inf
    got = pre_dev.transform(user, item, target, cat, num, noise_filter="fitted", device=dev)
    tc.assert_same_transformed(got, pre_host.transform_host(user, item, target, cat, num, noise_filter="fitted"))
    with pytest.raises(ValueError, match="infinity"):
        pre_dev.transform(user, item, target, cat, num, device=dev)              # ... and survives without it
    with pytest.raises(ValueError, match="infinity"):
        pre_host.transform_host(user, item, target, cat, num)


# -------------------------------------------------------------- 6: downstream
def test_feeds_evaluate_and_the_trainer(dev):
    import dcnr
    whole, pre_dev, _ = small_fit(dev)
    t = pre_dev.transform(*tc.part(whole, 300, 600), unknown="reference", fill_nan=True, device=dev)
    assert 0 < t.n <= 512 and t.n_unknown_users > 0 and t.n_unknown_items > 0 and sum(t.n_unknown_cat) > 0
    cat_dims = {name: int(len(k)) for name, k in zip(pre_dev.cat_names, pre_dev.cat_keys)}
    params = dict(emb_dim=8, hidden_dim=64, n_cross_layers=2, n_res_blocks=2, dropout=0.0)
    torch.manual_seed(0)
    model = dcnr.DCN_RecSys(len(pre_dev.user_ids), len(pre_dev.item_ids), cat_dims, pre_dev.n_num, params).to(dev)
    m = dcnr.evaluate(model, *t.tensors)
    assert m.n == t.n and np.isfinite(m.logloss)
    trainer = dcnr.FusedTrainer(model, lr=1e-3)
    loss = trainer.step(t.collab[:, 0], t.collab[:, 1], t.cat, t.num, t.y)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
