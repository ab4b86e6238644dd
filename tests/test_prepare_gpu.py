"""prepare_data on the device (dcnr_train_table_build, ``dcnr.prepare_data``).
Every comparison is an equality of values, bit for bit but for the sign of a
zero (``np.array_equal(..., equal_nan=True)``).

  1  the kernel through the C ABI against ``dcnr.prepare_data_host``: every
     output and the workspace inside sentinel-guarded buffers, every case twice
     with equal bytes, the pinned mirrors equal to the device words
  2  the data edge cases of the contract, and where the reference raises
  3  workspace and argument errors, each before any launch
  4  ``dcnr.prepare_data`` against the golden frame and the yardstick, host and
     device-resident inputs
  5  what comes out plugs into DeviceLoader, FusedTrainer.fit, DCN_RecSys and
     ItemFeatures.set_scaler
"""
import ctypes

import numpy as np
import pytest
import torch

import prepare_common as pc

pytestmark = pytest.mark.gpu

GUARD, SENT = 64, -7
OK, BAD_ARG, UNSUPPORTED, TOO_SMALL = 0, 1, 4, 5
BAD_DATA = 2


# ------------------------------------------------ 1: the kernel, through the C ABI
def keys_of(case):
    from dcnr import prepare as P
    M = len(case["user"])
    cols = P._cat_columns(case["cat"], M)
    return np.stack([k for k, _ in cols], axis=1) if cols else np.zeros((M, 0), np.int64)


def c_build(dev, case, ws_short=0):
    """dcnr_train_table_build with every output (and the workspace) inside a
    sentinel-filled buffer with GUARD words to spare at both ends.  Returns the
    status and the outputs' interiors; asserts the guards and the mirrors."""
    from dcnr import _lib, prepare as P
    lib = _lib.load()
    raw = np.ascontiguousarray(case["num"], dtype=np.float64)
    M, n_raw = raw.shape
    key = keys_of(case)
    n_cat = key.shape[1]
    dv = P._derived_arg(case.get("derived", ()), n_raw)
    n_num = n_raw + len(dv)
    fcol, lo, hi = P._filter_arg(case.get("noise_filter"), n_raw)
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).reshape(-1).to(dev)
    d_in = [up(case["user"], torch.int64), up(case["item"], torch.int64),
            up(np.asarray(case["target"]) != 0, torch.uint8), up(key, torch.int64), up(raw, torch.float64)]
    nc = P.N_COUNTS + n_cat
    sizes = dict(row=(M, torch.int32), collab=(2 * M, torch.int64), cat=(M * n_cat, torch.int64),
                 num=(M * n_num, torch.int32), y=(M, torch.int32), user_ids=(M, torch.int64),
                 item_ids=(M, torch.int64), cat_keys=(n_cat * M, torch.int64), stats=(5 * n_num, torch.int64),
                 counts=(nc, torch.int32))   # (float outputs as bits)
    bufs = {k: torch.full((n + 2 * GUARD,), SENT, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
    h_counts = torch.full((nc + 2 * GUARD,), SENT, dtype=torch.int32).pin_memory()
    h_stats = torch.full((5 * n_num + 2 * GUARD,), SENT, dtype=torch.int64).pin_memory()
    nb = int(lib.dcnr_train_table_workspace_size(M, n_cat, n_raw, len(dv)))
    assert nb > 0
    ws = torch.full((nb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    at = lambda b: b.data_ptr() + GUARD * b.element_size()
    p = lambda x: x.data_ptr() if x.numel() else None
    a = P.TrainTableArgs(*[p(t) for t in d_in], M, n_cat, n_raw, fcol, lo, hi, len(dv),
                         dv.ctypes.data if len(dv) else None,
                         *[at(bufs[k]) for k in ("row", "collab", "cat", "num", "y", "user_ids", "item_ids",
                                                 "cat_keys", "stats")],
                         at(h_stats), at(bufs["counts"]), at(h_counts))
    status = lib.dcnr_train_table_build(ctypes.byref(a), at(ws), nb - ws_short, _lib.stream_ptr(dev))
    torch.cuda.current_stream(dev).synchronize()
    out = {}
    for k, b in list(bufs.items()) + [("h_counts", h_counts), ("h_stats", h_stats)]:
        v = b.cpu().numpy()
        assert (v[:GUARD] == SENT).all() and (v[v.size - GUARD:] == SENT).all(), f"guard of {k}"
        out[k] = v[GUARD:v.size - GUARD]
    w = ws.cpu().numpy()
    assert (w[:GUARD] == 0xA5).all() and (w[w.size - GUARD:] == 0xA5).all(), "guard of the workspace"
    if status != OK:
        for k in bufs:
            assert (out[k] == SENT).all(), f"{k} written by a rejected call"
        return status, out
    assert np.array_equal(out["h_counts"], out["counts"])
    if M:
        assert np.array_equal(out["h_stats"], out["stats"])
    n, n_users, n_items = (int(v) for v in out["counts"][:3])
    out["n"] = n
    out["row"] = out["row"][:n]
    out["collab"] = out["collab"][:2 * n].reshape(n, 2)
    out["cat"] = out["cat"][:n * n_cat].reshape(n, n_cat)
    out["num"] = out["num"].view(np.float32)[:n * n_num].reshape(n, n_num)
    out["y"] = out["y"].view(np.float32)[:n]
    out["user_ids"], out["item_ids"] = out["user_ids"][:n_users], out["item_ids"][:n_items]
    out["cat_keys"] = [out["cat_keys"][c * M:c * M + int(out["counts"][P.N_COUNTS + c])] for c in range(n_cat)]
    out["stats"] = out["stats"].view(np.float64).reshape(5, n_num)
    return status, out


def check_case(dev, case, expect="equal"):
    """Two runs with equal bytes; both equal to the yardstick, or the status
    says DCNR_REQ_BAD_DATA / n = 0 where the yardstick raises."""
    from dcnr import prepare_data_host, prepare as P
    st1, a = c_build(dev, case)
    st2, b = c_build(dev, case)
    assert st1 == OK and st2 == OK
    for k in ("counts", "row", "collab", "cat", "y", "user_ids", "item_ids"):
        assert a[k].tobytes() == b[k].tobytes(), f"two runs differ in {k}"
    assert a["num"].tobytes() == b["num"].tobytes() and a["stats"].tobytes() == b["stats"].tobytes()
    try:
        h = pc.call(prepare_data_host, case)
    except ValueError:
        assert expect == "raises"
        n, status = int(a["counts"][0]), int(a["counts"][4])
        assert status == BAD_DATA or n <= 1
        return a
    assert expect == "equal"
    assert int(a["counts"][4]) == 0
    assert a["n"] == len(h.rows) and int(a["counts"][3]) == h.n_after_filter
    assert pc.same(a["row"], h.rows)
    for k, t in zip(("collab", "cat", "num", "y"), h.full):
        assert pc.same(a[k], t), k
    assert pc.same(a["user_ids"], h.user_ids) and pc.same(a["item_ids"], h.item_ids)
    for c, k in enumerate(h.cat_keys):
        assert pc.same(a["cat_keys"][c], k), f"cat_keys[{c}]"
    for q, k in enumerate(("median_", "data_min_", "data_max_", "scale_", "min_")):
        assert pc.same(a["stats"][q], getattr(h, k)), k
    return a


SHAPES = [dict(seed=1, M=2), dict(seed=3, M=63), dict(seed=4, M=64), dict(seed=5, M=65),
          dict(seed=13, M=4095), dict(seed=14, M=4096), dict(seed=7, M=4097),
          dict(seed=12, M=20000, n_users=50, n_items=7),                       # heavy duplication
          dict(seed=8, M=300, n_cat=0), dict(seed=15, M=257, n_raw=64, n_derived=0),
          dict(seed=16, M=1500, n_raw=40, n_derived=24, n_cat=3),              # 64 columns, derived among them
          dict(seed=10, M=500, nan=0.5, missing=0.3), dict(seed=17, M=9000, wide_ids=False, use_filter=False),
          # 17 and 34 sort units: the sort's totals kernel sums the units in 16 segments, of
          # two and of three units here (20000 rows are 5 units, one segment each); 65 and 133
          # scan tiles; few ids, so that every id repeats across the units
          dict(seed=18, M=65537, n_users=50, n_items=7), dict(seed=19, M=135173, n_users=300, n_items=40)]


@pytest.mark.parametrize("kw", SHAPES, ids=lambda kw: f"M{kw['M']}s{kw['seed']}")
def test_kernel_matches_yardstick(dev, kw):
    check_case(dev, pc.random_case(**kw))


def test_kernel_golden_frame(dev):
    a = check_case(dev, pc.golden_case())
    assert a["n"] == 250


def test_one_row(dev):
    a = check_case(dev, pc.random_case(3, 1, missing=0.0, use_filter=False), expect="raises")   # no train set
    assert a["n"] == 1 and a["collab"].tolist() == [[0, 0]] and int(a["counts"][4]) == 0


def test_no_rows(dev):
    st, a = c_build(dev, pc.random_case(1, 0))
    assert st == OK and (a["counts"] == 0).all() and (a["h_counts"] == 0).all()


# ------------------------------------------------------------ 2: the data rules
def test_edge_columns(dev):
    names, cols = pc.edge_columns()
    keep = [c for n, c in zip(names, cols) if n != "overflow_sum"]
    a = check_case(dev, pc.plain_case(101, keep))
    idx = {n: k for k, n in enumerate(n for n in names if n != "overflow_sum")}
    scale = a["stats"][3]
    assert np.isnan(a["stats"][:, idx["all_nan"]]).all() and np.isnan(a["num"][:, idx["all_nan"]]).all()
    assert scale[idx["constant"]] == 1.0 and scale[idx["range_5eps"]] == 1.0
    assert scale[idx["range_20eps"]] == 1.0 / (20 * pc.EPS)
    lo, hi = 0.1, np.nextafter(0.1, 1.0)
    assert a["stats"][0][idx["last_bit"]] == (lo + hi) / 2
    # even counts: the first row leaves through its category
    cat = [np.where(np.arange(101) == 0, -1, np.arange(101) % 3)]
    check_case(dev, pc.plain_case(101, keep, cat=cat))


def test_inf_is_bad_data(dev):
    names, cols = pc.edge_columns()
    over = [c for n, c in zip(names, cols) if n == "overflow_sum"]
    a = check_case(dev, pc.plain_case(101, over), expect="raises")     # the median's sum overflows
    assert a["stats"][0][0] == np.inf and int(a["counts"][4]) == BAD_DATA
    c = np.arange(300.0); c[123] = np.inf
    a = check_case(dev, pc.plain_case(300, [c, np.arange(300.0)]), expect="raises")
    assert int(a["counts"][4]) == BAD_DATA
    c = np.array([-np.inf, np.inf, np.nan, np.nan])                      # median of -inf and +inf
    a = check_case(dev, pc.plain_case(4, [c]), expect="raises")
    assert np.isnan(a["stats"][0][0]) and int(a["counts"][4]) == BAD_DATA
    # an inf in a row that is dropped does not count
    c = np.arange(50.0); c[7] = -np.inf
    cat = [np.where(np.arange(50) == 7, -1, 0)]
    check_case(dev, pc.plain_case(50, [np.arange(50.0), c], cat=cat, noise_filter=None))


def test_ids(dev):
    M = 700
    cols = [np.arange(M) % 13.0]
    check_case(dev, pc.plain_case(M, cols, user=np.arange(M)[::-1] * 3 - 1000))               # all distinct
    check_case(dev, pc.plain_case(M, cols, user=np.full(M, -5), item=np.full(M, 1 << 62)))   # one user
    lowsame = (np.arange(M) % 9).astype(np.int64) << 32                                        # equal low words
    check_case(dev, pc.plain_case(M, cols, user=lowsame + 17, item=-(lowsame + 17)))
    ext = np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, -1, 1 << 40, -(1 << 40)])
    check_case(dev, pc.plain_case(M, cols, user=ext[np.arange(M) % 6], item=ext[::-1][np.arange(M) % 4]))


def test_only_in_dropped_rows(dev):
    M = 400
    rating = np.where(np.arange(M) % 4 == 0, 6.0, 9.0)          # the filter drops every fourth row
    user = np.where(np.arange(M) % 4 == 0, 10 ** 12 + np.arange(M), np.arange(M) % 11)
    item = np.where(np.arange(M) % 8 == 1, 555 + np.arange(M), np.arange(M) % 7)
    c0 = np.where(np.arange(M) % 8 == 1, -1, np.arange(M) % 3)   # ... whose items only occur here
    c1 = np.where(np.arange(M) % 4 == 0, 99, np.arange(M) % 2)   # key 99 only in filtered rows
    a = check_case(dev, pc.plain_case(M, [rating, np.arange(M) * 0.5], user=user, item=item, cat=[c0, c1],
                                      noise_filter=(0, 4.0, 8.0)))
    assert a["user_ids"].max() < 10 ** 12 and a["item_ids"].max() < 555 and 99 not in a["cat_keys"][1]
    assert int(a["counts"][3]) == 300 and a["n"] == 250


def test_filter_drops_everything(dev):
    case = pc.random_case(3, 500)
    case["noise_filter"] = (0, -1.0, 100.0)
    a = check_case(dev, case, expect="raises")
    assert a["n"] == 0 and int(a["counts"][3]) == 0 and (a["counts"][:4] == 0).all()
    import dcnr
    with pytest.raises(ValueError):
        pc.call(dcnr.prepare_data, case, device=dev)


# ------------------------------------------------ 3: workspace and argument errors
def test_workspace_and_statuses(dev):
    from dcnr import _lib, prepare as P
    lib = _lib.load()
    case = pc.random_case(2, 100)
    assert c_build(dev, case, ws_short=1)[0] == TOO_SMALL
    size = lib.dcnr_train_table_workspace_size
    assert size(100, 2, 8, 3) > 0 and size(0, 0, 0, 0) > 0
    for bad in ((-1, 2, 8, 3), (100, -1, 8, 3), (100, 2, -1, 3), (100, 2, 8, -1), (2 ** 31 - 1, 2, 8, 3),
                (100, 65, 8, 3), (100, 2, 62, 3), (100, 2, 65, 0)):
        assert size(*bad) == 0, bad

    def status(**over):
        """A call that must be rejected before any launch: valid buffers, one
        argument wrong; the counts word stays as it was."""
        M, n_cat, n_raw = 100, 2, 8
        t = {k: torch.zeros(M * w, dtype=dt, device=dev) for k, (w, dt) in dict(
            user=(1, torch.int64), item=(1, torch.int64), target=(1, torch.uint8), cat_key=(n_cat, torch.int64),
            raw=(n_raw, torch.float64), row=(1, torch.int32), collab=(2, torch.int64), cat=(n_cat, torch.int64),
            num=(64, torch.float32), y=(1, torch.float32), user_ids=(1, torch.int64), item_ids=(1, torch.int64),
            cat_keys=(n_cat, torch.int64)).items()}
        stats = torch.zeros(5 * 64, dtype=torch.float64, device=dev)
        counts = torch.full((P.N_COUNTS + 64,), SENT, dtype=torch.int32, device=dev)
        null_derived = "derived" in over and over["derived"] is None
        dv = np.array(over.pop("derived", None) or [[0, 0, 1]], dtype=np.int32).reshape(-1, 3)
        f = dict(user=t["user"].data_ptr(), item=t["item"].data_ptr(), target=t["target"].data_ptr(),
                 cat_key=t["cat_key"].data_ptr(), raw=t["raw"].data_ptr(), M=M, n_cat=n_cat, n_raw=n_raw,
                 filter_col=-1, filter_lo=4.0, filter_hi=8.0, n_derived=len(dv),
                 derived=None if null_derived else dv.ctypes.data,
                 row=t["row"].data_ptr(), collab=t["collab"].data_ptr(), cat=t["cat"].data_ptr(),
                 num=t["num"].data_ptr(), y=t["y"].data_ptr(), user_ids=t["user_ids"].data_ptr(),
                 item_ids=t["item_ids"].data_ptr(), cat_keys=t["cat_keys"].data_ptr(),
                 stats=stats.data_ptr(), host_stats=None, counts=counts.data_ptr(), host_counts=None)
        f.update(over)
        ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
        ws_ptr = None if f.pop("no_ws", False) else ws.data_ptr()
        st = lib.dcnr_train_table_build(ctypes.byref(P.TrainTableArgs(**f)), ws_ptr, ws.numel(),
                                        _lib.stream_ptr(dev))
        torch.cuda.current_stream(dev).synchronize()
        assert (counts.cpu().numpy() == SENT).all() or st == OK
        return st
    assert status() == OK
    for name in ("user", "item", "target", "cat_key", "raw", "row", "collab", "cat", "num", "y", "user_ids",
                 "item_ids", "cat_keys", "stats", "counts", "derived"):
        assert status(**{name: None}) == BAD_ARG, name
    assert status(no_ws=True) == BAD_ARG
    assert status(M=-1) == BAD_ARG and status(n_cat=-1) == BAD_ARG and status(n_raw=-1) == BAD_ARG
    assert status(n_derived=-1) == BAD_ARG
    assert status(filter_col=8) == BAD_ARG and status(filter_col=-2) == BAD_ARG and status(filter_col=7) == OK
    assert status(derived=[[0, 8, 0]]) == BAD_ARG and status(derived=[[1, 0, -1]]) == BAD_ARG
    assert status(derived=[[2, 0, 1]]) == BAD_ARG
    assert status(M=2 ** 31 - 1) == UNSUPPORTED and status(n_cat=65) == UNSUPPORTED
    assert status(n_raw=64) == UNSUPPORTED          # 64 raw + 1 derived
    assert lib.dcnr_train_table_build(None, None, 0, _lib.stream_ptr(dev)) == BAD_ARG


# ------------------------------------------------------------- 4: the Python front
_prep = {}


def golden_prep(dev):
    import dcnr
    if "p" not in _prep:
        _prep["g"] = pc.load_golden()
        _prep["p"] = pc.call(dcnr.prepare_data, pc.golden_case(_prep["g"]), device=dev)
    return _prep["p"], _prep["g"]


def test_prepare_data_golden(dev):
    import dcnr
    p, g = golden_prep(dev)
    pc.assert_matches_golden(p, g)
    assert all(t.device.type == "cuda" for t in p.train + p.val)
    assert p.train[0].dtype == torch.int64 and p.train[2].dtype == torch.float32
    pc.assert_same_prepared(p, pc.call(dcnr.prepare_data_host, pc.golden_case(g)), "golden")


@pytest.mark.parametrize("kw", [dict(seed=21, M=3000), dict(seed=22, M=777, n_cat=0),
                                dict(seed=23, M=10, use_filter=False)],
                         ids=lambda kw: f"M{kw['M']}")
def test_prepare_data_matches_yardstick(dev, kw):
    import dcnr
    case = pc.random_case(**kw)
    pc.assert_same_prepared(pc.call(dcnr.prepare_data, case, device=dev),
                            pc.call(dcnr.prepare_data_host, case), str(kw))


def test_prepare_data_device_inputs(dev):
    import dcnr
    case = pc.random_case(24, 2500)
    on = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    dcase = dict(case, user=on(case["user"]), item=on(case["item"]), target=on(case["target"]),
                 cat=torch.stack([on(k) for k in case["cat"]], dim=1), num=on(case["num"]))
    a = pc.call(dcnr.prepare_data, dcase, device=dev)
    pc.assert_same_prepared(a, pc.call(dcnr.prepare_data, case, device=dev), "device inputs")
    pc.assert_same_prepared(a, pc.call(dcnr.prepare_data_host, case), "device inputs, host")
    # a list of device columns, and value columns through category_keys
    words = np.array(["b", "a", None, "c"], dtype=object)
    vcase = dict(case, cat=[on(case["cat"][0]), words[np.arange(2500) % 4]], cat_names=["k", "w"])
    v = pc.call(dcnr.prepare_data, vcase, device=dev)
    pc.assert_same_prepared(v, pc.call(dcnr.prepare_data_host, dict(vcase, cat=[case["cat"][0], vcase["cat"][1]])),
                            "values")
    assert v.cat_encoders["w"] == {"a": 0, "b": 1, "c": 2}


def test_prepare_data_raises(dev):
    import dcnr
    c = np.arange(40.0); c[5] = np.inf
    with pytest.raises(ValueError):
        pc.call(dcnr.prepare_data, pc.plain_case(40, [c]), device=dev)
    with pytest.raises(ValueError):
        pc.call(dcnr.prepare_data, pc.random_case(3, 1, missing=0.0, use_filter=False), device=dev)   # n = 1
    with pytest.raises(ValueError):
        pc.call(dcnr.prepare_data, pc.random_case(3, 0), device=dev)
    with pytest.raises(ValueError):
        pc.call(dcnr.prepare_data, dict(pc.random_case(3, 30), derived=[("ratio", 0, 8)]), device=dev)


# --------------------------------------------------------------- 5: the plumbing
def test_loader_batches(dev):
    import dcnr
    p, g = golden_prep(dev)
    host = [torch.from_numpy(g[f"train_{k}"].copy()) for k in ("collab", "cat", "num", "y")]
    torch.manual_seed(11)
    ours = [tuple(t.cpu() for t in b) for b in p.loader(32)]
    torch.manual_seed(11)
    ref = [tuple(t.cpu() for t in b) for b in dcnr.DeviceLoader(*host, batch_size=32, shuffle=True, device=dev)]
    assert len(ours) == len(ref) == -(-host[0].shape[0] // 32)
    for a, b in zip(ours, ref):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    ld = p.loader(64, shuffle=False)
    assert all(x.data_ptr() == y.data_ptr() for x, y in zip(ld.tensors, p.train))   # no copy


def test_fit_one_epoch(dev):
    import dcnr
    p, _ = golden_prep(dev)
    params = dict(emb_dim=8, hidden_dim=32, n_cross_layers=2, n_res_blocks=1, dropout=0.0)
    torch.manual_seed(3)
    model = dcnr.DCN_RecSys(*p.model_dims, params).to(dev)
    trainer = dcnr.FusedTrainer(model, lr=1e-3, weight_decay=1e-4)
    hist = trainer.fit(p.loader(64), p.val, n_epochs=1)
    m = hist["epochs"][0]["metrics"]
    assert len(hist["epochs"]) == 1 and np.isfinite(m.logloss) and 0.0 <= m.auc <= 1.0


def test_item_features_set_scaler(dev):
    import dcnr
    p, g = golden_prep(dev)
    rows = pc.to_np(p.rows)
    raw = g["raw"][rows]
    extra = []
    with np.errstate(all="ignore"):
        for op, i, j in g["derived"]:
            v = raw[:, i] / raw[:, j] if op == 0 else raw[:, i] - raw[:, j]
            if op == 0:
                v[~np.isfinite(v)] = 0.0
            extra.append(v)
    x = np.column_stack([raw] + extra)
    x = np.where(np.isnan(x), p.median_[None, :], x)            # the rows' values, filled
    collab, cat, num, _ = (pc.to_np(t) for t in p.full)
    n_items, n_num = p.model_dims[1], p.model_dims[3]
    feats = dcnr.ItemFeatures(collab[:, 1], cat, x, np.ones(n_num), np.zeros(n_num), n_items)
    feats.set_scaler(p.scale_, p.min_)
    gen = feats.on(dev)
    first = np.array([np.flatnonzero(collab[:, 1] == h)[0] for h in range(n_items)])
    assert pc.same(gen.item_num.cpu().numpy(), num[first])
    assert pc.same(gen.item_cat.cpu().numpy(), cat[first])
