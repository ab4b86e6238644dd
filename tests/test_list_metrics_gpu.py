"""GPU tests of dcnr_eval_list_metrics (intra-list diversity, coverage, Gini,
mean weight, held-out hits of served lists on the device), ``dcnr.list_metrics``,
``RankingPipeline.list_metrics`` and ``RankingPipeline.lambda_sweep``.

Bounds (tests/list_metrics_cases.py holds the cases and the host reference,
which reads the library's own inverse norms; u = 2^-53, e = 2^-24 the fp32
unit roundoff, K = at, d the embedding width):
  every integer     equal to the host's Python ints: every count of the
                    summary, n_distinct_items, gini_num, hit_lists, and m,
                    n_rel, hits, first_hit_rank of every record
  pair_cos_sum      pairs (d + 6) 2^-23 absolute.  One cosine is an fp32 dot of
                    d products: its error is at most d e sum|x_i y_i| inv inv
                    <= d e (1 + small) by Cauchy-Schwarz on rows of norm 1
                    (inv is the rounded inverse norm), plus at most three more
                    roundings (the two scalings and the conversion) of a value
                    <= 1: (d + 3) e per cosine whether the rows are scaled
                    before the dot or the dot after it.  The fp64 sum over the
                    pairs adds pairs u, far below.  The bound allows twice that:
                    (d + 6) 2^-23 = 2 (d + 3) e per pair.
  ild               (d + 6) 2^-23 + (n_lists_pairs + 8) 2^-52: each term 1 -
                    pair_cos_sum / pairs carries the per-cosine bound above; the
                    mean of m terms of magnitude <= 2 in a fixed order adds at
                    most (m + 8) 2^-52.
  info_sum, dcg[j]  (K + 2) 2^-53 relative: at most K positive terms, the same
                    doubles the host holds, in some fixed order ((K - 1) u), the
                    host's fsum one rounding.
  score_sum         K 2^-53 sum|z|: K terms of either sign in some fixed order.
  the fp64 means    (m + K + 8) 2^-52 absolute, m the number of lists averaged
                    (mrr, hit_rate, recall, ndcg: terms in [0, 1], the argument
                    of tests/test_grouped_metrics_gpu.py; mean_info: terms are
                    positive sums with the (K + 2) u above, a mean below 2 in
                    these cases, so (m + K) u relative is inside the bound);
                    mean_score: the same bound relative to the mean of |z|,
                    its terms having either sign.
  coverage, gini    one division of exact integers: equal to the host's
                    Python-float quotient.
"""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

import list_metrics_cases as lc

pytestmark = pytest.mark.gpu

U52, U53 = 2.0 ** -52, 2.0 ** -53
_cases = {}


def dev_case(dev, name):
    """The case's tensors on the device, the library's inverse norms and the
    host reference computed from them: built once per case."""
    if name not in _cases:
        from dcnr.serving import row_inv_norms
        c = lc.make_case(name)
        T = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        t = dict(rows=T(c["rows"]), offsets=T(c["offsets"]),
                 counts=None if c["counts"] is None else T(c["counts"]), table=T(c["table"]),
                 scores=T(c["scores"]), info=T(c["info"]))
        t["inv"] = row_inv_norms(t["table"])
        ref = lc.host_reference(c, t["inv"].cpu().numpy())
        _cases[name] = (c, t, ref)
    return _cases[name]


def c_call(dev, c, t, per_list=True, ws_bytes=None, fill=None):
    """dcnr_eval_list_metrics through the C entry point: (status, summary
    struct, records int64 [R, 14] or None, raw summary bytes)."""
    from dcnr import _lib
    from dcnr.metrics import _device_tables, relevant_csr
    lib = _lib.load()
    R, ks = c["R"], c["ks"]
    rr, ro = relevant_csr(c["relevant"], R, c["n_items"])
    d_rr, d_ro = torch.from_numpy(rr).to(dev), torch.from_numpy(ro).to(dev)
    disc, ideal = _device_tables(ks[-1], dev)
    need = lib.dcnr_eval_list_metrics_workspace_size(R, c["n_items"])
    ws = torch.empty(need if ws_bytes is None else ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.full((248,), 0 if fill is None else fill, dtype=torch.uint8, device=dev)
    rec = torch.zeros((R, 14), dtype=torch.int64, device=dev) if per_list else None
    arr = (ctypes.c_int32 * len(ks))(*ks)
    p = lambda x: x.data_ptr() if x is not None and x.numel() else None   # noqa: E731
    st = lib.dcnr_eval_list_metrics(
        p(t["rows"]), t["rows"].numel(), t["offsets"].data_ptr(), p(t["counts"]), R, c["at"],
        t["table"].data_ptr(), t["inv"].data_ptr(), c["d"], c["n_items"], p(t["scores"]),
        t["info"].data_ptr(), p(d_rr), d_rr.numel(), d_ro.data_ptr(), arr, len(ks), disc.data_ptr(),
        ideal.data_ptr(), out.data_ptr(), p(rec), p(ws), ws.numel(), _lib.stream_ptr(dev))
    raw = out.cpu().numpy().tobytes()
    return st, _lib.ListSummaryStruct.from_buffer_copy(raw), rec, raw


def close(a, b, bound):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return abs(a - b) <= bound


def check_summary(get, ref, c, tag):
    """``get(field)`` -> the device's value; tuples for the per-cutoff fields."""
    K, d, nk = c["at"], c["d"], len(c["ks"])
    for f in ("n_lists", "n_lists_scored", "n_lists_pairs", "n_marked", "n_bad_list", "n_entries",
              "n_distinct_items", "gini_num", "n_rel_lists"):
        assert get(f) == ref[f], (tag, f, get(f), ref[f])
    assert tuple(get("hit_lists"))[:nk] == ref["hit_lists"]
    bm = lambda m: (m + K + 8) * U52   # noqa: E731
    mabs = ref["mean_abs_score"]
    checks = [("ild", (d + 6) * 2.0 ** -23 + (ref["n_lists_pairs"] + 8) * U52),
              ("mrr", bm(ref["n_rel_lists"])),
              ("mean_info", bm(ref["n_lists_scored"])),
              ("mean_score", bm(ref["n_lists_scored"]) * (mabs if not math.isnan(mabs) else 1.0)),
              ("coverage", 0.0), ("gini", 0.0)]
    worst = {}
    for f, bound in checks:
        got, want = get(f), ref[f]
        print(f"{tag}: {f} = {got!r} (host {want!r}, bound {bound:.3e})")
        assert close(got, want, bound), (tag, f, got, want, bound)
        if bound and not math.isnan(want):
            worst[f] = abs(got - want) / bound
    for f in ("hit_rate", "recall", "ndcg"):
        for j in range(nk):
            got, want = get(f)[j], ref[f][j]
            assert close(got, want, bm(ref["n_rel_lists"])), (tag, f, j, got, want)
    print(f"{tag}: worst |d| / bound = " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def check_records(r, ref, c, tag):
    """``r``: dict of numpy arrays as ListMetrics.records holds them."""
    K, d, nk = c["at"], c["d"], len(c["ks"])
    want = ref["records"]
    for f in ("m", "n_rel", "first_hit_rank"):
        assert np.array_equal(r[f], want[f]), (tag, f)
    assert np.array_equal(r["hits"][:, :nk], want["hits"]), tag
    m = want["m"]
    pairs = m * (m - 1) // 2
    err = np.abs(r["pair_cos_sum"] - want["pair_cos_sum"])
    bound = pairs * (d + 6) * 2.0 ** -23
    print(f"{tag}: pair_cos_sum worst |d| / bound = "
          f"{float((err[pairs > 0] / bound[pairs > 0]).max()) if (pairs > 0).any() else 0.0:.2e}")
    assert np.all(err <= bound), (tag, float(err.max()))
    assert np.all(np.abs(r["info_sum"] - want["info_sum"]) <= (K + 2) * U53 * want["info_sum"]), tag
    assert np.all(np.abs(r["score_sum"] - want["score_sum"]) <= K * U53 * want["abs_score_sum"]), tag
    for j, k in enumerate(c["ks"]):
        assert np.all(np.abs(r["dcg"][:, j] - want["dcg"][:, j]) <= (k + 2) * U53 * want["dcg"][:, j]), (tag, j)


def rec_dict(rec, nk):
    a = rec.cpu().numpy()
    f = lambda x: np.ascontiguousarray(x).view(np.float64)   # noqa: E731
    return dict(m=a[:, 0], n_rel=a[:, 1], first_hit_rank=a[:, 2], hits=a[:, 3:3 + nk],
                pair_cos_sum=f(a[:, 7]), score_sum=f(a[:, 8]), info_sum=f(a[:, 9]),
                dcg=f(a[:, 10:10 + nk]).reshape(-1, nk))


@pytest.mark.parametrize("name", lc.NAMES)
def test_cases_through_the_c_entry_point(dev, name):
    from dcnr import _lib
    c, t, ref = dev_case(dev, name)
    st, m, rec, raw = c_call(dev, c, t)
    assert st == _lib.DCNR_OK
    get = lambda f: tuple(getattr(m, f)) if f in ("hit_lists", "hit_rate", "recall", "ndcg") \
        else getattr(m, f)   # noqa: E731
    check_summary(get, ref, c, name)
    check_records(rec_dict(rec, len(c["ks"])), ref, c, name)
    # entries j >= n_k are NaN (counts 0)
    for j in range(len(c["ks"]), 4):
        assert m.hit_lists[j] == 0 and math.isnan(m.hit_rate[j]) and math.isnan(m.ndcg[j])
    # two runs: the same bytes in the summary and in every record
    st2, _, rec2, raw2 = c_call(dev, c, t)
    assert st2 == _lib.DCNR_OK and raw2 == raw
    assert rec2.cpu().numpy().tobytes() == rec.cpu().numpy().tobytes()
    # closed forms
    if name.startswith("identical"):
        assert m.gini_num * 1000 == (1000 - 20) * (1000 * m.n_entries)     # gini = 1 - m / n_items
        assert m.gini == 1.0 - 20 / 1000 and m.n_distinct_items == 20
    if name == "equal":
        assert m.gini_num == 0 and m.gini == 0.0 and m.coverage == 1.0
    if name == "broken":
        assert (m.n_marked, m.n_bad_list) == (1, 7)


@pytest.mark.parametrize("name", lc.NAMES)
def test_cases_through_list_metrics(dev, name):
    import dcnr
    c, t, ref = dev_case(dev, name)
    m = dcnr.list_metrics(t["rows"], t["offsets"], t["counts"], table=t["table"], at=c["at"],
                          scores=t["scores"], info=c["info"], relevant=c["relevant"], ks=c["ks"],
                          per_list=True)
    assert m.ks == c["ks"] and m.records is not None
    check_summary(lambda f: getattr(m, f), ref, c, name + " (python)")
    check_records({k: v.cpu().numpy() for k, v in m.records.items()}, ref, c, name + " (python)")
    # the C call's bits: inv_norms=None computed the same inverse norms
    _, s, _, _ = c_call(dev, c, t, per_list=False)
    assert struct.pack("<2d", m.ild, m.mean_info) == struct.pack("<2d", s.ild, s.mean_info)
    # a (rows, offsets) tuple with unsorted, repeated sets gives the same hits
    flat = [list(s_)[::-1] * 2 for s_ in c["relevant"]]
    off = np.zeros(c["R"] + 1, np.int64)
    np.cumsum([len(x) for x in flat], out=off[1:])
    rows = np.array([v for x in flat for v in x], np.int64)
    m2 = dcnr.list_metrics(t["rows"], t["offsets"], t["counts"], table=t["table"], inv_norms=t["inv"],
                           at=c["at"], relevant=(rows, off), ks=c["ks"])
    assert m2.hit_lists == m.hit_lists and m2.n_rel_lists == m.n_rel_lists and m2.records is None
    assert math.isnan(m2.mean_score) and math.isnan(m2.mean_info)          # neither was given
    assert struct.pack("<d", m2.ild) == struct.pack("<d", m.ild)


def test_without_optional_inputs_and_empty(dev):
    """No scores, weights, held-out sets or cutoffs; R = 0."""
    import dcnr
    c, t, ref = dev_case(dev, "mix")
    m = dcnr.list_metrics(t["rows"], t["offsets"], t["counts"], table=t["table"], inv_norms=t["inv"],
                          at=c["at"], ks=())
    assert (m.n_entries, m.gini_num, m.n_rel_lists) == (ref["n_entries"], ref["gini_num"], 0)
    assert m.hit_rate == m.recall == m.ndcg == m.hit_lists == () and math.isnan(m.mrr)
    e = dcnr.list_metrics(t["rows"][:0], torch.zeros(1, dtype=torch.int64, device=dev), table=t["table"],
                          inv_norms=t["inv"], at=5, ks=(1, 5), per_list=True)
    assert e[10:19] == (0,) * 9 and e.hit_lists == (0, 0) and e.coverage == 0.0
    assert all(math.isnan(v) for v in (e.ild, e.gini, e.mean_score, e.mean_info, e.mrr) + e.ndcg)
    assert e.records["m"].shape[0] == 0


def test_second_stream_and_small_workspace(dev):
    from dcnr import _lib
    c, t, ref = dev_case(dev, "k33")
    _, _, rec, raw = c_call(dev, c, t)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        st, _, rec2, raw2 = c_call(dev, c, t)
    side.synchronize()
    assert st == _lib.DCNR_OK and raw2 == raw
    assert rec2.cpu().numpy().tobytes() == rec.cpu().numpy().tobytes()
    # one byte short: refused on the host, the summary untouched
    lib = _lib.load()
    need = lib.dcnr_eval_list_metrics_workspace_size(c["R"], c["n_items"])
    st, _, rec3, raw3 = c_call(dev, c, t, ws_bytes=need - 1, fill=0xAB)
    torch.cuda.synchronize()
    assert st == _lib.DCNR_WORKSPACE_TOO_SMALL
    assert raw3 == b"\xab" * 248 and not rec3.any()
    # the caller's workspace through the _raw variant
    import dcnr
    ws = torch.empty(need + 512, dtype=torch.uint8, device=dev)
    m = dcnr.list_metrics_raw(t["rows"], t["offsets"], t["counts"], table=t["table"],
                              inv_norms=t["inv"], at=c["at"], ks=c["ks"], ws=ws)
    assert (m.n_entries, m.gini_num) == (ref["n_entries"], ref["gini_num"])


@pytest.mark.parametrize("name", ["mix", "k128"])
def test_table_off_16_bytes_gives_the_same_bits(dev, name):
    """d % 4 == 0 takes 16-byte loads only when the table starts on 16 bytes;
    a table 4 bytes off takes the 4-byte path and sums each dot in the same order."""
    import dcnr
    c, t, _ = dev_case(dev, name)
    buf = torch.empty(t["table"].numel() + 1, dtype=torch.float32, device=dev)
    off = buf[1:].view_as(t["table"])
    off.copy_(t["table"])
    assert off.data_ptr() % 16 == 4 and t["table"].data_ptr() % 16 == 0 and c["d"] % 4 == 0
    kw = dict(inv_norms=t["inv"], at=c["at"], scores=t["scores"], ks=c["ks"], per_list=True)
    a = dcnr.list_metrics_raw(t["rows"], t["offsets"], t["counts"], table=t["table"], **kw)
    b = dcnr.list_metrics_raw(t["rows"], t["offsets"], t["counts"], table=off, **kw)
    assert metrics_bits(a) == metrics_bits(b)
    assert torch.equal(a.records["pair_cos_sum"].view(torch.int64), b.records["pair_cos_sum"].view(torch.int64))


# ------------------------------------------------------------------ the pipeline
def metrics_bits(m):
    """A ListMetrics' doubles as raw bits (NaN-safe equality) and its ints."""
    d = (m.ild, m.coverage, m.gini, m.mean_score, m.mean_info, m.mrr) + m.hit_rate + m.recall + m.ndcg
    return struct.pack(f"<{len(d)}d", *d), m.ks, m[10:20]


_nbr_pipes = {}


def sweep_pipe(dev, precision, table):
    import test_recommend_many_gpu as rm
    if not table:
        return rm.get_pipe(dev, precision)
    if precision not in _nbr_pipes:
        import dcnr
        base = rm.get_pipe(dev, precision)
        _nbr_pipes[precision] = dcnr.RankingPipeline(base.model, base.item_cat, base.item_num,
                                                     neighbor_table=True)
    return _nbr_pipes[precision]


def sweep_args(R, seed):
    import test_recommend_many_gpu as rm
    reqs, _, _ = rm.mixed_requests(R, seed)
    rng = np.random.default_rng(seed + 1)
    kw = dict(allowed=[q["allowed"] for q in reqs], excluded=[q["excluded"] for q in reqs],
              fallback=[q["fallback"] for q in reqs])
    relevant = [set(q["pos"][:2]) | {int(rng.integers(0, rm.N_ITEMS))} if r % 5 else set()
                for r, q in enumerate(reqs)]
    return [q["user"] for q in reqs], [q["pos"] for q in reqs], kw, relevant


LAMBDAS = (1.0, 0.7, 0.3, 0.0)


@pytest.mark.parametrize("table", [False, True], ids=["scan", "table"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_lambda_sweep_equals_recommend_many(dev, precision, table, monkeypatch):
    import dcnr
    import test_recommend_many_gpu as rm
    pipe = sweep_pipe(dev, precision, table)
    users, pos, kw, relevant = sweep_args(40, seed=5)
    info = dcnr.popularity_information(np.random.default_rng(3).integers(0, 50, rm.N_ITEMS))
    calls = []
    real = torch.cuda.Stream.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (calls.append(1), real(self))[1])
    sweep = pipe.lambda_sweep(users, pos, LAMBDAS, top_k=20, relevant=relevant, info=info, **kw)
    n_sync = len(calls)
    monkeypatch.undo()
    assert n_sync == 1, n_sync                    # the front's one wait, none per lambda
    assert sweep.lambdas == LAMBDAS and sweep.skipped == [] and len(sweep) == len(LAMBDAS)
    seen = set()
    for lam, (answers, m) in zip(LAMBDAS, sweep):
        want = pipe.recommend_many(users, pos, lam, 20, **kw)
        rm.assert_same(answers, want, f"{precision} lambda {lam}")
        mine = pipe.list_metrics(want, at=20, relevant=relevant, info=info)
        assert metrics_bits(m) == metrics_bits(mine), (lam, m, mine)
        assert m.n_lists == 40 and m.n_lists_scored > 20 and m.n_rel_lists > 10 and m.hit_lists[-1] > 0
        assert m.n_marked == m.n_bad_list == 0
        seen.add(metrics_bits(m)[0])
        print(f"{precision} table={table} lambda={lam}: ild={m.ild:.4f} coverage={m.coverage:.4f} "
              f"gini={m.gini:.4f} mean_score={m.mean_score:.4f} ndcg={m.ndcg}")
    assert len(seen) > 1                          # the lambdas' lists are not all the same lists


def test_lambda_sweep_skips_what_the_batched_kernels_hand_back(dev):
    import test_recommend_many_gpu as rm
    pipe = rm.get_pipe(dev, "bf16")
    users, pos, kw, relevant = sweep_args(6, seed=8)
    rng = np.random.default_rng(4)
    big = rng.choice(rm.N_ITEMS, 400, replace=False).tolist()
    assert len(big) * pipe.n_neighbors > rm.SV_MAX
    ins = lambda seq, v: seq[:3] + [v] + seq[3:]   # noqa: E731
    users2, pos2, rel2 = ins(users, 7), ins(pos, big), ins(relevant, set(big[:5]))
    kw2 = {k: ins(v, None) for k, v in kw.items()}
    lams = (1.0, 0.3)
    with_big = pipe.lambda_sweep(users2, pos2, lams, top_k=20, relevant=rel2, **kw2)
    without = pipe.lambda_sweep(users, pos, lams, top_k=20, relevant=relevant, **kw)
    assert with_big.skipped == [3] and without.skipped == []
    for (a2, m2), (a1, m1) in zip(with_big, without):
        assert a2[3] is None
        rm.assert_same(a2[:3] + a2[4:], a1, "others unchanged")
        assert m2.n_lists == 7 and m1.n_lists == 6
        assert m2[11:20] == m1[11:20]                                   # every other count
        b2, b1 = np.frombuffer(metrics_bits(m2)[0]), np.frombuffer(metrics_bits(m1)[0])
        assert np.allclose(b2, b1, rtol=1e-13, atol=0, equal_nan=True)  # (the sums' order depends on R)
        assert metrics_bits(pipe.list_metrics(a2, at=20, relevant=rel2)) == metrics_bits(m2)
    # a lambda that rounds to 1.0f from below: the batched kernels serve no request
    odd = pipe.lambda_sweep(users, pos, (0.3, 1.0 - 2.0 ** -30), top_k=20, relevant=relevant, **kw)
    assert odd.skipped == list(range(6))
    # (decided on the host: what comes back is what the device gives for six empty lists)
    empty = pipe.list_metrics([None] * 6, at=20, relevant=relevant)
    for answers, m in odd:
        assert answers == [None] * 6
        assert (m.n_lists, m.n_lists_scored, m.n_entries, m.n_rel_lists) == (6, 0, 0, 0)
        assert metrics_bits(m) == metrics_bits(empty)
    with pytest.raises(ValueError):                                      # the rows are still validated
        pipe.lambda_sweep(users, [[rm.N_ITEMS]] + pos[1:], (0.3, 1.0 - 2.0 ** -30), top_k=20)
    with pytest.raises(ValueError):
        pipe.lambda_sweep(users, pos, lams, top_k=200)                  # at <= 128
    with pytest.raises(ValueError):
        pipe.lambda_sweep(users, pos, lams, top_k=5)                    # the default ks reach 20


def test_recommend_users_answers(dev):
    """``recommend_users`` answers through ``pipeline.list_metrics``, the
    held-out set of a request its reviewer's first review: the hits are those
    of Python sets over ``to_lists``."""
    import test_recommend_users_gpu as ru
    pipe, store = ru.get_pipe(dev, "bf16"), ru.get_store()
    q = ru.mixed_requests(30, seed=11)
    q["top_k"] = [20] * 30
    res = ru.run_users(pipe, store, q)
    rev, item, *_ = ru.tables()
    relevant = []
    for r, u in enumerate(q["rv"]):
        mine = np.flatnonzero(rev == u) if u >= 0 else np.zeros(0, np.int64)
        s = {int(item[mine[0]])} if mine.size else set()
        if r % 3 == 0 and res[r][0].numel() >= 3:      # (and a hit for certain: its third hotel)
            s.add(int(res[r][0][2]))
        relevant.append(s)
    assert sum(r % 3 == 0 and res[r][0].numel() >= 3 for r in range(30)) > 0
    ks = (1, 5, 20)
    m = pipe.list_metrics(res, at=20, relevant=relevant, ks=ks, per_list=True)
    hits = m.records["hits"].cpu().numpy()
    fhr = m.records["first_hit_rank"].cpu().numpy()
    n_rel_lists, hit_lists = 0, [0, 0, 0]
    for r in range(30):
        rows = res.to_lists(r)[0][:20]
        where = [p for p, v in enumerate(rows) if v in relevant[r]]
        assert fhr[r] == (where[0] + 1 if where else 0)
        for j, k in enumerate(ks):
            assert hits[r, j] == sum(p < k for p in where)
            hit_lists[j] += bool(relevant[r]) and any(p < k for p in where)
        n_rel_lists += bool(relevant[r])
        assert int(m.records["m"][r]) == len(rows)
    assert m.n_rel_lists == n_rel_lists and m.hit_lists == tuple(hit_lists) and hit_lists[-1] > 0
    assert m.n_lists == 30 and m.n_marked == m.n_bad_list == 0
