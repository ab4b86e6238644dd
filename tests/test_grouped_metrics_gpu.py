"""GPU tests of dcnr_eval_group_metrics (per-group GAUC, NDCG@k, hit rate,
recall, MRR on the device), ``dcnr.group_metrics``, ``dcnr.evaluate_ranking``
and ``FusedTrainer.fit(ranking=...)``.

Bounds (tests/grouped_metrics_cases.py holds the cases and the host
reference; u = 2^-53 is the unit roundoff):
  every integer     equal to the host's Python ints: the summary's counts and
                    n, n_pos, auc_u2, first_pos_rank, hits of every record
  dcg[j] per record (k_j + 2) 2^-53 relative.  The device adds at most k_j
                    positive terms discount[r - 1], the same doubles the host
                    holds, in some fixed order: any order of an m-term sum of
                    positive terms is within (m - 1) u relative of the exact
                    sum, the host's long-double sum rounded once within u
  each fp64 mean    (m + k_max + 8) 2^-52 absolute, m the number of groups
                    averaged.  Every term (AUC_u, 1 / rank, hits / P_u,
                    dcg / ideal) lies in [0, 1] and is one or two roundings of
                    an exact quotient, except dcg, which carries the
                    (k_max + 2) u above; the device's m-term sum in its fixed
                    order is within (m - 1) u sum|x| <= (m - 1) u m of the
                    exact sum, i.e. (m - 1) u on the mean; the division and
                    the host's fsum add a rounding each.  Together under
                    (m + k_max + 8) u, and the bound allows twice that.  gauc
                    weights each term by n_u and divides by the sum of the
                    n_u: the same bound on a mean that is still in [0, 1].
"""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

import golden_common as gc
import grouped_metrics_cases as gm
import metrics_cases as mc
from helpers import our_model, to_dev

pytestmark = pytest.mark.gpu

IDS = [gm.case_id(c) for c in gm.CASES]
U52 = 2.0 ** -52


def on_dev(dev, case):
    z, y, g, ng, rec, ref = gm.case_with_reference(case)
    T = lambda a: torch.from_numpy(a.copy()).to(dev)   # noqa: E731
    return T(z), T(y), T(g), ng, rec, ref


def summary_bits(m):
    """A GroupMetrics' doubles as raw bits (NaN-safe equality) and its ints."""
    d = (m.gauc, m.auc_macro, m.mrr) + m.hit_rate + m.recall + m.ndcg
    return struct.pack(f"<{len(d)}d", *d), m[7:16]


def records_bytes(m):
    return {k: v.cpu().numpy().tobytes() for k, v in m.records.items()}


def close(a, b, bound):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return abs(a - b) <= bound


def check_against_reference(m, ref, ks, n_groups, tag=""):
    nk = len(ks)
    kmax = ks[-1] if nk else 0
    assert (m.n, m.n_bad_label, m.n_nan, m.n_bad_group) == (ref["n"], 0, 0, 0)
    assert (m.n_groups_present, m.n_groups_auc, m.n_groups_ranked, m.n_rows_auc) == \
        (ref["n_groups_present"], ref["n_groups_auc"], ref["n_groups_ranked"], ref["n_rows_auc"])
    assert m.hit_groups == ref["hit_groups"]
    ba = (ref["n_groups_auc"] + kmax + 8) * U52
    br = (ref["n_groups_ranked"] + kmax + 8) * U52
    worst = 0.0
    for name, got, want, bound in [("gauc", m.gauc, ref["gauc"], ba),
                                   ("auc_macro", m.auc_macro, ref["auc_macro"], ba),
                                   ("mrr", m.mrr, ref["mrr"], br)] + \
            [(f"{f}@{ks[j]}", getattr(m, f)[j], ref[f][j], br)
             for f in ("hit_rate", "recall", "ndcg") for j in range(nk)]:
        if not math.isnan(want):
            worst = max(worst, abs(got - want) / bound)
        assert close(got, want, bound), (name, got, want, bound)
    print(f"{tag}: gauc={m.gauc!r} mrr={m.mrr!r} ndcg={m.ndcg!r} worst |d| / bound = {worst:.2e}")
    if m.records is None:
        return
    r = {k: v.cpu().numpy() for k, v in m.records.items()}
    gids = ref["gids"]
    for name, want in (("n", ref["n_u"]), ("n_pos", ref["n_pos"]), ("auc_u2", ref["auc_u2"]),
                       ("first_pos_rank", ref["first_pos_rank"])):
        full = np.zeros(n_groups, np.int64)
        full[gids] = want
        assert np.array_equal(r[name], full), name
    full = np.zeros((n_groups, nk), np.int64)
    full[gids] = ref["hits"]
    assert np.array_equal(r["hits"], full)
    fulld = np.zeros((n_groups, nk), np.float64)
    fulld[gids] = ref["dcg"]
    for j in range(nk):
        assert np.all(np.abs(r["dcg"][:, j] - fulld[:, j]) <= (ks[j] + 2) * 2.0 ** -53 * fulld[:, j])


@pytest.mark.parametrize("idx", range(len(gm.CASES)), ids=IDS)
def test_group_metrics_cases(dev, idx):
    """Every case against the host reference (bounds in the module docstring)."""
    import dcnr
    case = gm.CASES[idx]
    z, y, g, ng, rec, ref = on_dev(dev, case)
    m = dcnr.group_metrics(z, y, g, ks=gm.KS, n_groups=ng, per_group=rec)
    assert (m.records is not None) == rec and m.ks == gm.KS
    check_against_reference(m, ref, gm.KS, ng, IDS[idx])


def test_no_cutoffs_and_default_n_groups(dev):
    """n_k = 0: the AUC means and MRR alone; n_groups=None takes max + 1."""
    import dcnr
    case = next(c for c in gm.CASES if c[0] == 3 * gm.UNIT + 3 and c[2] == "mean8" and c[1] == "distinct")
    z, y, g, ng, _, _ = on_dev(dev, case)
    zz, yy, gg = gm.case_with_reference(case)[:3]
    ref = gm.host_reference(zz, yy, gg, ng, ks=())
    m = dcnr.group_metrics(z, y, g, ks=(), n_groups=ng, per_group=True)
    assert m.hit_rate == m.recall == m.ndcg == m.hit_groups == ()
    check_against_reference(m, ref, (), ng, "n_k=0")
    ng2 = int(gg.max()) + 1
    d = dcnr.group_metrics(z, y, g, ks=(3, 7), per_group=True)
    assert d.records["n"].shape[0] == ng2
    check_against_reference(d, gm.host_reference(zz, yy, gg, ng2, ks=(3, 7)), (3, 7), ng2, "default")


def test_closed_forms(dev):
    """All scores equal: AUC_u = 0.5 in every AUC group, so both AUC means are
    exactly 0.5 (sums of halves of integers are exact).  Every positive above
    every negative: gauc, auc_macro, mrr and every hit rate exactly 1.0, the
    first positive first in every ranked group, NDCG 1.0 to the bound (the
    device adds a group's discounts in scan order, ``ideal`` in sequence)."""
    import dcnr
    n = 3 * gm.UNIT + 3
    for case in (c for c in gm.CASES if c[0] == n and c[1] == "equal" and c[2] in ("mean8", "one", "wave64")):
        z, y, g, ng, _, _ = on_dev(dev, case)
        m = dcnr.group_metrics(z, y, g, ks=gm.KS, n_groups=ng)
        assert m.n_groups_auc > 0 and m.gauc == 0.5 and m.auc_macro == 0.5
    zz, yy = mc.make_case((n, "sep_pos", 77))
    gg = np.random.default_rng(78).integers(0, 1500, n).astype(np.int64)
    z, y, g = (torch.from_numpy(a).to(dev) for a in (zz, yy, gg))
    m = dcnr.group_metrics(z, y, g, ks=gm.KS, n_groups=1500, per_group=True)
    assert m.gauc == 1.0 and m.auc_macro == 1.0 and m.mrr == 1.0
    assert m.hit_rate == (1.0,) * 4 and m.recall[-1] == 1.0
    ranked = m.records["n_pos"] > 0
    assert bool((m.records["first_pos_rank"][ranked] == 1).all())
    assert all(abs(v - 1.0) <= (m.n_groups_ranked + gm.KS[-1] + 8) * U52 for v in m.ndcg)


def test_deterministic(dev):
    """Two calls on the same input: bit-identical summaries and records."""
    import dcnr
    n = 3 * gm.UNIT + 3
    for case in (c for c in gm.CASES if (c[0] == n and c[2] in ("huge3", "mean8", "one"))
                 or (c[0] == 65539 and c[2] in ("mean8", "one"))):
        z, y, g, ng, _, _ = on_dev(dev, case)
        a = dcnr.group_metrics(z, y, g, ks=gm.KS, n_groups=ng, per_group=True)
        b = dcnr.group_metrics(z, y, g, ks=gm.KS, n_groups=ng, per_group=True)
        assert summary_bits(a) == summary_bits(b)
        assert records_bytes(a) == records_bytes(b)


def test_one_group_equals_eval_metrics(dev):
    import dcnr
    for case in (c for c in gm.CASES if c[2] == "one" and c[0] >= gm.TILE - 1):
        z, y, g, ng, _, _ = on_dev(dev, case)
        m = dcnr.group_metrics(z, y, g, ks=gm.KS, n_groups=1, per_group=True)
        e = dcnr.eval_metrics(z, y)
        r = {k: v.cpu().numpy() for k, v in m.records.items()}
        assert (int(r["auc_u2"][0]), int(r["n_pos"][0]), int(r["n"][0] - r["n_pos"][0])) == \
            (e.auc_u2, e.n_pos, e.n_neg)
        assert m.auc_macro == e.auc and abs(m.gauc - e.auc) <= 2 * U52


def test_row_permutation(dev):
    """Distinct scores: the records do not depend on the row order.  Equal
    scores: the order is the input's, so first_pos_rank moves as the
    positions say."""
    import dcnr
    n = 3 * gm.UNIT + 3
    case = next(c for c in gm.CASES if c[0] == n and c[1] == "distinct" and c[2] == "mean8")
    z, y, g, ng, _, _ = on_dev(dev, case)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(n)).to(dev)
    a = dcnr.group_metrics(z, y, g, ks=gm.KS, n_groups=ng, per_group=True)
    b = dcnr.group_metrics(z[perm], y[perm], g[perm], ks=gm.KS, n_groups=ng, per_group=True)
    assert records_bytes(a) == records_bytes(b)      # no ties: the same sorted rows, the same walk
    case = next(c for c in gm.CASES if c[0] == n and c[1] == "equal" and c[2] == "mean8")
    z, y, g, ng, _, _ = on_dev(dev, case)
    zz, yy, gg = (t[perm].cpu().numpy() for t in (z, y, g))
    m = dcnr.group_metrics(z[perm], y[perm], g[perm], ks=gm.KS, n_groups=ng, per_group=True)
    fpr = m.records["first_pos_rank"].cpu().numpy()
    want = np.zeros(ng, np.int64)
    seen = np.zeros(ng, np.int64)
    for i in range(n):                       # input order is the rank order
        seen[gg[i]] += 1
        if yy[i] == 1.0 and want[gg[i]] == 0:
            want[gg[i]] = seen[gg[i]]
    assert np.array_equal(fpr, want)
    assert not np.array_equal(fpr, dcnr.group_metrics(z, y, g, ks=gm.KS, n_groups=ng, per_group=True)
                              .records["first_pos_rank"].cpu().numpy())


def test_bad_rows_are_counted_and_stay_in_bounds(dev):
    """NaN logits, labels of 0.5, group ids of -1 and n_groups at the first
    row, the last row and a tile boundary: exact counters, and 4 KiB of a
    known byte either side of the records untouched."""
    import dcnr
    from dcnr import _lib, metrics
    lib = _lib.load()
    case = next(c for c in gm.CASES if c[0] == 3 * gm.UNIT + 3 and c[1] == "distinct" and c[2] == "mean8")
    z, y, g, ng, _, _ = on_dev(dev, case)
    n = z.numel()
    at = [0, gm.TILE - 1, gm.TILE, n - 1]
    zn, yb, gb = z.clone(), y.clone(), g.clone()
    zn[at] = float("nan")
    yb[[0, gm.TILE, n - 1]] = 0.5
    gb[[0, gm.TILE - 1]] = -1
    gb[[gm.TILE, n - 1, 7]] = ng
    gb[9] = (1 << 40) + 3
    for zz, yy, gg, want in ((zn, y, g, (0, 4, 0)), (z, yb, g, (3, 0, 0)), (z, y, gb, (0, 0, 6)),
                             (zn, yb, gb, (3, 4, 6))):
        guard = 4096
        rb = ctypes.sizeof(_lib.GroupRecordStruct)
        buf = torch.full((2 * guard + ng * rb,), 0xA5, dtype=torch.uint8, device=dev)
        out = torch.zeros(ctypes.sizeof(_lib.GroupSummaryStruct), dtype=torch.uint8, device=dev)
        ws = torch.empty(metrics.group_workspace_bytes(n, ng), dtype=torch.uint8, device=dev)
        ks = (ctypes.c_int32 * 4)(*gm.KS)
        disc, ideal = (torch.from_numpy(a).to(dev) for a in gm.dcg_tables(gm.KS[-1]))
        st = lib.dcnr_eval_group_metrics(zz.data_ptr(), yy.data_ptr(), gg.data_ptr(), n, ng, ks, 4,
                                         disc.data_ptr(), ideal.data_ptr(), out.data_ptr(),
                                         buf.data_ptr() + guard, ws.data_ptr(), ws.numel(),
                                         _lib.stream_ptr(dev))
        assert st == _lib.DCNR_OK
        s = _lib.GroupSummaryStruct.from_buffer_copy(out.cpu().numpy().tobytes())
        assert (s.n_bad_label, s.n_nan, s.n_bad_group) == want and s.n == n
        h = buf.cpu().numpy()
        assert np.all(h[:guard] == 0xA5) and np.all(h[-guard:] == 0xA5)
        r = metrics.group_metrics_raw(zz, yy, gg, ks=gm.KS, n_groups=ng, per_group=True)
        assert (r.n_bad_label, r.n_nan, r.n_bad_group) == want
        assert int(r.records["n"].sum()) == n - want[2]      # a row with a bad id is in no group
        with pytest.raises(ValueError):
            dcnr.group_metrics(zz, yy, gg, ks=gm.KS, n_groups=ng)
    with pytest.raises(ValueError):
        dcnr.group_metrics(z, y, g[:-1], ks=gm.KS, n_groups=ng)
    with pytest.raises(ValueError):
        dcnr.group_metrics(z, y, g, ks=(5, 5), n_groups=ng)


def test_workspace_too_small_and_empty(dev):
    from dcnr import _lib, metrics
    lib = _lib.load()
    n, ng = 1000, 10
    z = torch.zeros(n, device=dev)
    g = torch.zeros(n, dtype=torch.int64, device=dev)
    need = metrics.group_workspace_bytes(n, ng)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.zeros(216, dtype=torch.uint8, device=dev)
    ks = (ctypes.c_int32 * 1)(0)
    st = lib.dcnr_eval_group_metrics(z.data_ptr(), z.data_ptr(), g.data_ptr(), n, ng, ks, 0, None, None,
                                     out.data_ptr(), None, ws.data_ptr(), need - 1, _lib.stream_ptr(dev))
    assert st == _lib.DCNR_WORKSPACE_TOO_SMALL
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                      # nothing was enqueued
    # n = 0: a zeroed summary with NaN means, zeroed records, nothing read
    e = metrics.group_metrics_raw(torch.empty(0, device=dev), torch.empty(0, device=dev),
                                  torch.empty(0, dtype=torch.int64, device=dev), ks=(5, 10), n_groups=3,
                                  per_group=True)
    assert e[7:15] == (0,) * 8 and e.hit_groups == (0, 0)
    assert all(math.isnan(v) for v in (e.gauc, e.auc_macro, e.mrr) + e.hit_rate + e.recall + e.ndcg)
    assert int(e.records["n"].abs().sum()) == 0 and e.records["n"].shape[0] == 3


def test_evaluate_ranking(dev):
    """On the small F1 model: its Metrics is evaluate's bit for bit, its
    GroupMetrics that of group_metrics on the logits of a plain forward."""
    import dcnr
    cfg = gc.CFG1
    m = our_model(cfg).to(dev)
    N = 1501
    u, i, c, nn, y = to_dev(dev, *gc.make_inputs(cfg, N, 13))
    u = u % 97                                      # users with several rows each
    collab = torch.stack([u, i], 1)
    m.train()
    em, gmt = dcnr.evaluate_ranking(m, collab, c, nn, y, group_by='user', ks=(1, 5), batch_size=512)
    assert m.training
    m.eval()
    ev = dcnr.evaluate(m, collab, c, nn, y)
    assert struct.pack("<3d", *em[:3]) == struct.pack("<3d", *ev[:3]) and em[3:] == ev[3:]
    with torch.no_grad():
        z = m(u, i, c, nn)
    want = dcnr.group_metrics(z, y, u, ks=(1, 5))
    assert summary_bits(gmt) == summary_bits(want) and gmt.ks == (1, 5)
    assert gmt.n == N and gmt.n_groups_present == 97
    _, by_item = dcnr.evaluate_ranking(m, collab, c, nn, y, group_by='item', ks=(1, 5))
    assert summary_bits(by_item) == summary_bits(dcnr.group_metrics(z, y, i, ks=(1, 5)))
    _, by_t = dcnr.evaluate_ranking(m, collab.cpu(), c.cpu(), nn.cpu(), y.cpu(), group_by=(u % 5).cpu(),
                                    ks=(1, 5))
    assert summary_bits(by_t) == summary_bits(dcnr.group_metrics(z, y, u % 5, ks=(1, 5)))
    with pytest.raises(ValueError):
        dcnr.evaluate_ranking(m, collab, c, nn, y, group_by='hotel')


def test_fit_with_ranking(dev):
    """fit(ranking=...) adds the "ranking" entry and trains exactly as fit
    without it: the weights after two epochs are bit-identical."""
    import dcnr
    cfg = gc.CFG_ODD
    u, i, c, nn, _ = gc.make_inputs(cfg, 1024 + 300, 31)
    y = ((nn[:, 0] + 0.5 * nn[:, 1] + 0.02 * (u % 7)) > 0.8).astype(np.float32)
    u, i, c, nn, y = to_dev(dev, u, i, c, nn, y)
    collab = torch.stack([u, i], 1)
    tr = tuple(t[:1024] for t in (collab, c, nn, y))
    va = tuple(t[1024:] for t in (collab, c, nn, y))
    states, hist = [], []
    for ranking in (None, dict(group_by='user', ks=(1, 3))):
        m = our_model(cfg).to(dev)
        t = dcnr.FusedTrainer(m, lr=3e-3, weight_decay=1e-4)
        torch.manual_seed(9)
        loader = dcnr.DeviceLoader(*tr, batch_size=256, shuffle=True)
        seen = []
        h = t.fit(loader, va, n_epochs=2, on_epoch=lambda e, mm: seen.append(mm) and None,
                  **({} if ranking is None else {"ranking": ranking}))
        assert seen == [e["metrics"] for e in h["epochs"]]
        hist.append(h)
        states.append({k: v.detach().cpu().numpy().tobytes() for k, v in m.state_dict().items()})
        last = m
    assert states[0] == states[1]
    assert all("ranking" not in e for e in hist[0]["epochs"])
    assert [e["metrics"] for e in hist[0]["epochs"]] == [e["metrics"] for e in hist[1]["epochs"]]
    for e in hist[1]["epochs"]:
        assert isinstance(e["ranking"], dcnr.GroupMetrics) and e["ranking"].ks == (1, 3)
        assert e["ranking"].n == 300 and 0.0 <= e["ranking"].gauc <= 1.0
    _, again = dcnr.evaluate_ranking(last, *va, group_by='user', ks=(1, 3))
    assert summary_bits(again) == summary_bits(hist[1]["epochs"][-1]["ranking"])
