"""GPU tests of dcnr_eval_metrics (logloss, exact ROC AUC, RMSE on the
device), ``dcnr.evaluate`` and ``FusedTrainer.fit``.

Bounds (tests/metrics_cases.py holds the cases and the host reference):
  auc_u2, n_pos, n_neg   equal to the host integers
  auc                    bit-equal to U2 / (2.0 * P * N); within n 2^-52 of
                         sklearn's value (the rounding bound of its n-term
                         fp64 trapezoid sum)
  logloss                1e-10 relative to the exactly summed fp64 terms: the
                         device's fixed-order sum rounds by at most
                         (n + 4) 2^-53 < 1e-11 relative at these sizes, its
                         exp / log1p by a few ulps of a term
  rmse                   1e-9 of the host fp64 value (RMSE is 1-Lipschitz in
                         max |dp|; p differs only where the device's fp64 exp
                         moves a sigmoid across an fp32 rounding boundary);
                         2^-22 of sqrt(mean_squared_error(y, torch.sigmoid(z)))
                         with torch's fp32 sigmoid: 2 fp32 ulps of p each way
"""
import math
import struct

import numpy as np
import pytest
import torch

import golden_common as gc
import metrics_cases as mc
from conftest import golden
from helpers import our_model, to_dev

pytestmark = pytest.mark.gpu

IDS = [mc.case_id(c) for c in mc.CASES]


@pytest.fixture(scope="module")
def fx():
    f = golden("f10_metrics.npz")
    assert list(f["names"]) == IDS, "regenerate f10_metrics.npz"
    return {k: f[k] for k in f.files}


def bits(m):
    """The three doubles of a Metrics as raw bits (NaN-safe equality)."""
    return struct.pack("<3d", m.logloss, m.auc, m.rmse), tuple(m[3:])


def on_dev(dev, case):
    z, y, ref = mc.case_with_reference(case)
    return torch.from_numpy(z.copy()).to(dev), torch.from_numpy(y.copy()).to(dev), ref


@pytest.mark.parametrize("idx", range(len(mc.CASES)), ids=IDS)
def test_metrics_cases(dev, fx, idx):
    """Every case against the host integers, the host fp64 values and the
    fixture's sklearn / torch values (bounds in the module docstring).
    Largest |rmse - torch fp32-sigmoid rmse| seen over the cases on an
    MI355X: 4.8e-08 (the bound is 2^-22 = 2.4e-07)."""
    import dcnr
    case = mc.CASES[idx]
    n = case[0]
    z, y, ref = on_dev(dev, case)
    m = dcnr.eval_metrics(z, y)
    d_torch = abs(m.rmse - float(fx["rmse_torch"][idx]))
    print(f"{IDS[idx]}: u2={m.auc_u2} auc={m.auc!r} logloss={m.logloss!r} rmse={m.rmse!r} "
          f"|auc-sk|={abs(m.auc - float(fx['sk_auc'][idx])):.3e} "
          f"logloss_rel={abs(m.logloss - ref['logloss']) / abs(ref['logloss']) if math.isfinite(ref['logloss']) else float('nan'):.3e} "
          f"|rmse-host|={abs(m.rmse - ref['rmse']):.3e} |rmse-torch|={d_torch:.3e}")
    assert (m.n, m.n_bad_label, m.n_nan) == (n, 0, 0)
    assert (m.auc_u2, m.n_pos, m.n_neg) == (ref["u2"], ref["n_pos"], ref["n_neg"])
    assert (m.auc_u2, m.n_pos, m.n_neg) == (int(fx["u2"][idx]), int(fx["n_pos"][idx]), int(fx["n_neg"][idx]))
    assert struct.pack("<d", m.auc) == struct.pack("<d", ref["u2"] / (2.0 * ref["n_pos"] * ref["n_neg"]))
    assert abs(m.auc - float(fx["sk_auc"][idx])) <= n * 2.0 ** -52
    assert mc.same_or_close(m.logloss, ref["logloss"], rel=1e-10)
    assert abs(m.rmse - ref["rmse"]) <= 1e-9
    assert d_torch <= 2.0 ** -22


def test_exact_auc_patterns(dev):
    """All scores equal over several blocks: U2 == P N and AUC exactly 0.5 (one
    tie group spanning every tile); perfectly separated: exactly 1.0 and 0.0."""
    import dcnr
    n = 3 * mc.UNIT + 3
    by = {c[1]: c for c in mc.CASES if c[0] == n}
    z, y, _ = on_dev(dev, by["equal"])
    m = dcnr.eval_metrics(z, y)
    assert m.auc_u2 == m.n_pos * m.n_neg and m.auc == 0.5
    z, y, _ = on_dev(dev, by["sep_pos"])
    assert dcnr.eval_metrics(z, y).auc == 1.0
    z, y, _ = on_dev(dev, by["sep_neg"])
    m = dcnr.eval_metrics(z, y)
    assert m.auc == 0.0 and m.auc_u2 == 0
    # sklearn's argument order, numpy inputs
    z, y, ref = mc.case_with_reference(by["q16"])
    assert dcnr.roc_auc_score(y, z) == ref["auc"]
    assert dcnr.roc_auc_score(torch.from_numpy(y.copy()).to(dev), torch.from_numpy(z.copy())) == ref["auc"]


def test_deterministic_and_second_stream(dev):
    """Two calls give the three doubles bit for bit; so does a call on a
    second stream with a workspace of its own."""
    from dcnr import metrics
    for case in (c for c in mc.CASES if c[0] == 65539 and c[1] in ("distinct", "q16")):
        z, y, _ = on_dev(dev, case)
        a = metrics.eval_metrics_raw(z, y)
        b = metrics.eval_metrics_raw(z, y)
        assert bits(a) == bits(b)
        ws = torch.empty(metrics.workspace_bytes(z.numel()), dtype=torch.uint8, device=dev)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            c = metrics.eval_metrics_raw(z, y, ws=ws)
        torch.cuda.current_stream(dev).wait_stream(s)
        assert bits(a) == bits(c)


def test_workspace_too_small_and_empty(dev):
    from dcnr import _lib, metrics
    lib = _lib.load()
    n = 1000
    z = torch.zeros(n, device=dev)
    y = torch.zeros(n, device=dev)
    need = metrics.workspace_bytes(n)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.zeros(72, dtype=torch.uint8, device=dev)
    st = lib.dcnr_eval_metrics(z.data_ptr(), y.data_ptr(), n, out.data_ptr(), ws.data_ptr(), need - 1,
                               _lib.stream_ptr(dev))
    assert st == _lib.DCNR_WORKSPACE_TOO_SMALL
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                      # nothing was enqueued
    # n = 0: accepted, a zeroed struct with NaN metrics, no input or workspace touched
    st = lib.dcnr_eval_metrics(None, None, 0, out.data_ptr(), None, 0, _lib.stream_ptr(dev))
    assert st == _lib.DCNR_OK
    m = _lib.MetricsStruct.from_buffer_copy(out.cpu().numpy().tobytes())
    assert math.isnan(m.logloss) and math.isnan(m.auc) and math.isnan(m.rmse)
    assert (m.n, m.n_pos, m.n_neg, m.auc_u2, m.n_bad_label, m.n_nan) == (0, 0, 0, 0, 0, 0)
    e = metrics.eval_metrics_raw(torch.empty(0, device=dev), torch.empty(0, device=dev))
    assert e.n == 0 and math.isnan(e.auc)


def test_counters_and_errors(dev):
    """A NaN score, a label of 0.5 and a single class: counted by the native
    call, ValueError from the Python layer (as sklearn raises)."""
    import dcnr
    from dcnr import metrics
    z, y, _ = mc.case_with_reference(next(c for c in mc.CASES if c[0] == 65 and c[1] == "distinct"))
    zt, yt = torch.from_numpy(z.copy()).to(dev), torch.from_numpy(y.copy()).to(dev)
    zn = zt.clone()
    zn[17] = float("nan")
    assert metrics.eval_metrics_raw(zn, yt).n_nan == 1
    with pytest.raises(ValueError):
        dcnr.eval_metrics(zn, yt)
    with pytest.raises(ValueError):
        dcnr.roc_auc_score(yt, zn)
    yb = yt.clone()
    yb[3] = 0.5
    r = metrics.eval_metrics_raw(zt, yb)
    assert r.n_bad_label == 1 and r.n_nan == 0
    with pytest.raises(ValueError):
        dcnr.eval_metrics(zt, yb)
    for v in (0.0, 1.0):
        with pytest.raises(ValueError):
            dcnr.eval_metrics(zt, torch.full_like(yt, v))
    with pytest.raises(ValueError):
        dcnr.eval_metrics(zt, yt[:-1])
    assert metrics.eval_metrics_raw(zt, torch.full_like(yt, -0.0)).n_bad_label == 0   # -0.0 == 0.0


def test_evaluate_odd_config(dev):
    """evaluate() on the odd-shaped config in chunks that do not divide the
    split == one eval forward + eval_metrics, bit for bit; the fp64 logloss
    rounds to dcnr.ops.bce_with_logits' fp32 loss within 1e-6 relative; the
    model's mode is restored."""
    import dcnr
    cfg = gc.CFG_ODD
    m = our_model(cfg).to(dev)
    N = 301
    u, i, c, n, y = to_dev(dev, *gc.make_inputs(cfg, N, 11))
    collab = torch.stack([u, i], 1)
    m.train()
    got = dcnr.evaluate(m, collab, c, n, y, batch_size=128)
    assert m.training
    m.eval()
    whole = dcnr.evaluate(m, collab, c, n, y)
    assert not m.training
    with torch.no_grad():
        z = m(u, i, c, n)
    one = dcnr.eval_metrics(z, y)
    assert bits(got) == bits(one) == bits(whole)
    # host tensors, as the reference holds its validation split (train.py:230-231)
    assert bits(dcnr.evaluate(m, collab.cpu(), c.cpu(), n.cpu(), y.cpu(), batch_size=128)) == bits(one)
    loss, _ = dcnr.bce_with_logits(z, y, want_grad=False)
    assert abs(float(np.float32(one.logloss)) - float(loss)) <= 1e-6 * abs(float(loss))
    assert one.n == N and 0.0 <= one.auc <= 1.0


def _fit_data(dev, seed, n_train=1024, n_val=300):
    cfg = gc.CFG_ODD
    u, i, c, n, _ = gc.make_inputs(cfg, n_train + n_val, seed)
    y = ((n[:, 0] + 0.5 * n[:, 1] + 0.02 * (u % 7)) > 0.8).astype(np.float32)   # learnable
    u, i, c, n, y = to_dev(dev, u, i, c, n, y)
    collab = torch.stack([u, i], 1)
    tr = tuple(t[:n_train] for t in (collab, c, n, y))
    va = tuple(t[n_train:] for t in (collab, c, n, y))
    return cfg, tr, va


def test_fit_history_schedule_checkpoint(dev, tmp_path):
    """4 epochs at B = 256: one history entry per epoch, the recorded rates
    are PlateauLR replayed on the recorded losses, and the checkpoint
    reproduces the best epoch's metrics bit for bit."""
    import dcnr
    cfg, tr, va = _fit_data(dev, 21)
    m = our_model(cfg).to(dev)
    t = dcnr.FusedTrainer(m, lr=3e-3, weight_decay=1e-4)
    torch.manual_seed(9)
    loader = dcnr.DeviceLoader(*tr, batch_size=256, shuffle=True)
    path = tmp_path / "best.pth"
    seen = []
    h = t.fit(loader, va, n_epochs=4, patience=5, lr_scheduler_patience=0, lr_scheduler_factor=0.5,
              checkpoint_path=path, on_epoch=lambda e, mm: seen.append((e, mm)) and None)
    ep = h["epochs"]
    assert [e["epoch"] for e in ep] == [0, 1, 2, 3] and not h["stopped_early"]
    assert seen == [(e["epoch"], e["metrics"]) for e in ep]
    assert t.step_count == 4 * len(loader)
    replay = dcnr.PlateauLR(3e-3, patience=0, factor=0.5)
    assert [e["lr"] for e in ep] == [replay.step(e["metrics"].logloss) for e in ep]
    assert t.lr == ep[-1]["lr"]
    losses = [e["metrics"].logloss for e in ep]
    best = min(range(4), key=lambda k: (losses[k], k))
    assert h["best_epoch"] == best and h["best_val_loss"] == losses[best]
    assert all(e["metrics"].n == va[0].shape[0] for e in ep)
    m.load_state_dict(torch.load(path, weights_only=True))
    again = dcnr.evaluate(m, *va)
    assert bits(again) == bits(ep[best]["metrics"])
    # on_epoch's truthy return stops the loop
    h2 = t.fit(loader, va, n_epochs=3, on_epoch=lambda e, mm: True)
    assert len(h2["epochs"]) == 1 and not h2["stopped_early"]


def test_fit_stops_early_on_shuffled_labels(dev):
    """Validation labels that carry no signal: the validation loss stops
    improving once the model grows confident, and patience=1 ends the run."""
    import dcnr
    cfg, tr, va = _fit_data(dev, 22)
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(va[3].shape[0], generator=g).to(dev)
    va = va[:3] + (va[3][perm],)
    m = our_model(cfg).to(dev)
    t = dcnr.FusedTrainer(m, lr=1e-2, weight_decay=0.0)
    torch.manual_seed(10)
    loader = dcnr.DeviceLoader(*tr, batch_size=256, shuffle=True)
    h = t.fit(loader, va, n_epochs=40, patience=1)
    assert h["stopped_early"] and len(h["epochs"]) < 40
    losses = [e["metrics"].logloss for e in h["epochs"]]
    assert losses[-1] >= min(losses[:-1])
