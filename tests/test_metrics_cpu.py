"""CPU tests of the validation-metric feature: the host reference of
tests/metrics_cases.py reproduces the values the reference's own calls gave
(tests/golden/f10_metrics.npz, from sklearn and torch), and ``PlateauLR``
gives torch's ``ReduceLROnPlateau`` learning-rate sequence."""
import math

import numpy as np
import pytest
import torch

import metrics_cases as mc
from conftest import golden


@pytest.fixture(scope="module")
def fx():
    f = golden("f10_metrics.npz")
    assert list(f["names"]) == [mc.case_id(c) for c in mc.CASES], "regenerate f10_metrics.npz"
    return {k: f[k] for k in f.files}


@pytest.mark.parametrize("idx", range(len(mc.CASES)), ids=[mc.case_id(c) for c in mc.CASES])
def test_host_reference_reproduces_fixture(fx, idx):
    """U2, P, N are the fixture's integers; U2 / (2PN) is sklearn's AUC within
    n 2^-52 (the rounding bound of its n-term fp64 trapezoid sum); logloss is
    torch's fp64 BCEWithLogitsLoss within 1e-10 relative and RMSE the
    torch-fp32-sigmoid value within 2^-22 (2 fp32 ulps of p each way; RMSE is
    1-Lipschitz in max |dp|)."""
    case = mc.CASES[idx]
    n = case[0]
    _, _, ref = mc.case_with_reference(case)
    assert (ref["u2"], ref["n_pos"], ref["n_neg"]) == (int(fx["u2"][idx]), int(fx["n_pos"][idx]),
                                                       int(fx["n_neg"][idx]))
    assert abs(ref["auc"] - float(fx["sk_auc"][idx])) <= n * 2.0 ** -52
    assert mc.same_or_close(ref["logloss"], float(fx["bce_torch"][idx]), rel=1e-10)
    assert abs(ref["rmse"] - float(fx["rmse_torch"][idx])) <= 2.0 ** -22


def test_exact_patterns():
    """The closed forms the patterns were chosen for."""
    by = {mc.case_id(c): mc.case_with_reference(c)[2] for c in mc.CASES if c[0] == 3 * mc.UNIT + 3}
    n = 3 * mc.UNIT + 3
    eq = by[f"equal-{n}"]
    assert eq["u2"] == eq["n_pos"] * eq["n_neg"] and eq["auc"] == 0.5
    assert by[f"sep_pos-{n}"]["auc"] == 1.0 and by[f"sep_neg-{n}"]["auc"] == 0.0
    assert by[f"one_pos-{n}"]["n_pos"] == 1 and by[f"one_neg-{n}"]["n_neg"] == 1
    # -0.0 ties with +0.0; infinities and denormals are ordinary values
    z = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45], np.float32)
    y = np.array([1, 0, 0, 1, 1, 0], np.float32)
    # positives: +0 (negs below: -1e-45; tied: -0) -> 3, -inf -> 0, 1e-45 (below: -0, -1e-45) -> 4
    assert mc.exact_u2(z, y) == (7, 3, 3)


def _torch_lrs(losses, lr, patience, factor):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=lr)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, 'min', patience=patience, factor=factor)
    out = []
    for v in losses:
        sch.step(v)
        out.append(opt.param_groups[0]["lr"])
    return out


SEQS = {
    "strict_improvement": [1.0 - 0.05 * i for i in range(12)],
    # improvements below the relative threshold 1e-4 count as none
    "below_threshold": [1.0] + [1.0 - 2e-5 * i for i in range(1, 12)],
    "at_threshold": [1.0, 1.0 - 1e-4, 1.0 - 2.0001e-4, 0.9997, 0.9997, 0.9997, 0.9997],
    # plateaus of exactly `patience` bad epochs (no cut), then patience + 1 (cut)
    "plateau_patience": [1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.4, 0.4, 0.4, 0.3],
    "several_reductions": [1.0] * 14,
    "worse_then_better": [1.0, 2.0, 3.0, 0.5, 0.6, 0.7, 0.8, 0.1, 0.2, 0.3, 0.4, 0.5],
}


@pytest.mark.parametrize("name", sorted(SEQS))
@pytest.mark.parametrize("patience,factor", [(0, 0.5), (1, 0.1), (2, 0.3), (3, 0.5)])
def test_plateau_lr_is_torchs(name, patience, factor):
    from dcnr.train import PlateauLR
    losses = SEQS[name]
    ours = PlateauLR(1e-3, patience=patience, factor=factor)
    got = [ours.step(v) for v in losses]
    assert got == _torch_lrs(losses, 1e-3, patience, factor)


def test_plateau_lr_reduction_smaller_than_eps():
    """A cut that would change the rate by no more than eps = 1e-8 is not
    applied (torch's _reduce_lr), so the rate stops falling."""
    from dcnr.train import PlateauLR
    losses = [1.0] * 40
    for lr, factor in [(1.5e-8, 0.5), (1e-6, 0.1), (1e-3, 0.1)]:
        ours = PlateauLR(lr, patience=1, factor=factor)
        got = [ours.step(v) for v in losses]
        want = _torch_lrs(losses, lr, 1, factor)
        assert got == want
    assert got[-1] == got[-5] and got[-1] > 0.0   # floor reached: cuts below eps are dropped


def test_plateau_lr_nan_and_args():
    from dcnr.train import PlateauLR
    with pytest.raises(ValueError):
        PlateauLR(1e-3, patience=1, factor=1.0)
    losses = [1.0, float("nan"), float("nan"), float("nan"), 0.5]
    ours = PlateauLR(1e-2, patience=1, factor=0.5)
    assert [ours.step(v) for v in losses] == _torch_lrs(losses, 1e-2, 1, 0.5)


def test_symbols_bound_and_host_argument_checks():
    """The two new entry points are bound with the header's signatures, and
    the struct mirrors dcnr_metrics (9 eight-byte fields)."""
    import ctypes
    from dcnr import _lib
    assert ctypes.sizeof(_lib.MetricsStruct) == 72
    lib = _lib.load()
    assert lib.dcnr_eval_metrics_workspace_size(0) == 0
    sizes = [lib.dcnr_eval_metrics_workspace_size(n) for n in (1, 2, 4096, 4097, 1 << 20, (1 << 31) - 1)]
    assert all(a > 0 for a in sizes) and sizes == sorted(sizes)
    assert sizes[0] >= 16 and sizes[4] >= 16 << 20
    # host-side argument checks (no device needed): negative n, n >= 2^31, null out
    buf = ctypes.create_string_buffer(72)
    for n in (-1, 1 << 31):
        assert lib.dcnr_eval_metrics(None, None, n, ctypes.addressof(buf), None, 0, None) == _lib.DCNR_BAD_ARG
    assert lib.dcnr_eval_metrics(None, None, 0, None, None, 0, None) == _lib.DCNR_BAD_ARG
    assert math.isfinite(float(sizes[-1]))
