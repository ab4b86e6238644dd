"""Host side of DCNR_FLAG_HEAD_STATS / dcnr_forward_bce (no device): the flag
moves no byte of the workspace, the entry point is declared, exported and
bound, and a trainer over a model the fused head pass does not cover is built
as before."""
import os
import re

import pytest
import torch

from conftest import ROOT


def _model(hidden, precision, n_res=2):
    import dcnr
    torch.manual_seed(0)
    return dcnr.DCN_RecSys(64, 48, {"a": 7, "b": 5}, 3,
                           dict(emb_dim=8, hidden_dim=hidden, n_cross_layers=3, n_res_blocks=n_res,
                                dropout=0.6), precision=precision)


@pytest.mark.parametrize("hidden,precision", [(512, "bf16"), (505, "bf16"), (64, "bf16"), (512, "fp32")])
def test_flag_keeps_the_workspace_layout(hidden, precision):
    from dcnr import _lib
    m = _model(hidden, precision)
    F = _lib.FLAG_HEAD_STATS
    assert F == 16
    for B in (2, 33, 1000, 4099, 131072):
        for extra in (0, _lib.FLAG_ROW_MAP, _lib.FLAG_KEEP_INTERMEDIATES):
            for mode in (_lib.TRAIN, _lib.EVAL):
                assert m.workspace_bytes(B, mode, extra) == m.workspace_bytes(B, mode, extra | F)
            for kind in _lib.WS_KINDS:
                for idx in range(4):
                    assert m.workspace_offset(B, _lib.TRAIN, kind, idx, extra_flags=extra) == \
                        m.workspace_offset(B, _lib.TRAIN, kind, idx, extra_flags=extra | F), (kind, idx)


def test_entry_point_declared_exported_bound():
    from dcnr import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "dcnr.h")).read()
    assert re.search(r"\bdcnr_forward_bce\s*\(", txt)
    assert re.search(r"#define\s+DCNR_FLAG_HEAD_STATS\s+16u", txt)
    assert "dcnr_forward_bce" in _lib.exported_symbols()
    assert hasattr(lib, "dcnr_forward_bce")
    assert lib.dcnr_abi_version() == 4


def test_bad_arguments_are_refused():
    """Null loss operands are refused before anything is enqueued."""
    import ctypes
    from dcnr import _lib
    lib = _lib.load()
    m = _model(512, "bf16")
    desc = m.desc(extra_flags=_lib.FLAG_HEAD_STATS)
    st = lib.dcnr_forward_bce(ctypes.byref(desc), None, None, None, None, None, 8, 0, None, 1.0,
                              None, None, None, None, 0, None, 0, None)
    assert st == _lib.DCNR_BAD_ARG


@pytest.mark.parametrize("hidden,precision", [(16, "fp32"), (64, "bf16")])
def test_trainer_on_a_cpu_model(hidden, precision):
    """The switch is a constructor argument; the native plan, not the trainer,
    decides where the fused head pass applies, so a trainer over a CPU model
    (the exchange tests' kind) is built with either setting, and a step on it
    fails for the reason it always did: there is no CPU path."""
    import dcnr
    from dcnr import _lib
    for on in (True, False):
        tr = dcnr.FusedTrainer(_model(hidden, precision, n_res=1), head_stats=on)
        assert tr.head_stats == on
        assert bool(tr._flags & _lib.FLAG_HEAD_STATS) == on
        z = torch.zeros(4, dtype=torch.int64)
        with pytest.raises(RuntimeError, match="HIP device only"):
            tr.step(z, z, torch.zeros(4, 2, dtype=torch.int64), torch.zeros(4, 3), torch.zeros(4))
