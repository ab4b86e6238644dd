"""Host side of the set-scoped search (dcnr_cosine_topk_within): the symbols
are bound with the header's signatures, the size query behaves, every argument
error comes back with its status before any launch (no device is needed: a
rejected call touches neither a pointer nor the stream), and the Python
wrappers' own checks raise before they reach the device."""
import ctypes

import numpy as np
import pytest
import torch

from dcnr import _lib

NAMES = ["dcnr_cosine_topk_within_workspace_size", "dcnr_cosine_topk_within"]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_present(lib):
    assert set(NAMES) <= set(_lib.exported_symbols())
    for n in NAMES:
        assert getattr(lib, n) is not None
    assert lib.dcnr_abi_version() == 4   # added symbols only


def test_workspace_size(lib):
    size = lib.dcnr_cosine_topk_within_workspace_size
    # empty shapes: finite, no division by zero
    assert 0 < size(0, 10, 64, 0) <= 4096 and 0 < size(0, 10, 64, 2000) <= 4096
    assert 0 < size(8, 10, 64, 0) < 1 << 20
    by_q = [size(Q, 10, 64, 2000) for Q in (0, 1, 8, 9, 256, 2048, 100_000)]
    by_rows = [size(256, 10, 64, m) for m in (0, 1, 1024, 1025, 20_000, 1_000_000, (1 << 31) - 1)]
    assert by_q == sorted(by_q) and by_rows == sorted(by_rows)
    assert len(set(by_q)) == len(by_q)
    # queries + records + one k-list per chunk of 1024 rows at the least
    assert size(256, 10, 64, 2000) >= 256 * (64 * 4 + 16 + 2 * 10 * 8)
    # the chunk count is bounded: the whole-table set costs at most 256 lists per query
    assert size(256, 10, 64, 1_000_000) <= 256 * (64 * 4 + 16 + 256 * 10 * 8) + 4096
    # arguments the call rejects have no size
    assert size(-1, 10, 64, 100) == size(1, 0, 64, 100) == size(1, 65, 64, 100) == 0
    assert size(1, 10, 0, 100) == size(1, 10, 6, 100) == size(1, 10, 260, 100) == 0
    assert size(1, 10, 64, -1) == size(1, 10, 64, 1 << 31) == 0


# a non-null stand-in for device pointers: rejected calls never dereference it
P = ctypes.addressof(ctypes.create_string_buffer(64))


def call(lib, N=1000, d=64, Q=16, G=2, n_set_rows=100, S=3, max_set_rows=50, k=10, ld=None,
         ws_bytes=1 << 30, **ptr):
    a = dict(table=P, inv=P, queries=P, exclude=P, seg_offsets=P, seg_set=P, set_rows=P, set_offsets=P,
             idx=P, dist=P, seg_status=P, ws=P)
    a.update(ptr)
    return lib.dcnr_cosine_topk_within(a["table"], a["inv"], N, d, a["queries"], Q, a["exclude"],
                                       a["seg_offsets"], G, a["seg_set"], a["set_rows"], n_set_rows,
                                       a["set_offsets"], S, max_set_rows, k, k if ld is None else ld,
                                       a["idx"], a["dist"], a["seg_status"], a["ws"], ws_bytes, None)


def test_bad_arguments_are_rejected_before_any_launch(lib):
    BAD = _lib.DCNR_BAD_ARG
    assert call(lib, Q=-1) == BAD and call(lib, G=-1) == BAD and call(lib, S=-1) == BAD
    assert call(lib, k=0) == BAD and call(lib, k=-3) == BAD
    assert call(lib, ld=9) == BAD and call(lib, ld=0) == BAD
    assert b"ld" in lib.dcnr_last_error()
    assert call(lib, n_set_rows=-1) == BAD and call(lib, max_set_rows=-1) == BAD and call(lib, N=0) == BAD
    for name in ("table", "inv", "queries", "seg_offsets", "seg_set", "set_rows", "set_offsets", "idx",
                 "dist", "ws"):
        assert call(lib, **{name: None}) == BAD, name
    assert b"null" in lib.dcnr_last_error()


def test_unsupported_shapes_and_small_workspace(lib):
    UNS = _lib.DCNR_UNSUPPORTED_SHAPE
    assert call(lib, k=65, ld=65) == UNS
    assert call(lib, d=6) == UNS and call(lib, d=0) == UNS and call(lib, d=260) == UNS
    assert call(lib, N=1 << 31) == UNS and call(lib, n_set_rows=1 << 31) == UNS
    need = lib.dcnr_cosine_topk_within_workspace_size(16, 10, 64, 50)
    assert call(lib, ws_bytes=need - 1) == _lib.DCNR_WORKSPACE_TOO_SMALL
    assert b"workspace" in lib.dcnr_last_error()


def test_nothing_to_do_is_ok_without_pointers(lib):
    none = dict(queries=None, exclude=None, seg_offsets=None, seg_set=None, set_rows=None,
                set_offsets=None, idx=None, dist=None, seg_status=None, ws=None)
    assert call(lib, Q=0, G=0, S=0, n_set_rows=0, max_set_rows=0, ws_bytes=0, **none) == _lib.DCNR_OK
    assert call(lib, Q=0, ws_bytes=0) == _lib.DCNR_OK
    # queries that no segment holds: nothing is written, nothing launched
    assert call(lib, G=0, ws_bytes=0) == _lib.DCNR_OK
    # the optional pointers
    assert call(lib, exclude=None, seg_status=None, ws_bytes=0) == _lib.DCNR_WORKSPACE_TOO_SMALL


def test_python_wrappers_reject_on_the_host():
    import dcnr
    nn = dcnr.NearestNeighbors(n_neighbors=5)
    with pytest.raises(RuntimeError):
        nn.kneighbors(np.zeros((1, 4), np.float32), within=[0])
    with pytest.raises(RuntimeError):
        nn.kneighbors_within_device(torch.zeros(1, 4), 3, None, None, None, None, 0)
    nn._table = torch.zeros(10, 4)   # (fit needs the device; the row checks do not)
    nn.device = torch.device("cpu")
    for rows in ([0, 10], [-1, 3], [[2, 11]]):
        with pytest.raises(ValueError, match="outside the index"):
            nn.kneighbors(np.zeros((1, 4), np.float32), within=rows)
    assert nn._within_rows([7, 2, 7, 0]).tolist() == [0, 2, 7]
    i64 = lambda *a: torch.tensor(a, dtype=torch.int64)
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32)
    q = torch.zeros(2, 4)
    good = dict(set_rows=i64(1, 2), set_offsets=i64(0, 2), seg_offsets=i64(0, 2), seg_set=i32(0),
                max_set_rows=2)
    for bad in (dict(k=0), dict(k=65), dict(set_rows=i32(1, 2)), dict(seg_set=i64(0)),
                dict(seg_offsets=i64(0, 1, 2)), dict(exclude=i64(1)), dict(seg_status=i32(0, 0)),
                dict(out=(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 2))),
                dict(out=(torch.zeros(2, 4, dtype=torch.int64)[:, :3], torch.zeros(2, 3))),
                dict(out=(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3)))):
        a = dict(good, k=3)
        a.update(bad)
        with pytest.raises(ValueError):
            nn.kneighbors_within_device(q, **a)
