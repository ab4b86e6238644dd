"""Host side of the batched request path (dcnr_requests_*): the symbols are
bound with the header's signatures, the workspace size query behaves, and every
argument error is rejected with its status before any launch (no device is
needed: a rejected call touches neither a pointer nor the stream)."""
import ctypes

import pytest

from dcnr import _lib

NAMES = ["dcnr_requests_workspace_size", "dcnr_requests_candidates",
         "dcnr_requests_ranking_batch", "dcnr_requests_rank_mmr"]
SV_MAX = 4096


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_present(lib):
    assert set(NAMES) <= set(_lib.exported_symbols())
    for n in NAMES:
        assert getattr(lib, n) is not None
    assert lib.dcnr_abi_version() == 4   # added symbols only


def test_workspace_size(lib):
    size = lib.dcnr_requests_workspace_size
    assert size(0, 0, 11, 64) == 0
    one, many = size(1, 32, 11, 352), size(300, 9600, 11, 352)
    assert 12 * 352 <= one <= 12 * 352 + 1024
    assert 12 * 300 * 352 <= many <= 12 * 300 * 352 + 1024
    by_r = [size(R, 0, 11, 352) for R in (1, 2, 37, 300, 4096)]
    by_cap = [size(300, 0, 11, cap) for cap in (1, 2, 352, 4095, SV_MAX)]
    assert by_r == sorted(by_r) and len(set(by_r)) == len(by_r)
    assert by_cap == sorted(by_cap) and len(set(by_cap)) == len(by_cap)
    # arguments the calls reject have no size
    assert size(-1, 0, 11, 64) == size(1, -1, 11, 64) == size(1, 0, 0, 64) == 0
    assert size(1, 0, 11, 0) == size(1, 0, 11, SV_MAX + 1) == 0


# a non-null stand-in for device pointers: rejected calls never dereference it
P = ctypes.addressof(ctypes.create_string_buffer(64))


def cand(lib, R=2, Q=4, k=11, S=1, n_set_rows=8, n_items=100, cap=64, **null):
    a = dict(positives=P, pos_offsets=P, knn_idx=P, set_rows=P, set_offsets=P, allowed=P,
             excluded=P, fallback=P, out_rows=P, out_count=P, status=P, offsets=P, host_offsets=P,
             host_status=P)
    a.update(null)
    return lib.dcnr_requests_candidates(a["positives"], a["pos_offsets"], R, Q, a["knn_idx"], k,
                                        a["set_rows"], n_set_rows, a["set_offsets"], S,
                                        a["allowed"], a["excluded"], a["fallback"], 20, n_items,
                                        cap, a["out_rows"], a["out_count"], a["status"],
                                        a["offsets"], a["host_offsets"], a["host_status"], None)


def batch(lib, R=2, n=10, cap=64, n_items=100, **null):
    a = dict(cand_rows=P, offsets=P, user_rows=P, item_cat=P, item_num=P, user_ids=P, item_ids=P,
             cat=P, num=P)
    a.update(null)
    return lib.dcnr_requests_ranking_batch(a["cand_rows"], cap, a["offsets"], R, n,
                                           a["user_rows"], a["item_cat"], 3, a["item_num"], 4,
                                           n_items, a["user_ids"], a["item_ids"], a["cat"],
                                           a["num"], None)


def rank(lib, R=2, n=10, cap=64, d=32, n_items=100, ws_bytes=1 << 20, **null):
    a = dict(logits=P, cand_rows=P, offsets=P, table=P, inv=P, lam=P, top_k=P, out_rows=P,
             out_logits=P, out_count=P, status=P, ws=P)
    a.update(null)
    return lib.dcnr_requests_rank_mmr(a["logits"], n, a["cand_rows"], cap, a["offsets"], R,
                                      a["table"], a["inv"], d, n_items, a["lam"], a["top_k"],
                                      a["out_rows"], a["out_logits"], a["out_count"],
                                      a["status"], a["ws"], ws_bytes, None)


def test_bad_arguments_are_rejected_before_any_launch(lib):
    BAD = _lib.DCNR_BAD_ARG
    for call in (cand, batch, rank):
        assert call(lib, R=-1) == BAD
        assert call(lib, cap=0) == BAD and call(lib, cap=SV_MAX + 1) == BAD
        assert b"cap" in lib.dcnr_last_error()
    assert cand(lib, k=0) == BAD and cand(lib, Q=-1) == BAD and cand(lib, S=-1) == BAD
    assert cand(lib, n_set_rows=-1) == BAD and cand(lib, n_items=0) == BAD
    for name in ("pos_offsets", "positives", "knn_idx", "set_rows", "set_offsets", "out_rows",
                 "out_count", "status", "offsets"):
        assert cand(lib, **{name: None}) == BAD, name
    assert cand(lib, S=0, n_set_rows=0) == BAD          # set indices without sets
    assert rank(lib, d=0) == BAD and rank(lib, d=257) == BAD
    assert rank(lib, n=-1) == BAD and rank(lib, n=2 * 64 + 1) == BAD
    for name in ("logits", "cand_rows", "offsets", "table", "inv", "lam", "top_k", "out_rows",
                 "out_logits", "out_count", "status", "ws"):
        assert rank(lib, **{name: None}) == BAD, name
    assert batch(lib, n=-1) == BAD and batch(lib, n=2 * 64 + 1) == BAD
    for name in ("cand_rows", "offsets", "user_rows", "item_cat", "item_num", "user_ids",
                 "item_ids", "cat", "num"):
        assert batch(lib, **{name: None}) == BAD, name


def test_unsupported_shapes_and_small_workspace(lib):
    UNS = _lib.DCNR_UNSUPPORTED_SHAPE
    for call in (cand, batch, rank):
        assert call(lib, R=(1 << 22) + 1) == UNS
    assert cand(lib, k=65) == UNS
    assert cand(lib, n_set_rows=1 << 31) == UNS
    need = lib.dcnr_requests_workspace_size(2, 0, 11, 64)
    assert rank(lib, ws_bytes=need - 1) == _lib.DCNR_WORKSPACE_TOO_SMALL
    assert b"workspace" in lib.dcnr_last_error()


def test_no_requests_is_ok_without_pointers(lib):
    assert lib.dcnr_requests_candidates(None, None, 0, 0, None, 11, None, 0, None, 0, None, None,
                                        None, 20, 100, 64, None, None, None, None, None,
                                        None, None) == _lib.DCNR_OK
    assert lib.dcnr_requests_ranking_batch(None, 64, None, 0, 0, None, None, 0, None, 0, 100,
                                           None, None, None, None, None) == _lib.DCNR_OK
    assert lib.dcnr_requests_rank_mmr(None, 0, None, 64, None, 0, None, None, 32, 100, None, None,
                                      None, None, None, None, None, 0, None) == _lib.DCNR_OK
