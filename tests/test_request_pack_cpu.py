"""F14: the host half of the batched request path, ``dcnr.requests.pack_requests``,
needs no device and packs byte for byte what ``RankingPipeline._pack_requests``
packed before it (tests/golden/f14_request_pack.npz, recorded from that
method by tests/golden/make_request_pack_golden.py; the requests are
tests/golden/request_pack_cases.py's)."""
import numpy as np
import pytest

import request_pack_cases as rc
from conftest import golden
from dcnr.requests import pack_requests


def pack(q):
    city = None if q["cities"] is None else (rc.CITY_OFF, rc.N_CITIES,
                                             np.asarray(q["cities"], np.int64), q["in_city"])
    return pack_requests(q["users"], q["positive_rows"], q["lambda_param"], q["top_k"],
                         q["allowed"], q["excluded"], q["fallback"], q["neighbors_within"],
                         n_users=rc.N_USERS, n_rows=rc.N_ROWS, k=rc.K, reg_off=rc.REG_OFF, city=city)


@pytest.fixture(scope="module")
def recorded():
    """case -> ([(name, dtype, bytes)] of the upload in order, meta)"""
    g = golden("f14_request_pack.npz")
    upload, at, out = g["upload"], 0, {c: ([], m) for c, m in zip(g["cases"], g["meta"])}
    for line in g["layout"]:
        case, name, dtype, count = str(line).split()
        nbytes = int(count) * np.dtype(dtype).itemsize
        out[case][0].append((name, dtype, upload[at:at + nbytes].tobytes()))
        at += nbytes
    assert at == upload.size
    return out


def test_cases_cover_what_the_golden_holds(recorded):
    assert list(recorded) == list(rc.cases())
    sizes = {q["users"].size for q in rc.cases().values()}
    assert sizes == {1, 6}


@pytest.mark.parametrize("case", list(rc.cases()))
def test_upload_is_the_parent_packers(recorded, case):
    want, meta = recorded[case]
    p = pack(rc.cases()[case])
    got = [(name, a.dtype.name, np.ascontiguousarray(a).tobytes()) for name, a in p.arrays.items()]
    assert [g[:2] for g in got] == [w[:2] for w in want]   # names, order, dtypes
    for g, w in zip(got, want):
        assert g[2] == w[2], g[0]
    longest = -1 if p.within_longest is None else p.within_longest
    any_global = -1 if p.within_any_global is None else int(p.within_any_global)
    assert [p.cap, p.S, p.n_adhoc, longest, any_global] == meta.tolist()
    assert (p.within_idx is None) == ("within" not in p.arrays)


def test_named_fields_are_the_uploaded_arrays():
    q = rc.cases()["r6_sets"]
    p = pack(q)
    for name in ("pos", "pos_off", "lam", "topk"):
        assert getattr(p, name) is p.arrays[name]
    assert p.within_idx is p.arrays["within"]
    assert p.lam64.dtype == np.float64 and p.lam64.tolist() == q["lambda_param"]
    # the lambda that is below 1 as a double and 1.0f as the kernels' float32
    assert p.odd.tolist() == [False, False, True, False, False, False]
    assert pack(rc.cases()["r1_odd_lambda"]).odd.tolist() == [True]
    assert not pack(rc.cases()["r6_scalars"]).odd.any()


def test_all_none_lists_upload_nothing_about_sets():
    for case in ("r1_all_none", "r6_all_none"):
        p = pack(rc.cases()[case])
        assert list(p.arrays) == ["pos", "pos_off", "users", "lam", "topk"]
        assert (p.S, p.n_adhoc, p.within_idx) == (0, 0, None)


@pytest.mark.parametrize("name", list(rc.errors()))
def test_value_errors_keep_their_text(name):
    q, text = rc.errors()[name]
    with pytest.raises(ValueError) as e:
        pack(q)
    assert str(e.value) == text
