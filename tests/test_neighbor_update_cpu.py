"""The neighbour-table update's host side: the C ABI's new symbols, the
checks they make before anything is launched (no device here), and the numpy
restatement of the update rule (neighbor_update_rule.apply_rule) against a
brute-force rebuild -- the restatement is the GPU tests' oracle for the
device's counts, so it is checked where it can be checked exactly: with one
distance function on both sides, the updated table must equal the rebuilt one.
"""
import os
import re

import numpy as np
import pytest

import neighbor_update_rule as rule
from conftest import ROOT

OK, BAD_ARG, UNSUPPORTED_SHAPE, WORKSPACE_TOO_SMALL = 0, 1, 4, 5       # dcnr_status
NEW_SYMBOLS = ["dcnr_cosine_neighbor_table_update_workspace_size", "dcnr_cosine_neighbor_table_update",
               "dcnr_cosine_neighbor_table_rows"]
SHAPES = [(32, 11), (64, 11), (16, 11), (24, 11), (128, 11), (64, 32), (64, 51)]


def test_new_symbols_declared_and_exported():
    from dcnr import _lib
    with open(os.path.join(ROOT, "include", "dcnr.h")) as fh:
        header = fh.read()
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), f"{s} is not declared in include/dcnr.h"
        assert hasattr(lib, s), f"libdcnr.so does not export {s}"
        assert s in _lib.exported_symbols()
    assert lib.dcnr_abi_version() == 4
    import dcnr
    assert callable(dcnr.NearestNeighbors.update_rows)
    assert callable(dcnr.RankingPipeline.update_item_embeddings)


class Call:
    """dcnr_cosine_neighbor_table_update with made-up non-null pointers: every
    case here is answered on the host, before any of them is read."""

    def __init__(self, N=5003, d=64, k=11):
        from dcnr import _lib
        self.lib = _lib.load()
        self.N, self.d, self.k = N, d, k
        self.keep = np.zeros(64, np.int64)          # something non-null to point at
        self.p = self.keep.ctypes.data

    def size(self, m, **kw):
        a = dict(N=self.N, d=self.d, k=self.k)
        a.update(kw)
        return int(self.lib.dcnr_cosine_neighbor_table_update_workspace_size(a["N"], a["d"], a["k"], m))

    def update(self, ch_rows, m=None, nbytes=None, **null):
        ch = np.ascontiguousarray(ch_rows, dtype=np.int32)
        m = ch.size if m is None else m
        ptr = lambda name: None if null.get(name) else self.p
        return self.lib.dcnr_cosine_neighbor_table_update(
            ptr("table"), ptr("inv"), None, self.N, self.d, self.k,
            None if null.get("changed") else ch.ctypes.data, m, ptr("nbr"), ptr("counts"), None,
            ptr("research"), ptr("ws"), self.size(max(m, 0)) if nbytes is None else nbytes, None)

    def rows(self, n, nbytes, **null):
        ptr = lambda name: None if null.get(name) else self.p
        return self.lib.dcnr_cosine_neighbor_table_rows(
            ptr("table"), ptr("inv"), None, self.N, self.d, self.k, ptr("rows"), n, ptr("nbr"),
            ptr("ws"), nbytes, None)


def test_workspace_size_is_exact():
    c = Call()
    sizes = {m: c.size(m) for m in (0, 1, 37, 16384)}
    assert all(s > 256 for s in sizes.values())
    assert sizes[0] <= sizes[1] <= sizes[37] <= sizes[16384] < 1 << 30
    # one byte less: DCNR_WORKSPACE_TOO_SMALL (judged once the arguments are accepted, nothing launched)
    for m in (1, 37):
        assert c.update(np.arange(m), nbytes=sizes[m] - 1) == WORKSPACE_TOO_SMALL
    assert c.rows(5, sizes[0] - 1) == WORKSPACE_TOO_SMALL
    # shapes the calls reject have nothing to plan
    assert c.size(1, k=65) == 256 and c.size(1, d=30) == 256 and c.size(-1) == 256
    assert c.size(16385) == 256
    # the size grows with the table, not with a rebuild's scratch alone
    assert Call(N=1_000_000).size(1024) > sizes[37]


def test_bad_arguments_are_rejected_on_the_host():
    c = Call()
    for name in ("table", "inv", "changed", "nbr", "counts", "research", "ws"):
        assert c.update([3, 9], **{name: True}) == BAD_ARG, name
    assert c.update([9, 3]) == BAD_ARG                      # not ascending
    assert c.update([3, 3]) == BAD_ARG                      # not distinct
    assert c.update([3, c.N]) == BAD_ARG and c.update([-1, 3]) == BAD_ARG
    assert c.update([3], m=-1) == BAD_ARG
    assert c.update([3], m=16385, nbytes=1 << 20) == UNSUPPORTED_SHAPE
    assert Call(k=0).update([3], nbytes=1 << 20) == BAD_ARG
    assert Call(N=8, k=9).update([3], nbytes=1 << 20) == BAD_ARG
    assert Call(k=65).update([3], nbytes=1 << 20) == UNSUPPORTED_SHAPE
    assert Call(d=30).update([3], nbytes=1 << 20) == UNSUPPORTED_SHAPE
    # nothing to do: DCNR_OK whatever else is null
    assert c.update([], nbr=True, counts=True, research=True, ws=True, changed=True) == OK
    assert c.rows(0, 0, rows=True, nbr=True, ws=True) == OK
    for name in ("table", "inv", "rows", "nbr", "ws"):
        assert c.rows(4, 1 << 30, **{name: True}) == BAD_ARG, name
    assert c.rows(-1, 1 << 30) == BAD_ARG
    assert c.update([9, 3]) == BAD_ARG
    from dcnr import _lib
    assert b"ascending" in _lib.load().dcnr_last_error()


_cases = {}


def case(d, k):
    """The planted table, its brute-force neighbour table, a changed set and
    the brute-force table after it -- once per shape."""
    if (d, k) not in _cases:
        table, ties, zero = rule.planted_table(5003, d, seed=1000 + 7 * d + k)
        counts = (3, 3, 3) if k == 51 else (12, 12, 11)
        rows, vec = rule.changed_set(table, ties, zero, seed=d + k, counts=counts)
        new = table.copy()
        new[rows] = vec
        D_new = rule.distances(new)
        _cases[(d, k)] = dict(old=rule.brute_table(rule.distances(table), k), rows=rows, D_new=D_new,
                              want=rule.brute_table(D_new, k))
    return _cases[(d, k)]


@pytest.mark.parametrize("d,k", SHAPES)
def test_rule_restatement_equals_brute_force(d, k):
    c = case(d, k)
    assert c["rows"].size == (11 if k == 51 else 37) and np.unique(c["rows"]).size == c["rows"].size
    got, br = rule.apply_rule(c["old"], c["D_new"], c["rows"])
    assert np.array_equal(got, c["want"])
    n = {name: int(m.sum()) for name, m in br.items()}
    print(f"d={d} k={k}: {n}")
    assert sum(n.values()) == 5003 and n["changed"] == c["rows"].size
    # every branch the recipe reaches is taken
    assert n["untouched"] > 0 and n["gained"] > 0 and n["merged_hole"] + n["hole"] > 0
    assert n["hole"] > 0
    # what the update searches again stays under m + the rows holding a changed row
    holders = int((np.isin(c["old"], c["rows"]).any(1) & ~br["changed"]).sum())
    assert n["hole"] + n["emptied"] <= holders
