"""Shared by test_transform_cpu.py and test_transform_gpu.py: the fixture of
tests/golden/transform (the reference's ``preprocess_for_ranking`` on rows its
``prepare_data`` was not fitted on), frames cut in a fit part and a new part,
and the comparison of two ``Transformed``."""
import os

import numpy as np

import prepare_common as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transform", "transform_golden.npz")
FIELDS = ("collab", "cat", "num", "y", "rows", "unknown_bits")
COUNTS = ("n", "n_filtered", "n_unknown_users", "n_unknown_items", "n_unknown_cat")
RESERVED = -(1 << 63)


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_rows(g):
    """The fixture's input columns as ``transform``'s positional arguments."""
    values = lambda a: np.array([None if v == "" else v for v in a.tolist()], dtype=object)
    return g["user"], g["item"], None, [values(g["city"]), values(g["kind"])], g["raw"]


def assert_matches_golden(t, g):
    assert pc.same(pc.to_np(t.collab), np.stack([g["x_user"], g["x_item"]], axis=1))
    assert pc.same(pc.to_np(t.cat), g["x_cat"])
    assert pc.same(pc.to_np(t.num), g["x_num"])
    assert t.y is None and t.n == len(g["user"]) and t.n_filtered == 0
    assert pc.same(pc.to_np(t.rows), np.arange(t.n, dtype=np.int32))


def part(case, lo, hi):
    """Rows [lo, hi) of a case's columns, as the five positional arguments."""
    return (case["user"][lo:hi], case["item"][lo:hi], case["target"][lo:hi],
            [k[lo:hi] for k in case["cat"]], case["num"][lo:hi])


def fit_kwargs(case):
    return {k: case[k] for k in ("noise_filter", "derived", "cat_names") if k in case}


def assert_same_transformed(a, b, what=""):
    """Two results of transform / transform_host agree in every field and count."""
    for k in FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        if x is None or y is None:
            assert x is None and y is None, f"{what}: {k}"
        else:
            assert pc.same(pc.to_np(x), pc.to_np(y)), f"{what}: {k}"
    for k in COUNTS:
        assert getattr(a, k) == getattr(b, k), f"{what}: {k} {getattr(a, k)} != {getattr(b, k)}"
    assert len(a.tensors) == 4 and a.tensors[0] is a.collab and a.tensors[3] is a.y


def wide_ids(rng, n, multiples=False):
    """n distinct ids like random_case's (negative, above 2^40, equal low 32
    bits), or all multiples of 2^32."""
    base = rng.choice(np.arange(-2 * n - 5, 2 * n + 5, dtype=np.int64), n, replace=False)
    if multiples:
        return base * (1 << 32)
    return base * (1 << 32) + (np.abs(base) % 3) + (1 << 41) * (base % 2)
