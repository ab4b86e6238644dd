"""The item neighbour table's host side: the artifact pair
``item_neighbors.npy`` + ``item_neighbors_fingerprint.npy``
(dcnr.artifacts.save_neighbor_table / load_neighbor_table) and the C ABI's new
symbols.  No device: the tables here are made up, only their shapes and the
embeddings they claim to belong to matter.
"""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

N, D, K = 37, 8, 11


def embeddings(seed=0, n=N, d=D):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def table(n=N, k=K, seed=1):
    return np.random.default_rng(seed).integers(0, n, (n, k)).astype(np.int32)


def saved(tmp_path, emb=None, nbr=None):
    from dcnr import artifacts
    emb = embeddings() if emb is None else emb
    nbr = table(emb.shape[0]) if nbr is None else nbr
    np.save(os.path.join(tmp_path, artifacts.EMB_FILE), emb)
    artifacts.save_neighbor_table(nbr, str(tmp_path))
    return emb, nbr


def test_round_trip(tmp_path):
    from dcnr import artifacts
    emb, nbr = saved(tmp_path)
    got = artifacts.load_neighbor_table(str(tmp_path))
    assert got.dtype == np.int32 and np.array_equal(got, nbr)
    # ... and against embeddings handed in (what load_artifacts does)
    assert np.array_equal(artifacts.load_neighbor_table(str(tmp_path), emb.copy()), nbr)
    # a tensor is taken as well
    import torch
    artifacts.save_neighbor_table(torch.from_numpy(nbr), str(tmp_path))
    assert np.array_equal(artifacts.load_neighbor_table(str(tmp_path)), nbr)


def test_files_hold_no_pickle(tmp_path):
    from dcnr import artifacts
    _, nbr = saved(tmp_path)
    a = np.load(os.path.join(tmp_path, artifacts.NBR_FILE), allow_pickle=False)
    fp = np.load(os.path.join(tmp_path, artifacts.NBR_FP_FILE), allow_pickle=False)
    assert a.dtype == np.int32 and a.shape == (N, K) and np.array_equal(a, nbr)
    assert fp.dtype == np.int64 and fp[1:4].tolist() == [N, D, K]
    # the reference's files are untouched by the save
    assert sorted(os.listdir(tmp_path)) == sorted([artifacts.EMB_FILE, artifacts.NBR_FILE,
                                                   artifacts.NBR_FP_FILE])


def test_one_changed_element_is_rejected(tmp_path):
    from dcnr import artifacts
    emb, _ = saved(tmp_path)
    other = emb.copy()
    other[N // 2, 3] = np.nextafter(other[N // 2, 3], np.float32(np.inf))   # one ulp
    with pytest.raises(ValueError, match="checksum"):
        artifacts.load_neighbor_table(str(tmp_path), other)
    np.save(os.path.join(tmp_path, artifacts.EMB_FILE), other)              # ... or on disk
    with pytest.raises(ValueError, match="does not belong"):
        artifacts.load_neighbor_table(str(tmp_path))


def test_another_n_is_rejected(tmp_path):
    from dcnr import artifacts
    emb, _ = saved(tmp_path)
    with pytest.raises(ValueError, match="n_items"):
        artifacts.load_neighbor_table(str(tmp_path), emb[:-1])
    with pytest.raises(ValueError, match="emb_dim"):
        artifacts.load_neighbor_table(str(tmp_path), emb.reshape(N * 2, D // 2))


def test_another_k_is_rejected(tmp_path):
    from dcnr import artifacts
    saved(tmp_path)
    np.save(os.path.join(tmp_path, artifacts.NBR_FILE), table(k=K - 1))   # a table of another build
    with pytest.raises(ValueError, match=r"differs in: k\)"):
        artifacts.load_neighbor_table(str(tmp_path))


def test_save_rejects_a_table_of_another_shape(tmp_path):
    from dcnr import artifacts
    np.save(os.path.join(tmp_path, artifacts.EMB_FILE), embeddings())
    with pytest.raises(ValueError):
        artifacts.save_neighbor_table(table(n=N + 1), str(tmp_path))
    with pytest.raises(ValueError):
        artifacts.save_neighbor_table(table().astype(np.int64), str(tmp_path))


NEW_SYMBOLS = ["dcnr_cosine_neighbor_table", "dcnr_cosine_neighbor_table_workspace_size",
               "dcnr_candidate_union_table", "dcnr_requests_candidates_table"]


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
    # the size query answers on the host: one chunk's scratch, whatever the table's length
    small = lib.dcnr_cosine_neighbor_table_workspace_size(5003, 11)
    assert 0 < small < lib.dcnr_cosine_neighbor_table_workspace_size(1_000_000, 11) < 1 << 30
