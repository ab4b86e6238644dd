"""The reference's on-disk model artifacts (train.py:391-396 writes them,
main.py:256-270 loads them at API startup):

  final_dcn_model.pth   torch.save(final_model.state_dict())
  item_embeddings.npy   final_model.item_embedding.weight as float32 [n_items, emb_dim]
  model_dims.gz / best_params.gz / artifacts.gz   joblib pickles

``save_artifacts`` writes the first two exactly as train.py:391-394 does;
``load_artifacts`` reads them the way main.py:259-270 uses them, with
loaders that execute nothing from the files (``torch.load(weights_only=True)``,
``np.load(allow_pickle=False)``).  The joblib files are pickles: their
values (``model_dims = (n_users, n_items, cat_dims, n_num_features)`` and
``best_params``) are passed in by the caller, who decides whether to trust
them.  The state_dict is interchangeable both ways with the reference's
``DCN_RecSys`` (same keys, shapes, dtypes).

One file pair is this package's own and optional: ``item_neighbors.npy``, the
item neighbour table (int32 [n_items, k], ``NearestNeighbors.
build_neighbor_table``), with ``item_neighbors_fingerprint.npy`` beside it
(int64: format, n_items, emb_dim, k and a checksum of the embedding bytes), so
that a server start reads the table instead of building it and a table that
does not belong to ``item_embeddings.npy`` is refused.
"""
from __future__ import annotations

import hashlib
import os
from typing import Any, Dict, Tuple

import numpy as np
import torch

from .knn import NearestNeighbors
from .model import DCN_RecSys

MODEL_FILE = "final_dcn_model.pth"
EMB_FILE = "item_embeddings.npy"
NBR_FILE = "item_neighbors.npy"
NBR_FP_FILE = "item_neighbors_fingerprint.npy"
NBR_FORMAT = 1


def save_artifacts(model: DCN_RecSys, artifacts_dir: str) -> None:
    """train.py:391-394: the state_dict and the item-embedding table."""
    os.makedirs(artifacts_dir, exist_ok=True)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    torch.save(sd, os.path.join(artifacts_dir, MODEL_FILE))
    emb = model.item_embedding.weight.detach().cpu().numpy()
    np.save(os.path.join(artifacts_dir, EMB_FILE), emb)


def load_artifacts(artifacts_dir: str, model_dims: Tuple[int, int, Dict[str, int], int],
                   best_params: Dict[str, Any], device="cuda", precision="fp32",
                   n_neighbors: int = 16,
                   neighbor_table: bool = False) -> Tuple[DCN_RecSys, np.ndarray, NearestNeighbors]:
    """main.py:259-270: build DCN_RecSys(*model_dims, best_params), load the
    state_dict, move to the device in eval mode, load the item embeddings and
    fit the cosine index on them.  Returns (model, item_embeddings, index).
    ``neighbor_table=True`` also reads ``item_neighbors.npy`` (ValueError when
    it does not belong to these embeddings) onto the device as
    ``index.neighbor_table_``, which ``RankingPipeline(neighbor_table=...)``
    adopts."""
    n_users, n_items, cat_dims, n_num_features = model_dims
    model = DCN_RecSys(n_users, n_items, cat_dims, n_num_features, best_params,
                       precision=precision)
    sd = torch.load(os.path.join(artifacts_dir, MODEL_FILE), map_location="cpu",
                    weights_only=True)
    model.load_state_dict(sd)
    model.to(device)
    model.eval()
    emb = np.load(os.path.join(artifacts_dir, EMB_FILE), allow_pickle=False)
    index = NearestNeighbors(n_neighbors=n_neighbors, metric="cosine", algorithm="brute",
                             device=device).fit(emb)
    if neighbor_table:
        index.neighbor_table_ = torch.from_numpy(load_neighbor_table(artifacts_dir, emb)).to(device)
    return model, emb, index


def _fingerprint(emb: np.ndarray, k: int) -> np.ndarray:
    """int64 [5]: format, n_items, emb_dim, k, a 63-bit BLAKE2b of the fp32 embedding bytes."""
    e = np.ascontiguousarray(emb, dtype="<f4")
    if e.ndim != 2:
        raise ValueError("item embeddings must be [n_items, emb_dim]")
    h = int.from_bytes(hashlib.blake2b(e.tobytes(), digest_size=8).digest(), "little") >> 1
    return np.array([NBR_FORMAT, e.shape[0], e.shape[1], k, h], np.int64)


def save_neighbor_table(index_or_table, artifacts_dir: str) -> None:
    """Writes ``item_neighbors.npy`` (int32 [n_items, k]) for the
    ``item_embeddings.npy`` already in ``artifacts_dir``, and its fingerprint.
    ``index_or_table``: a fitted ``NearestNeighbors`` holding a full
    ``neighbor_table_`` (its table must be that file's embeddings), or the
    table itself (array or tensor)."""
    emb = np.load(os.path.join(artifacts_dir, EMB_FILE), allow_pickle=False)
    if isinstance(index_or_table, NearestNeighbors):
        index = index_or_table
        if index.neighbor_table_ is None:
            raise ValueError("save_neighbor_table: the index holds no neighbour table "
                             "(build_neighbor_table() first)")
        fitted = index._table.cpu().numpy()
        if fitted.shape != emb.shape or not np.array_equal(fitted.view(np.uint32),
                                                           emb.astype("<f4").view(np.uint32)):
            raise ValueError(f"save_neighbor_table: the index was not fitted on {EMB_FILE}")
        nbr = index.neighbor_table_
    else:
        nbr = index_or_table
    nbr = nbr.cpu().numpy() if torch.is_tensor(nbr) else np.asarray(nbr)
    if nbr.dtype != np.int32 or nbr.ndim != 2 or nbr.shape[0] != emb.shape[0]:
        raise ValueError(f"save_neighbor_table: expected int32 [{emb.shape[0]}, k], got "
                         f"{nbr.dtype} {list(nbr.shape)}")
    np.save(os.path.join(artifacts_dir, NBR_FILE), np.ascontiguousarray(nbr))
    np.save(os.path.join(artifacts_dir, NBR_FP_FILE), _fingerprint(emb, nbr.shape[1]))


def load_neighbor_table(artifacts_dir: str, emb: np.ndarray = None) -> np.ndarray:
    """``item_neighbors.npy`` as int32 [n_items, k] (host), checked against its
    fingerprint and against ``emb`` (default: ``item_embeddings.npy`` of the
    same directory): ValueError for a table saved for other embeddings
    (another n_items, emb_dim or content) or with another k than recorded."""
    if emb is None:
        emb = np.load(os.path.join(artifacts_dir, EMB_FILE), allow_pickle=False)
    nbr = np.load(os.path.join(artifacts_dir, NBR_FILE), allow_pickle=False)
    fp = np.load(os.path.join(artifacts_dir, NBR_FP_FILE), allow_pickle=False)
    if nbr.dtype != np.int32 or nbr.ndim != 2:
        raise ValueError(f"{NBR_FILE}: expected int32 [n_items, k], got {nbr.dtype} {list(nbr.shape)}")
    want = _fingerprint(emb, nbr.shape[1])
    if fp.dtype != np.int64 or fp.shape != want.shape or not np.array_equal(fp, want):
        names = ("format", "n_items", "emb_dim", "k", "embedding checksum")
        diff = [n for n, a, b in zip(names, fp.reshape(-1).tolist(), want.tolist()) if a != b] \
            if fp.shape == want.shape else ["layout"]
        raise ValueError(f"{NBR_FILE} does not belong to these item embeddings "
                         f"(fingerprint differs in: {', '.join(diff)})")
    return nbr
