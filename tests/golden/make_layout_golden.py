"""Records the library's workspace layouts (tests/golden/layout_offsets.json).

Only the host-side size queries are called (no device, no compute):
dcnr_workspace_size and dcnr_workspace_offset for every tensor kind and every
valid index over a grid of model shapes, modes, flags and batch sizes, plus
dcnr_cosine_topk_workspace_size and dcnr_linear_wgrad_workspace_size.
To keep the file small, a configuration's ~20-80 offsets are stored as the
first 16 hex digits of the SHA-256 of their decimal, comma-joined list (the
sizes are stored as numbers); on a mismatch the test prints the offsets the
library gives now, kind by kind.
tests/test_layout_cpu.py asserts that the library still answers exactly this,
so a change of the host code that is meant to leave the layouts alone can
prove it.  Run it (python tests/golden/make_layout_golden.py) only when a
change of the layout is intended.
"""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "hybrid-hotel-recommendation-system-based-on-friends-recommendations_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

OUT = os.path.join(HERE, "layout_offsets.json")

# everything but precision / hidden / n_res is fixed: D = 50 (Dp = 56, the
# deep dx0's row 64 floats), two categorical tables, two cross layers
MODEL = dict(n_users=1000, n_items=500, cat_rows=[30, 200], emb_dim=12, n_num=5, n_cross=2)
HIDDEN = [40, 96, 160, 256, 384, 512, 1024]
N_RES = [1, 2, 4]
BATCH = [2, 300, 16384, 131072]
TOPK = dict(N=[1, 20000, 1_000_000], Q=[1, 16, 17, 256, 1024], k=[1, 11, 32, 64])
WGRAD = [(512, 512, 131072), (512, 456, 131072), (96, 96, 300)]


def flag_sets(_lib, prec, mode):
    """The flag values that select a layout in (prec, mode): the row map is a
    train-mode buffer, the fused tower a bf16 eval path."""
    fl = [0, _lib.FLAG_KEEP_INTERMEDIATES]
    if mode == _lib.TRAIN:
        fl.append(_lib.FLAG_ROW_MAP)
    elif prec == _lib.PREC_BF16:
        fl.append(_lib.FLAG_FUSED_TOWER)
    return fl


def n_index(kind, R):
    if kind == "h":
        return R + 1
    if kind in ("t1", "t2", "a1", "mask_a1", "mask_h", "du", "dt2", "da", "dt1"):
        return R
    if kind.startswith("bn_"):
        return 2 * R
    return 1


def digest(offsets):
    return hashlib.sha256(",".join(str(o) for o in offsets).encode()).hexdigest()[:16]


def collect(with_offsets=False):
    """{"workspace": {"precision/hidden/n_res/mode/flags": [[workspace_bytes,
    offsets digest] for B in BATCH]}, ...}; with_offsets: the offset lists
    themselves as a third entry."""
    from dcnr import _lib
    lib = _lib.load()
    cat_rows = (ctypes.c_int64 * len(MODEL["cat_rows"]))(*MODEL["cat_rows"])
    rows = {}
    for prec in (_lib.PREC_FP32, _lib.PREC_BF16):
        for hidden in HIDDEN:
            for R in N_RES:
                desc = _lib.ModelDesc()
                desc.n_users, desc.n_items = MODEL["n_users"], MODEL["n_items"]
                desc.n_cat = len(MODEL["cat_rows"])
                desc.cat_rows = ctypes.cast(cat_rows, ctypes.POINTER(ctypes.c_int64))
                desc.emb_dim, desc.n_num, desc.n_cross = MODEL["emb_dim"], MODEL["n_num"], MODEL["n_cross"]
                desc.hidden, desc.n_res, desc.dropout, desc.precision = hidden, R, 0.0, prec
                for mode in (_lib.EVAL, _lib.TRAIN):
                    for flags in flag_sets(_lib, prec, mode):
                        desc.flags = flags
                        per_b = rows[f"{prec}/{hidden}/{R}/{mode}/{flags}"] = []
                        for B in BATCH:
                            n = ctypes.c_size_t(0)
                            _lib.check(lib.dcnr_workspace_size(ctypes.byref(desc), B, mode, ctypes.byref(n)))
                            offs = []
                            for ki, kind in enumerate(_lib.WS_KINDS):
                                for idx in range(n_index(kind, R)):
                                    o = ctypes.c_int64(0)
                                    _lib.check(lib.dcnr_workspace_offset(ctypes.byref(desc), B, mode, ki, idx,
                                                                         ctypes.byref(o)))
                                    offs.append(int(o.value))
                            per_b.append([int(n.value), digest(offs)] + ([offs] if with_offsets else []))
    topk = [[N, Q, k, int(lib.dcnr_cosine_topk_workspace_size(N, Q, k))]
            for N in TOPK["N"] for Q in TOPK["Q"] for k in TOPK["k"]]
    wgrad = [[N, K, B, int(lib.dcnr_linear_wgrad_workspace_size(N, K, B))] for N, K, B in WGRAD]
    return dict(model=MODEL, kinds=list(_lib.WS_KINDS), batch=BATCH, workspace=rows, cosine_topk=topk,
                linear_wgrad=wgrad)


if __name__ == "__main__":
    got = collect()
    with open(OUT, "w") as f:   # one configuration per line
        head = {k: v for k, v in got.items() if k != "workspace"}
        f.write(json.dumps(head, separators=(",", ":"))[:-1] + ',"workspace":{\n')
        f.write(",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}"
                           for k, v in got["workspace"].items()))
        f.write("\n}}\n")
    print(OUT, os.path.getsize(OUT), "bytes")
