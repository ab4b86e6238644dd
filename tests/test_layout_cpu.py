"""The workspace layouts are what tests/golden/layout_offsets.json records:
every size and every tensor offset, byte for byte (host-side queries only).
The fixture was recorded before the host code's path choices moved into one
plan and the kNN scratch into one carve; neither may move a byte."""
import json
import os

from conftest import GOLDEN
import make_layout_golden as mk


def test_layouts_match_recorded():
    want = json.load(open(os.path.join(GOLDEN, "layout_offsets.json")))
    got = json.loads(json.dumps(mk.collect(with_offsets=True)))   # tuples -> lists, as the file has them
    for k in ("kinds", "model", "batch", "cosine_topk", "linear_wgrad"):
        assert got[k] == want[k], k
    assert list(got["workspace"]) == list(want["workspace"]) and len(want["workspace"]) > 0
    for key, rows in want["workspace"].items():
        for B, w, g in zip(want["batch"], rows, got["workspace"][key]):
            where = f"precision/hidden/n_res/mode/flags = {key}, B = {B}"
            assert g[0] == w[0], f"workspace_bytes differ at {where}"
            assert g[1] == w[1], f"offsets differ at {where}; now (kinds {got['kinds']} in order): {g[2]}"
