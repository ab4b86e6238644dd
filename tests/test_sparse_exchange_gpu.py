"""The sparse exchange's three device calls (csrc/embed_bwd.hip), each on its
own against the host references of tests/sparse_exchange_ref.py, and chained
at worlds 3 and 8 -- all in one process on one GPU, no process group: the
all_to_all between pack and accumulate is slicing and concatenation.

  dcnr_emb_touched_rows   emb_touched_kernel        vs np.unique (touched_ref)
  dcnr_sparse_pack        sparse_pack_kernel<4|1>   vs pack_ref
  dcnr_sparse_accumulate  sparse_add_kernel<4|1>    vs accumulate_ref

The kernels copy rows and add them in a stated order, so every comparison is
integer equality or equality of fp32 bits; there is no tolerance anywhere.

Which kernel a case runs follows from the dispatch in sparse_pack (<4>: width
% 4 == 0, grad and out_rows on the 16-byte grid) and sparse_accumulate (<4>:
width % 4 == 0, shard_lo % 4 == 0, shard and rows on the 16-byte grid); the
parameter names below say which condition a case flips.  Inside <4>, an
offset with o % 4 != 0 (pack) or (off - lo) % 4 != 0 (accumulate) takes the
scalar branch.

Slots the calls must not read hold valid offsets of NaN-filled memory, and
everything they must not write holds a sentinel, so a kernel that strays
shows as a value mismatch.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from sparse_exchange_ref import HostSparseOps, accumulate_ref, pack_ref, touched_ref

pytestmark = pytest.mark.gpu

SENT = -7777                 # int64 sentinel of offset buffers
FSENT = -12345.5             # fp32 sentinel of row / shard margins
CHUNK = 4096                 # emb_touched_kernel: TR_T * TR_U positions per pass

N_USERS, N_ITEMS = 10_007, 300           # two-level sort | final after level 1
CATS = {"big": 1500, "small": 7}         # two-level, width 39 | level 1, width 3
ROWS = [N_USERS, N_ITEMS, 1500, 7]
# made-up flat offsets of the four tables (extent ~141.8k elements)
EOFF = [16, 80_200, 83_001, 141_777]
# (world, shard_elems, some offsets at or beyond world * shard_elems)
WORLDS = [(1, 200_000, False),       # one owner
          (3, 50_000, False),        # the user table straddles shards 0 / 1
          (3, 1 << 40, False),       # shards 1, 2 receive nothing
          (8, 20_000, False),        # user table over 5 shards, categorical in 4 and 7
          (8, 10_000, True),         # items, categoricals and the user table's tail beyond 80k
          (64, 4096, False),         # shards 35.. receive nothing
          (64, 1000, True)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tiny(dev, emb_dim=8, n_users=N_USERS, precision="fp32", hidden=32, on_device=False):
    import dcnr
    torch.manual_seed(3)
    params = dict(emb_dim=emb_dim, hidden_dim=hidden, n_cross_layers=1, n_res_blocks=1, dropout=0.0)
    if on_device:   # a huge table: initialise it on the device
        with torch.device(dev):
            m = dcnr.DCN_RecSys(n_users, N_ITEMS, CATS, 3, params, precision=precision)
    else:
        m = dcnr.DCN_RecSys(n_users, N_ITEMS, CATS, 3, params, precision=precision)
    return m.to(dev).train()


@pytest.fixture(scope="module")
def tiny(dev):
    return _tiny(dev)


def _widths(m):
    return [m._dims["emb_dim"]] * 2 + [int(math.sqrt(n)) + 1 for n in m._dims["cat_dims"]]


def _forward(m, dev, ids, seed=5):
    """Train-mode forward on the id columns ids = [user, item, cat0, cat1]
    (numpy); returns (logits, ws, device inputs)."""
    from dcnr.model import run_forward
    B = len(ids[0])
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    rng = np.random.default_rng(B)
    u, i = T(ids[0].astype(np.int64)), T(ids[1].astype(np.int64))
    c = T(np.stack(ids[2:], 1).astype(np.int64))
    n = T(rng.random((B, 3), dtype=np.float32))
    logits, ws = run_forward(m, True, seed, u, i, c, n)
    return logits, ws, (u, i, c, n)


def _check_touched(m, ws, ids, tables, eoff, world, shard, beyond=None):
    """dcnr.parallel.touched_rows of ``tables`` against np.unique."""
    from dcnr.parallel import touched_rows
    B = len(ids[0])
    w = _widths(m)
    out = torch.full((len(tables), B), SENT, dtype=torch.int64, device=ws.device)
    offs, tcnt, ocnt = touched_rows(m, ws, B, tables, eoff, shard, world, out=out)
    offs, tcnt, ocnt = offs.cpu().numpy(), tcnt.cpu().numpy(), ocnt.cpu().numpy()
    want_own = np.zeros(world, np.int64)
    for k, t in enumerate(tables):
        ref, own = touched_ref(ids[t], w[t], eoff[k], shard, world)
        want_own += own
        tag = f"table {t} (entry {k}), world {world}, shard {shard}"
        assert tcnt[k] == len(ref), tag
        assert np.array_equal(offs[k, :len(ref)], ref), tag
        assert np.all(offs[k, len(ref):] == SENT), tag + ": slots past the count written"
    assert np.array_equal(ocnt, want_own), (world, shard, ocnt.tolist(), want_own.tolist())
    if beyond is not None:
        assert (ocnt.sum() < tcnt.sum()) == beyond, (world, shard)
    return tcnt, ocnt


def _random_ids(rng, B):
    return [rng.integers(0, r, B) for r in ROWS]


def _around(rng, B, rows, pos, before, after):
    """B ids of [0, rows) whose sorted order has one id's run on positions
    [pos - before, pos + after), smaller ids before it and larger ones after
    it (before = 0: a new key exactly at sorted position pos); shuffled."""
    mid = rows // 2
    head = rng.integers(0, mid, pos - before)
    tail = rng.integers(mid + 1, rows, B - pos - after)
    ids = np.concatenate([head, np.full(before + after, mid), tail])
    s = np.sort(ids)
    assert s[pos - before] == mid and s[pos + after - 1] == mid and (pos + after == B or s[pos + after] > mid)
    assert pos - before == 0 or s[pos - before - 1] < mid
    return rng.permutation(ids)


def _case_ids(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("B"):
        return _random_ids(rng, int(name[1:]))
    if name == "all_equal":                      # one head per table: its last row
        return [np.full(CHUNK + 1, r - 1) for r in ROWS]
    if name == "all_distinct_users":             # count == B: row 0 of the output filled to its last slot
        ids = _random_ids(rng, 8200)
        ids[0] = rng.permutation(N_USERS)[:8200]
        return ids
    B, pos, before, after = {"run_across_4096": (8200, CHUNK, 5, 4),
                             "key_at_4096": (8200, CHUNK, 0, 3),
                             "key_at_4096_last": (CHUNK + 1, CHUNK, 0, 1),
                             "run_across_8192": (8200, 2 * CHUNK, 3, 3),
                             "key_at_8192": (8200, 2 * CHUNK, 0, 2)}[name]
    return [_around(rng, B, r, pos, before, after) for r in ROWS]


TOUCHED_CASES = ["B2", "B4095", "B4096", "B4097", "B8200", "all_equal", "all_distinct_users",
                 "run_across_4096", "key_at_4096", "key_at_4096_last", "run_across_8192",
                 "key_at_8192"]


# ------------------------------------------------- 1. dcnr_emb_touched_rows

@pytest.mark.parametrize("case", TOUCHED_CASES)
def test_touched_rows_equal_unique(dev, tiny, case):
    """All four tables (two-level sort, level 1 only, odd-width categorical
    with a nonzero key base) at worlds 1, 3, 8 and 64: offsets ascending and
    equal to np.unique, table counts, owner counts, sentinel past the counts."""
    ids = _case_ids(case)
    if case == "all_distinct_users":
        assert len(np.unique(ids[0])) == len(ids[0])
    _, ws, _ = _forward(tiny, dev, ids)
    for world, shard, beyond in WORLDS:
        _check_touched(tiny, ws, ids, (0, 1, 2, 3), EOFF, world, shard, beyond)


def test_touched_rows_table_lists(dev, tiny):
    """One table, and a non-ascending list: base and width are per entry."""
    ids = _random_ids(np.random.default_rng(1), 4097)
    _, ws, _ = _forward(tiny, dev, ids)
    for tables, eoff in (((2,), (5,)), ((3, 0), (1000, 7)), ((1,), (0,)), ((3, 2, 1, 0), (9, 1 << 33, 77, 3))):
        for world, shard in ((3, 30_000), (64, 777)):
            _check_touched(tiny, ws, ids, tables, eoff, world, shard)


def _raw_touched(m, ws, B, tables, eoff, shard, world, offs, tcnt, ocnt):
    from dcnr import _lib
    lib = _lib.load()
    n = len(tables)
    tabs = (ctypes.c_int32 * n)(*tables)
    eo = (ctypes.c_int64 * n)(*eoff)
    desc = m.desc()
    return lib.dcnr_emb_touched_rows(ctypes.byref(desc), ws.data_ptr(), ws.numel(), B, n,
                                     ctypes.cast(tabs, ctypes.c_void_p),
                                     ctypes.cast(eo, ctypes.c_void_p), shard, world,
                                     offs.data_ptr(), tcnt.data_ptr(), ocnt.data_ptr(),
                                     _lib.stream_ptr(ws.device))


def test_touched_rows_rejections_and_empty_batch(dev, tiny):
    """World 0, world 65, shard_elems 0 and a negative elem_off: nonzero
    status, nothing written.
    B = 0: zeroed table and owner counts, no offset written."""
    ids = _random_ids(np.random.default_rng(2), 64)
    _, ws, _ = _forward(tiny, dev, ids)
    new = lambda n: torch.full((n,), SENT, dtype=torch.int64, device=dev)   # noqa: E731
    for world, shard, eoff in ((0, 100, 99), (65, 100, 99), (8, 0, 99), (-1, 100, 99), (8, -5, 99),
                               (8, 100, -8)):
        offs, tcnt, ocnt = new(2 * 64), new(2), new(80)
        assert _raw_touched(tiny, ws, 64, (0, 1), (0, eoff), shard, world, offs, tcnt, ocnt) != 0
        torch.cuda.synchronize()
        for t in (offs, tcnt, ocnt):
            assert bool((t == SENT).all()), (world, shard, eoff)
    offs, tcnt, ocnt = new(2), new(2), new(8 + 3)
    assert _raw_touched(tiny, ws, 0, (0, 1), (0, 99), 100, 8, offs, tcnt, ocnt) == 0
    assert tcnt.tolist() == [0, 0] and ocnt.tolist() == [0] * 8 + [SENT] * 3
    assert offs.tolist() == [SENT, SENT]
    # the same through the wrapper
    from dcnr.parallel import touched_rows
    with pytest.raises(ValueError):
        touched_rows(tiny, ws, 64, (0, 1), (0, 99), 100, 65)
    with pytest.raises(ValueError):
        touched_rows(tiny, ws, 64, (0, 1), (0, 99), 0, 8)
    _, tcnt, ocnt = touched_rows(tiny, ws, 0, (0, 1), (0, 99), 100, 8)
    assert tcnt.tolist() == [0, 0] and ocnt.tolist() == [0] * 8


def test_touched_rows_radix_path(dev):
    """A user table of more than 2^24 rows (the stable radix sort of all
    tables' keys, as test_embed_bwd_gpu.py::test_huge_table_radix_fallback
    builds it): the touched rows of the user table and of a small table."""
    NS, MUL = 3000, 5600
    NB = NS * MUL + 16
    assert NB > (1 << 24)
    m = _tiny(dev, n_users=NB, on_device=True)
    rng = np.random.default_rng(7)
    B = CHUNK
    ids = _random_ids(rng, B)
    ids[0] = np.minimum(rng.zipf(1.3, B) - 1, NS - 1) * MUL + 11
    _, ws, _ = _forward(m, dev, ids)
    for world, shard, beyond in ((8, NB + 1000, False), (64, 1 << 20, True), (3, 1 << 40, False)):
        _check_touched(m, ws, ids, (0, 3), (64, NB * 8 + 640), world, shard, beyond)
    _check_touched(m, ws, ids, (0, 1, 2, 3), [8, NB * 8 + 64, NB * 8 + 4001, NB * 8 + 70_000], 8,
                   NB + 10_000, False)


@pytest.mark.parametrize("precision,hidden", [("fp32", 32), ("bf16", 128)])
@pytest.mark.parametrize("dense_table_grads", [False, True])
def test_trainer_touched_rows_match_step_flags(dev, precision, hidden, dense_table_grads):
    """FusedTrainer at world 1: its step's forward passes per-call flags (row
    map, head statistics), touched_rows builds the descriptor without them;
    both must place the sorted keys at the same workspace offset."""
    import dcnr
    m = _tiny(dev, precision=precision, hidden=hidden)
    tr = dcnr.FusedTrainer(m, dense_table_grads=dense_table_grads)
    B = 777
    rng = np.random.default_rng(4)
    ids = _random_ids(rng, B)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    u, i = T(ids[0]), T(ids[1])
    tr.step(u, i, T(np.stack(ids[2:], 1)), T(rng.random((B, 3), dtype=np.float32)),
            T((rng.random(B) < 0.5).astype(np.float32)))
    offs, tcnt, ocnt = tr.touched_rows()
    lay = tr._sparse_layout
    assert lay["tables"] == (0, 1) and lay["width"] == 8
    total = 0
    for k, col in enumerate((u, i)):
        want = torch.unique(col) * 8 + lay["elem_off"][k]
        assert int(tcnt[k]) == want.numel()
        assert torch.equal(offs[k, :want.numel()], want), k
        total += want.numel()
    assert ocnt.tolist() == [total]


# ------------------------------------------------------ 2. dcnr_sparse_pack

def _call_pack(grad, offsets, ld, tcnt, n_tables, width, out_off, out_rows):
    from dcnr import _lib
    return _lib.load().dcnr_sparse_pack(grad.data_ptr(), offsets.data_ptr(), ld, tcnt.data_ptr(),
                                        n_tables, width, out_off.data_ptr(), out_rows.data_ptr(),
                                        _lib.stream_ptr(grad.device))


def _pack_case(dev, width, counts, ld, odd_offsets, grad_shift=0, rows_shift=0, seed=0):
    """Runs dcnr_sparse_pack on synthetic tables and checks it against
    pack_ref.  grad[e] = e on its valid part and NaN after it; offset slots
    past a table's count point into the NaN part.  Returns (got rows, ref
    rows) for a caller's own assertion."""
    rng = np.random.default_rng(seed)
    nt, total = len(counts), int(sum(counts))
    stride = (width + 3) // 4 * 4 + 4               # rows apart, starts on multiples of 4
    slots = total + 8
    valid, nan_slots = slots * stride, 64
    G = valid + nan_slots * stride
    assert G < (1 << 24)                            # float(e) exact
    alloc = torch.full((G + 8,), float("nan"), dtype=torch.float32, device=dev)
    assert alloc.data_ptr() % 16 == 0
    grad = alloc[grad_shift:grad_shift + G]
    grad[:valid] = torch.arange(valid, dtype=torch.float32, device=dev)
    offsets = np.empty((nt, ld), np.int64)
    perm = rng.permutation(slots)[:total]
    pos = 0
    for t, c in enumerate(counts):
        o = np.sort(perm[pos:pos + c]) * stride
        if odd_offsets:
            o = o + rng.integers(1, 4, c)           # o % 4 in {1, 2, 3}
            o[::5] -= o[::5] % 4                    # ... and some on the grid among them
        offsets[t, :c] = o
        offsets[t, c:] = valid + rng.integers(0, nan_slots, ld - c) * stride
        pos += c
    tcnt = torch.tensor(counts, dtype=torch.int64, device=dev)
    pad = 5
    out_off = torch.full((total + pad,), SENT, dtype=torch.int64, device=dev)
    rows_alloc = torch.full(((total + pad) * width + 8,), FSENT, dtype=torch.float32, device=dev)
    out_rows = rows_alloc[rows_shift:rows_shift + (total + pad) * width]
    v4 = width % 4 == 0 and grad.data_ptr() % 16 == 0 and out_rows.data_ptr() % 16 == 0
    assert v4 == (width % 4 == 0 and not grad_shift and not rows_shift)
    assert _call_pack(grad, torch.from_numpy(offsets).to(dev), ld, tcnt, nt, width, out_off, out_rows) == 0
    ref_off, ref_rows = pack_ref(grad.cpu().numpy(), offsets, counts, width)
    assert not np.isnan(ref_rows).any()
    got_off, got_rows = out_off.cpu().numpy(), out_rows.cpu().numpy()
    assert np.array_equal(got_off[:total], ref_off)
    assert np.all(got_off[total:] == SENT), "offsets past sum(counts) written"
    got = got_rows[:total * width].reshape(total, width)
    assert np.array_equal(got.view(np.int32), ref_rows.view(np.int32)), \
        np.flatnonzero((got != ref_rows).any(1))[:8]
    assert np.all(got_rows[total * width:] == FSENT), "rows past sum(counts) written"
    ra = rows_alloc.cpu().numpy()
    assert np.all(ra[:rows_shift] == FSENT) and np.all(ra[rows_shift + (total + pad) * width:] == FSENT)
    return got, ref_rows


PACK_VARIANTS = {            # odd_offsets, grad_shift, rows_shift
    "grid": (False, 0, 0),                  # <4>, every row one float4 copy per 16 B
    "odd_offsets": (True, 0, 0),            # <4>, the o & 3 branch
    "grad_view": (False, 1, 0),             # grad % 16 != 0 -> <1>
    "rows_view": (False, 0, 1),             # out_rows % 16 != 0 -> <1>
    "grad_view_odd_offsets": (True, 1, 0)}  # <1>, offsets of any residue


@pytest.mark.parametrize("variant", list(PACK_VARIANTS))
@pytest.mark.parametrize("width", [8, 24, 32, 48])
def test_pack_vector_widths(dev, width, variant):
    odd, gs, rs = PACK_VARIANTS[variant]
    _pack_case(dev, width, (150, 0, 333), 400, odd, gs, rs, seed=width)


@pytest.mark.parametrize("odd_offsets", [False, True])
@pytest.mark.parametrize("width", [1, 3, 5])
def test_pack_scalar_widths(dev, width, odd_offsets):
    """width % 4 != 0 -> sparse_pack_kernel<1>."""
    _pack_case(dev, width, (150, 0, 333), 400, odd_offsets, seed=width)


@pytest.mark.parametrize("width", [8, 3])
@pytest.mark.parametrize("counts,ld", [((0, 70, 300), 300), ((70, 0, 300), 300), ((300, 70, 0), 300),
                                        ((0, 0, 0), 300), ((0,), 9), ((300,), 300), ((300,), 5000),
                                        ((70, 300, 1, 0, 129), 300), ((70, 300, 1, 0, 129), 4097),
                                        ((0, 0, 41), 41), ((1, 1), 1)])
def test_pack_table_counts(dev, width, counts, ld):
    """Empty tables (first, middle, last, all), one table, five tables; ld the
    largest count (no slack slot in that table) and much larger."""
    _pack_case(dev, width, counts, ld, odd_offsets=(width == 3), seed=len(counts) + ld)


def test_pack_first_row_past_grid_cap(dev):
    """Width 64 (16 threads per row), 2048 * 256 / 16 + 1 rows: the 2048-block
    grid covers rows 0 .. 32767 in its first pass, row 32768 in a second."""
    n = 2048 * 256 // 16 + 1
    got, ref = _pack_case(dev, 64, (n,), n, False)
    assert np.array_equal(got[n - 1], ref[n - 1]), f"row {n - 1}, the first past the grid cap"
    assert np.array_equal(got[n - 2], ref[n - 2]), f"row {n - 2}, the last of the first pass"


# ------------------------------------------------ 3. dcnr_sparse_accumulate

MARGIN = 128


def _acc_inputs(rng, width, lo, counts, misaligned, outside, nslots=96):
    """Per source: distinct, non-overlapping rows inside the shard (any two
    sources may overlap), optionally off the 4-element grid relative to lo,
    and, if ``outside``, rows below, beyond and straddling either end of the
    shard among them."""
    stride = (width + 3) // 4 * 4 + 4
    elems = nslots * stride + 2
    offs, rows = [], []
    real = []
    for c in counts:
        r = np.sort(rng.permutation(nslots)[:c]) * stride
        if misaligned:
            r = r + rng.integers(0, 4, c)
        o = (r + lo).tolist()
        if outside and c:
            extra = [lo - width - 4, lo - 1, lo + elems, lo + elems + 100, lo + elems - width + 1,
                     lo + elems - 1]
            for x in extra:
                o.insert(int(rng.integers(0, len(o) + 1)), x)
        real.append(len(o))
        offs += o
        rows.append((rng.standard_normal((len(o), width)) *
                     10.0 ** rng.integers(-3, 4, (len(o), 1))).astype(np.float32))
    offs = np.array(offs, np.int64)
    rows = np.concatenate(rows + [np.empty((0, width), np.float32)])
    return elems, offs, rows, real


def _acc_case(dev, width, lo, elems, offs, rows, counts, shard_shift=0, rows_shift=0):
    """DeviceSparseOps.accumulate into a NaN-filled shard carved out of a
    sentinel-filled allocation, against accumulate_ref."""
    from dcnr.parallel import DeviceSparseOps
    alloc = torch.full((elems + 2 * MARGIN + 8,), FSENT, dtype=torch.float32, device=dev)
    assert alloc.data_ptr() % 16 == 0
    a = MARGIN + shard_shift
    shard = alloc[a:a + elems]
    shard.fill_(float("nan"))
    n = len(offs)
    rows_alloc = torch.full((n * width + 8,), float("nan"), dtype=torch.float32, device=dev)
    d_rows = rows_alloc[rows_shift:rows_shift + n * width].view(n, width)
    d_rows.copy_(torch.from_numpy(rows))
    d_offs = torch.from_numpy(offs).to(dev)
    v4 = width % 4 == 0 and lo % 4 == 0 and shard.data_ptr() % 16 == 0 and \
        (n == 0 or d_rows.data_ptr() % 16 == 0)
    assert v4 == (width % 4 == 0 and lo % 4 == 0 and not shard_shift and not rows_shift)
    DeviceSparseOps().accumulate(shard, lo, width, d_offs, d_rows, counts)
    ref = accumulate_ref(lo, elems, width, offs, rows, counts)
    got = alloc.cpu().numpy()
    assert np.all(got[:a] == FSENT) and np.all(got[a + elems:] == FSENT), "written outside the shard"
    got = got[a:a + elems]
    assert np.array_equal(got.view(np.int32), ref.view(np.int32)), np.flatnonzero(got != ref)[:8]
    return got, ref


ACC_COUNTS = [[], [0], [17], [0, 23], [23, 0], [0, 0], [9, 0, 14], [0, 20, 0],
              [0, 5, 11, 0, 7, 90, 2, 0], [3, 5, 11, 1, 7, 90, 2, 6]]


@pytest.mark.parametrize("counts", ACC_COUNTS, ids=lambda c: "-".join(map(str, c)) or "none")
def test_accumulate_source_counts(dev, counts):
    """0, 1, 2, 3 and 8 sources, empty ones first, last and in the middle;
    rows of different sources overlap, rows outside the shard are skipped."""
    rng = np.random.default_rng(len(counts) + sum(counts))
    for width, lo in ((8, 4096), (3, 10)):
        elems, offs, rows, real = _acc_inputs(rng, width, lo, counts, False, True)
        got, ref = _acc_case(dev, width, lo, elems, offs, rows, real)
        if sum(counts) == 0:
            assert not got.any()           # zeroed, exactly 0.0 everywhere


ACC_VARIANTS = {             # shard_shift, rows_shift, misaligned rows
    "grid": (0, 0, False),                  # <4>, float4 read-add-write
    "rows_off_grid": (0, 0, True),          # <4>, the r & 3 branch when lo % 4 == 0
    "shard_view": (1, 0, False),            # shard % 16 != 0 -> <1>
    "rows_view": (0, 1, False),             # rows % 16 != 0 -> <1>
    "shard_view_rows_off_grid": (1, 0, True)}


@pytest.mark.parametrize("variant", list(ACC_VARIANTS))
@pytest.mark.parametrize("lo", [0, 4096, 4098])       # 4098: lo % 4 == 2 -> <1>
@pytest.mark.parametrize("width", [1, 3, 8, 32, 48])
def test_accumulate_widths_alignment(dev, width, lo, variant):
    """Every width at every alignment of shard_lo, the shard and rows
    pointers and the rows inside the shard; offsets below, beyond and
    straddling the shard's ends are skipped and the rows around them added."""
    ss, rs, mis = ACC_VARIANTS[variant]
    rng = np.random.default_rng(width * 7 + lo + ss + 2 * rs)
    elems, offs, rows, real = _acc_inputs(rng, width, lo, [40, 0, 61, 13], mis, True)
    _acc_case(dev, width, lo, elems, offs, rows, real, ss, rs)


def test_accumulate_rank_order_sum(dev):
    """All 8 sources send the same rows with magnitudes many binades apart:
    the result is ((0 + g0) + g1) + ..., bit for bit.  The reversed order
    gives other bits (checked on the host), so the order is what is tested."""
    rng = np.random.default_rng(11)
    W, K, width, lo = 8, 64, 8, 512
    elems = K * width
    offs, rows = [], []
    for s in range(W):
        p = rng.permutation(K)
        offs.append(lo + p * width)
        rows.append((rng.standard_normal((K, width)) * 10.0 ** rng.integers(-8, 9, (K, 1))).astype(np.float32))
    counts = [K] * W
    o, r = np.concatenate(offs), np.concatenate(rows)
    rev = accumulate_ref(lo, elems, width, np.concatenate(offs[::-1]), np.concatenate(rows[::-1]), counts)
    fwd = accumulate_ref(lo, elems, width, o, r, counts)
    assert (rev.view(np.int32) != fwd.view(np.int32)).any()   # the order shows in the bits
    _acc_case(dev, width, lo, elems, o, r, counts)


def test_accumulate_first_row_past_grid_cap(dev):
    """Width 64 (16 threads per row), one source of 4096 * 256 / 16 + 1
    distinct rows: the last row sent is the second pass of the 4096-block grid."""
    n, width, lo = 4096 * 256 // 16 + 1, 64, 64
    rng = np.random.default_rng(3)
    p = rng.permutation(n + 7)[:n]
    offs = lo + p * width
    rows = rng.standard_normal((n, width), dtype=np.float32)
    elems = (n + 7) * width
    got, ref = _acc_case(dev, width, lo, elems, offs, rows, [n])
    a = p[n - 1] * width
    assert np.array_equal(got[a:a + width], rows[n - 1]), f"sent row {n - 1}, the first past the grid cap"


def test_accumulate_rejections(dev):
    """The GPU-side twins of test_asan_cpu.py's argument checks: nonzero
    status and the shard left as it was."""
    from dcnr import _lib
    lib = _lib.load()
    shard = torch.full((64,), float("nan"), device=dev)
    offs = torch.zeros(8, dtype=torch.int64, device=dev)
    rows = torch.ones((8, 8), device=dev)
    s = _lib.stream_ptr(dev)
    c = lambda *v: ctypes.cast((ctypes.c_int64 * len(v))(*v), ctypes.c_void_p)   # noqa: E731
    assert lib.dcnr_sparse_accumulate(shard.data_ptr(), 0, 64, 8, offs.data_ptr(), rows.data_ptr(),
                                      c(3, -1), 2, s) != 0
    assert lib.dcnr_sparse_accumulate(shard.data_ptr(), 0, 64, 8, offs.data_ptr(), rows.data_ptr(),
                                      None, 2, s) != 0
    assert lib.dcnr_sparse_accumulate(shard.data_ptr(), 0, 64, 8, offs.data_ptr(), None,
                                      c(3, 4), 2, s) != 0
    assert lib.dcnr_sparse_accumulate(shard.data_ptr(), 0, 64, 8, None, rows.data_ptr(),
                                      c(3, 4), 2, s) != 0
    assert lib.dcnr_sparse_accumulate(shard.data_ptr(), 0, 64, 0, offs.data_ptr(), rows.data_ptr(),
                                      c(3, 4), 2, s) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(shard).all())
    assert lib.dcnr_sparse_accumulate(shard.data_ptr(), 0, 64, 8, offs.data_ptr(), rows.data_ptr(),
                                      c(1, 0), 2, s) == 0
    assert shard.tolist() == [1.0] * 8 + [0.0] * 56


def test_device_ops_equal_host_ops(dev):
    """DeviceSparseOps and HostSparseOps (the stand-in of the CPU protocol
    tests in test_parallel_cpu.py) on the same row-aligned inputs."""
    from dcnr.parallel import DeviceSparseOps
    rng = np.random.default_rng(21)
    for width in (8, 24, 3):
        n_rows_tab = (200, 50)
        grad = torch.from_numpy(rng.standard_normal(sum(n_rows_tab) * width).astype(np.float32))
        B = 128
        offsets = torch.zeros((2, B), dtype=torch.int64)
        tc = []
        base = 0
        for t, nr in enumerate(n_rows_tab):
            u = np.unique(rng.integers(0, nr, B)) * width + base
            offsets[t, :len(u)] = torch.from_numpy(u)
            tc.append(len(u))
            base += nr * width
        tcnt = torch.tensor(tc)
        h_off, h_rows = HostSparseOps().pack(grad, offsets, tcnt, width, sum(tc))
        d_off, d_rows = DeviceSparseOps().pack(grad.to(dev), offsets.to(dev), tcnt.to(dev), width, sum(tc))
        assert torch.equal(d_off.cpu(), h_off) and torch.equal(_bits(d_rows.cpu()), _bits(h_rows))
        # an owner of the middle half receives the rows three sources packed
        lo, elems = 60 * width, 120 * width
        keep = (h_off >= lo) & (h_off < lo + elems)
        r_off = torch.cat([h_off[keep]] * 3)
        r_rows = torch.cat([h_rows[keep] * s for s in (1.0, 1e-4, -3e5)])
        counts = [int(keep.sum())] * 3
        h_sh = torch.full((elems,), float("nan"))
        d_sh = torch.full((elems,), float("nan"), device=dev)
        HostSparseOps().accumulate(h_sh, lo, width, r_off, r_rows, counts)
        DeviceSparseOps().accumulate(d_sh, lo, width, r_off.to(dev), r_rows.to(dev), counts)
        assert torch.equal(_bits(d_sh.cpu()), _bits(h_sh)), width


# -------------------------------- 4. the three calls chained, worlds 3 and 8

@pytest.mark.parametrize("emb_dim", [8, 24])
@pytest.mark.parametrize("W", [3, 8])
def test_chain_equals_rank_order_dense_sum(dev, W, emb_dim):
    """W simulated ranks, each its own batch (many user rows shared): touched
    rows -> backward -> pack; every owner's accumulate of the slices sent to
    it equals ((0 + g_0) + g_1) + ... of the ranks' flat gradients on the
    user and item tables, bit for bit, and the rest of its shard is 0."""
    from dcnr.model import run_backward
    from dcnr.ops import bce_with_logits
    from dcnr.parallel import DeviceSparseOps, touched_rows
    m = _tiny(dev, emb_dim=emb_dim)
    unit = 64 * emb_dim // math.gcd(64, emb_dim)
    flat, gflat = m.flatten_(pad_to=unit * W, table_align=unit)
    E = m.flat_emb_end
    Es = E // W
    assert E % W == 0 and Es % emb_dim == 0
    fo = m.flat_offsets
    params = m.param_tensors()
    ops = DeviceSparseOps()
    B = 512
    sent = []
    for r in range(W):
        rng = np.random.default_rng(100 + r)
        ids = _random_ids(rng, B)
        ids[0] = np.minimum((N_USERS * rng.random(B) ** 4).astype(np.int64), N_USERS - 1)
        ids[0][:3] = N_USERS - 1                       # the table's last row, from every rank
        logits, ws, (u, i, c, n) = _forward(m, dev, ids, seed=r)
        offs, tcnt, ocnt = touched_rows(m, ws, B, (0, 1), fo[:2], Es, W)
        y = torch.from_numpy((rng.random(B) < 0.5).astype(np.float32)).to(dev)
        _, dz = bce_with_logits(logits, y)
        g = torch.zeros_like(gflat)
        grads = [g[o:o + p.numel()].view_as(p) for p, o in zip(params, fo)]
        run_backward(m, u, i, c, n, dz, ws, grads, r)
        own = ocnt.tolist()
        assert sum(own) == int(tcnt.sum()) == len(np.unique(ids[0])) + len(np.unique(ids[1]))
        s_off, s_rows = ops.pack(g, offs, tcnt, emb_dim, sum(own))
        sent.append((g, s_off, s_rows, np.r_[0, np.cumsum(own)]))
    shared = set.intersection(*[set(s[1].tolist()) for s in sent])
    assert len(shared) > 8                             # rows every rank touched
    sparse_end = fo[2]                                 # the categorical tables start here
    for o in range(W):
        lo = o * Es
        r_off = torch.cat([s[1][s[3][o]:s[3][o + 1]] for s in sent])
        r_rows = torch.cat([s[2][s[3][o]:s[3][o + 1]] for s in sent])
        counts = [int(s[3][o + 1] - s[3][o]) for s in sent]
        assert bool(((r_off >= lo) & (r_off < lo + Es)).all()), f"owner {o}: a row of another shard"
        shard = torch.full((Es,), float("nan"), device=dev)
        ops.accumulate(shard, lo, emb_dim, r_off, r_rows, counts)
        want = torch.zeros(Es, device=dev)
        for s in sent:
            want = want + s[0][lo:lo + Es]
        k = max(0, min(Es, sparse_end - lo))
        assert torch.equal(_bits(shard[:k]), _bits(want[:k])), f"owner {o}"
        assert not bool(shard[k:].any()), f"owner {o}: beyond the sparse tables"
