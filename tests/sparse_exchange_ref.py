"""Host references of the sparse exchange's three device calls, written from
their contracts in include/dcnr.h (not from the kernels):

  dcnr_emb_touched_rows   -> touched_ref
  dcnr_sparse_pack        -> pack_ref, HostSparseOps.pack
  dcnr_sparse_accumulate  -> accumulate_ref, HostSparseOps.accumulate

Everything is integer arithmetic or fp32 adds in a stated order, so the tests
compare with array equality.  tests/test_parallel_cpu.py checks each function
on a hand-written example and runs the exchange protocol over HostSparseOps;
tests/test_sparse_exchange_gpu.py runs the kernels against them.
"""
import numpy as np
import torch


class HostSparseOps:
    """Host restatement of libdcnr's sparse-exchange kernels (dcnr_sparse_pack:
    the tables' touched rows in flat order; dcnr_sparse_accumulate: zero,
    then every source's rows added in rank order) -- the CPU side of the
    protocol test; the GPU tests run the kernels."""

    def pack(self, grad, offsets, table_counts, width, n_rows):
        tc = table_counts.tolist()
        off = torch.cat([offsets[t, :tc[t]] for t in range(len(tc))])
        assert off.numel() == n_rows
        col = torch.arange(width, dtype=torch.int64)
        rows = grad[off[:, None] + col[None, :]] if n_rows else torch.empty((0, width))
        return off, rows

    def accumulate(self, shard, lo, width, offsets, rows, counts):
        shard.zero_()
        sv = shard.view(-1, width)
        pos = 0
        for c in counts:
            if c:
                sv.index_add_(0, torch.div(offsets[pos:pos + c] - lo, width, rounding_mode="floor"),
                              rows[pos:pos + c])
            pos += c


def touched_ref(ids, width, elem_off, shard, world):
    """Flat element offsets of the distinct rows ``ids`` name (ascending) and
    owner_counts[r] = how many of them lie in [r*shard, (r+1)*shard), r <
    world; an offset at or beyond world*shard is in no count."""
    offs = np.unique(np.asarray(ids, dtype=np.int64)) * int(width) + int(elem_off)
    owner = offs // int(shard)
    counts = np.bincount(owner[owner < world], minlength=world).astype(np.int64)
    return offs, counts


def pack_ref(grad, offsets, counts, width):
    """The send buffers: table t's first counts[t] offsets, tables in order,
    and the rows grad[o : o + width] they address."""
    grad = np.asarray(grad)
    offsets = np.asarray(offsets, dtype=np.int64)
    offs = np.concatenate([offsets[t, :int(c)] for t, c in enumerate(counts)] +
                          [np.empty(0, np.int64)])
    rows = np.empty((len(offs), width), grad.dtype)
    for i, o in enumerate(offs.tolist()):
        rows[i] = grad[o:o + width]
    return offs, rows


def accumulate_ref(shard_lo, shard_elems, width, offsets, rows, source_counts):
    """fp32 zeros [shard_elems], then source after source, row after row:
    shard[r : r + width] += row for r = off - shard_lo, where the whole row
    lies inside the shard; every other row is skipped."""
    shard = np.zeros(shard_elems, np.float32)
    offsets = np.asarray(offsets, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, width)
    pos = 0
    for c in source_counts:
        for i in range(pos, pos + int(c)):
            r = int(offsets[i]) - int(shard_lo)
            if 0 <= r and r + width <= shard_elems:
                shard[r:r + width] = shard[r:r + width] + rows[i]   # one fp32 rounding per add
        pos += int(c)
    return shard
