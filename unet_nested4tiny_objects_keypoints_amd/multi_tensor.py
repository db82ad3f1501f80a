"""Host side of the multi-tensor launch (package-private): the device table ``[segments | chunk -> segment map |
arrival counter]`` that the fused optimizers, ``clip_grad_norm_`` (optim.py) and the weight averager (averaging.py) hand
to their kernels, and the small LRU cache they keep their tables in.  The format, the chunk walk and the counter are
described once, in the header comment of csrc/multi_tensor.h.

The callers fill and validate the segments (what differs between them); this module lays the table out, stages it in a
page-locked buffer and uploads it.
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_TABLES = 8      # cached device tables per cache (the data-parallel averager alternates between two)


def chunk_layout(numels, chunk):
    """Segment i of ``numels[i]`` elements owns ``ceil(numels[i] / chunk)`` chunks, in segment order.  Returns
    (chunk_begin: the first chunk of every segment, chunk_seg: int32 array, the segment of every chunk)."""
    counts = [(int(n) + chunk - 1) // chunk for n in numels]
    chunk_begin, total = [], 0
    for k in counts:
        chunk_begin.append(total)
        total += k
    return chunk_begin, np.repeat(np.arange(len(counts), dtype=np.int32), counts)


def aligned16(*tensors) -> int:
    """The segment's vec flag: 1 when every stream starts on a 16-byte boundary."""
    return int(all(t.data_ptr() % 16 == 0 for t in tensors))


class Table:
    """One device table.  segs: ctypes segments of ONE struct type (``_lib.OptimSegment`` or ``_lib.AvgSegment``) with
    every field but ``chunk_begin`` filled, none of them empty.  with_counter: the table ends in the zeroed arrival
    counter of capturable launches.  staging(nbytes): where the page-locked host buffer comes from when the caller has
    to supply it (no page-locked allocation inside a stream capture); it stays alive with the table, for the upload on
    ``device``'s current stream is asynchronous."""
    pinned = False      # True: a captured graph replays the upload, the cache must not evict the table

    def __init__(self, segs, device, with_counter: bool, staging=None):
        L = _lib.lib()
        seg_type = type(segs[0])
        chunk_begin, chunk_seg = chunk_layout([s.numel for s in segs], int(L.unetpp_optim_chunk_elems()))
        for s, b in zip(segs, chunk_begin):
            s.chunk_begin = b
        self.n_seg, self.n_chunks = len(segs), len(chunk_seg)
        self.chunk_off = self.n_seg * C.sizeof(seg_type)
        self.done_off = self.chunk_off + 4 * self.n_chunks
        nbytes = self.done_off + (8 if with_counter else 0)
        self.host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) if staging is None else staging(nbytes)
        arr = self.host.numpy()
        C.memmove(self.host.data_ptr(), (seg_type * self.n_seg)(*segs), self.chunk_off)
        arr[self.chunk_off:self.done_off] = chunk_seg.view(np.uint8)
        arr[self.done_off:nbytes] = 0
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        base = self.dev.data_ptr()
        # the leading C arguments of every entry point: segments, n_segments, chunk_segment, n_chunks
        self.args = (C.c_void_p(base), self.n_seg, C.c_void_p(base + self.chunk_off), self.n_chunks)
        self.done = C.c_void_p(base + self.done_off) if with_counter else None
        _lib.check(L.unetpp_optim_upload(self.args[0], C.c_void_p(self.host.data_ptr()), nbytes,
                                         C.c_void_p(torch.cuda.current_stream(device).cuda_stream)),
                   "unetpp_optim_upload")


class TableCache(collections.OrderedDict):
    """key -> Table, least recently used first.  A hit is the caller's ``get`` and ``move_to_end``; ``add`` stores a new
    table and evicts down to MAX_TABLES, skipping pinned tables."""

    def add(self, key, table: Table) -> Table:
        self[key] = table
        while len(self) > MAX_TABLES:
            del self[next(k for k, v in self.items() if not v.pinned)]
        return table
