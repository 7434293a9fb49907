"""Host side of the multi-tensor launches (csrc/kernels/multi_tensor.h): device tables, work items and their cache.

A multi-tensor kernel (AdamW / Momentum / LAMB update, sum of squares, loss-scaling unscale) takes a device table of
int64 rows, one per tensor, and ``[tensor index, start element]`` work items, one per ``CHUNK`` elements. A row starts
with its key columns: every pointer the kernel follows, then the element count and the dtype word. Scalar columns
(weight decay, lr multiplier) follow. ``cached_tables`` keeps the uploaded tables until a key column changes:
optimizers hold one entry per parameter group, module-level users (norm, unscale) up to 64 in a dict of their own. A
module-level entry built while a hipGraph is being captured is written by captured kernels: only a replay of that graph
fills it.
"""
from __future__ import annotations

import collections
import ctypes
import struct

import torch

from . import _loader as L

CHUNK = 16384      # elements per work item (csrc/kernels/multi_tensor.h kChunk, exported as pa_multi_tensor_chunk)
NO_SHADOW = 3      # low-precision dtype code of an update row without a shadow copy (kNoShadow)
MODULE_BOUND = 64  # entries of a module-level cache

Tables = collections.namedtuple("Tables", "key table items n_items hosts extra")


def f32_bits(x):
    """The float32 bit pattern of ``x`` as an int: how scalar columns travel in an int64 row."""
    return struct.unpack("<i", struct.pack("<f", float(x)))[0]


def device_table(rows, dev):
    """int64 pointer / work-item table on ``dev`` (and the host buffer it came from). Eager: a pinned
    non-blocking copy. Inside a hipGraph capture (a captured optimizer step) the values are written by kernels
    that carry them as launch arguments (pa_write_i64), so the graph holds no reference to host memory."""
    host = torch.as_tensor(rows, dtype=torch.int64)
    if dev.type == "cuda":
        if torch.cuda.is_current_stream_capturing() and L.has("pa_write_i64"):
            out = torch.empty(host.shape, dtype=torch.int64, device=dev)
            L.call("pa_write_i64", L.ptr(out), ctypes.c_void_p(host.data_ptr()), host.numel(), L.stream_ptr())
            return out, host
        host = host.pin_memory()
    return host.to(dev, non_blocking=True), host


def item_offsets(numels):
    """int64 ``[n + 1]``: tensor ``i`` of a launch over ``numels`` owns the work items ``[off[i], off[i + 1])``,
    ``ceil(numel / CHUNK)`` of them (none for an empty tensor). What a per-tensor reduction over item partials
    (csrc/kernels/lamb.hip) walks."""
    per = (torch.tensor(numels, dtype=torch.int64) + (CHUNK - 1)) // CHUNK
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(per, 0)])


def build_tables(rows, numels, dev):
    """``(table, items, n_items, hosts)`` of one launch: ``rows`` on ``dev`` ([n, cols]), the [n_items, 2] work list
    in tensor order (the items of ``item_offsets``) and the host twins, which must outlive the asynchronous
    copies."""
    table, table_host = device_table(rows, dev)
    off = item_offsets(numels)
    first = off[:-1]  # position of each tensor's first item
    index = torch.repeat_interleave(torch.arange(len(numels)), off[1:] - first)
    start = (torch.arange(index.numel()) - first[index]) * CHUNK
    items, items_host = device_table(torch.stack([index, start], 1), dev)
    return table, items, index.numel(), (table_host, items_host)


def cached_tables(cache, slot, keys, dev, scalars=None, extra=None):
    """The ``Tables`` of one launch from ``cache``, built on a miss. ``keys``: per tensor the tuple of its row's key
    columns (pointers..., numel, dtype word); with ``dev`` they are the key of the entry. ``scalars()`` gives the
    scalar columns that complete the rows and ``extra()`` what else lives with the entry, both on a miss only. So
    scalar columns are outside the key: a group whose ``weight_decay`` or lr multiplier is edited after the first step
    keeps its old table. ``slot`` names the one entry its caller owns (an optimizer's parameter group), replaced when
    the key changes; ``slot=None`` (module-level users) files the entry under its key, and clears ``cache`` first
    when it already holds ``MODULE_BOUND`` entries."""
    key = (dev, *keys)
    where = key if slot is None else slot
    ent = cache.get(where)
    if ent is None or ent.key != key:
        rows = keys if scalars is None else [k + s for k, s in zip(keys, scalars())]
        ent = Tables(key, *build_tables(rows, [k[-2] for k in keys], dev), extra() if extra else None)
        if slot is None and len(cache) >= MODULE_BOUND:
            cache.clear()
        cache[where] = ent
    return ent


def tensor_keys(tensors):
    """(ptr, numel, dtype) rows of the norm and unscale kernels (TensorRow): every column is a key column."""
    return [(t.data_ptr(), t.numel(), L._DT[t.dtype]) for t in tensors]
