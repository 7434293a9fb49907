"""Multi-tensor optimizer kernels (HIP).

Reference: paddle/phi/kernels/gpu/fused_adam_kernel.cu (multi-tensor Adam/AdamW with master
weights), adamw_kernel.cu.
Kernel: csrc/kernels/adamw.hip — one launch updates every tensor of a parameter group:
a device-side table of {param_fp32, grad, m, v, param_lowp, numel, dtypes, wd, lr_mult} rows,
workgroups walk fixed 16384-element chunks (persistent-style work list computed on the host once
and cached), fp32 math, optional bf16/fp16 shadow copy written in the same pass, grads unscaled
by 1/loss_scale. The optimizers (optimizer/adam.py, optimizer/others.py) build their own row
tables; this module holds the table upload and the multi-tensor sum of squares.
"""
from __future__ import annotations

import ctypes

import torch

from . import _loader as L

_CHUNK = 16384  # elements per work item


def device_table(rows, dev):
    """int64 pointer / work-item table on ``dev`` (and the host buffer it came from). Eager: a pinned
    non-blocking copy. Inside a hipGraph capture (a captured optimizer step) the values are written by kernels
    that carry them as launch arguments (pa_write_i64), so the graph holds no reference to host memory."""
    host = torch.tensor(rows, dtype=torch.int64)
    if dev.type == "cuda":
        if torch.cuda.is_current_stream_capturing() and L.has("pa_write_i64"):
            out = torch.empty(host.shape, dtype=torch.int64, device=dev)
            L.call("pa_write_i64", L.ptr(out), ctypes.c_void_p(host.data_ptr()), host.numel(), L.stream_ptr())
            return out, host
        host = host.pin_memory()
    return host.to(dev, non_blocking=True), host


_SQ_CACHE = {}


def global_sq_norm(tensors):
    """Sum of squares over a list of tensors (fp32 0-d tensor): one multi-tensor HIP launch."""
    if not tensors:
        return None
    t0 = tensors[0]
    if L.hip_enabled_for(t0) and L.has("pa_sq_norm_multi") and all(t.is_contiguous() for t in tensors):
        # the table rows hold {ptr, numel, dtype}: all three are the key (the caching allocator hands the same
        # address to tensors of another length or type)
        key = tuple((t.data_ptr(), t.numel(), t.dtype) for t in tensors)
        ent = _SQ_CACHE.get(key)
        if ent is None:
            rows, items = [], []
            for i, t in enumerate(tensors):
                rows.append([t.data_ptr(), t.numel(), L._DT[t.dtype]])
                for s in range(0, t.numel(), _CHUNK):
                    items.append([i, s])
            ent = (torch.tensor(rows, dtype=torch.int64).to(t0.device), torch.tensor(items, dtype=torch.int64).to(t0.device),
                   len(items), torch.empty(1024, dtype=torch.float32, device=t0.device))
            if len(_SQ_CACHE) > 64:
                _SQ_CACHE.clear()
            _SQ_CACHE[key] = ent
        table, items, n, partial = ent
        L.call("pa_sq_norm_multi", L.ptr(table), L.ptr(items), n, L.ptr(partial), L.stream_ptr())
        return partial.sum()
    return torch.stack([t.float().pow(2).sum() for t in tensors]).sum()
