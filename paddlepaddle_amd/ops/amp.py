"""Loss-scaling gradient pass: non-finite check + unscale, in place, over a list of tensors.

Reference: paddle/phi/kernels/gpu/amp_kernel.cu (check_finite_and_unscale), python/paddle/amp/grad_scaler.py:315.
Kernel: csrc/kernels/amp.hip — one launch covers every tensor of every dtype (fp32 / bf16 / fp16) through the same
device table + work items as the multi-tensor sum of squares (ops/multi_tensor.py, ops/optim.py).
"""
from __future__ import annotations

import torch

from . import _loader as L
from . import multi_tensor as MT

_TABLE_CACHE = {}


def _unscale_ref(tensors, inv_scale, found_inf):
    by_dtype = {}
    for g in tensors:
        by_dtype.setdefault((g.device, g.dtype), []).append(g)
    for gs in by_dtype.values():
        torch._amp_foreach_non_finite_check_and_unscale_(gs, found_inf, inv_scale)


def check_finite_and_unscale_(tensors, inv_scale, found_inf):
    """tensors[i] *= inv_scale in place; found_inf[0] = 1 if any element was inf / nan before (never cleared here,
    so several calls accumulate into one flag). ``inv_scale`` and ``found_inf`` are 1-element fp32 tensors on the
    tensors' device."""
    if not tensors:
        return
    t0 = tensors[0]
    if (L.hip_enabled_for(t0) and L.has("pa_amp_check_unscale_multi")
            and all(t.device == t0.device and t.dtype in L._DT and t.is_contiguous()
                    and L.hip_enabled_for(t) for t in tensors)):
        live = [t for t in tensors if t.numel() > 0]
        if not live:
            return
        ent = MT.cached_tables(_TABLE_CACHE, None, MT.tensor_keys(live), t0.device)
        L.call("pa_amp_check_unscale_multi", L.ptr(ent.table), L.ptr(ent.items), ent.n_items, L.ptr(inv_scale),
               L.ptr(found_inf), L.stream_ptr())
        return
    _unscale_ref(tensors, inv_scale, found_inf)
