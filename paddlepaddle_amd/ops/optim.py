"""Multi-tensor optimizer kernels (HIP).

Reference: paddle/phi/kernels/gpu/fused_adam_kernel.cu (multi-tensor Adam/AdamW with master
weights), adamw_kernel.cu.
Kernel: csrc/kernels/adamw.hip — one launch updates every tensor of a parameter group:
a device-side table of {param_fp32, grad, m, v, param_lowp, numel, dtypes, wd, lr_mult} rows,
workgroups walk fixed-size chunks (work list computed on the host once and cached, ops/multi_tensor.py),
fp32 math, optional bf16/fp16 shadow copy written in the same pass, grads unscaled
by 1/loss_scale. The optimizers (optimizer/adam.py, optimizer/others.py) make their own rows;
this module holds the multi-tensor sum of squares.
"""
from __future__ import annotations

import torch

from . import _loader as L
from . import multi_tensor as MT

_SQ_CACHE = {}


def global_sq_norm(tensors):
    """Sum of squares over a list of tensors (fp32 0-d tensor): one multi-tensor HIP launch."""
    if not tensors:
        return None
    t0 = tensors[0]
    if L.hip_enabled_for(t0) and L.has("pa_sq_norm_multi") and all(t.is_contiguous() for t in tensors):
        ent = MT.cached_tables(_SQ_CACHE, None, MT.tensor_keys(tensors), t0.device,
                               extra=lambda: torch.empty(1024, dtype=torch.float32, device=t0.device))
        partial = ent.extra  # one float per workgroup
        L.call("pa_sq_norm_multi", L.ptr(ent.table), L.ptr(ent.items), ent.n_items, L.ptr(partial), L.stream_ptr())
        return partial.sum()
    return torch.stack([t.float().pow(2).sum() for t in tensors]).sum()
