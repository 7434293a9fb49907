"""Dynamic loss scaling. Reference: python/paddle/amp/grad_scaler.py:62 AmpScaler, :657 GradScaler.
The found-inf check and the unscale are one multi-tensor pass over the gradients (ops/amp.py: one HIP launch
for all dtypes on the GPU) with a device-side found_inf flag. Under sharding / tensor / pipeline parallelism the
flag is max-reduced over the scaler's ``_found_inf_groups`` so every rank takes or skips the same step; the host
reads it once per step, in step()."""
from __future__ import annotations

from enum import Enum

import torch
import torch.distributed as dist

from ..framework.tensor import Tensor, _wrap


class OptimizerState(Enum):
    INIT = 0
    UNSCALED = 1
    STEPPED = 2


def add_found_inf_groups(scaler, groups):
    """Add communication groups (``Group`` objects; None = the world group) over which ``scaler`` max-reduces its
    found_inf flag. Groups of one rank and groups already present (same ranks) are left out."""
    have = {ranks for ranks, _ in scaler._found_inf_groups}
    out = list(scaler._found_inf_groups)
    for g in groups:
        if g is None:
            if not (dist.is_available() and dist.is_initialized()):
                continue
            ranks, pg = tuple(range(dist.get_world_size())), None
        else:
            ranks, pg = tuple(g.ranks), g.process_group
        if len(ranks) > 1 and ranks not in have:
            have.add(ranks)
            out.append((ranks, pg))
    scaler._found_inf_groups = tuple(out)
    return scaler


class AmpScaler:
    _found_inf_groups = ()  # ((ranks, process group), ...): orthogonal groups, reduced one after the other

    def __init__(self, enable=True, init_loss_scaling=2.0 ** 15, incr_ratio=2.0, decr_ratio=0.5,
                 incr_every_n_steps=1000, decr_every_n_nan_or_inf=1, use_dynamic_loss_scaling=True):
        self._enable = enable
        self._scale = float(init_loss_scaling) if enable else 1.0
        self._incr_ratio, self._decr_ratio = incr_ratio, decr_ratio
        self._incr_every_n_steps, self._decr_every_n_nan_or_inf = incr_every_n_steps, decr_every_n_nan_or_inf
        self._use_dynamic = use_dynamic_loss_scaling
        self._incr_count = 0
        self._decr_count = 0
        self._found_inf = None
        self._found_host = None  # (flag tensor, its host value): read once per step
        self._opt_states = {}
        self._scale_t = None

    def is_enable(self):
        return self._enable

    def is_use_dynamic_loss_scaling(self):
        return self._use_dynamic

    def get_init_loss_scaling(self):
        return self._scale

    def set_init_loss_scaling(self, v):
        self._scale = float(v)

    def scale(self, var):
        if not self._enable:
            return var
        return _wrap(var._t * self._scale)

    def _amp_grads_of(self, optimizer):
        fn = getattr(optimizer, "_amp_grads", None)
        if fn is not None:  # optimizers whose gradients do not hang off _parameter_list (sharding engine)
            return [g for g in fn() if g is not None]
        return [p._t.grad for p in optimizer._parameter_list if p._t.grad is not None]

    def _sync_found_inf(self, found):
        """MAX over every group in turn (orthogonal groups: the result is the global flag). Runs on ranks without
        gradients too, so all members issue the same collectives."""
        for _, pg in self._found_inf_groups:
            want = "cpu" if dist.get_backend(pg) == "gloo" else "cuda"
            if found.device.type != want:
                found = found.cpu() if want == "cpu" else found.to(torch.device("cuda", torch.cuda.current_device()))
            dist.all_reduce(found, op=dist.ReduceOp.MAX, group=pg)
        return found

    def unscale_(self, optimizer):
        if not self._enable:
            return
        st = self._opt_states.get(id(optimizer), OptimizerState.INIT)
        if st == OptimizerState.UNSCALED:
            return
        grads = self._amp_grads_of(optimizer)
        if not grads:
            self._found_inf = self._sync_found_inf(torch.zeros(1))
            return
        from ..ops.amp import check_finite_and_unscale_
        dev = grads[0].device
        found = torch.zeros(1, dtype=torch.float32, device=dev)
        inv = torch.full((1,), 1.0 / self._scale, dtype=torch.float32, device=dev)
        check_finite_and_unscale_(grads, inv, found)
        self._found_inf = self._sync_found_inf(found)
        self._opt_states[id(optimizer)] = OptimizerState.UNSCALED

    def _found(self):
        """The step's found_inf as a host bool: one device read per flag tensor, kept until update()."""
        src = self._found_inf
        if self._found_host is None or self._found_host[0] is not src:
            self._found_host = (src, src is not None and bool(src.item()))
        return self._found_host[1]

    def minimize(self, optimizer, *args, **kwargs):
        self.step(optimizer)
        self.update()
        return None, None

    def step(self, optimizer):
        if not self._enable:
            optimizer.step()
            return
        self.unscale_(optimizer)
        if self._found():
            self._opt_states[id(optimizer)] = OptimizerState.STEPPED
            self._skip = True
            return
        self._skip = False
        optimizer.step()
        self._opt_states[id(optimizer)] = OptimizerState.STEPPED

    def update(self):
        if not self._enable:
            return
        found = self._found()  # read by step(); lazily here only when step() was not called
        if self._use_dynamic:
            if found:
                self._incr_count = 0
                self._decr_count += 1
                if self._decr_count >= self._decr_every_n_nan_or_inf:
                    self._scale = max(self._scale * self._decr_ratio, 1.0)
                    self._decr_count = 0
            else:
                self._decr_count = 0
                self._incr_count += 1
                if self._incr_count >= self._incr_every_n_steps:
                    self._scale *= self._incr_ratio
                    self._incr_count = 0
        self._opt_states = {}
        self._found_inf = None
        self._found_host = None

    def state_dict(self):
        return {"scale": self._scale, "incr_ratio": self._incr_ratio, "decr_ratio": self._decr_ratio,
                "incr_every_n_steps": self._incr_every_n_steps,
                "decr_every_n_nan_or_inf": self._decr_every_n_nan_or_inf, "incr_count": self._incr_count,
                "decr_count": self._decr_count, "use_dynamic_loss_scaling": self._use_dynamic}

    def load_state_dict(self, sd):
        self._scale = float(sd["scale"])
        self._incr_count = sd.get("incr_count", 0)
        self._decr_count = sd.get("decr_count", 0)

    set_state_dict = load_state_dict


class GradScaler(AmpScaler):
    def __init__(self, enable=True, init_loss_scaling=65536.0, incr_ratio=2.0, decr_ratio=0.5,
                 incr_every_n_steps=2000, decr_every_n_nan_or_inf=1, use_dynamic_loss_scaling=True):
        super().__init__(enable, init_loss_scaling, incr_ratio, decr_ratio, incr_every_n_steps,
                         decr_every_n_nan_or_inf, use_dynamic_loss_scaling)

    def get_loss_scaling(self):
        return self._scale
