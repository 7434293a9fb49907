#!/usr/bin/env python3
"""Step time of ``paddle.optimizer.Lamb`` on a BERT-large-like parameter list (24 layers, h 1024, ffn 4096, biases and
norm weights, embeddings; bf16 parameters and gradients with fp32 masters): the fused multi-tensor path
(csrc/kernels/lamb.hip) against the per-parameter path, forced by hiding the launcher, and AdamW on the same list for
scale. One process, rounds alternating between the three, median and minimum over the rounds; a step is timed by a
host clock around ``steps`` steps that end in a device synchronise.

Bytes per element: LAMB 40 + 2 (stage 1 reads p, g, m, v and writes m, v; stage 2 reads p, m, v and writes p and the
shadow; g counted as fp32), AdamW 28 + 2 (one pass, bf16 g). Prints one JSON line; needs a HIP device.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import paddlepaddle_amd as paddle  # noqa: E402
from paddlepaddle_amd.ops import _loader as L  # noqa: E402

LAMB_BYTES, ADAMW_BYTES = 42, 30


def bert_large_shapes(layers=24, h=1024, ffn=4096, vocab=30522, positions=512):
    shapes = [(vocab, h), (positions, h), (2, h), (h,), (h,)]
    for _ in range(layers):
        shapes += [(h, h), (h,)] * 4 + [(h,), (h,)] + [(h, ffn), (ffn,), (ffn, h), (h,)] + [(h,), (h,)]
    return shapes + [(h, h), (h,)]


def make_params(shapes, tag, dev):
    ps = []
    for i, s in enumerate(shapes):
        g = torch.Generator(device=dev).manual_seed(i)
        w = (torch.randn(s, device=dev, generator=g) * 0.02).to(torch.bfloat16)
        p = paddle.Parameter(w, name=f"{tag}_{i}")
        p._t.grad = (torch.randn(s, device=dev, generator=g) * 1e-2).to(torch.bfloat16)
        ps.append(p)
    return ps


def timed(opt, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


class _OpCount(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def launches(opt):
    """Device launches of one step: every ATen operator the step dispatches (each at least one kernel; a _foreach
    operator over the whole list is a handful) plus the kernels behind the native calls (pa_lamb_multi: 3,
    pa_adamw_multi: 1, pa_adam_hyper_step: 1)."""
    L.reset_calls()
    with _OpCount() as c:
        opt.step()
    torch.cuda.synchronize()
    per_call = {"pa_lamb_multi": 3}
    return {"aten_ops": c.n, "native_kernels": sum(per_call.get(k, 1) * v for k, v in L.CALLS.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50, help="timed steps per round of a fused path")
    ap.add_argument("--slow-steps", type=int, default=5, help="timed steps per round of the per-parameter path")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lamb needs a HIP device")
    dev = torch.device("cuda:0")
    shapes = bert_large_shapes(a.layers)
    numel = sum(torch.Size(s).numel() for s in shapes)
    hidden = []
    real_has = L.has
    L.has = lambda name: name not in hidden and real_has(name)

    def lamb(tag):
        return paddle.optimizer.Lamb(1e-3, lamb_weight_decay=0.01, parameters=make_params(shapes, tag, dev),
                                     multi_precision=True)

    arms = {"lamb_fused": (lamb("f"), a.steps, ()), "lamb_per_param": (lamb("s"), a.slow_steps, ("pa_lamb_multi",)),
            "adamw_fused": (paddle.optimizer.AdamW(1e-3, parameters=make_params(shapes, "a", dev), weight_decay=0.01,
                                                   multi_precision=True), a.steps, ())}
    times = {k: [] for k in arms}
    calls = {}
    for rnd in range(a.rounds + 1):  # round 0 warms every arm up and is dropped
        for name, (opt, steps, hide) in arms.items():
            hidden[:] = hide
            L.reset_calls()
            ms = timed(opt, 2 if rnd == 0 else steps)
            calls[name] = {k: v / (2 if rnd == 0 else steps) for k, v in L.CALLS.items() if "multi" in k}
            if rnd:
                times[name].append(ms)
    res = {"tensors": len(shapes), "elements": numel, "rounds": a.rounds}
    for name, ts in times.items():
        nbytes = numel * (ADAMW_BYTES if name.startswith("adamw") else LAMB_BYTES)
        med = statistics.median(ts)
        res[name] = {"ms_median": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                     "TB_per_s_at_median": round(nbytes / (med * 1e-3) / 1e12, 3), "native_calls_per_step": calls[name]}
    res["speedup_fused_over_per_param"] = round(res["lamb_per_param"]["ms_median"] / res["lamb_fused"]["ms_median"], 2)
    for name, (opt, _, hide) in arms.items():
        hidden[:] = hide
        res[name]["launches_per_step"] = launches(opt)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
