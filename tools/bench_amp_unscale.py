#!/usr/bin/env python3
"""A/B of the loss-scaling gradient pass on one GPU: the HIP multi-tensor kernel (ops/amp.py, one launch for all
dtypes) against torch._amp_foreach_non_finite_check_and_unscale_ (one launch group per dtype), in place, alternating
in one process.

Workload (a user-sized gradient set): 40 bf16 buffers of 64 Mi elements + 8 fp32 buffers of 1 Mi elements.
torch's foreach kernel has no bf16 instantiation on the GPU (it raises "not implemented for 'BFloat16'"), so the
A/B runs on an fp16 stand-in of the same shapes (same element size, same bytes); the HIP kernel is also timed on
the bf16 workload itself.
Bytes per call = 2 x buffer bytes (every element read once and written once), computed from the shapes.
Each repeat times each arm with device events over a window of at least ``--window`` seconds.

    python tools/bench_amp_unscale.py [--out profiles/amp_unscale.md]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_MEASURED_TBS = 6.29  # float4 copy on the MI355X (8.0 TB/s specified)


def shapes(scale=1.0):
    import torch
    big = max(1, int((64 << 20) * scale))
    small = max(1, int((1 << 20) * scale))
    return [(big, torch.bfloat16)] * 40 + [(small, torch.float32)] * 8


def bytes_per_call(shp):
    import torch
    return 2 * sum(n * torch.empty(0, dtype=dt).element_size() for n, dt in shp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="least timed seconds per arm and repeat")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the buffers (rehearsal only)")
    ap.add_argument("--out", default=None, help="write the markdown report here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_amp_unscale: needs a HIP device (no CPU fallback for a timing)")
    from paddlepaddle_amd.ops import _loader as L
    from paddlepaddle_amd.ops.amp import check_finite_and_unscale_

    dev = torch.device("cuda", 0)
    shp = shapes(args.scale)
    g = torch.Generator(device=dev).manual_seed(0)
    bufs = [(torch.randn(n, device=dev, generator=g) * 1024).to(dt) for n, dt in shp]
    # the same gradient set with fp16 in place of bf16: what both arms can run
    half = [b.to(torch.float16) if b.dtype == torch.bfloat16 else b.clone() for b in bufs]
    nbytes = bytes_per_call(shp)
    # scale 1: the pass costs the same and the data stays as generated over thousands of in-place calls
    inv = torch.ones(1, dtype=torch.float32, device=dev)
    found = torch.zeros(1, dtype=torch.float32, device=dev)
    by_dtype = {}
    for b in half:
        by_dtype.setdefault(b.dtype, []).append(b)

    def hip_bf16():
        check_finite_and_unscale_(bufs, inv, found)

    def hip():
        check_finite_and_unscale_(half, inv, found)

    def ref():
        for gs in by_dtype.values():
            torch._amp_foreach_non_finite_check_and_unscale_(gs, found, inv)

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n  # ms per call

    L.reset_calls()
    arms = (("hip", hip), ("torch", ref), ("hip_bf16", hip_bf16))
    for _, fn in arms:  # warm up: code objects, tables, allocator
        timed(fn, 5)
    assert L.calls("pa_amp_check_unscale_multi") == 10, "the HIP arms did not run the HIP kernel"
    n_calls = {}
    for name, fn in arms:
        n_calls[name] = max(10, int(args.window * 1e3 / timed(fn, 10)) + 1)
    res = {name: [] for name, _ in arms}
    for _ in range(args.repeats):
        for name, fn in arms:
            res[name].append(timed(fn, n_calls[name]))
    assert float(found.item()) == 0.0

    def tbs(ms):
        return nbytes / (ms * 1e-3) / 1e12

    lines = ["# Loss-scaling unscale pass: HIP multi-tensor kernel vs torch foreach", "",
             f"Device: {torch.cuda.get_device_name(0)}. Workload: 40 bf16 buffers of {shp[0][0]} elements + 8 fp32 "
             f"buffers of {shp[-1][0]} elements, in place. Bytes per call = 2 x buffer bytes = {nbytes} "
             f"({nbytes / 2**30:.2f} GiB), from the shapes.",
             "Arms: `hip` and `torch` run the fp16 stand-in of the workload (torch's foreach kernel has no bf16 "
             "instantiation on the GPU and raises for bf16 gradients); `hip_bf16` is the HIP kernel on the bf16 workload.",
             f"Arms alternate in one process; each figure is the mean call time over a device-event window of at "
             f"least {args.window} s; {args.repeats} repeats.", "",
             "| arm | calls / window | ms per call (each repeat) | median ms | min ms | max ms | median TB/s | "
             "share of measured HBM copy rate (6.29 TB/s) | share of specified HBM peak (8.0 TB/s) |",
             "|---|---|---|---|---|---|---|---|---|"]
    med = {}
    for name in ("hip", "torch", "hip_bf16"):
        r = res[name]
        med[name] = statistics.median(r)
        lines.append(f"| {name} | {n_calls[name]} | {', '.join(f'{x:.4f}' for x in r)} | {med[name]:.4f} | "
                     f"{min(r):.4f} | {max(r):.4f} | {tbs(med[name]):.3f} | "
                     f"{100 * tbs(med[name]) / HBM_MEASURED_TBS:.1f}% | {100 * tbs(med[name]) / 8.0:.1f}% |")
    spread = max(max(res[k]) - min(res[k]) for k in ("hip", "torch"))
    diff = med["hip"] - med["torch"]
    lines += ["", f"Same-call spread (largest max - min of an arm over the repeats): {spread:.4f} ms. "
                  f"HIP median - torch median: {diff:+.4f} ms ({100 * diff / med['torch']:+.1f}%).",
              "The TB/s figures are algorithm bytes over call time (launch gaps included), not a kernel-only rate.", ""]
    if diff <= spread:
        lines.append("Decision: the HIP path is not slower than the torch arm by more than the spread; it stays the "
                     "GPU default.")
    else:
        lines.append("Decision: the HIP path is slower than the torch arm by more than the spread. It is kept as the "
                     "default only for the sharding engine's flat buffers.")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
