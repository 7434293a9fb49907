"""fp8 linear microbenchmark: forward + backward of incubate.nn.FP8Linear against nn.Linear in bf16, and pa_fp8_quant
alone (row-major only / with transpose / with transpose and amax), at M = 8192 and the four GPT-3 13B weight shapes.

Method: one process, device events around each call, a 512 MiB buffer rewritten before every timed call (cold L2 /
Infinity Cache), the variants interleaved call by call, median and min-max of the repeats reported. FP8Linear runs the
delayed recipe in steady state (warmed up past its first call), once with the weight's fp8 pair cached (the
micro-batches of a gradient-accumulation window) and once with the weight touched before every call (an optimizer
step per call: the weight is quantized again inside the timed region). Writes the table to --out.

    python tools/bench_fp8_linear.py --out profiles/fp8_linear.md [--commit ID] [--reps 12]
"""
import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import paddlepaddle_amd as paddle  # noqa: E402
from paddlepaddle_amd.incubate.nn import FP8Linear  # noqa: E402
from paddlepaddle_amd.ops import _loader as L  # noqa: E402
from paddlepaddle_amd.ops import fp8 as F8  # noqa: E402

M = 8192
SHAPES = [(5120, 15360), (5120, 5120), (5120, 20480), (20480, 5120)]  # (K, N): qkv, proj, fc1, fc2
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12  # bytes/s: float4 copy measured / spec (MI355X_MICROARCH.md)


class Flusher:
    def __init__(self):
        self.buf = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
        self.v = 0

    def __call__(self):
        self.v = (self.v + 1) & 0x7F
        self.buf.fill_(self.v)


def timed(fn, flush, pre=None):
    if pre is not None:
        pre()
    flush()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def interleaved(variants, reps, flush, warmup=4):
    """variants: {name: (fn, pre or None)} -> {name: [ms] * reps}, one call of each per round."""
    for _ in range(warmup):
        for fn, pre in variants.values():
            if pre is not None:
                pre()
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(reps):
        for k, (fn, pre) in variants.items():
            out[k].append(timed(fn, flush, pre))
    return out


def stat(v):
    return statistics.median(v), min(v), max(v)


def fmt_ms(v):
    m, lo, hi = stat(v)
    return f"{m:.3f} ({lo:.3f}-{hi:.3f})"


def bench_linear(K, N, reps, flush):
    paddle.set_default_dtype("bfloat16")
    try:
        ref = paddle.nn.Linear(K, N)
        lin = FP8Linear.from_linear(ref, recipe="delayed")
    finally:
        paddle.set_default_dtype("float32")
    x = paddle.to_tensor(torch.randn(M, K, device="cuda").to(torch.bfloat16), stop_gradient=False)
    dy = torch.randn(M, N, device="cuda").to(torch.bfloat16) * 1e-3

    def step(layer):
        def run():
            y = layer(x)
            y._t.backward(dy)
            x._t.grad = None
            ref.weight._t.grad = None
            ref.bias._t.grad = None
        return run

    def touch():  # what an optimizer's in-place update does to the weight's version
        with torch.no_grad():
            ref.weight._t.add_(0.0)

    n0 = dict(F8.CALLS)
    res = interleaved({"bf16": (step(ref), None), "fp8 cached": (step(lin), None), "fp8 requant": (step(lin), touch)},
                      reps, flush)
    assert F8.CALLS["fallback"] == n0["fallback"] and F8.CALLS["hip"] > n0["hip"], "FP8Linear left the HIP path"
    y8, y16 = lin(x)._t.float(), ref(x)._t.float()
    err = ((y8 - y16).norm() / y16.norm()).item()
    return res, err


def bench_quant(R, C, reps, flush):
    x = torch.randn(R, C, device="cuda").to(torch.bfloat16)
    scale = torch.full((1,), 100.0, device="cuda")
    parts = F8.new_parts(x.device)
    e4 = torch.float8_e4m3fn
    variants = {
        "q": (lambda: F8.quantize_fp8(x, e4, scale, False), None),
        "q + qT": (lambda: F8.quantize_fp8(x, e4, scale, True), None),
        "q + qT + amax": (lambda: F8.quantize_fp8(x, e4, scale, True, parts), None),
    }
    n0 = L.calls("pa_fp8_quant")
    res = interleaved(variants, reps, flush)
    assert L.calls("pa_fp8_quant") > n0
    nbytes = {"q": 3 * R * C, "q + qT": 4 * R * C, "q + qT + amax": 4 * R * C}
    return res, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/fp8_linear.md")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=12)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fp8_linear needs a HIP device")
    paddle.set_device("gpu:0")
    flush = Flusher()
    lines = ["# FP8Linear against nn.Linear (bf16), forward + backward; pa_fp8_quant alone", "",
             f"Box: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}, "
             f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs), torch {torch.__version__}. "
             f"Date: {time.strftime('%Y-%m-%d')}. "
             f"Commit: {a.commit}.", "",
             f"Written by `tools/bench_fp8_linear.py --reps {a.reps}`: M = {M} rows, bf16 parameters, one process, "
             "device events around each call, a 512 MiB buffer rewritten before every timed call (cold caches), the "
             f"variants interleaved call by call; each cell is the median of {a.reps} calls with (min-max) behind it. "
             "The allocation of the outputs and every small launch of a call (scale updates, scale-inverse copies) are "
             "inside the timed region.", "",
             "## Linear, forward + backward (ms)", "",
             "`fp8 cached`: the weight's fp8 pair is reused (micro-batches of a gradient-accumulation window). "
             "`fp8 requant`: the weight is touched before every call, so its quantization is inside the timed region "
             "(one optimizer step per call). Delayed recipe in steady state. `rel. diff`: relative Frobenius "
             "difference of the fp8 layer's output from the bf16 layer's on N(0, 1) inputs.", "",
             "| K x N | bf16 | fp8 cached | fp8 requant | bf16 / fp8 cached | bf16 / fp8 requant | rel. diff |",
             "|---|---|---|---|---|---|---|"]
    for K, N in SHAPES:
        res, err = bench_linear(K, N, a.reps, flush)
        b, c, r = (statistics.median(res[k]) for k in ("bf16", "fp8 cached", "fp8 requant"))
        lines.append(f"| {K} x {N} | {fmt_ms(res['bf16'])} | {fmt_ms(res['fp8 cached'])} | "
                     f"{fmt_ms(res['fp8 requant'])} | {b / c:.2f}x | {b / r:.2f}x | {err:.3f} |")
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    lines += ["", "## pa_fp8_quant alone, bf16 -> e4m3fn (us; achieved bytes/s)", "",
              "Bytes counted: 2 per element read, 1 per element for q, 1 more for qT. HBM reference of "
              f"MI355X_MICROARCH.md: {HBM_MEASURED / 1e12:.2f} TB/s measured with a float4 copy "
              f"({HBM_SPEC / 1e12:.1f} TB/s spec); the last column is the share of the measured figure.", "",
              "| R x C | mode | us | TB/s | of 6.29 TB/s |", "|---|---|---|---|---|"]
    for R, C in [(M, 5120), (M, 20480), (5120, 15360), (5120, 20480)]:
        res, nbytes = bench_quant(R, C, a.reps, flush)
        for k, v in res.items():
            med = statistics.median(v)
            rate = nbytes[k] / (med * 1e-3)
            lines.append(f"| {R} x {C} | {k} | {med * 1e3:.1f} ({min(v) * 1e3:.1f}-{max(v) * 1e3:.1f}) | "
                         f"{rate / 1e12:.2f} | {100 * rate / HBM_MEASURED:.0f} % |")
            print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
