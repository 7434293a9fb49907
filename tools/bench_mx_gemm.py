"""MX linear microbenchmark: pa_mx_quant, pa_gemm_mx (M = 8192) and pa_gemm_mx_small_m (M = 1 / 16 / 32 / 64) against
the paths the same linear has without MX: the bf16 GEMM ops.linear picks, gemm_fp8 on per-tensor e4m3 operands and,
for decode, wo_linear with int4 weights. LLaMA-2 7B and 70B linear shapes.

Method (tools/bench_fp8_linear.py's): one process, device events around each call, a 512 MiB buffer rewritten before
every timed call (cold L2 / Infinity Cache), the contenders interleaved call by call, median and min-max of the repeats.
Output allocation is inside the timed region. Writes the tables to --out.

    python tools/bench_mx_gemm.py --out profiles/mx_gemm_tables.md [--reps 7] [--only decode|prefill]
"""
import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from bench_fp8_linear import Flusher, fmt_ms, interleaved  # noqa: E402  (tools/ is the script's directory)
from paddlepaddle_amd.ops import _loader as L  # noqa: E402
from paddlepaddle_amd.ops import fp8 as F8  # noqa: E402
from paddlepaddle_amd.ops import linear as LIN  # noqa: E402
from paddlepaddle_amd.ops import mx as MX  # noqa: E402
from paddlepaddle_amd.ops import quant as Q  # noqa: E402

# (K, N): qkv, o, gate+up, down
SHAPES = {"7B": [(4096, 12288), (4096, 4096), (4096, 22016), (11008, 4096)],
          "70B": [(8192, 10240), (8192, 8192), (8192, 57344), (28672, 8192)]}
E4 = torch.float8_e4m3fn


def contenders(M, K, N, decode):
    x = torch.randn(M, K, device="cuda").bfloat16()
    w = (torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16()
    w_q, w_s = MX.quantize_mx(w, "mxfp4")
    a8, a4 = MX.quantize_mx(x, "mxfp8"), MX.quantize_mx(x, "mxfp4")
    x8, w8 = x.to(E4), w.to(E4)
    v = {"bf16": (lambda: LIN.linear_nt(x, w), None),
         "fp8": (lambda: F8.gemm_fp8(x8, w8, out_dtype=torch.bfloat16), None),
         "mx quant": (lambda: MX.quantize_mx(x, "mxfp8"), None),
         "mxfp8 x mxfp4": (lambda: MX.gemm_mx(*a8, "mxfp8", w_q, w_s), None),
         "mxfp4 x mxfp4": (lambda: MX.gemm_mx(*a4, "mxfp4", w_q, w_s), None),
         "mx_linear": (lambda: MX.mx_linear(x, w_q, w_s), None)}
    if decode:
        wi = torch.randint(-128, 128, (N // 2, K), device="cuda", dtype=torch.int8)
        si = torch.rand(N, device="cuda") * 0.01
        v["wo int4"] = (lambda: Q.wo_linear(x, wi, si, None, 4, -1), None)
    return v


def table(M, reps, flush, lines):
    decode = M <= 64
    names = ["bf16", "fp8", "mx quant", "mxfp8 x mxfp4", "mxfp4 x mxfp4", "mx_linear"] + (["wo int4"] if decode else [])
    rate = "weight TB/s (mxfp8 x mxfp4)" if decode else "PFLOP/s (mxfp8 x mxfp4 / mxfp4 x mxfp4)"
    lines += ["", f"## M = {M} (ms)", "", "| model | K x N | " + " | ".join(names) + f" | {rate} |",
              "|" + "---|" * (len(names) + 3)]
    launcher = "pa_gemm_mx_small_m" if decode else "pa_gemm_mx"
    for model, shapes in SHAPES.items():
        for K, N in shapes:
            n0 = L.calls(launcher)
            res = interleaved(contenders(M, K, N, decode), reps, flush, warmup=2)
            assert L.calls(launcher) > n0, f"{launcher} did not run"
            t8, t4 = (statistics.median(res[k]) * 1e-3 for k in ("mxfp8 x mxfp4", "mxfp4 x mxfp4"))
            r = f"{N * K * (0.5 + 1 / 32) / t8 / 1e12:.2f}" if decode else \
                f"{2 * M * N * K / t8 / 1e15:.2f} / {2 * M * N * K / t4 / 1e15:.2f}"
            lines.append(f"| {model} | {K} x {N} | " + " | ".join(fmt_ms(res[k]) for k in names) + f" | {r} |")
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()


def format_error(lines):
    """Relative Frobenius error of the MX linear against the unquantised bf16 linear: a property of the format."""
    x = torch.randn(1024, 4096, device="cuda").bfloat16()
    w = (torch.randn(4096, 4096, device="cuda") / 64).bfloat16()
    ref = x.float() @ w.float().t()
    w_q, w_s = MX.quantize_mx(w, "mxfp4")
    lines += ["", "## Error of the format", "", "Relative Frobenius error against the fp32 product of the bf16 operands, "
              "x ~ N(0, 1) [1024, 4096], w ~ N(0, 1) / 64 [4096, 4096], mxfp4 weight:", ""]
    for f in ("mxfp8", "mxfp4"):
        err = ((MX.mx_linear(x, w_q, w_s, act_fmt=f).float() - ref).norm() / ref.norm()).item()
        lines.append(f"- activations {f}: {err:.4f}")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mx_gemm_tables.md")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["decode", "prefill"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mx_gemm needs a HIP device")
    flush = Flusher()
    p = torch.cuda.get_device_properties(0)
    lines = ["# MX linear: pa_mx_quant, pa_gemm_mx, pa_gemm_mx_small_m against bf16 / fp8 / int4 weight-only", "",
             f"Box: {torch.cuda.get_device_name(0)} ({p.gcnArchName}, {p.multi_processor_count} CUs), torch "
             f"{torch.__version__}. Date: {time.strftime('%Y-%m-%d')}. Written by `tools/bench_mx_gemm.py --reps "
             f"{a.reps}`: cold caches, device events, contenders interleaved; each cell is the median of {a.reps} calls "
             "with (min-max) behind it. `fp8`: gemm_fp8 on operands quantised beforehand. `mx quant`: pa_mx_quant of "
             "the activations to mxfp8 alone. `mx_linear`: quantiser and GEMM together (activations mxfp8)."]
    for M in ([] if a.only == "decode" else [8192]) + ([] if a.only == "prefill" else [1, 16, 32, 64]):
        table(M, a.reps, flush, lines)
    format_error(lines)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
