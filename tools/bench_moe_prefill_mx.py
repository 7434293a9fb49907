"""MoE prefill microbenchmark over MXFP4 expert weights: incubate.nn.functional.fused_moe(quant_method="mxfp4") at
T = 128 / 512 / 2048 / 8192 tokens on the grouped kernels (csrc/kernels/moe_grouped_mx.hip) against the path the same
call took before them (ops.moe.moe_ffn_mx_reference, the torch fallback; up to --fallback-max-tokens, it is a host loop
over the experts) and against the bf16 grouped path on the unquantised weights (pa_grouped_gemm + swiglu).

Method (tools/bench_fp8_linear.py's): one process, device events around each call, a 512 MiB buffer rewritten before
every timed call (cold L2 / Infinity Cache), the contenders interleaved call by call, median and min-max of the repeats.
`rel err` is the Frobenius norm of (mxfp4 output - bf16 output) over that of the bf16 output, the unquantised FFN.

    python tools/bench_moe_prefill_mx.py --out profiles/moe_prefill_mx_tables.md [--reps 7]
"""
import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from bench_fp8_linear import Flusher, fmt_ms, interleaved  # noqa: E402  (tools/ is the script's directory)
import paddlepaddle_amd as paddle  # noqa: E402
from paddlepaddle_amd.ops import _loader as L  # noqa: E402
from paddlepaddle_amd.ops import moe as M  # noqa: E402

# (d, f, E, topk)
SHAPES = [(4096, 14336, 8, 2), (2048, 1408, 64, 6), (7168, 2048, 256, 8)]
TOKENS = [128, 512, 2048, 8192]
fused_moe = paddle.incubate.nn.functional.fused_moe


def bold_if_slower(ratio):
    return f"{ratio:.2f}" if ratio <= 1 else f"**{ratio:.2f}**"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/moe_prefill_mx_tables.md")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fallback-max-tokens", type=int, default=512)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe_prefill_mx needs a HIP device")
    flush = Flusher()
    p = torch.cuda.get_device_properties(0)
    lines = ["# MoE prefill: MXFP4 expert weights on the grouped block-scaled kernels", "",
             f"Box: {torch.cuda.get_device_name(0)} ({p.gcnArchName}, {p.multi_processor_count} CUs), torch "
             f"{torch.__version__}. Date: {time.strftime('%Y-%m-%d')}. Written by `tools/bench_moe_prefill_mx.py --reps "
             f"{a.reps}`: cold caches, device events, contenders interleaved; each time is the median of {a.reps} calls "
             "in ms with (min-max) behind it. `mxfp4`: fused_moe(quant_method=\"mxfp4\") on the grouped kernels. "
             "`fallback`: the same call on ops.moe.moe_ffn_mx_reference, its path before these kernels (up to "
             f"{a.fallback_max_tokens} tokens). `bf16`: fused_moe on the unquantised weights (grouped bf16 GEMMs). "
             "`TFLOP/s`: 6 T topk d f over the median mxfp4 time. `rel err`: Frobenius norm of the difference of the "
             "mxfp4 and bf16 outputs over that of the bf16 output. A ratio above 1 (mxfp4 slower) is bold.", "",
             "| d / f / E / top-k | T | mxfp4 | fallback | bf16 | mxfp4 / fallback | mxfp4 / bf16 | TFLOP/s | rel err |",
             "|" + "---|" * 9]
    for d, f, E, k in SHAPES:
        w1 = torch.empty(E, d, 2 * f, dtype=torch.bfloat16, device="cuda").normal_(0, d ** -0.5)
        w2 = torch.empty(E, f, d, dtype=torch.bfloat16, device="cuda").normal_(0, f ** -0.5)
        w1_q, w1_s, w2_q, w2_s = map(paddle.Tensor, M.quantize_experts_mx(w1, w2))
        w1, w2 = paddle.Tensor(w1), paddle.Tensor(w2)
        for T in TOKENS:
            torch.manual_seed(T)
            x = paddle.Tensor(torch.randn(T, d, device="cuda").bfloat16())
            logits = paddle.Tensor(torch.randn(T, E, device="cuda"))

            def mx(min_tokens=M.GROUPED_MX_MIN_TOKENS):
                keep, M.GROUPED_MX_MIN_TOKENS = M.GROUPED_MX_MIN_TOKENS, min_tokens
                try:
                    with torch.no_grad():
                        return fused_moe(x, logits, w1_q, w2_q, ffn1_scale=w1_s, ffn2_scale=w2_s, quant_method="mxfp4",
                                         moe_topk=k)
                finally:
                    M.GROUPED_MX_MIN_TOKENS = keep

            def bf():
                with torch.no_grad():
                    return fused_moe(x, logits, w1, w2, moe_topk=k)

            n0, fb0 = L.calls("pa_moe_grouped_up_mx"), M.CALLS["mx_fallback"]
            o_mx, o_bf = mx(T)._t.float(), bf()._t.float()
            assert L.calls("pa_moe_grouped_up_mx") == n0 + 1 and M.CALLS["mx_fallback"] == fb0
            err = float((o_mx - o_bf).norm() / o_bf.norm())
            variants = {"mxfp4": (lambda: mx(T), None), "bf16": (bf, None)}
            if T <= a.fallback_max_tokens:
                variants["fallback"] = (lambda: mx(1 << 30), None)
            res = interleaved(variants, a.reps, flush, warmup=2)
            med = {n: statistics.median(v) for n, v in res.items()}
            fb = "fallback" in res
            lines.append(f"| {d} / {f} / {E} / {k} | {T} | {fmt_ms(res['mxfp4'])} | "
                         + (fmt_ms(res["fallback"]) if fb else "not measured") + f" | {fmt_ms(res['bf16'])} | "
                         + (bold_if_slower(med["mxfp4"] / med["fallback"]) if fb else "not measured")
                         + f" | {bold_if_slower(med['mxfp4'] / med['bf16'])} | "
                         f"{6 * T * k * d * f / (med['mxfp4'] * 1e-3) / 1e12:.0f} | {err:.4f} |")
            print(lines[-1], flush=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        del w1, w2, w1_q, w1_s, w2_q, w2_s
        torch.cuda.empty_cache()
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
