"""MoE prefill microbenchmark over weight-only int8 / int4 expert weights: incubate.nn.functional.fused_moe(
quant_method="weight_only_int8" | "weight_only_int4") at T = 128 / 512 / 2048 / 8192 tokens on the grouped kernels that
read the codes (csrc/kernels/moe_grouped_wo.hip) against the path the same call took before them
(ops.moe.moe_grouped_ffn_wo: dequantise both stacks to bf16 images, the bf16 grouped kernel, torch epilogues) and
against the bf16 grouped path on the unquantised weights.

Method (tools/bench_fp8_linear.py's): one process, device events around each call, a 512 MiB buffer rewritten before
every timed call (cold L2 / Infinity Cache), the contenders interleaved call by call, median and min-max of the repeats.
The last shape's T = 128 row also gets the peak allocated bytes of one call above what is resident before it.

    python tools/bench_moe_prefill_wo.py --out profiles/moe_prefill_wo_tables.md [--reps 7]
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
ALGO = {8: "weight_only_int8", 4: "weight_only_int4"}
fused_moe = paddle.incubate.nn.functional.fused_moe


def bold_if_slower(ratio):
    return f"{ratio:.2f}" if ratio <= 1 else f"**{ratio:.2f}**"


def peak_bytes(fn):
    """peak allocated bytes during one call of fn above what was allocated before it"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/moe_prefill_wo_tables.md")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))), help="indices into SHAPES")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe_prefill_wo needs a HIP device")
    flush = Flusher()
    p = torch.cuda.get_device_properties(0)
    lines = ["# MoE prefill: weight-only int8 / int4 expert weights on the grouped kernels that read the codes", "",
             f"Box: {torch.cuda.get_device_name(0)} ({p.gcnArchName}, {p.multi_processor_count} CUs), torch "
             f"{torch.__version__}. Date: {time.strftime('%Y-%m-%d')}. Written by `tools/bench_moe_prefill_wo.py --reps "
             f"{a.reps}`: cold caches, device events, contenders interleaved; each time is the median of {a.reps} calls "
             "in ms with (min-max) behind it. `int8` / `int4`: fused_moe(quant_method=\"weight_only_int8\" / "
             "\"weight_only_int4\") on the grouped kernels. `dq+grouped`: the same call on ops.moe.moe_grouped_ffn_wo, "
             "its path before these kernels. `bf16`: fused_moe on the unquantised weights (grouped bf16 GEMMs). `TFLOP/s`: "
             "6 T topk d f over the median time of the new kernels. A ratio above 1 (new kernels slower) is bold.", "",
             "| d / f / E / top-k | T | int8 | int4 | dq+grouped int8 | dq+grouped int4 | bf16 | int8 / dq+grouped | "
             "int4 / dq+grouped | int8 / bf16 | int4 / bf16 | TFLOP/s int8 / int4 |",
             "|" + "---|" * 12]
    mem = []
    for si in a.shapes:
        d, f, E, k = SHAPES[si]
        w1 = torch.empty(E, d, 2 * f, dtype=torch.bfloat16, device="cuda").normal_(0, d ** -0.5)
        w2 = torch.empty(E, f, d, dtype=torch.bfloat16, device="cuda").normal_(0, f ** -0.5)
        wq = {b: tuple(map(paddle.Tensor, M.quantize_experts_wo(w1, w2, algo))) for b, algo in ALGO.items()}
        w1, w2 = paddle.Tensor(w1), paddle.Tensor(w2)
        for T in TOKENS:
            torch.manual_seed(T)
            x = paddle.Tensor(torch.randn(T, d, device="cuda").bfloat16())
            logits = paddle.Tensor(torch.randn(T, E, device="cuda"))

            def wo(b, min_tokens):
                def run():
                    q = wq[b]
                    keep, M.GROUPED_WO_MIN_TOKENS = M.GROUPED_WO_MIN_TOKENS, min_tokens
                    try:
                        with torch.no_grad():
                            return fused_moe(x, logits, q[0], q[2], ffn1_scale=q[1], ffn2_scale=q[3],
                                             quant_method=ALGO[b], moe_topk=k)
                    finally:
                        M.GROUPED_WO_MIN_TOKENS = keep
                return run

            def bf():
                with torch.no_grad():
                    return fused_moe(x, logits, w1, w2, moe_topk=k)

            n0 = L.calls("pa_moe_grouped_up_wo"), L.calls("pa_wo_dequant"), M.CALLS["wo_fallback"]
            for b in ALGO:
                wo(b, T)(), wo(b, 1 << 30)()
            assert (L.calls("pa_moe_grouped_up_wo"), L.calls("pa_wo_dequant"), M.CALLS["wo_fallback"]) == \
                (n0[0] + 2, n0[1] + 4, n0[2])
            variants = {"int8": (wo(8, T), None), "dq8": (wo(8, 1 << 30), None), "int4": (wo(4, T), None),
                        "dq4": (wo(4, 1 << 30), None), "bf16": (bf, None)}
            res = interleaved(variants, a.reps, flush, warmup=2)
            med = {n: statistics.median(v) for n, v in res.items()}
            tf = lambda n: 6 * T * k * d * f / (med[n] * 1e-3) / 1e12
            lines.append(f"| {d} / {f} / {E} / {k} | {T} | " + " | ".join(fmt_ms(res[n]) for n in
                                                                          ("int8", "int4", "dq8", "dq4", "bf16"))
                         + f" | {bold_if_slower(med['int8'] / med['dq8'])} | {bold_if_slower(med['int4'] / med['dq4'])}"
                         f" | {bold_if_slower(med['int8'] / med['bf16'])} | {bold_if_slower(med['int4'] / med['bf16'])}"
                         f" | {tf('int8'):.0f} / {tf('int4'):.0f} |")
            print(lines[-1], flush=True)
            if si == a.shapes[-1] and T == TOKENS[0]:
                torch.cuda.empty_cache()
                mem = ["", f"Peak allocated bytes of one call above the resident tensors, {d} / {f} / {E} / {k}, T = {T} "
                       f"(the transient images are E 3 f d 2 = {E * 3 * f * d * 2 / 2 ** 30:.2f} GiB):", ""]
                for b in ALGO:
                    mem.append(f"- int{b}: dq+grouped {peak_bytes(wo(b, 1 << 30)) / 2 ** 30:.3f} GiB, grouped kernels "
                               f"{peak_bytes(wo(b, T)) / 2 ** 30:.3f} GiB")
                print("\n".join(mem), flush=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines + mem) + "\n")
        del w1, w2, wq
        torch.cuda.empty_cache()
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
