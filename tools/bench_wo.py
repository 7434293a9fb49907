"""``--prefill``: the prefill GEMM on the codes (csrc/kernels/wo_gemm_prefill.hip) against per-call dequantise + bf16
GEMM and the bf16 GEMM on a cached image, LLaMA-2 7B / 70B linear shapes at M = 256 .. 8192, int8 / int4, per-channel
and group-128 scales: the three paths alternate in one run, caches flushed before every timed call, device events,
minimum and median of ``--reps`` rounds after a warm-up per shape, with the transient bytes of each path.
Default: decode-shape microbench of the weight-only GEMMs (ops/quant.py, csrc/kernels/wo_gemm.hip) against bf16 GEMMs on
the same shapes: hipBLASLt (torch.mm) and this framework's small-M bf16 kernel (ops.gemm.gemm_small_m).
LLaMA-2 7B / GPT-3 13B projection shapes, M = 1 .. 64 rows, median of 3 rounds x 50 launches."""
import argparse
import ctypes
import sys

import torch

sys.path.insert(0, ".")
import paddlepaddle_amd as paddle  # noqa: E402
from paddlepaddle_amd.nn import quant as Q  # noqa: E402
from paddlepaddle_amd.ops import gemm as G  # noqa: E402
from paddlepaddle_amd.ops import quant as OQ  # noqa: E402


def timeit(fn, iters=50):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1000.0  # us


PREFILL_SHAPES = {"7b": [(4096, 4096), (4096, 11008), (11008, 4096)],      # (K, N)
                  "70b": [(8192, 8192), (8192, 28672), (28672, 8192)]}


def prefill(which, reps):
    """one markdown row per point: times in us as min / median, then wo / dequant+GEMM and wo / cached-image ratios of
    the minima (bold when the new kernel is the slower one) and the transient MiB of wo | dequant+GEMM"""
    dev = torch.cuda.current_device()
    print("| K | N | M | format | tile x splits | wo | dequant + GEMM | cached image | wo / dq | wo / img | transient MiB |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for K, N in [s for w in which for s in PREFILL_SHAPES[w]]:
        for bits, group in ((8, -1), (8, 128), (4, -1), (4, 128)):
            q = torch.randint(-128, 128, (N * bits // 8, K), device="cuda", dtype=torch.int8)
            sc = torch.rand((N,) if group == -1 else (K // group, N), device="cuda") * 0.01 + 0.001
            img = OQ.dequantize(q, sc, bits, group, K, N)
            for M in (256, 512, 2048, 8192):
                x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
                plan = (ctypes.c_int * 2)()
                OQ.L.lib().pa_wo_gemm_prefill_plan(M, N, K, ctypes.byref(plan, 0), ctypes.byref(plan, 4))
                arms = {"wo": lambda: OQ.wo_prefill(x, q, sc, None, bits, group),
                        "dq": lambda: OQ._bf16_linear(x, OQ.dequantize(q, sc, bits, group, K, N), None),
                        "img": lambda: OQ._bf16_linear(x, img, None)}
                times = {n: [] for n in arms}
                for r in range(reps + 1):  # round 0 warms up (and lets the bf16 GEMM make its per-shape choice)
                    for n, fn in arms.items():
                        G._flush_caches(dev)
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        fn()
                        e.record()
                        e.synchronize()
                        if r:
                            times[n].append(s.elapsed_time(e) * 1000.0)
                t = {n: (min(v), sorted(v)[len(v) // 2]) for n, v in times.items()}
                ratio = lambda a: (lambda v: f"**{v:.2f}**" if v > 1 else f"{v:.2f}")(t["wo"][0] / t[a][0])
                ws = plan[1] * M * N * 4 if plan[1] > 1 else 0
                print(f"| {K} | {N} | {M} | int{bits} g{group} | {plan[0]} x {plan[1]} | " +
                      " | ".join(f"{t[n][0]:.0f} / {t[n][1]:.0f}" for n in arms) +
                      f" | {ratio('dq')} | {ratio('img')} | {ws / 2**20:.0f} \\| {2 * N * K / 2**20:.0f} |", flush=True)
            del q, sc, img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefill", action="store_true")
    ap.add_argument("--shapes", default="7b,70b")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    paddle.set_device("gpu:0")
    if args.prefill:
        return prefill(args.shapes.split(","), args.reps)
    shapes = [(4096, 4096), (4096, 11008), (11008, 4096), (5120, 15360), (20480, 5120)]  # (K, N)
    for K, N in shapes:
        w = torch.randn(K, N, device="cuda", dtype=torch.bfloat16) * 0.02
        q8, s8 = [t._t for t in Q.weight_quantize(paddle.Tensor(w.float().cpu()), "weight_only_int8")]
        q4, s4 = [t._t for t in Q.weight_quantize(paddle.Tensor(w.float().cpu()), "weight_only_int4")]
        q8, s8, q4, s4 = q8.cuda(), s8.cuda(), q4.cuda(), s4.cuda()
        for M in (1, 8, 16, 32, 64):
            x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
            arms = {"bf16_hipblaslt": lambda: torch.mm(x, w),
                    "int8": lambda: OQ.wo_linear(x, q8, s8, None, 8, -1),
                    "int4": lambda: OQ.wo_linear(x, q4, s4, None, 4, -1)}
            if G.small_m_supported(x, w):
                arms["bf16_ours_small_m"] = lambda: G.gemm_small_m(x, w)
            res = {k: sorted(timeit(f) for _ in range(3))[1] for k, f in arms.items()}
            best_bf16 = min(v for k, v in res.items() if k.startswith("bf16"))
            line = f"K={K:5d} N={N:5d} M={M:2d}: " + "  ".join(f"{k} {v:7.1f}us" for k, v in res.items())
            line += f"  | int8 {best_bf16 / res['int8']:.2f}x  int4 {best_bf16 / res['int4']:.2f}x of best bf16"
            wb = K * N
            line += f"  | int8 weight stream {wb / res['int8'] / 1e6:.2f} TB/s"
            print(line, flush=True)


if __name__ == "__main__":
    main()
