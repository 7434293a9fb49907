"""MoE decode microbenchmark: incubate.nn.functional.fused_moe at T = 1 / 4 / 16 / 64 tokens on the decode kernels
(csrc/kernels/moe_decode.hip) against the same call on the grouped path (ops.moe.USE_DECODE = False: torch gate math,
pa_moe_route, gathers, pa_grouped_gemm + swiglu + pa_grouped_gemm, index_add), eager and replayed from a hipGraph.

Method (tools/bench_fp8_linear.py's): one process, device events around each call, a 512 MiB buffer rewritten before
every timed call (cold L2 / Infinity Cache: in a real step the weights stream from HBM), the contenders interleaved
call by call, median and min-max of the repeats. The stream rate is the bf16 bytes of w1[e] and w2[e] of the experts
the gate picked, over the median time. Launches are the device kernels a profiler sees in one eager call.

    python tools/bench_moe_decode.py --out profiles/moe_decode_tables.md [--reps 9]

``--mx`` measures the MXFP4 expert FFN instead (fused_moe(quant_method="mxfp4"), the *_mx kernels of moe_decode.hip)
against the bf16 decode kernels on the same shapes and tokens, alternating with them in the same run; its stream rate
counts 4.25 bits a weight, and `rel err` is the Frobenius norm of (mxfp4 output - bf16 output) over that of the bf16
output, the unquantised FFN.

    python tools/bench_moe_decode.py --mx --out profiles/moe_decode_mx_tables.md [--reps 9]

``--wo`` does the same for the weight-only int8 / int4 expert FFN (fused_moe(quant_method="weight_only_int8" |
"weight_only_int4"), csrc/kernels/moe_decode_wo.hip); at 64 tokens it also times the dequantise + grouped path that
fused_moe takes above ops.moe.WO_DECODE_DISPATCH_TOKENS.

    python tools/bench_moe_decode.py --wo --out profiles/moe_decode_wo_tables.md [--reps 9]
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
TOKENS = [1, 4, 16, 64]
NAMES = ["grouped", "decode", "grouped graph", "decode graph"]
fused_moe = paddle.incubate.nn.functional.fused_moe


def call(args, k, decode):
    """fused_moe on the grouped path, or on the decode kernels at every token count they take (fused_moe's own
    threshold, ops.moe.DECODE_DISPATCH_TOKENS, comes from this table)."""
    keep = M.DECODE_DISPATCH_TOKENS
    M.USE_DECODE, M.DECODE_DISPATCH_TOKENS = decode, M.DECODE_MAX_TOKENS
    try:
        return fused_moe(*args, moe_topk=k)
    finally:
        M.USE_DECODE, M.DECODE_DISPATCH_TOKENS = True, keep


def graphed(args, k, decode):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(args, k, decode)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(args, k, decode)
    return g, out


def launches(fn):
    """Device kernels of one call, or None where the profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                and not e.name.lower().startswith(("memcpy", "memset")))
        return n or None
    except Exception as e:  # noqa: BLE001  (reported in the table, the timings stand without it)
        print(f"profiler: {e}", flush=True)
        return None


def main_mx(a, flush, head):
    names = ["decode", "mxfp4", "decode graph", "mxfp4 graph"]
    lines = ["# MoE decode: MXFP4 expert weights against the bf16 decode kernels", "",
             head + " `decode`: the bf16 decode kernels. `mxfp4`: fused_moe(quant_method=\"mxfp4\"). `graph`: the same "
             "call replayed from a hipGraph. `TB/s`: weight bytes of the active experts (bf16: 16 bits a weight, mxfp4: "
             "4.25) over the median time of the graph replay. `rel err`: Frobenius norm of the difference of the two "
             "outputs over that of the bf16 output.", "",
             "| d / f / E / top-k | T | active | splits bf16 / mxfp4 | " + " | ".join(names) +
             " | mxfp4 graph / decode graph | TB/s decode / mxfp4 | rel err |", "|" + "---|" * 11]
    for d, f, E, k in SHAPES:
        w1 = torch.empty(E, d, 2 * f, dtype=torch.bfloat16, device="cuda").normal_(0, d ** -0.5)
        w2 = torch.empty(E, f, d, dtype=torch.bfloat16, device="cuda").normal_(0, f ** -0.5)
        w1_q, w1_s, w2_q, w2_s = map(paddle.Tensor, M.quantize_experts_mx(w1, w2))
        w1, w2 = paddle.Tensor(w1), paddle.Tensor(w2)
        for T in TOKENS:
            torch.manual_seed(T)
            args = (paddle.Tensor(torch.randn(T, d, device="cuda").bfloat16()),
                    paddle.Tensor(torch.randn(T, E, device="cuda")), w1, w2)
            mx = lambda: fused_moe(args[0], args[1], w1_q, w2_q, ffn1_scale=w1_s, ffn2_scale=w2_s,
                                   quant_method="mxfp4", moe_topk=k)
            n_act = int(M.decode_plan(args[1]._t, k)[6])
            n0 = L.calls("pa_moe_decode_ffn"), L.calls("pa_moe_decode_up_mx")
            o_bf, o_mx = call(args, k, True)._t.float(), mx()._t.float()
            assert L.calls("pa_moe_decode_ffn") == n0[0] + 1 and L.calls("pa_moe_decode_up_mx") == n0[1] + 1
            err = float((o_mx - o_bf).norm() / o_bf.norm())
            g_bf = graphed(args, k, True)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                mx()
            torch.cuda.current_stream().wait_stream(s)
            g_mx = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_mx):
                keep = mx()
            variants = {"decode": (lambda: call(args, k, True), None), "mxfp4": (mx, None),
                        "decode graph": (g_bf[0].replay, None), "mxfp4 graph": (g_mx.replay, None)}
            res = interleaved(variants, a.reps, flush, warmup=2)
            med = {n: statistics.median(res[n]) for n in names}
            wb = n_act * 3 * d * f
            ratio = med["mxfp4 graph"] / med["decode graph"]
            lines.append(f"| {d} / {f} / {E} / {k} | {T} | {n_act} | {M.decode_splits(T * k, E, d, f)} / "
                         f"{M.decode_splits_mx(T * k, E, d, f)} | " + " | ".join(fmt_ms(res[n]) for n in names)
                         + (f" | {ratio:.2f}" if ratio <= 1 else f" | **{ratio:.2f}**")
                         + f" | {wb * 2 / (med['decode graph'] * 1e-3) / 1e12:.2f} / "
                         f"{wb * 4.25 / 8 / (med['mxfp4 graph'] * 1e-3) / 1e12:.2f} | {err:.4f} |")
            print(lines[-1], flush=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
            del g_bf, g_mx, keep
        del w1, w2, w1_q, w1_s, w2_q, w2_s
        torch.cuda.empty_cache()
    print(f"wrote {a.out}")


def main_wo(a, flush, head):
    """--wo: the weight-only int8 / int4 decode kernels (csrc/kernels/moe_decode_wo.hip) against the bf16 decode
    kernels on the unquantised weights, all replayed from hipGraphs and alternating in the same run; at T = 64 also
    fused_moe's dequantise + grouped path (eager: it allocates its images per call)."""
    algos = {8: "weight_only_int8", 4: "weight_only_int4"}
    names = ["bf16 graph", "int8 graph", "int4 graph"]
    lines = ["# MoE decode: weight-only int8 / int4 expert weights against the bf16 decode kernels", "",
             head + " `bf16`: the bf16 decode kernels on the unquantised weights. `int8` / `int4`: fused_moe("
             "quant_method=\"weight_only_int8\" / \"weight_only_int4\") on the decode kernels. All three are replayed "
             "from a hipGraph. `dq+grouped`: the same call forced onto the dequantise + grouped path, eager, T = 64 "
             "only. `TB/s`: weight bytes of the active experts (16 / 8 / 4 bits a weight) over the median time. `rel "
             "err`: Frobenius norm of (quantised output - bf16 output) over that of the bf16 output, Gaussian weights: "
             "a property of the format. A ratio above 1 (quantised slower than bf16) is bold.", "",
             "| d / f / E / top-k | T | active | splits bf16 / int8 / int4 | " + " | ".join(names) +
             " | int8 / bf16 | int4 / bf16 | TB/s bf16 / int8 / int4 | dq+grouped int8 / int4 | rel err int8 / int4 |",
             "|" + "---|" * 12]
    for d, f, E, k in SHAPES:
        w1 = torch.empty(E, d, 2 * f, dtype=torch.bfloat16, device="cuda").normal_(0, d ** -0.5)
        w2 = torch.empty(E, f, d, dtype=torch.bfloat16, device="cuda").normal_(0, f ** -0.5)
        wq = {b: tuple(map(paddle.Tensor, M.quantize_experts_wo(w1, w2, algo))) for b, algo in algos.items()}
        w1, w2 = paddle.Tensor(w1), paddle.Tensor(w2)
        for T in TOKENS:
            torch.manual_seed(T)
            args = (paddle.Tensor(torch.randn(T, d, device="cuda").bfloat16()),
                    paddle.Tensor(torch.randn(T, E, device="cuda")), w1, w2)

            def wo(b):
                q = wq[b]
                return lambda: fused_moe(args[0], args[1], q[0], q[2], ffn1_scale=q[1], ffn2_scale=q[3],
                                         quant_method=algos[b], moe_topk=k)

            def grouped(b):
                def run():
                    keep, M.WO_DECODE_DISPATCH_TOKENS = M.WO_DECODE_DISPATCH_TOKENS, 0
                    try:
                        return wo(b)()
                    finally:
                        M.WO_DECODE_DISPATCH_TOKENS = keep
                return run

            n_act = int(M.decode_plan(args[1]._t, k)[6])
            n0 = L.calls("pa_moe_decode_ffn"), L.calls("pa_moe_decode_up_wo")
            o_bf = call(args, k, True)._t.float()
            err = {b: float((wo(b)()._t.float() - o_bf).norm() / o_bf.norm()) for b in algos}
            assert L.calls("pa_moe_decode_ffn") == n0[0] + 1 and L.calls("pa_moe_decode_up_wo") == n0[1] + 2
            graphs = {"bf16 graph": graphed(args, k, True)}
            for b in algos:
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    wo(b)()
                torch.cuda.current_stream().wait_stream(s)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    keep = wo(b)()
                graphs[f"int{b} graph"] = (g, keep)
            variants = {n: (graphs[n][0].replay, None) for n in names}
            if T == 64:
                n1 = L.calls("pa_wo_dequant")
                variants.update({f"int{b} dq+grouped": (grouped(b), None) for b in algos})
            res = interleaved(variants, a.reps, flush, warmup=2)
            assert T != 64 or L.calls("pa_wo_dequant") > n1
            med = {n: statistics.median(v) for n, v in res.items()}
            wb = n_act * 3 * d * f
            bold = lambda r: f"{r:.2f}" if r <= 1 else f"**{r:.2f}**"
            tb = [wb * bits / 8 / (med[n] * 1e-3) / 1e12 for n, bits in zip(names, (16, 8, 4))]
            dq = " / ".join(fmt_ms(res[f"int{b} dq+grouped"]) for b in algos) if T == 64 else "-"
            lines.append(f"| {d} / {f} / {E} / {k} | {T} | {n_act} | {M.decode_splits(T * k, E, d, f)} / "
                         f"{M.decode_splits_wo(T * k, E, d, f, 8)} / {M.decode_splits_wo(T * k, E, d, f, 4)} | "
                         + " | ".join(fmt_ms(res[n]) for n in names)
                         + f" | {bold(med['int8 graph'] / med['bf16 graph'])} | "
                         f"{bold(med['int4 graph'] / med['bf16 graph'])} | {tb[0]:.2f} / {tb[1]:.2f} / {tb[2]:.2f} | "
                         f"{dq} | {err[8]:.4f} / {err[4]:.4f} |")
            print(lines[-1], flush=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
            del graphs, variants, keep
        del w1, w2, wq
        torch.cuda.empty_cache()
    print(f"wrote {a.out}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/moe_decode_tables.md")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--mx", action="store_true", help="MXFP4 expert weights against the bf16 decode kernels")
    ap.add_argument("--wo", action="store_true", help="weight-only int8 / int4 expert weights against the bf16 kernels")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe_decode needs a HIP device")
    flush = Flusher()
    p = torch.cuda.get_device_properties(0)
    if a.wo:
        return main_wo(a, flush, f"Box: {torch.cuda.get_device_name(0)} ({p.gcnArchName}, {p.multi_processor_count} "
                       f"CUs), torch {torch.__version__}. Date: {time.strftime('%Y-%m-%d')}. Written by "
                       f"`tools/bench_moe_decode.py --wo --reps {a.reps}`: cold caches, device events, contenders "
                       f"interleaved; each time is the median of {a.reps} calls in ms with (min-max) behind it.")
    if a.mx:
        return main_mx(a, flush, f"Box: {torch.cuda.get_device_name(0)} ({p.gcnArchName}, {p.multi_processor_count} "
                       f"CUs), torch {torch.__version__}. Date: {time.strftime('%Y-%m-%d')}. Written by "
                       f"`tools/bench_moe_decode.py --mx --reps {a.reps}`: cold caches, device events, contenders "
                       f"interleaved; each time is the median of {a.reps} calls in ms with (min-max) behind it.")
    lines = ["# MoE decode: fused_moe on the decode kernels against the grouped path", "",
             f"Box: {torch.cuda.get_device_name(0)} ({p.gcnArchName}, {p.multi_processor_count} CUs), torch "
             f"{torch.__version__}. Date: {time.strftime('%Y-%m-%d')}. Written by `tools/bench_moe_decode.py --reps "
             f"{a.reps}`: cold caches, device events, contenders interleaved; each time is the median of {a.reps} calls "
             "in ms with (min-max) behind it. `grouped`: the path fused_moe took before the decode kernels. `graph`: "
             "the same call replayed from a hipGraph. `TB/s`: weight bytes of the active experts over the median "
             "time of `decode graph` / `grouped graph`. `max diff`: largest difference of the two outputs over the "
             "largest output magnitude.", "",
             "| d / f / E / top-k | T | active | splits | " + " | ".join(NAMES) +
             " | launches grouped / decode | TB/s decode / grouped | max diff |", "|" + "---|" * 11]
    for d, f, E, k in SHAPES:
        w1 = paddle.Tensor(torch.empty(E, d, 2 * f, dtype=torch.bfloat16, device="cuda").normal_(0, d ** -0.5))
        w2 = paddle.Tensor(torch.empty(E, f, d, dtype=torch.bfloat16, device="cuda").normal_(0, f ** -0.5))
        for T in TOKENS:
            torch.manual_seed(T)
            args = (paddle.Tensor(torch.randn(T, d, device="cuda").bfloat16()),
                    paddle.Tensor(torch.randn(T, E, device="cuda")), w1, w2)
            n_act = int(M.decode_plan(args[1]._t, k)[6])
            n0 = L.calls("pa_moe_decode_ffn"), L.calls("pa_grouped_gemm")
            o_old, o_new = call(args, k, False)._t.float(), call(args, k, True)._t.float()
            assert L.calls("pa_moe_decode_ffn") == n0[0] + 1 and L.calls("pa_grouped_gemm") == n0[1] + 2
            diff = float((o_old - o_new).abs().max() / o_old.abs().max())
            g_old, g_new = graphed(args, k, False), graphed(args, k, True)
            variants = {"grouped": (lambda: call(args, k, False), None), "decode": (lambda: call(args, k, True), None),
                        "grouped graph": (g_old[0].replay, None), "decode graph": (g_new[0].replay, None)}
            res = interleaved(variants, a.reps, flush, warmup=2)
            nl = (None, None) if a.no_launch_count else (launches(lambda: call(args, k, False)),
                                                         launches(lambda: call(args, k, True)))
            wbytes = n_act * 3 * d * f * 2
            tb = [wbytes / (statistics.median(res[n]) * 1e-3) / 1e12 for n in ("decode graph", "grouped graph")]
            lines.append(f"| {d} / {f} / {E} / {k} | {T} | {n_act} | {M.decode_splits(T * k, E, d, f)} | "
                         + " | ".join(fmt_ms(res[n]) for n in NAMES)
                         + f" | {nl[0] or 'not measured'} / {nl[1] or 'not measured'} | {tb[0]:.2f} / {tb[1]:.2f} | "
                         f"{diff:.4f} |")
            print(lines[-1], flush=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
            del g_old, g_new
        del w1, w2
        torch.cuda.empty_cache()
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
