"""Paged prefill attention (ops.paged_prefill_attention) against its two baselines (results:
profiles/paged_prefill_attn.md).

Per point (batch 8, head_dim 128, a chunk of new tokens per sequence over a context already in a shuffled paged cache):
* ``hip``  : the MFMA kernel over the bf16 cache, and ``q8`` over the uint8 cache;
* ``math`` : block_multihead_attention's former prefix path ``_blha_prefill_math`` on the same inputs (the prefix
  handed over as the dense tensor that path takes);
* ``gather`` + ``flash``: a contiguous copy of each sequence's keys gathered through the block table, then
  ops.flash_attention (causal, bottom-right) on it: the bound a gather-free kernel should approach is ``flash``.

Timing: device events around each eager call, a 512 MiB buffer rewritten before every timed call (cold caches),
3 warm-up calls, median (min-max) of ``--iters`` calls, in ms. The hip / q8 figures include the op's zero-fill of the
output. Kernel-only times come from a trace of the same script:
``rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_paged_prefill.py --trace``.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import paddlepaddle_amd.incubate.nn.functional as IF  # noqa: E402
from paddlepaddle_amd import ops  # noqa: E402

DEV, D, B = "cuda", 128, 8
POINTS = [(512, 512), (512, 4096), (4, 2048)]   # (chunk, context incl. the chunk)


def timed(fn, flush, iters):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(iters):
        flush.add_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return f"{ts[len(ts) // 2]:.3f} ({ts[0]:.3f}-{ts[-1]:.3f})"


def point(H, Hkv, chunk, ctx, bs, flush, iters, trace):
    gen = torch.Generator(device=DEV).manual_seed(ctx + bs)
    nbps = ctx // bs
    k8 = torch.randint(1, 256, (B * nbps, Hkv, bs, D), device=DEV, dtype=torch.uint8, generator=gen)
    v8 = torch.randint(1, 256, (B * nbps, Hkv, bs, D), device=DEV, dtype=torch.uint8, generator=gen)
    kc, vc = ((k8.float() - 128) / 32).bfloat16(), ((v8.float() - 128) / 32).bfloat16()   # the same values
    tab = torch.randperm(B * nbps, device=DEV, generator=gen).int().view(B, nbps)
    q = (0.5 * torch.randn(B * chunk, H, D, device=DEV, generator=gen)).bfloat16()
    cu = torch.arange(B + 1, device=DEV, dtype=torch.int32) * chunk
    cl = torch.full((B,), ctx, device=DEV, dtype=torch.int32)
    dq = torch.full((Hkv,), 1 / 32, device=DEV)

    def hip():
        return ops.paged_prefill_attention(q, kc, vc, tab, cu, cl, max_q=chunk)

    def q8():
        return ops.paged_prefill_attention(q, k8, v8, tab, cu, cl, max_q=chunk, k_dequant=dq, v_dequant=dq)

    def gather():
        K = kc[tab.long()].permute(0, 1, 3, 2, 4).reshape(B, ctx, Hkv, D)
        V = vc[tab.long()].permute(0, 1, 3, 2, 4).reshape(B, ctx, Hkv, D)
        return K, V

    K, V = gather()
    q4 = q.view(B, chunk, H, D)

    def flash():
        return ops.flash_attention(q4, K, V, causal=True)

    P = ctx - chunk
    kk = K[:, P:].reshape(B * chunk, Hkv, D)
    vv = V[:, P:].reshape(B * chunk, Hkv, D)
    pk = K[:, :P].permute(0, 2, 1, 3).contiguous() if P else None
    pv = V[:, :P].permute(0, 2, 1, 3).contiguous() if P else None
    enc = torch.full((B,), chunk, device=DEV)

    def math():
        return IF._blha_prefill_math(q, kk, vv, cu.long(), enc, pk, pv, None)

    err = float((hip().float() - flash().reshape(B * chunk, H, D).float()).abs().max())
    err8 = float((q8().float() - hip().float()).abs().max())
    if trace:   # one cold call of each kernel path for the kernel trace
        for fn in (hip, q8, flash):
            flush.add_(1)
            fn()
        torch.cuda.synchronize()
        return
    cols = [timed(fn, flush, iters) for fn in (hip, q8, math, gather, flash)]
    print(f"| {H}/{Hkv} | {chunk} | {ctx} | {bs} | " + " | ".join(cols) + f" | {err:.3g} | {err8:.3g} |", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
    print("| H/Hkv | chunk | ctx | bs | hip ms | q8 ms | math ms | gather ms | flash ms | max|hip-flash| | max|q8-hip| |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for H, Hkv in ((32, 32), (32, 8)):
        for chunk, ctx in POINTS:
            for bs in (16, 64):
                point(H, Hkv, chunk, ctx, bs, flush, a.iters, a.trace)
