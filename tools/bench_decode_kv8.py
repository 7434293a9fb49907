"""int8 KV cache against the bf16 cache, three measurements (results: profiles/decode_kv8.md).

1. ``kernel``: pa_paged_decode_attn_q8 against pa_paged_decode_attn through ops.paged_decode_attention at batch 32,
   32 / 32 and 32 / 8 heads, head_dim 128, lens 512 / 2048 / 8192. Cold caches: each timed launch reads another copy
   of the cache, the copies together exceeding 2 GiB (the 256 MB Infinity Cache cannot hold a launch's cache from
   the launch before), and the launches of one round run from one captured graph, so no host time lies between
   them. Reports us per launch and achieved GB/s on the K + V bytes of the valid keys.
2. ``blha``: one block_multihead_attention decode step on uint8 caches with static scales over a 4096-block pool
   (batch 32, 32 / 8 heads, block 64, 1024 cached tokens per sequence), cold caches, device events around each
   eager call. It uses only arguments the op had before the int8 kernel, so the figure of an older commit is this
   file run in a checkout of that commit (``python tools/bench_decode_kv8.py blha``); ``time_blha`` takes the
   function, so two implementations can also be timed in one process on the same inputs.
3. ``llama``: LLaMA-2 7B, batch 32, prompt 512, decode ms per token with the captured decode step, bf16 and int8
   cache: (generate(16 + n) - generate(16)) / n.

Usage: python tools/bench_decode_kv8.py [kernel] [blha] [llama]   (default: all three)
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import paddlepaddle_amd as paddle  # noqa: E402
from paddlepaddle_amd import ops  # noqa: E402

DEV = "cuda"
D = 128


def _graph_time(fns, rounds=5):
    """us per call of ``fns`` (callables, run in order) from one captured graph, the median of ``rounds`` replays."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in fns:
            f()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / len(fns))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def kernel_case(N, H, Hkv, ctx, bs=64):
    nbps = ctx // bs
    gen = torch.Generator(device=DEV).manual_seed(ctx + Hkv)
    q = torch.randn(N, H, D, device=DEV, generator=gen).bfloat16()
    lens = torch.full((N,), ctx, dtype=torch.int32, device=DEV)
    kdq = torch.full((Hkv,), 1 / 32, device=DEV) * (1 + 0.01 * torch.arange(Hkv, device=DEV))
    vdq = kdq * 0.9
    elems = N * nbps * Hkv * bs * D
    out = {}
    for name, esz in (("bf16", 2), ("int8", 1)):
        copies = max(3, -(-(2 << 30) // (2 * elems * esz)))
        fns = []
        keep = []
        for c in range(copies):
            ki = torch.randint(1, 256, (N * nbps, Hkv, bs, D), device=DEV, dtype=torch.uint8, generator=gen)
            vi = torch.randint(1, 256, (N * nbps, Hkv, bs, D), device=DEV, dtype=torch.uint8, generator=gen)
            tab = torch.randperm(N * nbps, device=DEV, generator=gen).int().view(N, nbps)
            if esz == 1:
                kc, vc, kw = ki, vi, dict(k_dequant=kdq, v_dequant=vdq)
            else:   # the same values as bf16 (integers up to 127 times 1 / 32 are exact)
                kc, vc, kw = ((ki.float() - 128) / 32).bfloat16(), ((vi.float() - 128) / 32).bfloat16(), {}
                del ki, vi
            keep.append((kc, vc, tab))
            fns.append(lambda kc=kc, vc=vc, tab=tab, kw=kw: ops.paged_decode_attention(q, kc, vc, tab, lens,
                                                                                        max_len=ctx, **kw))
        us, lo, hi = _graph_time(fns)
        gbs = 2 * N * ctx * Hkv * D * esz / (us * 1e-6) / 1e9
        out[name] = (us, lo, hi, gbs, copies)
        del keep, fns
        torch.cuda.empty_cache()
    b, i = out["bf16"], out["int8"]
    print(f"| {N} | {H}/{Hkv} | {ctx} | {b[0]:.1f} ({b[1]:.1f}-{b[2]:.1f}) | {b[3]:.0f} | {i[0]:.1f} ({i[1]:.1f}-{i[2]:.1f}) "
          f"| {i[3]:.0f} | {b[0] / i[0]:.2f}x | {b[4]}/{i[4]} |", flush=True)


def bench_kernel():
    print("| batch | H/Hkv | len | bf16 us (min-max) | bf16 GB/s | int8 us (min-max) | int8 GB/s | bf16 / int8 time "
          "| cache copies bf16/int8 |")
    print("|---|---|---|---|---|---|---|---|---|")
    for Hkv in (32, 8):
        for ctx in (512, 2048, 8192):
            kernel_case(32, 32, Hkv, ctx)


def blha_inputs(B=32, H=32, Hk=8, bs=64, pool=4096, cached=1024):
    """A decode step of B sequences holding ``cached`` tokens each in a ``pool``-block uint8 cache pool."""
    gen = torch.Generator(device=DEV).manual_seed(1)
    kc = torch.randint(1, 256, (pool, Hk, bs, D), device=DEV, dtype=torch.uint8, generator=gen)
    vc = torch.randint(1, 256, (pool, Hk, bs, D), device=DEV, dtype=torch.uint8, generator=gen)
    per = pool // B
    tables = torch.randperm(pool, device=DEV, generator=gen).int().view(B, per)
    x = (torch.randn(B, (H + 2 * Hk) * D, device=DEV, generator=gen) * 0.5).bfloat16()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731
    ksc = torch.full((Hk,), 40.0, device=DEV)
    vsc = torch.full((Hk,), 50.0, device=DEV)
    import numpy as np
    P = paddle.to_tensor
    cu = torch.arange(B + 1, dtype=torch.int32, device=DEV)
    args = (P(x), P(kc), P(vc), P(i32([0] * B)), P(i32([cached] * B)), P(i32([1] * B)), None, None, P(cu), P(cu),
            P(tables))
    kw = dict(block_size=bs, cache_k_quant_scales=P(ksc), cache_v_quant_scales=P(vsc),
              cache_k_dequant_scales=P(1 / ksc), cache_v_dequant_scales=P(1 / vsc),
              max_enc_len_this_time=paddle.to_tensor(np.array([0], "int32"), place=paddle.CPUPlace()),
              max_dec_len_this_time=paddle.to_tensor(np.array([cached], "int32"), place=paddle.CPUPlace()))
    return args, kw


def time_blha(fn, iters=15):
    """ms per call of ``fn`` (a block_multihead_attention) on ``blha_inputs``: device events around each eager call,
    a 512 MiB buffer rewritten before every timed call (cold caches), 3 warm-up calls; median and (min, max).
    Also returns the output of the last call."""
    args, kw = blha_inputs()
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
    for _ in range(3):
        out = fn(*args, **kw)[0]
    ts = []
    for _ in range(iters):
        flush.add_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*args, **kw)[0]
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], (ts[0], ts[-1]), out._t.float()


def bench_blha():
    import paddlepaddle_amd.incubate.nn.functional as IF
    ms, (lo, hi), _ = time_blha(IF.block_multihead_attention)
    print(f"block_multihead_attention int8 decode step, 4096-block pool (batch 32, 32/8 heads, block 64, 1024 cached "
          f"tokens): {ms:.3f} ms ({lo:.3f}-{hi:.3f})", flush=True)


def bench_llama(B=32, prompt=512, base=16, n=64):
    from paddlepaddle_amd.models.llama import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig.llama2_7b(max_position_embeddings=prompt + base + n + 64)
    paddle.set_device("gpu")
    paddle.set_default_dtype("bfloat16")
    paddle.seed(0)
    model = LlamaForCausalLM(cfg)
    paddle.set_default_dtype("float32")
    model.eval()
    ids = paddle.Tensor(torch.randint(0, cfg.vocab_size, (B, prompt), device=DEV))
    Hkv, L = cfg.num_key_value_heads, cfg.num_hidden_layers
    for kv in (None, "int8", None, "int8"):
        def run(m):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.generate(ids, max_new_tokens=m, eos_token_id=-1, use_graph=True, kv_cache_dtype=kv)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        run(4)
        t_a, t_b = run(base), run(base + n)
        per_tok = 2 * L * Hkv * cfg.head_dim * (1 if kv else 2)
        print(f"llama2-7b batch {B} prompt {prompt} cache {kv or 'bf16'}: {(t_b - t_a) / n * 1e3:.3f} ms/token "
              f"(decode step, captured graph); cache bytes per token {per_tok}", flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    which = sys.argv[1:] or ["kernel", "blha", "llama"]
    if "kernel" in which:
        bench_kernel()
    if "blha" in which:
        bench_blha()
    if "llama" in which:
        bench_llama()
