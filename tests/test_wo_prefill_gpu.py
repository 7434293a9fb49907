"""Weight-only int8 / int4 prefill GEMM on the codes (csrc/kernels/wo_gemm_prefill.hip): the product bit for bit on
drawn codes with both tiles and forced K splits, nn.quant.weight_only_linear's dispatch from 256 rows with the image
cache off against the float64 dequantised product, its capture, and the launcher's plan."""
import ctypes

import pytest
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.nn import quant as Q
from paddlepaddle_amd.ops import _loader as L
from paddlepaddle_amd.ops import quant as OQ

gpu = pytest.mark.gpu
ALGOS = [("weight_only_int8", -1), ("weight_only_int8", 64), ("weight_only_int4", -1), ("weight_only_int4", 128)]


def _dequant64(q, s, bits, group):
    """float64 [N, K] of codes q (int8 [N, K], or int4 pair-rows [N / 2, K] stored + 8) and scales s ([N] or [K / G, N])"""
    if bits == 4:
        b = q.view(torch.uint8).to(torch.int32)
        q = torch.stack([(b & 15) - 8, (b >> 4) - 8], 1).reshape(-1, b.shape[1])  # rows 2j, 2j + 1
    K = q.shape[1]
    s = s.double()
    sk = s[None].expand(K, -1) if group == -1 else s.repeat_interleave(group, 0)[:K]  # [K, N]
    return q.double() * sk.t()


# M: below a tile, ragged 128, one full tile, one row into the next, two tiles and one row. N: a lone ragged band, a
# full band and a ragged one. K: one tile, both stages, an odd count (the prefetch clamps), three groups of 128.
@gpu
@pytest.mark.parametrize("bits,group,M,N,K,tile_m,splits,bias", [
    (8, -1, 1, 64, 64, 128, 1, True), (4, -1, 130, 64, 128, 128, 2, False), (8, 64, 256, 320, 320, 256, 5, True),
    (4, 128, 257, 320, 384, 256, 2, True), (8, 128, 513, 320, 384, 256, 1, True), (4, 64, 513, 64, 320, 128, 1, True),
    (8, -1, 257, 320, 384, 128, 2, True), (4, -1, 256, 320, 64, 256, 1, True), (4, 128, 130, 320, 128, 256, 1, False),
    (8, 64, 130, 64, 128, 256, 2, True)])
def test_product_is_exact(bits, group, M, N, K, tile_m, splits, bias):
    """x: integers in [-3, 3]; every code; scales 2^-((3 g + n) % 6); bias: integers in [-8, 8]. Every product is exact
    in bf16 and every partial sum a multiple of 2^-5 below 3 * 127 * 384 < 2^18, so fp32 accumulation is exact in any
    order, over any split: the float64 product rounded once to bf16 is the only right answer."""
    g = torch.Generator().manual_seed(M + N + K + bits)
    x = torch.randint(-3, 4, (M, K), generator=g).bfloat16()
    if bits == 8:
        q = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8)
    else:
        q = torch.randint(0, 256, (N // 2, K), generator=g, dtype=torch.uint8)
        assert len(torch.unique(q & 15)) == 16 and len(torch.unique(q >> 4)) == 16
        q = q.view(torch.int8)
    groups = torch.arange(1 if group == -1 else K // group)[:, None]
    s = 2.0 ** -((3 * groups + torch.arange(N)) % 6).float()  # [K / G, N]
    s = s[0] if group == -1 else s
    b = torch.randint(-8, 9, (N,), generator=g).bfloat16() if bias else None
    y = OQ.wo_prefill(x.cuda(), q.cuda(), s.cuda(), b.cuda() if bias else None, bits, group, tile_m, splits)
    ref = x.double() @ _dequant64(q, s, bits, group).t() + (b.double() if bias else 0)
    assert torch.equal(y.cpu(), ref.float().bfloat16())


def _quantized(algo, group):
    g = torch.Generator().manual_seed(3)
    w = torch.randn(1024, 1536, generator=g) * 0.05
    q, s = Q.weight_quantize(paddle.Tensor(w), algo, group_size=group)
    x = torch.randn(300, 1024, generator=g).bfloat16()
    bias = (torch.randn(1536, generator=g) * 0.1).bfloat16()
    return q._t.cpu(), s._t.cpu(), x, bias


def _linear_cache_off(x, q, s, bias, algo, group):
    paddle.set_flags({"FLAGS_weight_only_dequant_cache_mb": 0})
    try:
        return Q.weight_only_linear(paddle.Tensor(x), paddle.Tensor(q), paddle.Tensor(bias), paddle.Tensor(s),
                                    algo.split("_")[-1], group_size=group)._t
    finally:
        paddle.set_flags({"FLAGS_weight_only_dequant_cache_mb": 4096})


@gpu
@pytest.mark.parametrize("algo,group", ALGOS)
def test_weight_only_linear_reads_the_codes(algo, group):
    q, s, x, bias = _quantized(algo, group)
    L.reset_calls()
    y = _linear_cache_off(x.cuda(), q.cuda(), s.cuda(), bias.cuda(), algo, group)
    assert L.calls("pa_wo_gemm_prefill") == 1 and L.calls("pa_wo_dequant") == 0
    ref = x.double() @ _dequant64(q, s, int(algo[-1]), group).t() + bias.double()
    err = float((y.cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"{algo} group {group}: max err / max |ref| = {err:.2e}")
    assert err < 1e-2


@gpu
def test_capture_replays_equal_eager():
    algo, group = "weight_only_int4", 128
    q, s, x, bias = (t.cuda() for t in _quantized(algo, group))
    xs = x.clone()
    _linear_cache_off(xs, q, s, bias, algo, group)  # warm-up: the kernels' attributes are set outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _linear_cache_off(xs, q, s, bias, algo, group)
    for seed in range(3):
        xs.copy_(torch.randn(x.shape, generator=torch.Generator().manual_seed(seed)).bfloat16())
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, _linear_cache_off(xs.clone(), q, s, bias, algo, group))


@pytest.mark.parametrize("M,N,K", [(1, 64, 64), (256, 4096, 4096), (1024, 4096, 11008), (2048, 28672, 8192),
                                   (300, 1536, 1024), (8192, 64, 320)])
def test_plan_fills_the_chip_within_its_cap(M, N, K):
    tm, sp = ctypes.c_int(0), ctypes.c_int(0)
    assert L.lib().pa_wo_gemm_prefill_plan(M, N, K, ctypes.byref(tm), ctypes.byref(sp)) == 0
    tm, sp, nk = tm.value, sp.value, K // 64
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    assert tm in (128, 256) and sp >= 1 and nk % sp == 0
    cap = max(d for d in range(1, 9) if nk % d == 0)  # the largest split the plan may choose
    assert -(-M // tm) * -(-N // 256) * sp >= cus or sp == cap
    assert L.lib().pa_wo_gemm_prefill_plan(M, N + 32, K, ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_int())) != 0
