"""MoE prefill FFN over MXFP4 expert weights (csrc/kernels/moe_grouped_mx.hip): the grouped down projection and combine
exactly on drawn codes, the whole FFN against ops.moe.moe_ffn_mx_reference in float64 on the CPU, and
fused_moe(quant_method="mxfp4")'s dispatch from 128 tokens up, its capture and the 127-token fallback."""
import pytest
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.ops import _loader as L
from paddlepaddle_amd.ops import moe as M
from paddlepaddle_amd.ops import mx as MX

pytestmark = pytest.mark.gpu
fused_moe = paddle.incubate.nn.functional.fused_moe
NEW = ("pa_moe_grouped_up_mx", "pa_moe_grouped_down_mx")
OLD = ("pa_grouped_gemm", "pa_moe_decode_up_mx", "pa_moe_decode_down_mx")
CRAFTED = [0, 128, 129, 0]  # empty first and last expert, an exactly full tile, one row spilling into a second tile


def _assigned_logits(T, E, g, counts=None):
    """logits that send token t to one chosen expert (8 * one_hot): drawn, or ``counts`` tokens per expert, shuffled"""
    e = torch.randint(0, E, (T,), generator=g) if counts is None else \
        torch.repeat_interleave(torch.arange(E), torch.tensor(counts))[torch.randperm(T, generator=g)]
    return (8.0 * torch.nn.functional.one_hot(e, E)).float().cuda()


def _logits(T, E, g):
    """every token's logits a permutation of 0.25 arange(E): distinct, so the top-k set is unambiguous"""
    return torch.stack([0.25 * torch.randperm(E, generator=g) for _ in range(T)]).float().cuda()


def _gate(logits, k):
    val, idx = torch.softmax(logits.float(), -1).topk(k, -1)
    return val / val.sum(-1, keepdim=True), idx


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("T,E,d,f,counts", [(130, 2, 128, 128, None), (257, 4, 256, 384, CRAFTED),
                                            (200, 8, 384, 1152, None)])
def test_down_and_combine_exact(T, E, d, f, counts, bias):
    """h_q: multiples of 0.5 up to 6; w2_q: every e2m1 code; scales 2^-1 .. 2^2: every product is a multiple of 2^-4 and
    a sum over K <= 1152 stays under 2^20, so fp32 accumulation is exact in any order. top-k 1 with renormalisation
    makes val exactly 1."""
    g = torch.Generator().manual_seed(T + E + f)
    scales = lambda R: torch.randint(126, 130, (R, f // 32), generator=g, dtype=torch.uint8)
    h_q, h_s = (torch.randint(-12, 13, (T, f), generator=g) * 0.5).to(torch.float8_e4m3fn), scales(T)
    c = torch.randint(0, 16, (E * d, f), generator=g, dtype=torch.uint8)
    w_q, w_s = c[:, 0::2] | (c[:, 1::2] << 4), scales(E * d)
    b2 = (0.5 * torch.randn(E, d, generator=g)).bfloat16() if bias else None
    val, idx = _gate(_assigned_logits(T, E, g, counts), 1)
    assert torch.equal(val, torch.ones_like(val))
    offs, perm = M.route(idx.reshape(-1), E)
    if counts:
        assert offs.tolist() == [0, 0, 128, 257, 257]
    pos = torch.empty(T, dtype=torch.int32, device="cuda")
    pos[perm] = torch.arange(T, dtype=torch.int32, device="cuda")
    out = M._grouped_down_mx(h_q.cuda(), h_s.cuda(), w_q.view(E, d, f // 2).cuda(), w_s.view(E, d, f // 32).cuda(),
                             b2.cuda() if bias else None, val.contiguous(), idx.int().contiguous(), offs, pos)
    idx, pos = idx.cpu().reshape(-1), pos.cpu().long()
    h = MX.dequantize_mx(h_q, h_s, "mxfp8", torch.float64)[pos]                      # token t's sorted row
    w = MX.dequantize_mx(w_q, w_s, "mxfp4", torch.float64).view(E, d, f)[idx]        # token t's expert
    ref = torch.einsum("tk,tdk->td", h, w) + (b2.double()[idx] if bias else 0)
    torch.testing.assert_close(out.cpu(), ref.float().bfloat16(), rtol=0, atol=0)


def _inputs(T, E, d, f, counts=None):
    """x ~ N(0, 1), w1 ~ N(0, 1) / sqrt(d), w2 ~ N(0, 1) / sqrt(f) quantised to mxfp4, biases ~ N(0, 0.25) -> device"""
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    x, w1, w2, b1, b2 = r(T, d), r(E, d, 2 * f) / d ** 0.5, r(E, f, d) / f ** 0.5, 0.5 * r(E, 2 * f), 0.5 * r(E, d)
    t = {"x": x.bfloat16(), "w": M.quantize_experts_mx(w1, w2), "b1": b1.bfloat16(), "b2": b2.bfloat16()}
    t = {n: tuple(u.cuda() for u in v) if n == "w" else v.cuda() for n, v in t.items()}
    t["logits"] = _assigned_logits(T, E, g, counts) if counts else _logits(T, E, g)
    return t


def _check(out, t, k, bias, what):
    """against moe_ffn_mx_reference in float64 on the CPU, on the same codes, scale bytes and routing"""
    c = lambda v: v.cpu()
    val, idx = _gate(t["logits"], k)
    ref = M.moe_ffn_mx_reference(c(t["x"]), c(val), c(idx), *map(c, t["w"]), c(t["b1"]) if bias else None,
                                 c(t["b2"]) if bias else None, dtype=torch.float64)
    err, bound = float((out.double().cpu() - ref).abs().max()), float(ref.abs().max()) / 64
    print(f"{what}: max err {err:.5f}, bound {bound:.5f}")
    assert err <= bound


@pytest.mark.parametrize("T,E,topk,d,f,bias,counts", [
    (3, 8, 2, 128, 256, True, None), (130, 2, 2, 128, 128, True, None), (130, 2, 2, 128, 128, False, None),
    (200, 8, 2, 384, 384, True, None), (200, 8, 2, 384, 384, False, None), (257, 4, 1, 256, 128, True, CRAFTED),
    (300, 64, 8, 256, 128, True, None)])
def test_ffn_matches_reference(T, E, topk, d, f, bias, counts):
    t = _inputs(T, E, d, f, counts)
    b1, b2 = (t["b1"], t["b2"]) if bias else (None, None)
    L.reset_calls()
    out = M.moe_grouped_ffn_mx(t["x"], t["logits"], *t["w"], b1, b2, topk, True)
    assert [L.calls(n) for n in NEW + ("pa_mx_quant",) + OLD] == [1, 1, 1, 0, 0, 0]
    _check(out, t, topk, bias, f"T {T}")


def test_fused_moe_mxfp4_prefill_dispatch_and_capture():
    E, k, d, f = 8, 2, 128, 256
    t = _inputs(128, E, d, f)
    P = paddle.Tensor
    w1_q, w1_s, w2_q, w2_s = map(P, t["w"])
    kw = dict(ffn1_bias=P(t["b1"].reshape(E, 1, 2 * f)), ffn1_scale=w1_s, ffn2_bias=P(t["b2"].reshape(E, 1, d)),
              ffn2_scale=w2_s, quant_method="mxfp4", moe_topk=k)
    run = lambda x, logits: fused_moe(P(x), P(logits), w1_q, w2_q, **kw)
    L.reset_calls()
    before = M.CALLS["mx_fallback"]
    out = run(t["x"], t["logits"])
    assert [L.calls(n) for n in NEW + OLD] == [1, 1, 0, 0, 0] and M.CALLS["mx_fallback"] == before
    _check(out._t, t, k, True, "fused_moe, 128 tokens")
    assert torch.equal(run(t["x"], t["logits"])._t, out._t)
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(t["x"], t["logits"])
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        o2 = run(t["x"], t["logits"])
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o2._t, out._t)
    # 127 tokens: the same chain in torch
    t127 = dict(t, x=t["x"][:127].contiguous(), logits=t["logits"][:127].contiguous())
    L.reset_calls()
    out = run(t127["x"], t127["logits"])
    assert M.CALLS["mx_fallback"] == before + 1 and [L.calls(n) for n in NEW] == [0, 0]
    _check(out._t, t127, k, True, "127 tokens")
