"""MoE prefill FFN over weight-only int8 / int4 expert weights (csrc/kernels/moe_grouped_wo.hip): the grouped down
projection and combine exactly on drawn codes, the whole FFN against ops.moe.moe_ffn_wo_reference in float64 on the CPU,
and fused_moe(quant_method="weight_only_int8" | "weight_only_int4")'s dispatch from 128 tokens up, its capture and the
127-token dequantise + grouped path."""
import pytest
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.ops import _loader as L
from paddlepaddle_amd.ops import moe as M

pytestmark = pytest.mark.gpu
fused_moe = paddle.incubate.nn.functional.fused_moe
NEW = ("pa_moe_grouped_up_wo", "pa_moe_grouped_down_wo")
OLD = ("pa_wo_dequant", "pa_grouped_gemm", "pa_moe_decode_up_wo", "pa_moe_decode_down_wo")
ALGO = {8: "weight_only_int8", 4: "weight_only_int4"}
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
@pytest.mark.parametrize("T,E,d,f,counts", [(130, 2, 64, 64, None), (257, 4, 320, 128, CRAFTED),
                                            (200, 8, 128, 1152, None)])
@pytest.mark.parametrize("bits", [8, 4])
def test_down_and_combine_exact(bits, T, E, d, f, counts, bias):
    """h: integers in [-4, 4]; w2_q: every code (-127 .. 127, or all 16 nibbles); scales 2^-3 .. 2^0; biases multiples
    of 2^-3 in [-2, 2]: every partial sum is a multiple of 2^-3 below 2^20 (f <= 1152), so fp32 is exact in any order.
    top-k 1 with renormalisation makes val exactly 1."""
    g = torch.Generator().manual_seed(T + E + f + bits)
    h = torch.randint(-4, 5, (T, f), generator=g).bfloat16()
    if bits == 8:
        w_q = torch.randint(-127, 128, (E, d, f), generator=g, dtype=torch.int8)
    else:
        c = torch.randint(0, 16, (E, d, f), generator=g, dtype=torch.uint8)
        w_q = (c[:, 0::2] | (c[:, 1::2] << 4)).view(torch.int8).contiguous()
    w_s = 2.0 ** -torch.randint(0, 4, (E, d), generator=g).float()
    b2 = (torch.randint(-16, 17, (E, d), generator=g) / 8).bfloat16() if bias else None
    val, idx = _gate(_assigned_logits(T, E, g, counts), 1)
    assert torch.equal(val, torch.ones_like(val))
    offs, perm = M.route(idx.reshape(-1), E)
    if counts:
        assert offs.tolist() == [0, 0, 128, 257, 257]
    pos = torch.empty(T, dtype=torch.int32, device="cuda")
    pos[perm] = torch.arange(T, dtype=torch.int32, device="cuda")
    out = M._prefill_down_wo(h.cuda()[perm], w_q.cuda(), w_s.cuda(), b2.cuda() if bias else None, val.contiguous(),
                             idx.int().contiguous(), offs, pos, bits)
    idx = idx.cpu().reshape(-1)
    w = torch.stack([M._dequant_wo(w_q[e], w_s[e], bits, torch.float64) for e in range(E)])[idx]  # token t's expert
    ref = torch.einsum("tk,tdk->td", h.double(), w) + (b2.double()[idx] if bias else 0)  # sorted row pos[t] is h[t]
    torch.testing.assert_close(out.cpu(), ref.float().bfloat16(), rtol=0, atol=0)


def _inputs(T, E, d, f, bits, counts=None):
    """x ~ N(0, 1), w1 ~ N(0, 1) / sqrt(d), w2 ~ N(0, 1) / sqrt(f) quantised weight-only, biases ~ N(0, 0.25) -> device"""
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    x, w1, w2, b1, b2 = r(T, d), r(E, d, 2 * f) / d ** 0.5, r(E, f, d) / f ** 0.5, 0.5 * r(E, 2 * f), 0.5 * r(E, d)
    t = {"x": x.bfloat16(), "w": M.quantize_experts_wo(w1, w2, ALGO[bits]), "b1": b1.bfloat16(), "b2": b2.bfloat16()}
    t = {n: tuple(u.cuda() for u in v) if n == "w" else v.cuda() for n, v in t.items()}
    t["logits"] = _assigned_logits(T, E, g, counts) if counts else _logits(T, E, g)
    return t


def _check(out, t, k, bits, bias, what):
    """against moe_ffn_wo_reference in float64 on the CPU, on the same codes, scales and routing"""
    c = lambda v: v.cpu()
    val, idx = _gate(t["logits"], k)
    ref = M.moe_ffn_wo_reference(c(t["x"]), c(val), c(idx), *map(c, t["w"]), c(t["b1"]) if bias else None,
                                 c(t["b2"]) if bias else None, bits, dtype=torch.float64)
    err, bound = float((out.double().cpu() - ref).abs().max()), float(ref.abs().max()) / 64
    print(f"{what}: max err {err:.5f}, bound {bound:.5f}")
    assert err <= bound


@pytest.mark.parametrize("T,E,topk,d,f,bias,counts", [
    (3, 8, 2, 64, 64, True, None), (130, 2, 2, 128, 320, True, None), (130, 2, 2, 128, 320, False, None),
    (257, 4, 1, 320, 128, True, CRAFTED), (300, 64, 8, 576, 128, True, None)])
@pytest.mark.parametrize("bits", [8, 4])
def test_ffn_matches_reference(bits, T, E, topk, d, f, bias, counts):
    t = _inputs(T, E, d, f, bits, counts)
    b1, b2 = (t["b1"], t["b2"]) if bias else (None, None)
    L.reset_calls()
    out = M.moe_prefill_ffn_wo(t["x"], t["logits"], *t["w"], b1, b2, topk, True, bits)
    assert [L.calls(n) for n in NEW + OLD] == [1, 1, 0, 0, 0, 0]
    _check(out, t, topk, bits, bias, f"T {T}")


@pytest.mark.parametrize("bits", [8, 4])
def test_fused_moe_wo_prefill_dispatch_and_capture(bits):
    E, k, d, f = 8, 2, 128, 256
    t = _inputs(128, E, d, f, bits)
    P = paddle.Tensor
    w1_q, w1_s, w2_q, w2_s = map(P, t["w"])
    kw = dict(ffn1_bias=P(t["b1"].reshape(E, 1, 2 * f)), ffn1_scale=w1_s, ffn2_bias=P(t["b2"].reshape(E, 1, d)),
              ffn2_scale=w2_s, quant_method=ALGO[bits], moe_topk=k)
    run = lambda x, logits: fused_moe(P(x), P(logits), w1_q, w2_q, **kw)
    L.reset_calls()
    before = M.CALLS["wo_fallback"]
    out = run(t["x"], t["logits"])
    assert [L.calls(n) for n in NEW + OLD] == [1, 1, 0, 0, 0, 0] and M.CALLS["wo_fallback"] == before
    _check(out._t, t, k, bits, True, "fused_moe, 128 tokens")
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
    # 127 tokens: dequantise + the bf16 grouped kernel
    t127 = dict(t, x=t["x"][:127].contiguous(), logits=t["logits"][:127].contiguous())
    L.reset_calls()
    out = run(t127["x"], t127["logits"])
    assert L.calls("pa_wo_dequant") == 2 and [L.calls(n) for n in NEW] == [0, 0]
    assert M.CALLS["wo_fallback"] == before
    _check(out._t, t127, k, bits, True, "127 tokens")
