"""MoE decode FFN over weight-only int8 / int4 expert weights (csrc/kernels/moe_decode_wo.hip): the down projection
and combine exactly on drawn codes, the whole FFN against ops.moe.moe_ffn_wo_reference in float64 on the CPU, and
fused_moe(quant_method="weight_only_int8" | "weight_only_int4")'s dispatch, capture and dequantise + grouped path."""
import pytest
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.ops import _loader as L
from paddlepaddle_amd.ops import moe as M

pytestmark = pytest.mark.gpu
fused_moe = paddle.incubate.nn.functional.fused_moe
NEW = ("pa_moe_decode_up_wo", "pa_moe_decode_down_wo")
ALGO = {8: "weight_only_int8", 4: "weight_only_int4"}


def _logits(T, E, g):
    """every token's logits a permutation of 0.25 arange(E): distinct, so the top-k set is unambiguous"""
    return torch.stack([0.25 * torch.randperm(E, generator=g) for _ in range(T)]).float().cuda()


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("T,E,d,f,splits", [(1, 8, 64, 64, None), (17, 4, 128, 320, None), (64, 2, 64, 640, None),
                                            (64, 2, 64, 640, 1), (5, 16, 128, 1152, 1)])
@pytest.mark.parametrize("bits", [8, 4])
def test_down_and_combine_exact(bits, T, E, d, f, splits, bias):
    """h: integers in [-4, 4]; w2_q: every code (-127 .. 127, or all 16 nibbles); scales 2^-3 .. 2^0; biases multiples
    of 2^-3 in [-2, 2]: every partial sum is a multiple of 2^-3 below 2^20, so fp32 is exact in any order and over
    any split. top-k 1 with renormalisation makes val exactly 1."""
    g = torch.Generator().manual_seed(T + E + f + bits)
    h = torch.randint(-4, 5, (T, f), generator=g).bfloat16()
    if bits == 8:
        w_q = torch.randint(-127, 128, (E, d, f), generator=g, dtype=torch.int8)
    else:
        c = torch.randint(0, 16, (E, d, f), generator=g, dtype=torch.uint8)
        w_q = (c[:, 0::2] | (c[:, 1::2] << 4)).view(torch.int8).contiguous()
    w_s = 2.0 ** -torch.randint(0, 4, (E, d), generator=g).float()
    b2 = (torch.randint(-16, 17, (E, d), generator=g) / 8).bfloat16() if bias else None
    plan = M.decode_plan(_logits(T, E, g), 1, True)
    out = M._decode_down_wo(h.cuda(), w_q.cuda(), w_s.cuda(), b2.cuda() if bias else None, plan, 1, bits, splits)
    val, idx, pos = plan[0].cpu(), plan[1].cpu().long().reshape(-1), plan[4].cpu().long()
    assert torch.equal(val, torch.ones_like(val))
    w = torch.stack([M._dequant_wo(w_q[e], w_s[e], bits, torch.float64) for e in range(E)])[idx]  # token t's expert
    ref = torch.einsum("tk,tdk->td", h.double()[pos], w) + (b2.double()[idx] if bias else 0)      # and sorted row
    torch.testing.assert_close(out.cpu(), ref.float().bfloat16(), rtol=0, atol=0)


def _inputs(T, E, d, f, bits):
    """x ~ N(0, 1), w1 ~ N(0, 1) / sqrt(d), w2 ~ N(0, 1) / sqrt(f) quantised weight-only, biases ~ N(0, 0.25) -> device"""
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    x, w1, w2, b1, b2 = r(T, d), r(E, d, 2 * f) / d ** 0.5, r(E, f, d) / f ** 0.5, 0.5 * r(E, 2 * f), 0.5 * r(E, d)
    t = {"x": x.bfloat16(), "w": M.quantize_experts_wo(w1, w2, ALGO[bits]), "b1": b1.bfloat16(), "b2": b2.bfloat16()}
    t = {k: tuple(u.cuda() for u in v) if k == "w" else v.cuda() for k, v in t.items()}
    t["logits"] = _logits(T, E, g)
    return t


def _ref(t, val, idx, bits, bias=True):
    """moe_ffn_wo_reference in float64 on the CPU, on the same codes, scales and routing"""
    c = lambda v: v.cpu()
    return M.moe_ffn_wo_reference(c(t["x"]), c(val), c(idx).long(), *map(c, t["w"]), c(t["b1"]) if bias else None,
                                  c(t["b2"]) if bias else None, bits, dtype=torch.float64)


def _check(out, ref, what):
    err, bound = float((out.double().cpu() - ref).abs().max()), float(ref.abs().max()) / 64
    print(f"{what}: max err {err:.5f}, bound {bound:.5f}")
    assert err <= bound


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("T,E,topk,d,f,splits", [
    (1, 8, 2, 64, 64, (None,)), (3, 8, 2, 320, 128, (None,)), (17, 4, 4, 128, 320, (None,)),
    (64, 2, 2, 128, 64, (None,)), (64, 64, 8, 576, 128, (None,)), (5, 16, 1, 64, 64, (None,)),
    (33, 8, 2, 128, 512, (1, 2, 4))])
@pytest.mark.parametrize("bits", [8, 4])
def test_ffn_matches_reference(bits, T, E, topk, d, f, splits, bias):
    t = _inputs(T, E, d, f, bits)
    val, idx = M.decode_plan(t["logits"], topk, True)[:2]
    ref = _ref(t, val, idx, bits, bias)
    b1, b2 = (t["b1"], t["b2"]) if bias else (None, None)
    for s in splits:
        L.reset_calls()
        out = M.moe_decode_ffn_wo(t["x"], t["logits"], *t["w"], b1, b2, topk, True, bits, splits=s)
        assert [L.calls(n) for n in NEW + ("pa_moe_decode_plan", "pa_grouped_gemm")] == [1, 1, 1, 0]
        _check(out, ref, f"splits {s}")


@pytest.mark.parametrize("bits", [8, 4])
def test_fused_moe_wo_dispatch_and_capture(bits):
    T, E, k, d, f = 4, 8, 2, 128, 256
    t = _inputs(T, E, d, f, bits)
    ref = _ref(t, *M.decode_plan(t["logits"], k, True)[:2], bits)
    P = paddle.Tensor
    w1_q, w1_s, w2_q, w2_s = map(P, t["w"])
    kw = dict(ffn1_bias=P(t["b1"].reshape(E, 1, 2 * f)), ffn1_scale=w1_s, ffn2_bias=P(t["b2"].reshape(E, 1, d)),
              ffn2_scale=w2_s, quant_method=ALGO[bits], moe_topk=k)
    run = lambda x, logits: fused_moe(P(x), P(logits), w1_q, w2_q, **kw)
    L.reset_calls()
    out = run(t["x"], t["logits"])
    assert [L.calls(n) for n in NEW + ("pa_moe_decode_plan", "pa_grouped_gemm")] == [1, 1, 1, 0]
    _check(out._t, ref, "fused_moe")
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
    # 65 tokens: dequantise + the grouped kernel
    t65 = dict(t, **{n: v for n, v in _inputs(65, E, d, f, bits).items() if n in ("x", "logits")})
    val, idx = torch.softmax(t65["logits"].double().cpu(), -1).topk(k, -1)
    L.reset_calls()
    before = M.CALLS["wo_fallback"]
    out = run(t65["x"], t65["logits"])
    assert M.CALLS["wo_fallback"] == before and [L.calls(n) for n in NEW] == [0, 0]
    assert L.calls("pa_wo_dequant") == 2 and L.calls("pa_grouped_gemm") == 2
    _check(out._t, _ref(t65, val / val.sum(-1, keepdim=True), idx, bits), "65 tokens")
    with pytest.raises(RuntimeError, match="inference-only"):
        fused_moe(P(t["x"].clone(), stop_gradient=False), P(t["logits"]), w1_q, w2_q, **kw)
    with pytest.raises(ValueError, match="quant_method"):
        fused_moe(P(t["x"]), P(t["logits"]), w1_q, w2_q, **dict(kw, quant_method="bogus"))
