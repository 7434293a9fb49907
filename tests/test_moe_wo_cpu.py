"""Weight-only int8 / int4 expert weights of fused_moe off the device: the expert quantiser against
nn.quant.weight_quantize, and fused_moe(quant_method="weight_only_int8" | "weight_only_int4") on CPU tensors against
fused_moe(quant_method="None") on the dequantised weights."""
import pytest
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.ops import moe as M

F = paddle.incubate.nn.functional
Q = paddle.nn.quant
P = lambda t: None if t is None else paddle.Tensor(t)


def _weights(E, d, f):
    g = torch.Generator().manual_seed(E + d + f)
    return torch.randn(E, d, 2 * f, generator=g) / d ** 0.5, torch.randn(E, f, d, generator=g) / f ** 0.5, g


@pytest.mark.parametrize("algo,pack", [("weight_only_int8", 1), ("weight_only_int4", 2)])
def test_quantize_experts_is_weight_quantize_per_expert(algo, pack):
    E, d, f = 3, 64, 64
    w1, w2, _ = _weights(E, d, f)
    w1_q, w1_s, w2_q, w2_s = (t._t for t in F.fused_moe_quantize_wo(P(w1), P(w2), algo))
    assert w1_q.shape == (E, 2 * f // pack, d) and w1_s.shape == (E, 2 * f) and w1_s.dtype == torch.float32
    assert w2_q.shape == (E, d // pack, f) and w2_s.shape == (E, d) and w1_q.dtype == torch.int8
    for e in range(E):
        for (q, s), w in (((w1_q, w1_s), w1), ((w2_q, w2_s), w2)):
            rq, rs = Q.weight_quantize(P(w[e]), algo)
            assert torch.equal(q[e], rq._t) and torch.equal(s[e], rs._t.float())


@pytest.mark.parametrize("algo", ["weight_only_int8", "weight_only_int4"])
@pytest.mark.parametrize("T,E,k,d,f,bias", [(5, 4, 2, 64, 64, True), (70, 3, 1, 128, 64, False)])
def test_fused_moe_wo_on_cpu_is_fused_moe_on_the_dequantised_weights(algo, T, E, k, d, f, bias):
    """The two differ only by the bf16 rounding of h (the kernels keep h in bf16, so the reference path does too):
    the project's bound for this chain, max |ref| / 64."""
    w1, w2, g = _weights(E, d, f)
    w = M.quantize_experts_wo(w1, w2, algo)
    x, logits = torch.randn(T, d, generator=g), torch.randn(T, E, generator=g)
    b1, b2 = (0.5 * torch.randn(E, 1, 2 * f, generator=g), 0.5 * torch.randn(E, 1, d, generator=g)) if bias else (None, None)
    before = M.CALLS["wo_fallback"]
    out = F.fused_moe(P(x), P(logits), P(w[0]), P(w[2]), ffn1_bias=P(b1), ffn1_scale=P(w[1].double()), ffn2_bias=P(b2),
                      ffn2_scale=P(w[3]), quant_method=algo, moe_topk=k)._t
    assert M.CALLS["wo_fallback"] == before + 1 and out.dtype == x.dtype
    dq = lambda q, s: torch.stack([Q.weight_dequantize(P(q[e]), P(s[e]), algo, "float32")._t for e in range(E)])
    ref = F.fused_moe(P(x), P(logits), P(dq(w[0], w[1])), P(dq(w[2], w[3])), ffn1_bias=P(b1), ffn2_bias=P(b2),
                      moe_topk=k)._t
    assert float((out - ref).abs().max()) <= float(ref.abs().max()) / 64
    with pytest.raises(RuntimeError, match="inference-only"):
        F.fused_moe(paddle.Tensor(x.clone(), stop_gradient=False), P(logits), P(w[0]), P(w[2]), ffn1_scale=P(w[1]),
                    ffn2_scale=P(w[3]), quant_method=algo, moe_topk=k)
    with pytest.raises(ValueError, match="quant_method"):
        F.fused_moe(P(x), P(logits), P(w[0]), P(w[2]), ffn1_scale=P(w[1]), ffn2_scale=P(w[3]), quant_method="bogus")
