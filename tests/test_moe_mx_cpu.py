"""MXFP4 expert weights of fused_moe off the device: the expert quantiser against mx.quantize_weight, and
fused_moe(quant_method="mxfp4") on CPU tensors against ops.moe.moe_ffn_mx_reference."""
import pytest
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.ops import moe as M
from paddlepaddle_amd.ops import mx as MX

F = paddle.incubate.nn.functional


def _weights(E, d, f):
    g = torch.Generator().manual_seed(E + d + f)
    return torch.randn(E, d, 2 * f, generator=g) / d ** 0.5, torch.randn(E, f, d, generator=g) / f ** 0.5, g


@pytest.mark.parametrize("E,d,f", [(3, 64, 32), (2, 128, 128)])
def test_quantize_experts_is_quantize_weight_per_expert(E, d, f):
    w1, w2, _ = _weights(E, d, f)
    w1_q, w1_s, w2_q, w2_s = (t._t for t in F.fused_moe_quantize_mx(paddle.Tensor(w1), paddle.Tensor(w2)))
    assert w1_q.shape == (E, 2 * f, d // 2) and w1_s.shape == (E, 2 * f, d // 32)
    assert w2_q.shape == (E, d, f // 2) and w2_s.shape == (E, d, f // 32)
    for e in range(E):
        for (q, s), w in (((w1_q, w1_s), w1), ((w2_q, w2_s), w2)):
            rq, rs = MX.quantize_weight(w[e])
            assert torch.equal(q[e], rq) and torch.equal(s[e], rs)


@pytest.mark.parametrize("T,E,k,d,f,bias", [(5, 4, 2, 64, 32, True), (70, 3, 1, 128, 128, False)])
def test_fused_moe_mxfp4_on_cpu_is_the_reference(T, E, k, d, f, bias):
    w1, w2, g = _weights(E, d, f)
    w = M.quantize_experts_mx(w1, w2)
    x, logits = torch.randn(T, d, generator=g).bfloat16(), torch.randn(T, E, generator=g)
    b1, b2 = (0.5 * torch.randn(E, 2 * f, generator=g), 0.5 * torch.randn(E, d, generator=g)) if bias else (None, None)
    P = lambda t: None if t is None else paddle.Tensor(t)
    before = M.CALLS["mx_fallback"]
    out = F.fused_moe(P(x), P(logits), P(w[0]), P(w[2]), ffn1_bias=P(b1), ffn1_scale=P(w[1]), ffn2_bias=P(b2),
                      ffn2_scale=P(w[3]), quant_method="mxfp4", moe_topk=k)
    assert M.CALLS["mx_fallback"] == before + 1
    val, idx = torch.softmax(logits, -1).topk(k, -1)
    ref = M.moe_ffn_mx_reference(x, val / val.sum(-1, keepdim=True), idx, *w, b1, b2)
    assert out._t.dtype == x.dtype and torch.equal(out._t, ref.to(x.dtype))
    # by hand for one token, in float64: the chain of the issue, entry by entry
    dq = lambda q, s, fmt: MX.dequantize_mx(q, s, fmt, torch.float64)
    val, xd, row = (val / val.sum(-1, keepdim=True)).double(), dq(*MX.quantize_mx(x, "mxfp8"), "mxfp8"), torch.zeros(d).double()
    for j in range(k):
        e = int(idx[0, j])
        a, gt = (dq(w[0][e], w[1][e], "mxfp4") @ xd[0] + (b1[e].double() if bias else 0)).chunk(2)
        h = dq(*MX.quantize_mx((torch.nn.functional.silu(a) * gt)[None], "mxfp8"), "mxfp8")[0]
        row += val[0, j] * (dq(w[2][e], w[3][e], "mxfp4") @ h + (b2[e].double() if bias else 0))
    ref64 = M.moe_ffn_mx_reference(x, val, idx, *w, b1, b2, dtype=torch.float64)  # same arithmetic, other sum order
    torch.testing.assert_close(ref64[0], row, rtol=1e-12, atol=1e-12)
    with pytest.raises(RuntimeError, match="inference-only"):
        F.fused_moe(paddle.Tensor(x.clone(), stop_gradient=False), P(logits), P(w[0]), P(w[2]), ffn1_scale=P(w[1]), ffn2_scale=P(w[3]),
                    quant_method="mxfp4", moe_topk=k)
