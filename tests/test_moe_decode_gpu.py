"""MoE decode kernels (csrc/kernels/moe_decode.hip): the plan exactly, the FFN against a float64 per-token loop, and
fused_moe's dispatch between them and the grouped path."""
import pytest
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.ops import _loader as L
from paddlepaddle_amd.ops import moe as M

pytestmark = pytest.mark.gpu
fused_moe = paddle.incubate.nn.functional.fused_moe


def _inputs(T, E, d, f, seed=0):
    """x ~ N(0, 1), w1 ~ N(0, 1) / sqrt(d), w2 ~ N(0, 1) / sqrt(f), biases ~ N(0, 0.25), all bf16; every token's
    logits a permutation of 0.25 arange(E) (distinct, so the top-k set is unambiguous)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    t = {"x": r(T, d), "w1": r(E, d, 2 * f) / d ** 0.5, "w2": r(E, f, d) / f ** 0.5, "b1": 0.5 * r(E, 2 * f),
         "b2": 0.5 * r(E, d)}
    t = {k: v.bfloat16().cuda() for k, v in t.items()}
    t["logits"] = torch.stack([0.25 * torch.randperm(E, generator=g) for _ in range(T)]).float().cuda()
    return t


def _ref(t, topk, norm=True, bias=True):
    """The per-token loop of test_fused_moe_matches_reference_and_captures in float64 -> (out, val, idx)."""
    x, w1, w2, b1, b2 = (t[k].double().cpu() for k in ("x", "w1", "w2", "b1", "b2"))
    val, idx = torch.softmax(t["logits"].double().cpu(), -1).topk(topk, -1)
    if norm:
        val = val / val.sum(-1, keepdim=True)
    out = torch.zeros_like(x)
    for r in range(x.shape[0]):
        for j in range(topk):
            e = int(idx[r, j])
            a, g = (x[r] @ w1[e] + (b1[e] if bias else 0)).chunk(2)
            out[r] += val[r, j] * ((torch.nn.functional.silu(a) * g) @ w2[e] + (b2[e] if bias else 0))
    return out, val, idx


@pytest.mark.parametrize("T,E,topk,norm", [(1, 8, 2, True), (64, 64, 8, True), (17, 4, 4, False), (5, 16, 1, True),
                                           (64, 256, 8, True)])
def test_plan_exact(T, E, topk, norm):
    t = _inputs(T, E, 64, 64)
    val, idx, offs, perm, pos, active, n_active = (v.cpu() for v in M.decode_plan(t["logits"], topk, norm))
    _, rval, ridx = _ref(t, topk, norm)
    assert torch.equal(idx.long(), ridx)
    flat = ridx.reshape(-1)
    rperm = torch.argsort(flat, stable=True)
    counts = torch.bincount(flat, minlength=E)
    assert torch.equal(perm.long(), rperm)
    assert offs.tolist() == [0] + torch.cumsum(counts, 0).tolist()
    assert torch.equal(pos.long()[rperm], torch.arange(T * topk))
    assert active[:int(n_active)].tolist() == torch.nonzero(counts).reshape(-1).tolist()
    torch.testing.assert_close(val.double(), rval, rtol=2e-5, atol=0)


FFN_SHAPES = [(1, 8, 2, 64, 64), (3, 8, 2, 320, 192), (17, 4, 4, 128, 448), (64, 64, 8, 256, 128),
              (5, 16, 1, 128, 64), (64, 2, 2, 128, 128), (33, 8, 2, 192, 256)]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("T,E,topk,d,f", FFN_SHAPES)
def test_ffn_matches_float64(T, E, topk, d, f, bias):
    t = _inputs(T, E, d, f)
    ref = _ref(t, topk, bias=bias)[0]
    b1, b2 = (t["b1"], t["b2"]) if bias else (None, None)
    for splits in (1, 2) if (f // 64) % 2 == 0 else (1,):
        L.reset_calls()
        out = M.moe_decode_ffn(t["x"], t["logits"], t["w1"], t["w2"], b1, b2, topk, True, splits=splits)
        assert L.calls("pa_moe_decode_ffn") == 1 and L.calls("pa_moe_decode_plan") == 1
        assert L.calls("pa_grouped_gemm") == 0
        err, bound = float((out.double().cpu() - ref).abs().max()), float(ref.abs().max()) / 64
        print(f"splits {splits}: max err {err:.5f}, bound {bound:.5f}")
        assert err <= bound


def test_fused_moe_dispatch_and_capture():
    T, E, k, d, f = 4, 8, 2, 128, 256
    t = _inputs(T, E, d, f)
    ref = _ref(t, k)[0]
    a = [paddle.Tensor(t[n]) for n in ("x", "logits", "w1", "w2")]
    kw = dict(ffn1_bias=paddle.Tensor(t["b1"].reshape(E, 1, 2 * f)), ffn2_bias=paddle.Tensor(t["b2"].reshape(E, 1, d)),
              moe_topk=k)
    L.reset_calls()
    out = fused_moe(*a, **kw)
    assert L.calls("pa_moe_decode_ffn") == 1 and L.calls("pa_moe_decode_plan") == 1
    assert L.calls("pa_grouped_gemm") == 0 and L.calls("pa_moe_route") == 0
    assert float((out._t.double().cpu() - ref).abs().max()) <= float(ref.abs().max()) / 64
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fused_moe(*a, **kw)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        o2 = fused_moe(*a, **kw)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o2._t, out._t)
    # something to differentiate, or more than 64 tokens: the grouped path, as before
    L.reset_calls()
    xg = paddle.Tensor(t["x"].clone(), stop_gradient=False)
    assert xg._t.requires_grad and torch.is_grad_enabled()
    fused_moe(xg, *a[1:], **kw)
    assert L.calls("pa_grouped_gemm") == 2 and L.calls("pa_moe_decode_ffn") == 0
    L.reset_calls()
    t65 = _inputs(65, E, d, f)
    fused_moe(*[paddle.Tensor(t65[n]) for n in ("x", "logits")], *a[2:], **kw)
    assert L.calls("pa_grouped_gemm") == 2 and L.calls("pa_moe_decode_ffn") == 0
