"""ops.paged_prefill_attention / dense_prefill_attention on the CPU: the fp32 fallback against the fp64 reference on
the poisoned needle batch of tests/paged_prefill_cases.py, the clamp of a ragged ctx_lens < n_b, the argument errors,
and the rounding model that backs the tolerance the GPU tests use."""
import pytest
import torch

import attn_needles as A
import paged_prefill_cases as C
from paddlepaddle_amd import ops

BF16 = torch.bfloat16


def _check(got, c, what):
    atol, rtol = A.tolerances(BF16, "o", c.ref)
    print(f"[prefill] {what}: {A.excess(got, c.ref, atol, rtol)[0]:.3f} x tol")
    A.check(got, c.ref, atol, rtol, what)
    assert float(got[c.cu[2]:c.cu[3]].abs().sum()) == 0 and float(got[-c.pad:].abs().max()) == 0


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("quant", [False, True], ids=["float", "uint8"])
@pytest.mark.parametrize("dense_lc", [None, 256], ids=["paged", "dense"])
def test_prefill_fallback(dtype, quant, dense_lc):
    c = C.build(4, 16, quant=quant, dense_lc=dense_lc, dtype=dtype)
    got = C.run(ops.paged_prefill_attention, ops.dense_prefill_attention, c)
    assert got.dtype == dtype
    _check(got, c, f"fallback {dtype} quant={quant} dense={dense_lc}")


@pytest.mark.parametrize("G", [1, 4, 8])
def test_rounding_model_within_tolerance(G):
    """The bf16-P rounding model (what a correct kernel may lose) passes the check the GPU tests apply."""
    c = C.build(G, 16)
    atol, rtol = A.tolerances(BF16, "o", c.ref)
    r, _ = A.excess(c.model, c.ref, atol, rtol)
    print(f"[prefill] rounding model G{G}: {r:.3f} x tol")
    assert r <= 1.0


def test_ragged_ctx_is_clamped():
    """ctx_lens < n_b: start clamps to 0, token i sees keys 0 .. min(i, ctx - 1); nothing reads a negative position
    or a slot at or past ctx (NaN here)."""
    n, ctx, H = 5, 3, 4
    vis = A.causal_keep(n, n)[:, :ctx]
    q, k, v, do = A.needle_inputs(1, n, ctx, H, C.HKV, C.D, BF16, vis)
    ref = A.reference(q, k, v, do, vis)["o"][0]
    kc = torch.full((1, C.HKV, 64, C.D), float("nan"), dtype=BF16)
    vc = kc.clone()
    kc[0, :, :ctx], vc[0, :, :ctx] = k[0].transpose(0, 1), v[0].transpose(0, 1)
    cu, cl = torch.tensor([0, n], dtype=torch.int32), torch.tensor([ctx], dtype=torch.int32)
    for got in (ops.dense_prefill_attention(q[0], kc, vc, cu, cl),
                ops.paged_prefill_attention(q[0], kc, vc, torch.zeros(1, 1).int(), cu, cl)):   # one 64-slot block
        A.check(got, ref, *A.tolerances(BF16, "o", ref), "ragged")


def test_argument_errors():
    c, f = C.build(4, 16, quant=True), C.build(4, 16)
    a8 = (c.q, c.kc, c.vc, c.tables, c.cu, c.ctx)
    with pytest.raises(ValueError):
        ops.paged_prefill_attention(*a8)                                       # uint8 without scales
    with pytest.raises(ValueError):
        ops.paged_prefill_attention(f.q, f.kc, f.vc, f.tables, f.cu, f.ctx, **c.kw)   # scales with a float cache
    with pytest.raises(ValueError):
        ops.paged_prefill_attention(f.q[:, :7], f.kc, f.vc, f.tables, f.cu, f.ctx)    # 7 heads over 2 kv heads
