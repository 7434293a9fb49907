"""The paged prefill MFMA kernel (csrc/kernels/prefill_paged_attn.hip) through ops.paged_prefill_attention,
dense_prefill_attention and block_multihead_attention's prefix-cache prefill, against the fp64 reference on the
poisoned needle batch of tests/paged_prefill_cases.py. Tolerance: attn_needles' forward bound (bf16-P rounding model)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_needles as A  # noqa: E402
import paged_prefill_cases as C  # noqa: E402
import paddlepaddle_amd as paddle  # noqa: E402
import paddlepaddle_amd.incubate.nn.functional as IF  # noqa: E402
from paddlepaddle_amd import ops  # noqa: E402
from paddlepaddle_amd.ops import _loader as L  # noqa: E402

DEV = "cuda"
BF, Q8 = "pa_paged_prefill_attn", "pa_paged_prefill_attn_q8"


def _run_check(c, name, what):
    for hint in (c.max_q, None):   # the exact bound on n_b, then the default (T)
        before = L.calls(name)
        got = C.run(ops.paged_prefill_attention, ops.dense_prefill_attention, c, DEV, max_q=hint).cpu()
        assert L.calls(name) > before
        atol, rtol = A.tolerances(torch.bfloat16, "o", c.ref)
        print(f"[prefill] {what} max_q={hint}: {A.excess(got, c.ref, atol, rtol)[0]:.3f} x tol")
        A.check(got, c.ref, atol, rtol, what)
        assert float(got[c.cu[2]:c.cu[3]].abs().sum()) == 0, "the empty chunk writes nothing"
        assert float(got[-c.pad:].abs().max()) == 0, "rows past cu_q[B] are zero"


@pytest.mark.parametrize("bs", [16, 64])
@pytest.mark.parametrize("G", [1, 4, 8])
def test_paged_prefill_needles(G, bs):
    _run_check(C.build(G, bs), BF, f"G{G}-bs{bs}")


@pytest.mark.parametrize("bs", [16, 64])
def test_paged_prefill_q8_needles(bs):
    _run_check(C.build(4, bs, quant=True), Q8, f"q8-bs{bs}")


def test_dense_prefill_needles():
    _run_check(C.build(4, 64, dense_lc=256), BF, "dense-Lc256")


def test_block_mha_prefix_prefill_runs_the_kernel():
    """bf16 prefix-cache prefill (P = 19, sequences of 21 and 3 tokens, H 8 / Hk 2, bs 16) against fp64 attention over
    prefix + tokens; an additive ``mask`` keeps the math path."""
    H, Hk, D, bs, P, ns = 8, 2, 128, 16, 19, [21, 3]
    gen = torch.Generator().manual_seed(4)
    Pt = lambda t, dt=None: paddle.to_tensor(t.to(device=DEV, dtype=dt))  # noqa: E731
    i32 = torch.int32
    x = (0.5 * torch.randn(sum(ns), H + 2 * Hk, D, generator=gen)).bfloat16()
    pk, pv = (torch.randn(2, Hk, P, D, generator=gen).bfloat16() for _ in range(2))
    tables = torch.randperm(8, generator=gen).view(2, 4)
    cu = torch.tensor([0, ns[0], sum(ns)])

    def call(mask=None):
        kc = torch.full((8, Hk, bs, D), float("nan"), dtype=torch.bfloat16, device=DEV)
        out = IF.block_multihead_attention(
            Pt(x.view(sum(ns), -1)), Pt(kc), Pt(kc.clone()), Pt(torch.tensor(ns), i32), Pt(torch.zeros(2), i32),
            Pt(torch.tensor(ns), i32), None, None, Pt(cu, i32), Pt(cu, i32), Pt(tables, i32), pre_key_cache=Pt(pk),
            pre_value_cache=Pt(pv), mask=mask, block_size=bs)[0]
        return out.reshape([sum(ns), H, D])._t.cpu()

    before = L.calls(BF)
    got = call()
    assert L.calls(BF) == before + 1
    for b, n in enumerate(ns):
        k = torch.cat([pk[b].transpose(0, 1), x[cu[b]:cu[b + 1], H:H + Hk]])[None]
        v = torch.cat([pv[b].transpose(0, 1), x[cu[b]:cu[b + 1], H + Hk:]])[None]
        q = x[cu[b]:cu[b + 1], :H][None]
        ref = A.reference(q, k, v, torch.zeros_like(q), A.causal_keep(n, P + n))["o"][0]
        A.check(got[cu[b]:cu[b + 1]], ref, *A.tolerances(torch.bfloat16, "o", ref), f"blha seq {b}")
    keep = torch.arange(P + 21)[None] <= torch.arange(21)[:, None] + P
    call(mask=Pt(torch.zeros(2, 1, 21, P + 21).masked_fill(~keep, -1e4)))
    assert L.calls(BF) == before + 1, "a mask keeps the math path"
