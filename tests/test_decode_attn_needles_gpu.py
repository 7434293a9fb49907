"""HIP paged / dense decode attention against an fp64 reference that gathers the valid keys only, on needle
inputs (tests/attn_needles.py): every head of a sequence aims at another key the kernel's index arithmetic could
lose (key 0, len - 1, the ends of each split range, 16-key chunk edges), and everything the kernel must never
read is NaN: slots >= len, unreferenced blocks, and the block the spare table entries point to."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_needles as A  # noqa: E402
from paddlepaddle_amd import ops  # noqa: E402
from paddlepaddle_amd.ops import _loader as L  # noqa: E402

DEV = "cuda"


def _check(case, got):
    ref = case.reference().to(DEV)
    r, idx = A.excess(got, ref, A.DECODE_ATOL, A.RTOL[torch.bfloat16])
    print(f"[needle] {case.id} splits {case.splits}: {r:.3f} x tol at {idx}")
    A.check(got, ref, A.DECODE_ATOL, A.RTOL[torch.bfloat16], what=case.id)
    for n, ln in enumerate(case.lens_list):
        if ln == 0:
            assert float(got[n].abs().max()) == 0.0, "an empty sequence gives zeros"
    assert L.calls("pa_paged_decode_attn") > 0


@pytest.mark.parametrize("spec", A.decode_specs(), ids=lambda s: f"G{s[0]}-bs{s[1]}-hint{s[3]}")
def test_paged_decode_needles(spec):
    G, bs, lens, hint, seed = spec
    case = A.DecodeCase(G, bs, lens, hint, seed=seed)
    want_splits = 1 if hint == 4 * bs else 2 if hint == 8 * bs else None
    assert case.splits == want_splits or (want_splits is None and case.splits >= 2)
    if want_splits is None:   # the maximum: the short sequences of the batch leave splits without a block
        assert case.splits > (min(l for l in lens if l) + bs - 1) // bs
    assert int(case.tables.max()) < case.kc.shape[0] and int(case.tables.min()) >= 0
    q, kc, vc, tab, ln = (t.to(DEV) for t in (case.q, case.kc, case.vc, case.tables, case.lens))
    _check(case, ops.paged_decode_attention(q, kc, vc, tab, ln, max_len=hint))


@pytest.mark.parametrize("spec", A.dense_decode_specs(), ids=lambda s: f"G{s[0]}-Lc{s[1]}")
def test_dense_decode_needles(spec):
    G, Lc, lens, seed = spec
    case = A.DenseDecodeCase(G, Lc, lens, seed=seed)
    q, kc, vc, ln = (t.to(DEV) for t in (case.q, case.kc, case.vc, case.lens))
    _check(case, ops.dense_decode_attention(q, kc, vc, ln))
