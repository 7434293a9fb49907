"""The needle harness (tests/attn_needles.py) checked on the CPU: its tolerances follow from the rounding model,
the rounding model passes them, and every reference mutant that loses or leaks ONE key (block) is flagged by a
wide margin -- the property the randn-based attention tests lack. Also the CPU fallbacks of the decode ops and of
the LSE: stale cache slots holding NaN, empty sequences, rows without a visible key."""
import math

import pytest
import torch

import attn_needles as A
from paddlepaddle_amd import ops
from paddlepaddle_amd.ops import attention as attn_mod

NAMES = ("o", "dq", "dk", "dv")


def _ratios(out, ref, dtype):
    return {n: A.excess(out[n], ref[n], *A.tolerances(dtype, n, ref[n]))[0] for n in NAMES}


def _assert_flagged(case, vis_mut, what, **mut_kw):
    """The mutant (reference evaluated with a wrong visibility) must exceed the forward tolerance >= 10x and at
    least one gradient tolerance; the rounding model of the right computation must pass everything."""
    t, kw = case.dense()
    ref = A.reference(*t, **kw)
    model = A.rounding_model(*t, **kw)
    for n in NAMES:
        A.check(model[n], ref[n], *A.tolerances(case.dtype, n, ref[n]), what=f"{what}: rounding model {n}")
    A.check(model["lse"], ref["lse"], A.LSE_ATOL, 0.0, what=f"{what}: rounding model lse")
    mut = A.reference(*t, **dict(kw, vis=vis_mut, **mut_kw))
    r = _ratios(mut, ref, case.dtype)
    assert r["o"] >= 10.0, f"{what}: forward error only {r['o']:.3g} x tolerance"
    assert max(r["dq"], r["dk"], r["dv"]) > 1.0, f"{what}: no gradient flags it: {r}"


def test_constants_follow_from_the_rounding_model():
    """TOL / LSE_ATOL / DECODE_ATOL are 4 x (8 x) the measured figures, capped by the older tests' bounds; the
    measurement itself is redone here over every case of the GPU files."""
    worst, lse_w, dec_w, dec_bound = A.measure(verbose=False)
    for dt, d in worst.items():
        for n, (e, cid) in d.items():
            cap = A.FWD_CAP if n == "o" else A.GRAD_CAP
            assert A.TOL[dt][n] <= cap
            assert A.TOL[dt][n] == min(4 * A.MEASURED[dt][n], cap)
            assert 0.8 <= A.MEASURED[dt][n] / e <= 1.25, f"{dt} {n}: recorded {A.MEASURED[dt][n]}, measured {e} ({cid})"
            assert e <= A.TOL[dt][n], f"{dt} {n}: the rounding model itself needs {e} ({cid})"
    assert 0.8 <= A.LSE_MEASURED / lse_w[0] <= 1.25 and A.LSE_ATOL == 8 * A.LSE_MEASURED <= 1e-3
    assert dec_w[0] == 0.0, "an fp32 decode is inside rtol everywhere"
    assert dec_bound <= A.DECODE_ATOL <= 2e-2


def test_needles_and_traps_dominate_their_rows():
    c = A.Case((1, 257, 193, 4, 2), 128, causal=True, feature="bool", seed=2)
    (q, k, v, do), kw = c.dense()
    tgt, role = A.needle_targets(c.vis)
    qh, kh, _ = A._heads(q.double(), k.double(), v.double())
    raw = torch.softmax(torch.matmul(qh, kh.transpose(-1, -2)) / math.sqrt(c.D), -1)      # no mask at all
    w = torch.gather(raw, 3, tgt.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    aimed = tgt >= 0
    assert aimed.float().mean() > 0.6
    assert float(w[aimed].median()) > 0.5, "a target key holds most of its row"
    tvis = torch.gather(c.vis, 3, tgt.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    assert bool(tvis[aimed & (role != 1)].all()) and not bool(tvis[aimed & (role == 1)].any())
    # different heads of one GQA group aim elsewhere
    assert float((tgt[:, 0] != tgt[:, 1])[aimed[:, 0] & aimed[:, 1]].float().mean()) > 0.5


def test_mutant_diagonal_lost_in_last_q_block():
    c = A.Case((1, 512, 512, 2, 2), 128, causal=True)
    vis = c.vis.clone()
    r = torch.arange(384, 512)
    vis[:, :, r, r] = False
    _assert_flagged(c, vis, "diagonal lost, rows >= 384")


def test_mutant_diagonal_plus_one_visible():
    c = A.Case((1, 512, 512, 2, 2), 128, causal=True)
    vis = c.vis.clone()
    r = torch.arange(384, 511)
    vis[:, :, r, r + 1] = True
    _assert_flagged(c, vis, "diag + 1 visible, rows >= 384")


def test_mutant_diagonal_bottom_right_alignment():
    c = A.Case((1, 65, 200, 2, 1), 128, causal=True)
    vis = c.vis.clone()
    r = torch.arange(65)
    vis[:, :, r, r + 135] = False
    _assert_flagged(c, vis, "diagonal lost, Sq != Sk")


def test_mutant_last_key_lost():
    c = A.Case((1, 65, 200, 2, 1), 128, causal=False)
    vis = c.vis.clone()
    vis[..., 199] = False
    _assert_flagged(c, vis, "key Sk - 1 lost")


@pytest.mark.parametrize("causal", [False, True])
def test_mutant_varlen_leak(causal):
    c = A.Case((1, 257, 193, 4, 2), 128, causal=causal, feature="varlen", seed=2)
    vis = c.vis.clone()
    vis[:, :, 65:130, 130] = True            # the 65-token sequence sees the first key of the next one
    _assert_flagged(c, vis, "first key of the next sequence leaked")
    if not causal:                           # (causal: only one row sees that key)
        vis = c.vis.clone()
        vis[:, :, 65:130, 129] = False       # ... or loses its own last key
        _assert_flagged(c, vis, "last key of a sequence lost")


@pytest.mark.parametrize("feature,causal,col,delta", [
    ("fm1", True, 0, 1), ("fm1", True, 0, -1), ("fm2", True, 1, 1), ("fm2", False, 1, -1), ("fm4", False, 2, 1),
    ("fm4", False, 1, -1)])
def test_mutant_flashmask_bound_off_by_one(feature, causal, col, delta):
    c = A.Case((2, 130, 130, 2, 2), 128, causal=causal, feature=feature, seed=2)
    se = c.startend.clone()
    se[..., col] += delta
    _assert_flagged(c, A.flashmask_keep(se, c.Sq, c.Sk, causal).expand_as(c.vis), f"{feature} column {col} {delta:+d}")


@pytest.mark.parametrize("which", ["causal", "lower", "upper"])
def test_mutant_flashmask_tile_class(which):
    """The tile classes taken one row too wide: 'skip' also when row q_lo is still visible (tile 1 of block 1)."""
    c = A.tile_edge_case(which)
    vis = c.vis.clone()
    vis[:, :, 128, 64:128] = False
    _assert_flagged(c, vis, "tile 1 skipped for block 1 although row 128 sees it")


@pytest.mark.parametrize("feature", ["bool", "add_bf16", "add_f32"])
def test_mutant_masked_key_visible(feature):
    c = A.Case((1, 257, 193, 4, 2), 128, causal=False, feature=feature, seed=2)
    vis = c.vis.clone()
    bias = c.bias
    if feature == "bool":
        first_masked = ~c.vis & torch.roll(c.vis, 1, -1)
        first_masked[..., 0] = False
        vis |= first_masked
        _assert_flagged(c, vis, "first masked key of each range visible")
    else:
        inf = torch.isinf(bias)
        first = inf & ~torch.roll(inf, 1, -1)
        first[..., 0] = False
        _assert_flagged(c, vis, "first -inf entry of each row read as 0", bias=bias.masked_fill(first, 0.0))


def test_dead_rows_reference_contract():
    c = A.Case((1, 257, 193, 4, 2), 64, causal=True)
    t, kw = c.dense()
    ref = A.reference(*t, **kw)
    assert bool((ref["o"][:, :64] == 0).all()) and bool((ref["dq"][:, :64] == 0).all())
    assert bool(torch.isposinf(ref["lse"][:, :, :64]).all()) and bool(torch.isfinite(ref["lse"][:, :, 64:]).all())


# ------------------------------------------------------------------------------------------------- decode
def _decode_case():
    return A.DecodeCase(4, 16, [0, 1, 15, 16, 17, 63, 64, 65, 1025], None, seed=3)


def _decode_ratio(got, ref):
    return A.excess(got, ref, A.DECODE_ATOL, A.RTOL[torch.bfloat16])[0]


def test_decode_rounding_model_passes_and_mutants_are_flagged():
    c = _decode_case()
    ref = c.reference()
    n = 8
    ln = c.lens_list[n]
    assert c.splits > 2 and float(ref[0].abs().max()) == 0.0
    A.check(c.reference(dt=torch.float32).bfloat16(), ref, A.DECODE_ATOL, A.RTOL[torch.bfloat16], "fp32 model")
    assert _decode_ratio(c.reference(drop=(n, [ln - 1])), ref) >= 10, "last key lost"
    assert _decode_ratio(c.reference(drop=(3, [15])), ref) >= 10, "last key lost, len == block size"
    for m in (2, 3, 8):
        assert _decode_ratio(c.reference(stale=m), ref) == A.INF, "a stale slot is NaN: reading it must show"
    chunk_tgts = [t for t in c.targets[n].tolist() if t >= 16 and t // 16 * 16 + 16 <= ln]
    for t in chunk_tgts[:3]:
        lost = list(range(t // 16 * 16, t // 16 * 16 + 16))
        assert _decode_ratio(c.reference(drop=(n, lost)), ref) >= 10, f"16-key chunk at {lost[0]} lost"
    per = -(-((ln + 15) // 16) // c.splits) * 16
    for sp in (1, (ln - 1) // per):          # a middle one and the last non-empty one
        lost = list(range(sp * per, min(ln, (sp + 1) * per)))
        assert lost and _decode_ratio(c.reference(drop=(n, lost)), ref) >= 10, f"split {sp} lost"


def test_decode_splits_mirror():
    for N, Hkv, ml, bs in [(9, 16, 64, 16), (9, 2, 1040, 8), (4, 4, 512, 64), (9, 4, 128 * 11, 128),
                           (1, 1, 10 ** 5, 16)]:
        assert A.decode_splits(N, Hkv, ml, bs) == attn_mod._decode_splits(N, Hkv, ml, bs)
    hints = {A.DecodeCase(2, 16, [1, 1025], h).splits for h in (64, 128, None)}
    assert 1 in hints and 2 in hints and max(hints) > 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_paged_fallback_ignores_stale_slots_and_empty_sequences(dtype):
    """NaN in every slot >= len and in every unreferenced block; len 0 gives zeros (as the HIP kernel)."""
    c = _decode_case()
    q, kc, vc = (t.to(dtype) for t in (c.q, c.kc, c.vc))
    for fn in (attn_mod.paged_decode_reference, ops.paged_decode_attention):
        got = fn(q, kc, vc, c.tables, c.lens)
        assert bool(torch.isfinite(got).all()), "stale NaN slots leaked into the output"
        assert float(got[0].abs().max()) == 0.0
        if dtype == torch.float32:
            A.check(got, c.reference(), 1e-5, 1e-5, "paged fallback")
        else:
            A.check(got, c.reference(), A.DECODE_ATOL, A.RTOL[dtype], "paged fallback")


def test_paged_fallback_ignores_inf_in_stale_slots():
    c = A.DecodeCase(2, 8, [3, 8, 9], None, H=4, D=32, seed=1)
    kc = torch.nan_to_num(c.kc.float(), nan=float("inf"))
    vc = torch.nan_to_num(c.vc.float(), nan=float("-inf"))
    got = attn_mod.paged_decode_reference(c.q.float(), kc, vc, c.tables, c.lens)
    A.check(got, c.reference(), 1e-5, 1e-5, "paged fallback, Inf poison")


@pytest.mark.parametrize("Lc", [64, 80])
def test_dense_fallback_ignores_stale_positions(Lc):
    c = A.DenseDecodeCase(2, Lc, [1, 64, 33, Lc], H=4, D=32, seed=2)
    got = ops.dense_decode_attention(c.q.float(), c.kc.float(), c.vc.float(), c.lens)
    A.check(got, c.reference(), 1e-5, 1e-5, "dense fallback")
    lens0 = c.lens.clone()
    lens0[2] = 0
    got0 = ops.dense_decode_attention(c.q.float(), c.kc.float(), c.vc.float(), lens0)
    assert float(got0[2].abs().max()) == 0.0 and bool(torch.isfinite(got0).all())


def test_lse_reference_dead_rows_are_plus_inf():
    c = A.Case((1, 65, 33, 2, 1), 32, causal=True, seed=1)       # rows 0..31 see no key
    lse = attn_mod._lse_reference(c.q.float(), c.k.float(), True, 1 / math.sqrt(32), None)
    ref = A.reference(*c.dense()[0], **c.dense()[1])["lse"]
    assert bool(torch.isposinf(lse[:, :, :32]).all())
    A.check(lse, ref, A.LSE_ATOL, 0.0, "lse fallback")
    keep = torch.ones(1, 1, 65, 33, dtype=torch.bool)
    keep[:, :, 40] = False
    lse = attn_mod._lse_reference(c.q.float(), c.k.float(), False, 1 / math.sqrt(32), keep)
    assert bool(torch.isposinf(lse[:, :, 40]).all()) and bool(torch.isfinite(lse[:, :, :40]).all())
    add = torch.zeros(1, 1, 65, 33).masked_fill(~keep, float("-inf"))
    assert torch.equal(attn_mod._lse_reference(c.q.float(), c.k.float(), False, 1 / math.sqrt(32), add), lse)
    _, lse_op = attn_mod.attention(c.q.float(), c.k.float(), c.v.float(), mask=keep, return_lse=True)
    assert bool(torch.isposinf(lse_op[:, :, 40]).all())
