"""CPU proof that the exact small-integer inputs of tests/gemm_exact.py catch the bugs the older GEMM tests let
through: every listed mutant of the reference fails ``assert_bits_equal``, while the two cast mutants pass the older
criteria (largest error over largest value < 1e-2; atol 0.15 + rtol 1e-2) at the older tests' own shapes.
Also checks the exactness bound and the rounding share of every GPU case of tests/test_gemm_exact_gpu.py and the
measured constants of the inexact (GELU) epilogues."""
import pytest
import torch

import gemm_exact as X

BF16, F32 = X.BF16, X.F32


def _caught(got, want, what):
    with pytest.raises(AssertionError):
        X.assert_bits_equal(got, want, what)


# ------------------------------------------------------------------------------------------------ the helper
def test_assert_bits_equal_semantics():
    w = torch.tensor([[0.0, 1.0], [2.0, -3.0]])
    for dt in (BF16, F32):
        X.assert_bits_equal(w.to(dt), w.to(dt), "same")
        X.assert_bits_equal((w * torch.tensor([[-1.0, 1.0], [1.0, 1.0]])).to(dt), w.to(dt), "-0 == +0")
        g = w.clone()
        g[1, 1] = float("nan")
        _caught(g.to(dt), w.to(dt), "nan")
    g = w.clone()
    g[1, 0] = 2.0 + 2.0 ** -22      # one fp32 ulp
    with pytest.raises(AssertionError, match=r"1 of 4 elements differ.*bounding box \[1, 0\] \.\. \[1, 0\]"):
        X.assert_bits_equal(g, w, "ulp")
    _caught(w.to(BF16), w, "dtype")


def test_exact_ref_rejects_inexact_cases():
    a, b = X.ints((8, 64), seed=1), X.ints((64, 8), seed=2)
    X.exact_ref(a, b, alpha=0.5)
    with pytest.raises(AssertionError):
        X.exact_ref(a, b, alpha=0.3)                    # not a power of two
    with pytest.raises(AssertionError):
        X.exact_ref(a * 2 ** 12, b * 2 ** 12)           # sums beyond 2^24
    with pytest.raises(AssertionError):                 # half-integers beyond 2^23
        X.exact_ref(a, b, base=torch.full((8, 8), 2.0 ** 23 + 0.5, dtype=torch.float64))
    with pytest.raises(AssertionError):                 # not a bf16 value
        X.exact_ref(a, b, bias=torch.full((8,), 257.0, dtype=torch.float64))


def test_placed_guards():
    v = X.ints((5, 16), seed=3)
    for tr in (False, True):
        p = X.place(v, BF16, "cpu", pad=8, guard=2, transposed=tr)
        assert torch.equal(p.view.double(), v) and int(torch.isnan(p.buf).sum()) == p.buf.numel() - v.numel()
    o = X.place((5, 16), F32, "cpu", pad=4, guard=2, poison=False)
    o.view.zero_()
    o.guards_intact("untouched")
    o.buf[5, 0] = 1.0
    with pytest.raises(AssertionError, match="guard"):
        o.guards_intact("row M written")


# ------------------------------------------------------------------------ every GPU case: bound and rounding
def test_every_gpu_case_is_exact_and_checks_the_cast():
    exempt, total, ties_total = [], 0, 0.0
    for cid, ref, is_bf16 in X.all_cases():       # building the case asserts its exactness bound
        assert not bool(torch.isnan(ref).any())
        if not is_bf16:
            continue
        inexact, ties = X.rounding_share(ref)
        if ties < X.MIN_TIES and ref.numel() <= 64:
            exempt.append(cid)
            X.assert_rounding_checked(ref, cid, need_ties=False)
        else:
            X.assert_rounding_checked(ref, cid)
        total += ref.numel()
        ties_total += ties * ref.numel()
    # rows of a few elements may miss the tie share; they are listed, and the cases as a whole satisfy it
    assert set(exempt) <= set(X.TIE_EXEMPT_IDS), exempt
    assert ties_total / total >= X.MIN_TIES


def test_narrow_range_does_not_round():
    """+-1 .. +-3 operands round nothing at these K: the wide range is what exercises the cast."""
    p = X.problem(257, 136, 64, seed=40, hi=3)
    assert X.rounding_share(p.ref.f64)[0] < X.MIN_INEXACT


# ----------------------------------------------------------------------------------------------- the mutants
def _tile(M, N, bm=256, bn=256):
    """Row / column slices of the last output tile."""
    return slice((M - 1) // bm * bm, M), slice((N - 1) // bn * bn, N)


def _mutants():
    """(name, mutated output, correct output) on a representative subset of the GPU cases."""
    for (M, N, K) in [(257, 136, 192), (264, 264, 64), (8, 120, 64)]:
        p = X.problem(M, N, K)
        a, b, ref = p.a, p.b, p.ref
        tag = f"{M}x{N}x{K}"
        yield f"truncating cast {tag}", X.cast_trunc(ref.f64), ref.bf16
        yield f"round half away {tag}", X.cast_half_away(ref.f64), ref.bf16
        for dt in (BF16, F32):
            m = ref.f64.clone()
            m[M - 1] -= a[M - 1, K - 1] * b[K - 1]
            yield f"last k dropped in the last row {tag} {dt}", m.to(dt), ref.f64.to(dt)
            m = ref.f64.clone()
            m[:, N - 8:] -= a[:, K - 8:] @ b[K - 8:, N - 8:]
            yield f"last 16-byte k chunk dropped for the last 8 columns {tag} {dt}", m.to(dt), ref.f64.to(dt)
            rs, cs = _tile(M, N)
            for name, ks in (("first", slice(0, 64)), ("last", slice(K - 64, K))):
                m = ref.f64.clone()
                m[rs, cs] -= a[rs, ks] @ b[ks, cs]
                yield f"{name} K tile dropped for one output tile {tag} {dt}", m.to(dt), ref.f64.to(dt)
            m = ref.f64.clone()
            m[[M - 2, M - 1]] = m[[M - 1, M - 2]]
            yield f"two adjacent rows swapped in the last M tile {tag} {dt}", m.to(dt), ref.f64.to(dt)
    M, N, K = 257, 136, 192
    pb = X.problem(M, N, K, seed=3, bias=True)
    _, cs = _tile(M, N, bn=128)
    m = pb.ref.f64.clone()
    shifted = torch.roll(pb.bias, -4)
    m[:, cs] += (shifted - pb.bias)[None, cs]
    yield "bias shifted by 4 columns in the last N tile", m.to(BF16), pb.ref.bf16
    pa = X.problem(M, N, K, seed=3, alpha=0.5, bias=True)
    yield "bias added before alpha", (0.5 * (pa.a @ pa.b + pa.bias)).to(BF16), pa.ref.bf16
    for base, dt in (("bf16", BF16), ("f32", F32)):
        pc = X.problem(M, N, K, seed=3, base=base)
        rs, cs = _tile(M, N)
        m = pc.ref.f64.clone()
        m[rs, cs] -= pc.base[rs, cs]
        yield f"base ignored by accumulate in the last tile ({base})", m.to(dt), pc.ref.f64.to(dt)
    pc = X.problem(M, N, K, seed=3, base="f32")
    m = pc.a @ pc.b + pc.base.to(BF16).double()
    yield "accumulate base read after rounding to bf16, fp32 output", m.to(F32), pc.ref.f32
    for (M, N, K, s) in X.PP_SPLITK:
        if s > 1:
            p = X.problem(M, N, K, seed=11)
            ks = slice(K - K // s, K)
            part = p.a[:, ks] @ p.b[ks]
            yield f"one split-K slice lost {M}x{N}x{K}", (p.ref.f64 - part).to(BF16), p.ref.bf16
            yield f"one split-K slice counted twice {M}x{N}x{K}", (p.ref.f64 + part).to(F32), p.ref.f32
    lens = (64, 128, 64)
    p = X.kseg_problem(lens)
    # the K tile after the first seam read through segment 0's operands (its last tile again)
    m = p.ref.f64 - p.a[:, 64:128] @ p.b[64:128] + p.a[:, 0:64] @ p.b[0:64]
    yield "K-segment seam off by one K tile", m.to(BF16), p.ref.bf16
    widths = (128, 256, 136)
    p = X.nseg_problem(widths, 257)
    m = p.ref.f64.clone()
    m[:, 120:128] = p.a @ p.b[:, 128:136]      # the seam 8 columns early: segment 1's first columns
    yield "N-segment seam off by 8 columns", m.to(BF16), p.ref.bf16
    g = X.grouped_problem(X.GROUPED_COUNTS, 128, 192, X.GROUPED_TAIL)
    for e in range(g.E - 1):
        t = g.offs[e + 1]
        if g.offs[e + 1] == g.offs[e] or g.offs[e + 2] == t:
            continue
        m = g.y.clone()
        m[t] = g.x[t] @ g.w[e] + g.bias[e]
        yield f"grouped row at the seam of experts {e} / {e + 1} times the neighbour's weight", m.to(BF16), g.y.to(BF16)
        m = g.dw.clone()
        m[e] += torch.outer(g.x[t], g.dy[t])
        yield f"token of expert {e + 1} in the weight gradient of expert {e}", m.to(BF16), g.dw.to(BF16)


_NEED = ["truncating cast", "round half away", "last k dropped in the last row",
         "last 16-byte k chunk dropped for the last 8 columns", "first K tile dropped", "last K tile dropped",
         "two adjacent rows swapped", "bias shifted by 4 columns", "bias added before alpha",
         "base ignored by accumulate", "accumulate base read after rounding", "one split-K slice lost",
         "one split-K slice counted twice", "K-segment seam off by one", "N-segment seam off by 8",
         "times the neighbour's weight", "in the weight gradient of expert"]


def test_every_mutant_is_caught_by_the_bit_check():
    names = []
    for name, got, want in _mutants():
        names.append(name)
        _caught(got, want, name)
    for need in _NEED:
        assert any(need in n for n in names), need


def test_dgelu_partial_mutants_are_caught():
    for M in X.DGELU_MS:
        p, pre, dh = X.dgelu_problem(M)
        s, _ = X.colsum_parts_ref(dh, M)
        X.check_colsum_parts(s.to(F32), dh, M, "correct partials")
        X.check_colsum_parts(torch.stack([X.dgelu_model(p.ref.f64, pre)[t * 256:(t + 1) * 256].double().sum(0)
                                          for t in range(s.shape[0])]).to(F32), dh, M, "sums of the stored bf16")
        m = s.clone()
        m[-1] += dh[M - 1]        # a clamped row >= M of the ragged last tile counted
        with pytest.raises(AssertionError):
            X.check_colsum_parts(m.to(F32), dh, M, "row of the ragged tile included")
        if M > 256:
            m = s.clone()
            r = (M - 1) // 256 * 256 - 1    # the last row of the tile before the ragged one
            m[-2] -= dh[r]
            m[-1] += dh[r]
            with pytest.raises(AssertionError):
                X.check_colsum_parts(m.to(F32), dh, M, "row attributed to the neighbouring tile")
            # folded, the misplaced row is invisible: the older test's criterion cannot see it
            assert float((m.sum(0) - s.sum(0)).abs().max()) < 1e-9


# ----------------------------------------------------------------------- what the older criteria let through
def _old_rel(out, ref):
    return float((out.float() - ref.float()).abs().max() / ref.float().abs().max())


def _old_close(out, ref):
    try:
        torch.testing.assert_close(out.float(), ref.float(), atol=0.15, rtol=1e-2)
        return True
    except AssertionError:
        return False


OLD_SHAPES = [(512, 512, 256), (264, 392, 128), (1000, 776, 320), (1000, 768, 512), (512, 4096, 256), (264, 136, 4096)]


@pytest.mark.parametrize("M,N,K", OLD_SHAPES)
def test_cast_mutants_pass_the_older_criteria(M, N, K, capsys):
    """randn operands as in the older tests: a biased cast passes both older criteria at every shape (and the
    exact check catches it, above). The dropped element is recorded, not asserted."""
    g = torch.Generator().manual_seed(K)
    a = torch.randn(M, K, generator=g).to(BF16).double()
    b = torch.randn(K, N, generator=g).to(BF16).double()
    ref = (a @ b)
    for name, cast in (("truncating", X.cast_trunc), ("half away", X.cast_half_away)):
        out = cast(ref)
        rel = _old_rel(out, ref)
        assert rel < 1e-2 and _old_close(out, ref), f"{name}: rel {rel}"
    m = ref.clone()
    m[M - 1] -= a[M - 1, K - 1] * b[K - 1]
    out = m.to(BF16)
    with capsys.disabled():
        print(f"\n  {M}x{N}x{K}: truncating cast rel {_old_rel(X.cast_trunc(ref), ref):.4f}; dropped k element rel "
              f"{_old_rel(out, ref):.4f} ({'passes' if _old_rel(out, ref) < 1e-2 else 'fails'} rel < 1e-2, "
              f"{'passes' if _old_close(out, ref) else 'fails'} atol 0.15 + rtol 1e-2)")


# ---------------------------------------------------------------------------------------- inexact epilogues
def test_gelu_constants_match_the_rounding_model():
    fwd, bwd = X.measure_gelu()
    assert fwd <= X.GELU_MEASURED <= 2 * fwd and bwd <= X.DGELU_MEASURED <= 2 * bwd, (fwd, bwd)
    assert X.GELU_ATOL == 4 * X.GELU_MEASURED and X.DGELU_ATOL == 4 * X.DGELU_MEASURED
    for shape in X.GELU_SHAPES:
        p, ref = X.gelu_problem(*shape)
        assert float(p.ref.f64.abs().max()) < 9.0           # the pre-activations lie within about +-8
        X.check_close(X.gelu_model(p.ref.f64), ref, X.GELU_ATOL, "model")
        # one dropped k element in the last row is far outside the tolerance
        pre = p.ref.f64.clone()
        pre[-1] -= p.alpha * p.a[-1, -1] * p.b[-1]
        with pytest.raises(AssertionError):
            X.check_close(X.gelu_model(pre), ref, X.GELU_ATOL, "dropped element")
    for M in X.DGELU_MS:
        p, pre, ref = X.dgelu_problem(M)
        assert float(p.ref.f64.abs().max()) <= 256
        X.check_close(X.dgelu_model(p.ref.f64, pre), ref, X.DGELU_ATOL, "model")
        acc = p.ref.f64.clone()
        acc[-1] -= p.a[-1, -1] * p.b[-1]
        with pytest.raises(AssertionError):
            X.check_close(X.dgelu_model(acc, pre), ref, X.DGELU_ATOL, "dropped element")


# ------------------------------------------------------------------------------------- statistics mappings
def test_stats_chunk_maps_cover_every_row_once():
    for bn in (128, 160, 256):
        for M in (8, 257, 520):
            rows = X.stats_rows_tile(M, bn)
            assert sorted(r for c in rows for r in c) == list(range(M))
            assert len(rows) == -(-M // 256) * (4 if bn == 160 else 2)
    rows = X.stats_rows_skinny(X.SKINNY_M, 36)
    assert sorted(r for c in rows for r in c) == list(range(X.SKINNY_M))
    rows = X.stats_rows_skinny(X.SKINNY_M, 8)       # fewer waves than blocks: a wave walks several blocks
    assert sorted(r for c in rows for r in c) == list(range(X.SKINNY_M)) and rows[0][32] == 8 * 32
    p = X.stats_problem(257, 136)
    st = X.stats_ref(p.ref.f64, X.stats_rows_tile(257, 160))
    assert torch.equal(st[0].sum(0), p.ref.f64.sum(0))
    # a row counted in the neighbouring chunk changes two chunks and no total
    m = st.clone()
    m[0, 0] -= p.ref.f64[63]
    m[0, 1] += p.ref.f64[63]
    _caught(m[0].to(F32), st[0].to(F32), "row in the neighbouring chunk")
    assert torch.equal(m[0].sum(0), st[0].sum(0))
