"""Bit-exact tests of the bf16 GEMM family on small-integer operands (tests/gemm_exact.py): every output element of
every kernel must equal the exact product (fp32) or its round-to-nearest-even cast (bf16); NaN-poisoned operand
padding must not reach a result and the sentinel-filled output padding must stay untouched. The inputs are shown
to catch the listed mutants by tests/test_gemm_exact_cpu.py; profiles/gemm_exact_tests.md has the case list."""
import pytest
import torch

import gemm_exact as X
from paddlepaddle_amd.ops import _loader as L
from paddlepaddle_amd.ops import gemm as G
from paddlepaddle_amd.ops import moe as MOE

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = X.BF16, X.F32


@pytest.fixture(autouse=True)
def _hip_backend():
    from paddlepaddle_amd.framework.flags import get_flags, set_flags
    old = get_flags(["FLAGS_gemm_backend"])["FLAGS_gemm_backend"]
    set_flags({"FLAGS_gemm_backend": "hip"})
    try:
        yield
    finally:
        set_flags({"FLAGS_gemm_backend": old})


class Checks:
    """Runs every sub-case of a test and reports all that failed (a mismatch is a finding: see them all)."""

    def __init__(self):
        self.failed, self.ran = [], 0

    def __call__(self, what, fn, *args):
        self.ran += 1
        try:
            fn(*args)
        except AssertionError as e:
            self.failed.append(f"[{what}] {e}")

    def done(self):
        assert self.ran > 0
        assert not self.failed, f"{len(self.failed)} of {self.ran} sub-cases failed:\n" + "\n".join(self.failed[:12])


def _ab(p, ak, bk, padded):
    """A [M, K] and B [K, N] of problem p in the given layouts; padded: leading dimension + 8, two guard rows, NaN."""
    pad, guard = (8, 2) if padded else (0, 0)
    return (X.place(p.a, BF16, DEV, pad, guard, transposed=not ak),
            X.place(p.b, BF16, DEV, pad, guard, transposed=bk))


def _out(M, N, dt, padded, base=None, pad=4):
    o = X.place((M, N), dt, DEV, pad if padded else 0, 2 if padded else 0, poison=False)
    if base is not None:
        o.view.copy_(base.to(device=DEV, dtype=dt))
    return o


def _vec(v, padded):
    return None if v is None else X.place(v, BF16, DEV, 8 if padded else 0).view


def _want(ref, dt):
    return ref.bf16 if dt == BF16 else ref.f32


def _supported_m(M, ak):
    return M if ak else X.mn_major_m(M)


# ------------------------------------------------------------------------------------ a. the tile kernels
@pytest.mark.parametrize("ak,bk", X.LAYOUTS)
@pytest.mark.parametrize("bn", X.TILE_BNS)
def test_tile_kernels_every_layout(bn, ak, bk):
    """1 .. 5 K tiles at a ragged (M, N), every (M, N) edge at 1 and 3 K tiles; bf16 and fp32 output; contiguous and
    padded lda / ldb / ldc."""
    ck = Checks()
    n = 0
    for i, (M, N, K) in enumerate(X.TILE_SHAPES):
        p = X.problem(_supported_m(M, ak), N, K)
        for dt in (BF16, F32):
            for padded in ((False, True) if i < len(X.K_SWEEP) else (bool((i + (dt == F32)) % 2),)):
                def run(p=p, dt=dt, padded=padded):
                    A, B = _ab(p, ak, bk, padded)
                    assert G.supported(A.view, B.view)
                    o = _out(p.M, p.N, dt, padded)
                    G.gemm(A.view, B.view, out=o.view, bn=bn)
                    X.assert_bits_equal(o.view, _want(p.ref, dt), "C")
                    o.guards_intact("C")
                ck(f"{p.M}x{N}x{K} {dt} padded={padded}", run)
                n += 1
    assert L.calls(X.LAUNCHER[bn]) == n
    ck.done()


@pytest.mark.parametrize("bn", X.TILE_BNS)
def test_tile_kernel_epilogues(bn):
    """bias, alpha, accumulate into bf16 / fp32 (with alpha), bias + aux; layouts and padding rotate over the cases."""
    ck = Checks()
    n = 0
    for (M, N, K) in X.EPI_SHAPES:
        for i, (name, kw, dt) in enumerate(X.EPILOGUES):
            ak, bk = X.LAYOUTS[(i + (M == 264)) % 4]
            if not ak and M % 8:
                ak = True
            padded = bool((i + M) % 2)
            p = X.problem(M, N, K, seed=3, **kw)

            def run(p=p, name=name, dt=dt, ak=ak, bk=bk, padded=padded):
                A, B = _ab(p, ak, bk, padded)
                o = _out(p.M, p.N, dt, padded, base=p.base)
                aux = _out(p.M, p.N, BF16, padded) if name == "bias_aux" else None
                G.gemm(A.view, B.view, bias=_vec(p.bias, padded), out=o.view, accumulate=p.base is not None,
                       alpha=p.alpha, aux=None if aux is None else aux.view, bn=bn)
                X.assert_bits_equal(o.view, _want(p.ref, dt), "C")
                o.guards_intact("C")
                if aux is not None:
                    X.assert_bits_equal(aux.view, p.ref.bf16, "aux")
                    aux.guards_intact("aux")
            ck(f"{name} {M}x{N}x{K} ak={ak} bk={bk} padded={padded}", run)
            n += 1
    assert L.calls(X.LAUNCHER[bn]) == n
    ck.done()


@pytest.mark.parametrize("bn", X.TILE_BNS)
def test_tile_kernel_gelu(bn):
    """gelu=True: aux is the exact pre-activation (bit-checked); the GELU output is within one bf16 ulp + GELU_ATOL
    of the fp64 tanh-GELU of the exact pre-activation."""
    ck = Checks()
    for i, shape in enumerate(X.GELU_SHAPES):
        p, ref = X.gelu_problem(*shape)
        padded = bool(i)

        def run(p=p, ref=ref, padded=padded):
            A, B = _ab(p, True, bool(padded), padded)
            o, aux = _out(p.M, p.N, BF16, padded), _out(p.M, p.N, BF16, padded)
            G.gemm(A.view, B.view, bias=_vec(p.bias, padded), gelu=True, aux=aux.view, out=o.view, alpha=p.alpha,
                   bn=bn)
            X.assert_bits_equal(aux.view, p.ref.bf16, "aux")
            X.check_close(o.view, ref, X.GELU_ATOL, "gelu")
            o.guards_intact("C")
            aux.guards_intact("aux")
        ck(f"{shape}", run)
    assert L.calls(X.LAUNCHER[bn]) == len(X.GELU_SHAPES)
    ck.done()


# ---------------------------------------------------------------------------------------- b. balanced tail
@pytest.mark.parametrize("bn", [1, 2])
def test_balanced_tail(bn):
    """cus + 16 tiles of 256 x 256: 16 tail tiles cut in two along K and summed by the tail reduction; bias + aux,
    then fp32 accumulate. The only large shape of the file."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, N, K = X.tail_shape(cus)
    assert L.lib().pa_gemm_pp_ws_bytes(M, N, K) > 0
    p = X.problem(M, N, K, seed=4, bias=True)
    A, B = _ab(p, True, False, True)
    o, aux = _out(M, N, BF16, True), _out(M, N, BF16, True)
    G.gemm(A.view, B.view, bias=_vec(p.bias, True), aux=aux.view, out=o.view, bn=bn)
    ck = Checks()
    ck("C", X.assert_bits_equal, o.view, p.ref.bf16, "C")
    ck("aux", X.assert_bits_equal, aux.view, p.ref.bf16, "aux")
    ck("C guards", o.guards_intact, "C")
    ck("aux guards", aux.guards_intact, "aux")
    p = X.problem(M, N, K, seed=4, base="f32")
    A, B = _ab(p, True, True, False)
    o = _out(M, N, F32, True, base=p.base)
    G.gemm(A.view, B.view, out=o.view, accumulate=True, bn=bn)
    ck("accumulate", X.assert_bits_equal, o.view, p.ref.f32, "fp32 accumulate")
    ck("accumulate guards", o.guards_intact, "fp32 accumulate")
    assert L.calls(X.LAUNCHER[bn]) == 2
    ck.done()


# --------------------------------------------------------------------------------- c. ping-pong split-K
def test_pp_splitk():
    ck = Checks()
    n = 0
    for i, (M, N, K, splits) in enumerate(X.PP_SPLITK):
        for base, dt in ((None, BF16), (None, F32), ("f32", F32), ("bf16", BF16)):
            ak = not (M % 8 == 0 and i % 2 == 1)      # MN-major A on the shapes that allow it
            p = X.problem(M, N, K, seed=11, base=base)

            def run(p=p, dt=dt, ak=ak, splits=splits, padded=bool(i % 2)):
                A, B = _ab(p, ak, not ak, padded)
                assert G.gemm_pp_splitk_ok(A.view, B.view, splits)
                o = _out(p.M, p.N, dt, padded, base=p.base)
                G.gemm_pp_splitk(A.view, B.view, splits, out=o.view, accumulate=p.base is not None)
                X.assert_bits_equal(o.view, _want(p.ref, dt), "C")
                o.guards_intact("C")
            ck(f"{M}x{N}x{K} / {splits} base={base} {dt} ak={ak}", run)
            n += 1
    assert L.calls("pa_gemm_bf16_pp_splitk") == n
    ck.done()


# ------------------------------------------------------------------------ d. split-K slabs + slab reduction
@pytest.mark.parametrize("bn,splits", X.SPLITK)
def test_splitk_slabs(bn, splits):
    p = X.problem(257, 136, 64 * splits, seed=12)
    ck = Checks()
    for padded, (ak, bk) in ((False, (True, False)), (True, (True, True))):
        A, B = _ab(p, ak, bk, padded)
        ck(f"bf16 padded={padded}", X.assert_bits_equal, G.gemm_splitk(A.view, B.view, splits, BF16, bn=bn),
           p.ref.bf16, "C")
        ck(f"fp32 padded={padded}", X.assert_bits_equal, G.gemm_splitk(A.view, B.view, splits, F32, bn=bn), p.ref.f32,
           "C")
    assert L.calls("pa_gemm_bf16") == 4 and L.calls("pa_slab_reduce_bf16") == 2
    ck.done()


# ------------------------------------------------------------------------------------- e. K segments
@pytest.mark.parametrize("lens", X.KSEG, ids=str)
def test_kseg(lens):
    """Every segment its own allocation and leading dimension; a seam after one K tile; with and without accumulate."""
    ck = Checks()
    for ak, bk in X.LAYOUTS:
        for acc in (False, True):
            p = X.kseg_problem(tuple(lens), M=257 if ak else 264, base="bf16" if acc else None,
                               alpha=0.5 if acc else 1.0)

            def run(p=p, ak=ak, bk=bk, acc=acc):
                As, Bs, k0 = [], [], 0
                for i, kl in enumerate(lens):
                    As.append(X.place(p.a[:, k0:k0 + kl], BF16, DEV, 8 * (i + 1), 2, transposed=not ak).view)
                    Bs.append(X.place(p.b[k0:k0 + kl], BF16, DEV, 8 * (len(lens) - i), 2, transposed=bk).view)
                    k0 += kl
                assert G.gemm_kseg_supported(As, Bs)
                o = _out(p.M, p.N, BF16, True, base=p.base)
                G.gemm_kseg(As, Bs, out=o.view, accumulate=acc, alpha=p.alpha)
                X.assert_bits_equal(o.view, p.ref.bf16, "C")
                o.guards_intact("C")
            ck(f"ak={ak} bk={bk} accumulate={acc}", run)
    assert L.calls("pa_gemm_bf16_pp_segs") == 8
    ck.done()


# ------------------------------------------------------------------------------------- f. N segments
@pytest.mark.parametrize("M", [8, 257])
@pytest.mark.parametrize("widths", X.NSEG, ids=str)
def test_nseg(widths, M):
    ck = Checks()
    p = X.nseg_problem(tuple(widths), M)
    for bk in (False, True):
        for dt in (BF16, F32):
            def run(bk=bk, dt=dt):
                A = X.place(p.a, BF16, DEV, 8, 2)
                Bs, n0 = [], 0
                for i, w in enumerate(widths):
                    Bs.append(X.place(p.b[:, n0:n0 + w], BF16, DEV, 8 * (i + 1), 2, transposed=bk).view)
                    n0 += w
                assert G.gemm_nseg_supported(A.view, Bs)
                o = _out(p.M, p.N, dt, True)
                G.gemm_nseg(A.view, Bs, out=o.view)
                X.assert_bits_equal(o.view, _want(p.ref, dt), "C")
                o.guards_intact("C")
            ck(f"bk={bk} {dt}", run)
    assert L.calls("pa_gemm_bf16_pp_segs") == 4
    ck.done()


# ---------------------------------------------------------------------------------------- g. residual
@pytest.mark.parametrize("bias", [False, True])
def test_gemm_res(bias):
    """The residual lives in a larger allocation: the rows after row M - 1 hold NaN."""
    ck = Checks()
    for (M, N, K) in X.EPI_SHAPES:
        p = X.problem(M, N, K, seed=13, bias=bias, res=True)
        for ak, bk in X.LAYOUTS:
            if not ak and M % 8:
                continue

            def run(p=p, ak=ak, bk=bk):
                A, B = _ab(p, ak, bk, True)
                res = X.place(p.res, BF16, DEV, 0, 2)      # contiguous rows (res_supported), guard rows poisoned
                assert G.res_supported(A.view, B.view, res.view)
                X.assert_bits_equal(G.gemm_res(A.view, B.view, res.view, bias=_vec(p.bias, True)), p.ref.bf16, "C")
            ck(f"{M}x{N}x{K} ak={ak} bk={bk}", run)
    assert L.calls("pa_gemm_bf16_res") == ck.ran
    ck.done()


# --------------------------------------------------------------------------- h. batch-norm partials
def _check_stats(stats, chunks, c64, rows_of_chunk, what):
    want = X.stats_ref(c64, rows_of_chunk)
    assert chunks == len(rows_of_chunk), f"{what}: {chunks} chunks, expected {len(rows_of_chunk)}"
    X.assert_bits_equal(stats.view(2, chunks, c64.shape[1]), want.to(F32), what)


@pytest.mark.parametrize("bn,M,N", X.STATS_TILE)
def test_gemm_bn_stats(bn, M, N):
    """Every chunk of stats[2][chunks][N] against the rows it owns; rows >= M contribute nothing."""
    ck = Checks()
    for bias in (False, True):
        p = X.stats_problem(M, N, bias=bias)
        assert float(p.ref.f64.abs().max()) <= 256
        for ak, bk in ((True, True), (True, False)):
            def run(p=p, ak=ak, bk=bk):
                A, B = _ab(p, ak, bk, True)
                c, stats, chunks = G.gemm_bn_stats(A.view, B.view, bias=_vec(p.bias, True), bn=bn)
                X.assert_bits_equal(c, p.ref.bf16, "C")
                _check_stats(stats, chunks, p.ref.f64, X.stats_rows_tile(M, bn), "stats")
            ck(f"bias={bias} bk={bk}", run)
    assert L.calls("pa_gemm_bf16_stats") == 4
    ck.done()


@pytest.mark.parametrize("N,K", X.STATS_SKINNY)
def test_gemm_skinny_bn_stats(N, K):
    ck = Checks()
    for bias in (False, True):
        p = X.skinny_stats_problem(N, K, bias)
        assert float(p.ref.f64.abs().max()) <= 256
        for bk in (False, True):
            def run(p=p, bk=bk):
                A, B = _ab(p, True, bk, True)
                c, stats, chunks = G.gemm_skinny_bn_stats(A.view, B.view, bias=_vec(p.bias, True))
                X.assert_bits_equal(c, p.ref.bf16, "C")
                _check_stats(stats, chunks, p.ref.f64, X.stats_rows_skinny(X.SKINNY_M, chunks), "stats")
            ck(f"bias={bias} bk={bk}", run)
    assert L.calls("pa_gemm_skinny_stats") == 4
    ck.done()


# ------------------------------------------------------------------------------------------ i. small M
@pytest.mark.parametrize("stages", [4, 3])
@pytest.mark.parametrize("M,N", X.SMALL_M)
def test_gemm_small_m(M, N, stages):
    """1, 2, 3 and 5 K tiles per slice on both LDS ring depths, with and without bias."""
    ck = Checks()
    for K, splits in X.SMALL_M_SPLITS:
        for bias in (False, True):
            p = X.small_m_problem(M, N, K, bias)

            def run(p=p, splits=splits):
                A, B = _ab(p, True, False, True)
                assert G.small_m_supported(A.view, B.view)
                c = G.gemm_small_m(A.view, B.view, _vec(p.bias, True), splits=splits, stages=stages)
                X.assert_bits_equal(c, p.ref.bf16, "C")
            ck(f"K={K} splits={splits} bias={bias}", run)
    assert L.calls("pa_gemm_small_m") == 2 * len(X.SMALL_M_SPLITS)
    ck.done()


# ------------------------------------------------------------------------------------------- j. skinny
@pytest.mark.parametrize("epi", ["none", "bias_relu", "accum"])
@pytest.mark.parametrize("bk", [True, False])
def test_gemm_skinny(bk, epi):
    """M = 1024 + 8 (ragged last 16-row block), every (N, K) in {32, 64, 128, 256}^2, padded lda / ldb / ldc."""
    ck = Checks()
    for N in X.SKINNY_NK:
        for K in X.SKINNY_NK:
            p = X.skinny_problem(N, K, epi)

            def run(p=p):
                A, B = _ab(p, True, bk, True)
                assert G.skinny_supported(A.view, B.view)
                o = _out(p.M, p.N, BF16, True, base=p.base, pad=8)
                G.gemm_skinny(A.view, B.view, bias=_vec(p.bias, True), out=o.view, accumulate=epi == "accum",
                              relu=epi == "bias_relu")
                X.assert_bits_equal(o.view, X.skinny_ref(p, epi).to(BF16), "C")
                o.guards_intact("C")
            ck(f"N={N} K={K}", run)
    assert L.calls("pa_gemm_skinny") == 16
    ck.done()


# ------------------------------------------------------------------------------------------ k. grouped
def _grouped(g, ck):
    x = g.x.to(device=DEV, dtype=BF16).requires_grad_()
    w = g.w.to(device=DEV, dtype=BF16).requires_grad_()
    b = g.bias.to(device=DEV, dtype=BF16).requires_grad_()
    offs = torch.tensor(g.offs, dtype=torch.int32, device=DEV)
    y = MOE.grouped_linear(x, w, offs, b)
    assert L.calls("pa_grouped_gemm") == 1
    ck("y", X.assert_bits_equal, y.detach(), g.y.to(BF16), "y (rows past offs[E] are zero)")
    y.backward(g.dy.to(device=DEV, dtype=BF16))
    assert L.calls("pa_grouped_gemm") == 3
    ck("dx", X.assert_bits_equal, x.grad, g.dx.to(BF16), "dx")
    live = [e for e in range(g.E) if g.offs[e + 1] > g.offs[e]]
    ck("dw", X.assert_bits_equal, w.grad[live], g.dw[live].to(BF16), f"dw of experts {live}")
    empty = [e for e in range(g.E) if e not in live]
    if empty:
        ck("dw of empty experts", X.assert_bits_equal, w.grad[empty], g.dw[empty].to(BF16), f"dw of experts {empty}")


def test_grouped_linear_expert_seams():
    """Experts of 0, 1, 7, 63 .. 65, 127 .. 129 and 300 rows: 128-row tiles and 64-token K tiles span expert seams;
    every expert has its own weights and bias, so a neighbour's weights give a different answer."""
    ck = Checks()
    _grouped(X.grouped_problem(X.GROUPED_COUNTS, 128, 192, X.GROUPED_TAIL), ck)
    ck.done()


def test_grouped_linear_big_tiles():
    """Average >= 1024 rows per expert and N >= 1024: the 256 x 256 variant, uneven counts."""
    ck = Checks()
    _grouped(X.grouped_problem(X.GROUPED_BIG, 64, 1024, 0, seed=1), ck)
    ck.done()


# ---------------------------------------------------------------------------------- GELU backward (dgelu)
@pytest.mark.parametrize("M", X.DGELU_MS)
@pytest.mark.parametrize("kern", [1, 2])
def test_gemm_dgelu(kern, M):
    """dh = (a @ b) * gelu'(pre) within one bf16 ulp + DGELU_ATOL of the fp64 value; every 256-row tile's column
    sums against its own rows (the ragged last tile leaves out rows >= M)."""
    p, pre, ref = X.dgelu_problem(M)
    ck = Checks()
    for ak, bk in ((True, False), (True, True), (False, False)):
        if not ak and M % 8:
            continue
        A, B = _ab(p, ak, bk, True)
        pr = X.place(pre, BF16, DEV, 0, 2)
        assert G.gemm_dgelu_supported(A.view, B.view, pr.view)
        dh, parts = G.gemm_dgelu(A.view, B.view, pr.view, kern=kern)
        ck(f"dh ak={ak} bk={bk}", X.check_close, dh, ref, X.DGELU_ATOL, "dh")
        ck(f"parts ak={ak} bk={bk}", X.check_colsum_parts, parts, ref, M, "column sums")
    assert L.calls("pa_gemm_bf16_dgelu") == ck.ran // 2
    ck.done()
