"""Exact small-integer inputs, references and bit-wise checks for the bf16 GEMM family (csrc/kernels/gemm.hip,
gemm_skinny.hip, grouped_gemm.hip). Plain helper module, imported by the tests like ``attn_needles``.

Why integers: operands whose entries are non-zero integers in +-1 .. +-15 are exact in bf16, every product and
every partial sum is an integer below 2^24, so fp32 accumulation is exact in any order (split-K slabs and tail
reductions included). A correct kernel then returns the exact product bit for bit in fp32, and its
round-to-nearest-even cast in bf16: one wrong element anywhere fails, and no tolerance has to be chosen.

* ``ints`` / ``place`` build operands in any layout, optionally as a view inside a larger buffer whose padding
  columns and guard rows hold NaN (inputs) or a sentinel bit pattern (outputs). All guards live inside the same
  allocation as the data.
* ``exact_ref`` is the epilogue value in fp64 with the exactness bound asserted per case.
* ``assert_bits_equal`` compares raw bit patterns and reports where the mismatches sit.
* ``rounding_share`` / ``assert_rounding_checked`` make sure a bf16 case really exercises the cast.
* ``gelu_*`` hold the rounding model and the measured constants of the two inexact epilogues.
* The case tables and ``all_cases`` list the GPU cases; tests/test_gemm_exact_cpu.py checks the bound and the
  rounding share of every one of them without a device.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import torch

BF16, F32 = torch.bfloat16, torch.float32
TWO24 = float(1 << 24)
# sentinels of output padding / guard rows: NaN bit patterns, so a sentinel that leaks into a result also fails
SENT_BF16 = 0x7FA5
SENT_F32 = 0x7FA55AA5


# ------------------------------------------------------------------------------------------------ operands
def ints(shape, lo=1, hi=15, seed=0):
    """Non-zero integers in +-lo .. +-hi, fp64 on the CPU (every value exact in bf16 for hi <= 256)."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.randint(lo, hi + 1, tuple(shape), generator=g)
    sign = torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1
    return (mag * sign).double()


def _fill(shape, dtype, device, poison):
    """A buffer of NaN (``poison``: an input) or of the sentinel bit pattern (an output)."""
    if poison:
        return torch.full(shape, float("nan"), dtype=dtype, device=device)
    if dtype == BF16:
        return torch.full(shape, SENT_BF16, dtype=torch.int16, device=device).view(BF16)
    return torch.full(shape, SENT_F32, dtype=torch.int32, device=device).view(F32)


class Placed:
    """``view``: the [R, C] tensor handed to the kernel; ``buf``: the allocation it lives in; ``mask``: True where
    ``buf`` holds data."""

    def __init__(self, view, buf, mask, poison):
        self.view, self.buf, self.mask, self.poison = view, buf, mask, poison

    def guards_intact(self, what):
        """Every padding / guard element of an output still holds the sentinel bits."""
        it = torch.int16 if self.buf.dtype == BF16 else torch.int32
        sent = SENT_BF16 if self.buf.dtype == BF16 else SENT_F32
        bad = (self.buf.view(it) != sent) & ~self.mask
        if bool(bad.any()):
            idx = bad.nonzero()[:6].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} guard elements overwritten, first (buffer row, col) {idx}")


def place(vals, dtype, device, pad=0, guard=0, transposed=False, poison=True):
    """``vals`` [R, C] as a tensor of ``dtype`` on ``device``. ``transposed``: stored [C][R] and viewed back (the
    MN-major layout of an A operand, the K-major layout of a B operand). ``pad`` extra elements per stored row and
    ``guard`` extra stored rows hold NaN (``poison``) or the sentinel. ``vals`` may be a shape instead of a tensor:
    an output of that shape whose data region, too, starts out as the sentinel."""
    shape = tuple(vals.shape) if torch.is_tensor(vals) else tuple(vals)
    if len(shape) == 1:
        buf = _fill((shape[0] + pad,), dtype, device, poison)
        mask = torch.zeros(buf.shape, dtype=torch.bool, device=device)
        mask[:shape[0]] = True
        view = buf[:shape[0]]
    else:
        R, C = (shape[1], shape[0]) if transposed else shape
        buf = _fill((R + guard, C + pad), dtype, device, poison)
        mask = torch.zeros(buf.shape, dtype=torch.bool, device=device)
        mask[:R, :C] = True
        view = buf[:R, :C]
    if torch.is_tensor(vals):
        src = vals.t() if (transposed and vals.dim() == 2) else vals
        view.copy_(src.to(device=device, dtype=dtype))
    if transposed and len(shape) == 2:
        view = view.t()
    return Placed(view, buf, mask, poison)


# ------------------------------------------------------------------------------------------------ reference
def _is_bf16(x):
    return bool((x.to(BF16).double() == x).all())


def exact_ref(a, b, alpha=1.0, bias=None, res=None, base=None):
    """fp64 epilogue value alpha * a @ b (+ bias) (+ res) (+ base) of fp64 integer operands, with the exactness
    condition asserted: every term is a multiple of a power-of-two unit u and the sum of magnitudes is below
    2^24 u, so every fp32 partial sum, in any order, is exact. Returns (f64, f32, bf16)."""
    m = math.frexp(abs(alpha))[0]
    assert m == 0.5, f"alpha {alpha} is not a power of two"
    assert _is_bf16(a) and _is_bf16(b) and bool((a == a.round()).all()) and bool((b == b.round()).all())
    unit = min(1.0, abs(alpha))
    val = alpha * (a @ b)
    mag = abs(alpha) * (a.abs() @ b.abs())
    assert float((a.abs() @ b.abs()).max()) < TWO24, "accumulator bound"
    if bias is not None:
        assert _is_bf16(bias) and bool((bias == bias.round()).all())
        val = val + bias[None, :]
        mag = mag + bias.abs()[None, :]
    if res is not None:
        assert _is_bf16(res) and bool((res == res.round()).all())
        val = val + res
        mag = mag + res.abs()
    if base is not None:
        twice = base * 2
        assert bool((twice == twice.round()).all()), "base is integer or half-integer valued"
        if not bool((base == base.round()).all()):
            unit = min(unit, 0.5)
        val = val + base
        mag = mag + base.abs()
    worst = float(mag.max()) / unit
    assert worst < TWO24, f"exactness bound: {worst:.4g} >= 2^24 (unit {unit})"
    f32 = val.to(F32)
    assert bool((f32.double() == val).all())
    return SimpleNamespace(f64=val, f32=f32, bf16=val.to(BF16))


def _canon_bits(t):
    """Raw bit patterns as integers, with -0 mapped to +0."""
    t = t.detach().cpu().contiguous()
    if t.dtype == BF16:
        bits = t.view(torch.int16).to(torch.int32) & 0xFFFF
        return torch.where(bits == 0x8000, torch.zeros_like(bits), bits)
    assert t.dtype == F32, t.dtype
    bits = t.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(bits == 0x80000000, torch.zeros_like(bits), bits)


def assert_bits_equal(got, want, what):
    """Bit-for-bit equality (an exact zero of either sign passes); NaN anywhere fails. The message gives the
    mismatch count, the first few (row, col, got, want) and the bounding box of the mismatches."""
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} != {want.dtype}"
    assert tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    g, w = got.detach().cpu(), want.detach().cpu()
    nan = torch.isnan(g)
    bad = (_canon_bits(g) != _canon_bits(w)) | nan
    if not bool(bad.any()):
        return
    idx = bad.nonzero()
    first = [tuple(i.tolist()) + (float(g[tuple(i)]), float(w[tuple(i)])) for i in idx[:5]]
    lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({int(nan.sum())} NaN); first "
                         f"(index..., got, want) {first}; bounding box {lo} .. {hi}")


# ------------------------------------------------------------------------------------------ rounding share
def rounding_share(f64):
    """(share of elements not representable in bf16, share that are exact ties between two bf16 values)."""
    low = f64.to(F32).contiguous().view(torch.int32) & 0xFFFF
    n = max(low.numel(), 1)
    return float((low != 0).sum()) / n, float((low == 0x8000).sum()) / n


MIN_INEXACT, MIN_TIES = 0.10, 0.01


def assert_rounding_checked(f64, what, need_ties=True):
    """Condition on the inputs of a bf16-output case: the cast is exercised (>= 10 % inexact, >= 1 % ties)."""
    inexact, ties = rounding_share(f64)
    assert inexact >= MIN_INEXACT, f"{what}: only {inexact:.3f} of the reference needs rounding"
    if need_ties:
        assert ties >= MIN_TIES, f"{what}: only {ties:.4f} of the reference are ties"


def cast_trunc(f64):
    """Mutant cast: fp32 -> bf16 by dropping the low 16 bits."""
    bits = f64.to(F32).contiguous().view(torch.int32) & -65536
    return bits.view(F32).to(BF16)


def cast_half_away(f64):
    """Mutant cast: round to nearest, ties away from zero."""
    bits = ((f64.to(F32).contiguous().view(torch.int32).to(torch.int64) + 0x8000) & 0xFFFF0000)
    return bits.to(torch.int32).view(F32).to(BF16)


# -------------------------------------------------------------------------------------------- shared problems
@functools.lru_cache(maxsize=None)
def problem(M, N, K, seed=0, hi=15, alpha=1.0, bias=False, res=False, base=None, bias_hi=127):
    """Operands and exact reference of one case, computed once and shared (callers must not modify it).
    base: None | 'bf16' (integer multiples of 8, |.| <= 1016) | 'f32' (half-integers, not representable in bf16)."""
    s = seed * 7919 + M * 31 + N * 17 + K
    p = SimpleNamespace(M=M, N=N, K=K, alpha=alpha)
    p.a, p.b = ints((M, K), 1, hi, s), ints((K, N), 1, hi, s + 1)
    p.bias = ints((N,), 1, bias_hi, s + 2) if bias else None
    p.res = ints((M, N), 1, 127, s + 3) * 8 if res else None
    p.base = None
    if base == "bf16":
        p.base = ints((M, N), 1, 127, s + 4) * 8
    elif base == "f32":
        p.base = ints((M, N), 1025, 4000, s + 4) + 0.5
    p.ref = exact_ref(p.a, p.b, alpha, p.bias, p.res, p.base)
    return p


# --------------------------------------------------------------------------------------------------- cases
LAYOUTS = [(True, False), (True, True), (False, False), (False, True)]   # (A K-major, B K-major)
TILE_BNS = [1, 2, 4, 128, 160, 256]
LAUNCHER = {1: "pa_gemm_bf16_pp", 2: "pa_gemm_bf16_4w", 4: "pa_gemm_bf16", 128: "pa_gemm_bf16", 160: "pa_gemm_bf16",
            256: "pa_gemm_bf16"}
# every K (1 .. 5 K tiles) at one ragged (M, N); every (M, N) edge at K = 64 and K = 192
K_SWEEP = [(257, 136, K) for K in (64, 128, 192, 256, 320)]
MN_EDGES = [(1, 8), (8, 120), (255, 128), (256, 136), (257, 160), (264, 168), (8, 256), (264, 264)]
TILE_SHAPES = K_SWEEP + [(M, N, K) for (M, N) in MN_EDGES for K in (64, 192)]


def mn_major_m(M):
    """The M used when A is MN-major (``supported`` requires M % 8 == 0): the next multiple of 8."""
    return -(-M // 8) * 8


# epilogues of G.gemm: (name, problem kwargs, out dtype)
EPILOGUES = [
    ("bias", dict(bias=True), BF16),
    ("alpha0.5", dict(alpha=0.5), BF16),
    ("alpha2", dict(alpha=2.0), BF16),
    ("alpha2_f32", dict(alpha=2.0), F32),
    ("acc_bf16", dict(base="bf16"), BF16),
    ("acc_bf16_alpha0.5", dict(base="bf16", alpha=0.5), BF16),
    ("acc_f32", dict(base="f32"), F32),
    ("acc_f32_alpha0.5", dict(base="f32", alpha=0.5), F32),
    ("bias_aux", dict(bias=True), BF16),
]
EPI_SHAPES = [(257, 136, 192), (264, 264, 64)]

# cases with rows of one or a few elements: exempt from the tie share (the file's cases as a whole satisfy it,
# tests/test_gemm_exact_cpu.py::test_tie_share_of_all_cases)
TIE_EXEMPT_IDS = (
    ["tile-1x8x64", "tile-1x8x192", "tile-8x8x64", "tile-8x8x192", "ppsplitk-8x8x192", "ppsplitk-accbf-8x8x192"]
    + [f"small_m-1x8x{K}-{b}" for K in (64, 256, 192, 320, 384) for b in (False, True)])

PP_SPLITK = [(257, 136, 128, 2), (264, 264, 256, 2), (255, 168, 192, 1), (8, 8, 192, 3), (257, 264, 384, 2)]
SPLITK = [(bn, s) for bn in (128, 160, 256) for s in (1, 2, 4)]   # one K tile per slice: K = 64 s
KSEG = [[64, 64], [64, 128, 64], [128, 64, 64, 64]]
NSEG = [[128, 256, 136], [128, 8], [256, 128, 128, 120]]
SMALL_M = [(M, N) for M in (1, 17, 64) for N in (8, 120, 128, 136)]
SMALL_M_SPLITS = [(64, 1), (256, 2), (192, 1), (320, 1), (384, 2)]   # (K, splits): 1, 2, 3, 5, 3 K tiles per slice
SKINNY_NK = [32, 64, 128, 256]
SKINNY_M = 1024 + 8
GROUPED_COUNTS = [63, 1, 65, 0, 127, 129, 7, 64, 128, 300]   # 128-row tiles and 64-token K tiles span the seams
GROUPED_TAIL = 37
GROUPED_BIG = [1500, 700]     # average >= 1024 rows per expert with N >= 1024: the 256 x 256 variant


def tail_shape(cus):
    """The balanced-tail shape: cus + 16 tiles of 256 x 256, ragged in M and N."""
    return 256 * (cus // 16 + 1) - 7, 4096 - 8, 512


def grouped_problem(counts, K, N, tail, seed=0, hi=15):
    """x [T, K], w [E, K, N] and bias [E, N] (every expert from its own seed), dy [T, N] (zero past offs[E]) and the
    exact y / dx / dw of ops.moe.grouped_linear."""
    E = len(counts)
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    T = offs[-1] + tail
    p = SimpleNamespace(E=E, K=K, N=N, T=T, offs=offs)
    p.x = ints((T, K), 1, hi, seed * 101 + 1)
    p.w = torch.stack([ints((K, N), 1, hi, seed * 101 + 1000 + e) for e in range(E)])
    p.bias = torch.stack([ints((N,), 1, 127, seed * 101 + 2000 + e) for e in range(E)])
    p.dy = ints((T, N), 1, hi, seed * 101 + 2)
    p.dy[offs[-1]:] = 0
    p.y = torch.zeros(T, N, dtype=torch.float64)
    p.dx = torch.zeros(T, K, dtype=torch.float64)
    p.dw = torch.zeros(E, K, N, dtype=torch.float64)
    for e in range(E):
        s, t = offs[e], offs[e + 1]
        if t > s:
            p.y[s:t] = exact_ref(p.x[s:t], p.w[e], bias=p.bias[e]).f64
            p.dx[s:t] = exact_ref(p.dy[s:t], p.w[e].t()).f64
            p.dw[e] = exact_ref(p.x[s:t].t(), p.dy[s:t]).f64
    return p


def kseg_problem(lens, M=257, N=136, base=None, alpha=1.0):
    """K-segmented product: one problem over K = sum(lens), cut along K."""
    return problem(M, N, sum(lens), seed=21, base=base, alpha=alpha)


def nseg_problem(widths, M, K=192):
    """N-segmented product: one problem over N = sum(widths), cut along N."""
    return problem(M, sum(widths), K, seed=22)


STATS_TILE = [(bn, M, N) for bn in (128, 160, 256) for (M, N) in ((257, 136), (520, 264))]
STATS_SKINNY = [(32, 64), (128, 64), (64, 128)]   # (N, K); N <= 128 has the statistics variant


def stats_problem(M, N, K=64, bias=False):
    """|C| <= 256, so the fp32 value and the stored bf16 value coincide and the partials are exact integers."""
    if bias:
        return problem(M, N, K, seed=23, hi=1, bias=True, bias_hi=100)
    return problem(M, N, K, seed=23, hi=2)


def skinny_stats_problem(N, K, bias):
    if bias:
        return problem(SKINNY_M, N, K, seed=23, hi=1, bias=True, bias_hi=100)
    return problem(SKINNY_M, N, K, seed=23, hi=2 if K <= 64 else 1)


def small_m_problem(M, N, K, bias):
    return problem(M, N, K, seed=24, bias=bias)


def skinny_problem(N, K, epi):
    return problem(SKINNY_M, N, K, seed=25, bias=epi == "bias_relu", base="bf16" if epi == "accum" else None)


def skinny_ref(p, epi):
    return p.ref.f64.clamp_min(0) if epi == "bias_relu" else p.ref.f64


def all_cases(cus=256):
    """(id, fp64 reference, is the bf16 cast exercised?) of every exact GPU case: building one asserts its exactness
    bound. The cast flag is False for fp32 outputs and for the statistics cases, whose |C| <= 256 is exact in bf16
    by construction."""
    seen = set()
    for (M, N, K) in TILE_SHAPES:
        for m in {M, mn_major_m(M)}:
            if (m, N, K) not in seen:
                seen.add((m, N, K))
                yield f"tile-{m}x{N}x{K}", problem(m, N, K).ref.f64, True
    for (M, N, K) in EPI_SHAPES:
        for name, kw, dt in EPILOGUES:
            yield f"epi-{name}-{M}x{N}x{K}", problem(M, N, K, seed=3, **kw).ref.f64, dt == BF16
    M, N, K = tail_shape(cus)
    yield "tail-bias", problem(M, N, K, seed=4, bias=True).ref.f64, True
    yield "tail-acc", problem(M, N, K, seed=4, base="f32").ref.f64, False
    for (M, N, K, s) in PP_SPLITK:
        yield f"ppsplitk-{M}x{N}x{K}", problem(M, N, K, seed=11).ref.f64, True
        yield f"ppsplitk-acc-{M}x{N}x{K}", problem(M, N, K, seed=11, base="f32").ref.f64, False
        yield f"ppsplitk-accbf-{M}x{N}x{K}", problem(M, N, K, seed=11, base="bf16").ref.f64, True
    for s in (1, 2, 4):
        yield f"splitk-{s}", problem(257, 136, 64 * s, seed=12).ref.f64, True
    for lens in KSEG:
        yield f"kseg-{lens}", kseg_problem(tuple(lens)).ref.f64, True
        yield f"kseg-acc-{lens}", kseg_problem(tuple(lens), base="bf16", alpha=0.5).ref.f64, True
        yield f"kseg-264-{lens}", kseg_problem(tuple(lens), M=264).ref.f64, True
        yield f"kseg-264-acc-{lens}", kseg_problem(tuple(lens), M=264, base="bf16", alpha=0.5).ref.f64, True
    for widths in NSEG:
        for M in (8, 257):
            yield f"nseg-{widths}-{M}", nseg_problem(tuple(widths), M).ref.f64, True
    for bias in (False, True):
        for (M, N, K) in EPI_SHAPES:
            yield f"res-{bias}-{M}x{N}x{K}", problem(M, N, K, seed=13, bias=bias, res=True).ref.f64, True
    for (M, N) in SMALL_M:
        for (K, s) in SMALL_M_SPLITS:
            for bias in (False, True):
                yield f"small_m-{M}x{N}x{K}-{bias}", small_m_problem(M, N, K, bias).ref.f64, True
    for N in SKINNY_NK:
        for K in SKINNY_NK:
            for epi in ("none", "bias_relu", "accum"):
                yield f"skinny-{N}x{K}-{epi}", skinny_ref(skinny_problem(N, K, epi), epi), True
    for (bn, M, N) in STATS_TILE:
        for bias in (False, True):
            yield f"stats-{M}x{N}-{bias}", stats_problem(M, N, bias=bias).ref.f64, False
    for (N, K) in STATS_SKINNY:
        for bias in (False, True):
            yield f"stats-skinny-{N}x{K}-{bias}", skinny_stats_problem(N, K, bias).ref.f64, False
    g = grouped_problem(GROUPED_COUNTS, 128, 192, GROUPED_TAIL)
    live = g.offs[-1]
    yield "grouped-y", g.y[:live], True
    yield "grouped-dx", g.dx[:live], True
    yield "grouped-dw", g.dw[[e for e, c in enumerate(GROUPED_COUNTS) if c]].reshape(-1, g.N), True
    g = grouped_problem(GROUPED_BIG, 64, 1024, 0, seed=1)
    yield "grouped-big-y", g.y, True


# ------------------------------------------------------------------------------- batch-norm partials (stats)
def stats_rows_tile(M, bn):
    """Rows of every chunk of pa_gemm_bf16_stats: chunk = m-tile * waves along M + wave row (csrc/kernels/gemm.hip:
    4 waves of 64 rows in the 256 x 160 kernel, 2 waves of 128 rows in the two-stage kernels)."""
    wm = 4 if bn == 160 else 2
    rows = 256 // wm
    return [range(min(c * rows, M), min((c + 1) * rows, M)) for c in range(-(-M // 256) * wm)]


def stats_rows_skinny(M, chunks, R=2):
    """Rows of every chunk of pa_gemm_skinny_stats: chunk = global wave id (chunks = sk_grid * 4); wave w owns the
    16 R-row blocks w, w + chunks, w + 2 chunks, ... (csrc/kernels/gemm_skinny.hip; R = 2 for N <= 128)."""
    nb = -(-M // (16 * R))
    out = []
    for w in range(chunks):
        rows = []
        for blk in range(w, nb, chunks):
            rows.extend(range(blk * 16 * R, min((blk + 1) * 16 * R, M)))
        out.append(rows)
    return out


def stats_ref(c64, rows_of_chunk):
    """[2][chunks][N] fp64: per-chunk column sums and sums of squares of the stored C over the chunk's rows."""
    N = c64.shape[1]
    out = torch.zeros(2, len(rows_of_chunk), N, dtype=torch.float64)
    for i, rows in enumerate(rows_of_chunk):
        if len(rows):
            blk = c64[list(rows)]
            out[0, i] = blk.sum(0)
            out[1, i] = (blk * blk).sum(0)
    assert float(out.abs().max()) < TWO24
    return out


# ------------------------------------------------------------------------------ inexact epilogues: GELU
# check: |got - ref| <= atol + 2^-7 |ref| (one bf16 ulp). atol = 4 x the worst error of the rounding model (the
# kernel's formula of csrc/kernels/common.h evaluated in fp32 on the CPU, then cast to bf16) that the relative term
# does not cover, over every pre-activation the cases produce (measure_gelu(); profiles/gemm_exact_tests.md). The 4
# is the margin of the attention needle tests: room for the device's exp2 / rcp being a few fp32 ulps off.
GELU_RTOL = 2.0 ** -7
GELU_MEASURED = 0.0      # forward: uncovered model error, see measure_gelu()
DGELU_MEASURED = 0.0     # backward (dh = acc * gelu'(pre)): uncovered model error
GELU_ATOL = 4 * GELU_MEASURED
DGELU_ATOL = 4 * DGELU_MEASURED
GELU_SHAPES = [(257, 136, 64, 2.0 ** -9), (264, 264, 192, 2.0 ** -10)]   # (M, N, K, alpha): pre within about +-8
DGELU_MS = [8, 257, 520]
DGELU_NK = (136, 64)
_C0, _C1, _L2E2 = 0.7978845608028654, 0.044715, 2.8853900817779268


def _sig2u_ref(x):
    return 1.0 / (1.0 + torch.exp(-2.0 * _C0 * (x + _C1 * x ** 3)))


def gelu_ref(x):
    """fp64 tanh-GELU, 0.5 x (1 + tanh u) written as x sigmoid(2u): the same function without the cancellation of
    1 + tanh u at large negative x."""
    return x * _sig2u_ref(x)


def gelu_grad_ref(x):
    """fp64 derivative of the tanh-GELU (0.5 (1 - tanh^2 u) = 2 s (1 - s) with s = sigmoid(2u))."""
    s = _sig2u_ref(x)
    return s + 2.0 * x * s * (1.0 - s) * _C0 * (1.0 + 3.0 * _C1 * x * x)


def _sig2u_f32(x):
    c = lambda v: torch.tensor(v, dtype=F32)   # noqa: E731
    u = c(_C0) * (x + c(_C1) * x * x * x)
    return torch.reciprocal(c(1.0) + torch.exp2(c(-_L2E2) * u))


def gelu_model(x64):
    """The kernel's forward formula (x * s, s = 1 / (1 + 2^(-2 u log2 e))) in fp32, cast to bf16."""
    x = x64.to(F32)
    return (x * _sig2u_f32(x)).to(BF16)


def dgelu_model(acc64, pre64):
    """The kernel's backward formula acc * (s + 2 x s (1 - s) sqrt(2/pi) (1 + 0.134145 x^2)) in fp32, cast to bf16."""
    x, acc = pre64.to(F32), acc64.to(F32)
    s = _sig2u_f32(x)
    c = lambda v: torch.tensor(v, dtype=F32)   # noqa: E731
    g = s + c(2.0) * x * s * (c(1.0) - s) * c(_C0) * (c(1.0) + c(0.134145) * x * x)
    return (acc * g).to(BF16)


def uncovered(model, ref64, rtol=GELU_RTOL):
    """Largest error of ``model`` against ``ref64`` that the relative term does not cover."""
    return float(((model.double() - ref64).abs() - rtol * ref64.abs()).clamp_min(0).max())


def gelu_problem(M, N, K, alpha, seed=5):
    p = problem(M, N, K, seed=seed, alpha=alpha, bias=True, bias_hi=2)
    return p, gelu_ref(p.ref.f64)


@functools.lru_cache(maxsize=None)
def dgelu_problem(M, seed=6):
    """a @ b with +-1 .. +-2 operands (|acc| <= 256), pre on the 1/4 grid within +-3.75 (exact in bf16)."""
    N, K = DGELU_NK
    p = problem(M, N, K, seed=seed, hi=2)
    pre = ints((M, N), 1, 15, seed * 13 + M) / 4
    return p, pre, p.ref.f64 * gelu_grad_ref(pre)


def measure_gelu():
    """(forward, backward) uncovered error of the rounding model over every pre-activation of the cases."""
    fwd = max(uncovered(gelu_model(p.ref.f64), ref) for p, ref in (gelu_problem(*s) for s in GELU_SHAPES))
    bwd = 0.0
    for M in DGELU_MS:
        p, pre, ref = dgelu_problem(M)
        bwd = max(bwd, uncovered(dgelu_model(p.ref.f64, pre), ref))
    return fwd, bwd


def check_close(got, ref64, atol, what, rtol=GELU_RTOL):
    """|got - ref| <= atol + rtol |ref| per element; NaN fails; reports the worst element."""
    g = got.detach().cpu().double()
    assert tuple(g.shape) == tuple(ref64.shape), f"{what}: shape"
    over = (g - ref64).abs() - (atol + rtol * ref64.abs())
    over = torch.where(torch.isnan(over), torch.full_like(over, float("inf")), over)
    if float(over.max()) > 0:
        i = tuple(int(v) for v in torch.unravel_index(over.reshape(-1).argmax(), over.shape))
        raise AssertionError(f"{what}: {int((over > 0).sum())} elements out of tolerance; worst {i}: got "
                             f"{float(g[i]):.8g}, want {float(ref64[i]):.8g} (atol {atol:.3g}, rtol {rtol:.3g})")


def colsum_parts_ref(dh64, M):
    """(sums, abs sums) [ceil(M / 256), N] of every 256-row tile's own rows."""
    tiles = -(-M // 256)
    s = torch.stack([dh64[t * 256:min((t + 1) * 256, M)].sum(0) for t in range(tiles)])
    a = torch.stack([dh64[t * 256:min((t + 1) * 256, M)].abs().sum(0) for t in range(tiles)])
    return s, a


def check_colsum_parts(parts, dh64, M, what):
    """Every (tile, column) partial within 2^-8 sum_rows |dh_ref| of its own rows' sum: 256 fp32 additions plus at
    most one bf16 rounding per term, whichever side of the cast the kernel sums on."""
    s, a = colsum_parts_ref(dh64, M)
    g = parts.detach().cpu().double()
    assert tuple(g.shape) == tuple(s.shape), f"{what}: shape {tuple(g.shape)} != {tuple(s.shape)}"
    over = (g - s).abs() - 2.0 ** -8 * a
    over = torch.where(torch.isnan(over), torch.full_like(over, float("inf")), over)
    if float(over.max()) > 0:
        i = tuple(int(v) for v in torch.unravel_index(over.reshape(-1).argmax(), over.shape))
        raise AssertionError(f"{what}: {int((over > 0).sum())} (tile, column) partials out of bound; worst {i}: got "
                             f"{float(g[i]):.8g}, want {float(s[i]):.8g}, bound {float(2.0 ** -8 * a[i]):.4g}")


if __name__ == "__main__":
    f, b = measure_gelu()
    print(f"GELU forward uncovered model error {f:.4g}; backward {b:.4g}")
