"""fp8 quantization (csrc/kernels/quant_fp8.hip, ops.fp8.quantize_fp8 / Fp8TensorState, incubate fp8_quantize).

CPU: the public function and the scaling-state rule in torch against hand-written references. GPU: pa_fp8_quant bit for
bit against the torch conversion on the CPU — both formats, three input dtypes, scalar / vector / ragged / misaligned
geometry, with and without the transposed copy and the amax partials, on data that reaches both denormal ranges,
saturation and exact round-to-nearest-even ties — and pa_fp8_amax / pa_fp8_scale_update against the same rule."""
import functools
import zlib

import pytest
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.incubate.nn import functional as IF
from paddlepaddle_amd.ops import _loader as L
from paddlepaddle_amd.ops import fp8 as F8

E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
FMAX = {E4: 448.0, E5: 57344.0}


def _ref_quant(x, fmt, scale):
    return (x.float() * scale).clamp(-FMAX[fmt], FMAX[fmt]).to(fmt)


def _bits(q):
    return q.view(torch.uint8)


# ------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("fmt,name", [(E4, "float8_e4m3fn"), (E5, "float8_e5m2")])
def test_fp8_quantize_semantics_cpu(fmt, name):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 5, 16, generator=g) * 7
    # explicit scale, with the transpose of the [15, 16] view
    q, sinv, qT = IF.fp8_quantize(paddle.to_tensor(x), name, scale=4.0, return_transpose=True)
    ref = _ref_quant(x, fmt, 4.0)
    assert q._t.dtype == fmt and list(q.shape) == [3, 5, 16] and list(qT.shape) == [16, 15]
    assert torch.equal(_bits(q._t), _bits(ref))
    assert torch.equal(_bits(qT._t), _bits(ref.reshape(15, 16).t().contiguous()))
    assert sinv._t.item() == 0.25
    # saturation instead of NaN / inf
    big = torch.tensor([1e6, -1e6, 0.0, -0.0])
    qb = IF.fp8_quantize(paddle.to_tensor(big), name, scale=1.0)[0]._t
    assert qb.float().tolist()[:2] == [FMAX[fmt], -FMAX[fmt]] and _bits(qb).tolist()[2:] == [0, 0x80]
    # current scaling: amax lands on fmax, margin halves the scale per unit
    for margin in (0, 2):
        q, sinv = IF.fp8_quantize(paddle.to_tensor(x), name, margin=margin)
        scale = (torch.tensor(FMAX[fmt]) / x.abs().max()) * 2.0 ** -margin
        assert torch.equal(sinv._t.reshape(()), 1.0 / scale)
        assert torch.equal(_bits(q._t), _bits(_ref_quant(x, fmt, scale)))
        assert q._t.float().abs().max().item() == FMAX[fmt] * 2.0 ** -margin


def _r32(v):
    return (torch.tensor(1.0) / torch.tensor(v)).item()


def test_fp8_state_rule_cpu():
    st = F8.Fp8TensorState(E4, "delayed", amax_history_len=4, margin=0)
    x1, x2, x3 = torch.full((4, 8), 2.0), torch.full((4, 8), 8.0), torch.full((4, 8), 1.0)
    # the first call is current: the tensor's own amax sets the scale it is quantized with
    q, _, sinv = st.quantize(x1)
    assert q.float().max().item() == 448.0 and sinv.item() == _r32(224.0)
    assert st.amax_history.tolist() == [2.0, 0.0, 0.0, 0.0] and st.scale.item() == 448.0 / 2.0
    # delayed: x2 is quantized with the scale of the history before it (224: 8 * 224 saturates), then enters it
    q, _, sinv = st.quantize(x2)
    assert sinv.item() == _r32(224.0) and q.float().max().item() == 448.0
    assert st.amax_history.tolist() == [8.0, 2.0, 0.0, 0.0] and st.scale.item() == 448.0 / 8.0
    q, _, _ = st.quantize(x3)
    assert q.float().max().item() == 56.0  # 1 * 448 / 8
    assert st.amax_history.tolist() == [1.0, 8.0, 2.0, 0.0] and st.scale.item() == 448.0 / 8.0
    # the history shifts its oldest entry out: after two more calls the 8 is gone
    st.quantize(x3), st.quantize(x3)
    assert st.amax_history.tolist() == [1.0, 1.0, 1.0, 8.0]
    st.quantize(x3)
    assert st.amax_history.tolist() == [1.0, 1.0, 1.0, 1.0] and st.scale.item() == 448.0
    # a non-finite amax leaves scale, its inverse and the history as they are
    for bad in (float("inf"), float("nan")):
        xb = x3.clone()
        xb[1, 2] = bad
        st.quantize(xb)
        assert st.amax_history.tolist() == [1.0, 1.0, 1.0, 1.0]
        assert st.scale.item() == 448.0 and st.scale_inv.item() == _r32(448.0)
    # so does a zero amax: on a fresh state (all-zero history) and under the current recipe
    for recipe in ("delayed", "current"):
        z = F8.Fp8TensorState(E5, recipe, amax_history_len=3)
        z.quantize(torch.zeros(2, 8))
        assert z.scale.item() == 1.0 and z.scale_inv.item() == 1.0 and z.amax_history.tolist() == [0.0, 0.0, 0.0]
    cur = F8.Fp8TensorState(E5, "current", amax_history_len=3)
    cur.quantize(x2)
    cur.quantize(torch.zeros(2, 8))
    assert cur.scale.item() == 57344.0 / 8.0
    # margin halves the scale per unit
    for m in (0, 1, 3):
        s = F8.Fp8TensorState(E4, "current", margin=m)
        s.quantize(x2)
        assert s.scale.item() == (448.0 / 8.0) / 2 ** m and s.scale_inv.item() == _r32((448.0 / 8.0) / 2 ** m)


# ------------------------------------------------------------------------------------------------- GPU
SCALE = {E4: 8.0, E5: 128.0}  # powers of two: x * scale is exact, so a planted tie stays a tie


@functools.lru_cache(maxsize=None)
def _codes(fmt):
    """Every finite non-negative value of the format, ascending."""
    v = torch.arange(0, 0x7F if fmt == E4 else 0x7C, dtype=torch.uint8).view(fmt).float()
    assert torch.isfinite(v).all() and v[-1].item() == FMAX[fmt]
    return v


def _planted(fmt, dtype):
    """Zeros, +-fmax / scale, values beyond it, and the midpoint of every pair of neighbouring codes, all divided by
    the (power-of-two) scale and kept only if the input dtype holds them exactly."""
    s, c = SCALE[fmt], _codes(fmt)
    mid = (c[:-1] + c[1:]) / 2
    v = torch.cat([torch.tensor([0.0, -0.0, FMAX[fmt], -FMAX[fmt], FMAX[fmt] * 1.0625, -FMAX[fmt] * 1.0625,
                                 FMAX[fmt] * 4, -FMAX[fmt] * 4]), mid, -mid]) / s
    keep = v.to(dtype).float() == v
    assert keep[:8].all() and keep.sum() > 100
    return v[keep].to(dtype)


@functools.lru_cache(maxsize=None)
def _data(shape, dtype, fmt):
    """(x on the CPU, reference bits): randn * 2^k, k in [-12, 8] per element, with the planted values in front."""
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, dtype, fmt)).encode()))
    n = 1
    for d in shape:
        n *= d
    x = (torch.randn(n, generator=g) * torch.exp2(torch.randint(-12, 9, (n,), generator=g).float())).to(dtype)
    p = _planted(fmt, dtype)
    k = min(n, p.numel()) if n > 8 else 0
    x[:k] = p[:k]
    x = x[torch.randperm(n, generator=g)].reshape(shape) if n > 1 else x.reshape(shape)
    return x, _bits(_ref_quant(x, fmt, SCALE[fmt]))


def _run_quant(xg, fmt, scale, transpose, with_parts):
    parts = torch.full((F8.n_parts(),), -1.0, device="cuda") if with_parts else None
    n0 = L.calls("pa_fp8_quant")
    q, qT = F8.quantize_fp8(xg, fmt, scale, transpose, parts)
    assert L.calls("pa_fp8_quant") == n0 + 1
    return q, qT, parts


def _check_quant(xg, x, ref_bits, fmt):
    scale = torch.tensor([SCALE[fmt]], device="cuda")
    C = x.shape[-1]
    for transpose in (False, True):
        for with_parts in (False, True):
            q, qT, parts = _run_quant(xg, fmt, scale, transpose, with_parts)
            assert q.shape == x.shape and q.dtype == fmt
            torch.testing.assert_close(_bits(q).cpu(), ref_bits, rtol=0, atol=0)
            if transpose:
                assert qT.shape == (C, x.numel() // C)
                torch.testing.assert_close(_bits(qT).cpu(), ref_bits.reshape(-1, C).t().contiguous(), rtol=0, atol=0)
            else:
                assert qT is None
            if with_parts:
                assert parts.max().item() == x.float().abs().max().item() and parts.min().item() >= 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [E4, E5])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("shape", [(1, 1), (33, 17), (64, 64), (130, 200), (256, 384)])
def test_fp8_quant_bit_exact_gpu(shape, dtype, fmt):
    """(33, 17): everything on the scalar path; (130, 200): ragged tiles and a byte-wise transposed store on the vector
    path; (256, 384): several whole tiles."""
    x, ref_bits = _data(shape, dtype, fmt)
    _check_quant(x.cuda(), x, ref_bits, fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [E4, E5])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_fp8_quant_misaligned_base_gpu(dtype, fmt):
    """A contiguous (384, 128) view one element into a larger buffer: C % 8 == 0 but the base is not 16-byte aligned."""
    x, ref_bits = _data((384, 128), dtype, fmt)
    buf = torch.zeros(384 * 128 + 8, dtype=dtype, device="cuda")
    xg = buf[1:1 + 384 * 128].view(384, 128)
    xg.copy_(x)
    assert xg.data_ptr() % 16 != 0 and xg.is_contiguous()
    _check_quant(xg, x, ref_bits, fmt)
    parts = torch.empty(F8.n_parts(), device="cuda")
    F8.amax_parts(xg, parts)
    assert L.calls("pa_fp8_amax") == 1 and parts.max().item() == x.float().abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,name", [(E4, "float8_e4m3fn"), (E5, "float8_e5m2")])
def test_fp8_quantize_public_3d_gpu(fmt, name):
    x, ref_bits = _data((3, 40, 64), torch.bfloat16, fmt)
    q, sinv, qT = IF.fp8_quantize(paddle.to_tensor(x.cuda()), name, scale=SCALE[fmt], return_transpose=True)
    assert L.calls("pa_fp8_quant") == 1
    assert list(q.shape) == [3, 40, 64] and list(qT.shape) == [64, 120] and sinv._t.item() == 1.0 / SCALE[fmt]
    torch.testing.assert_close(_bits(q._t).cpu(), ref_bits, rtol=0, atol=0)
    torch.testing.assert_close(_bits(qT._t).cpu(), ref_bits.reshape(120, 64).t().contiguous(), rtol=0, atol=0)
    # current scaling: the device's own scale is read back and fed to the reference
    st = F8.Fp8TensorState(fmt, "current", device="cuda")
    q, _, sinv = st.quantize(x.cuda(), transpose=False)
    assert L.calls("pa_fp8_amax") == 1 and L.calls("pa_fp8_scale_update") == 1 and L.calls("pa_fp8_quant") == 2
    scale = st.scale.cpu().reshape(())
    torch.testing.assert_close(scale, torch.tensor(FMAX[fmt]) / x.float().abs().max(), rtol=1e-6, atol=0)
    torch.testing.assert_close(sinv.cpu().reshape(()), 1.0 / scale, rtol=1e-6, atol=0)
    torch.testing.assert_close(_bits(q).cpu(), _bits(_ref_quant(x, fmt, scale)), rtol=0, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("n", [1, 1000, 8 * 1024 * 5 + 3, 9 * 1024 * 1024 + 5])
def test_fp8_amax_exact_gpu(n, dtype):
    """One element, a scalar tail, and enough for several workgroups with the unrolled body (9M: every slot of the
    partials buffer is owned by a workgroup)."""
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n, generator=g) * torch.exp2(torch.randint(-12, 9, (n,), generator=g).float())).to(dtype)
    parts = torch.full((F8.n_parts(),), -1.0, device="cuda")
    F8.amax_parts(x.cuda(), parts)
    assert L.calls("pa_fp8_amax") == 1
    assert parts.min().item() >= 0.0 and parts.max().item() == x.float().abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("shape", [(33, 17), (256, 384)])
def test_fp8_amax_non_finite_gpu(shape, bad):
    x, _ = _data(shape, torch.bfloat16, E4)
    x = x.clone()
    x[shape[0] // 2, shape[1] // 3] = bad
    xg = x.cuda()
    parts = torch.zeros(F8.n_parts(), device="cuda")
    F8.amax_parts(xg, parts)
    assert L.calls("pa_fp8_amax") == 1 and not torch.isfinite(parts.max()).item()
    parts.zero_()
    F8.quantize_fp8(xg, E4, torch.ones(1, device="cuda"), True, parts)
    assert L.calls("pa_fp8_quant") == 1 and not torch.isfinite(parts.max()).item()


def _update_gpu(a_new, hist, scale, scale_inv, fmax, margin, mode):
    parts = torch.zeros(F8.n_parts(), device="cuda")
    parts[37] = a_new
    n0 = L.calls("pa_fp8_scale_update")
    L.call("pa_fp8_scale_update", L.ptr(parts), parts.numel(), L.ptr(hist), hist.numel(), L.ptr(scale),
           L.ptr(scale_inv), fmax, margin, mode, L.stream_ptr())
    assert L.calls("pa_fp8_scale_update") == n0 + 1


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [E4, E5])
@pytest.mark.parametrize("margin", [0, 3])
def test_fp8_scale_update_gpu(fmt, margin):
    fmax = FMAX[fmt]
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    want = lambda a: (f32(fmax) / f32(a)) * f32(2.0 ** -margin)  # noqa: E731
    hist = torch.zeros(5, device="cuda")
    scale, sinv = torch.ones(1, device="cuda"), torch.ones(1, device="cuda")
    expect_hist = [0.0] * 5
    last = None
    for a in (0.3712, 11.25, 2.5e-3, 0.7, 0.9, 0.1, 0.2, 0.05):  # 11.25 leaves the 5-slot history at the 7th call
        _update_gpu(a, hist, scale, sinv, fmax, margin, 1)
        expect_hist = [f32(a).item()] + expect_hist[:-1]
        assert hist.cpu().tolist() == expect_hist
        last = want(max(expect_hist))
        torch.testing.assert_close(scale.cpu().reshape(()), last, rtol=1e-6, atol=0)
        torch.testing.assert_close(sinv.cpu().reshape(()), 1.0 / last, rtol=1e-6, atol=0)
    assert max(expect_hist) == f32(0.9).item()
    # a zero history with a zero amax, and any non-finite amax: nothing moves
    before = (hist.clone(), scale.clone(), sinv.clone())
    for bad in (float("inf"), float("nan")):
        for mode in (0, 1):
            _update_gpu(bad, hist, scale, sinv, fmax, margin, mode)
            assert torch.equal(hist, before[0]) and torch.equal(scale, before[1]) and torch.equal(sinv, before[2])
    _update_gpu(0.0, hist, scale, sinv, fmax, margin, 0)
    assert torch.equal(hist, before[0]) and torch.equal(scale, before[1]) and torch.equal(sinv, before[2])
    zh = torch.zeros(5, device="cuda")
    _update_gpu(0.0, zh, scale, sinv, fmax, margin, 1)
    assert zh.abs().max().item() == 0.0 and torch.equal(scale, before[1]) and torch.equal(sinv, before[2])
    # current mode: the fresh amax alone, history untouched
    _update_gpu(4.0, hist, scale, sinv, fmax, margin, 0)
    assert torch.equal(hist, before[0])
    torch.testing.assert_close(scale.cpu().reshape(()), want(4.0), rtol=1e-6, atol=0)
