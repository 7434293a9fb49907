"""Argument rejection of the GEMM launchers (csrc/kernels/gemm.hip): every call here is refused by the host checks
before anything is launched, with the return code L.call raises. 64 x 64 bf16 operands."""
import pytest
import torch

from paddlepaddle_amd.ops import _loader as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t():
    class T:
        a = torch.zeros(64, 64, device="cuda", dtype=torch.bfloat16)
        b = torch.zeros(64, 64, device="cuda", dtype=torch.bfloat16)
        c = torch.zeros(64, 64, device="cuda", dtype=torch.bfloat16)
        pre = torch.zeros(64, 64, device="cuda", dtype=torch.bfloat16)
        f32 = torch.zeros(64 * 64 * 4, device="cuda", dtype=torch.float32)
    return T


def _rejected(code, name, *args):
    n0 = L.calls(name)
    with pytest.raises(RuntimeError, match=rf"{name} failed with code {code}$"):
        L.call(name, *args)
    assert L.calls(name) == n0 + 1


def _gemm(t, M=64, N=64, K=64, lda=64, ldb=64, ldc=64, ak=1, bk=0):
    return ("pa_gemm_bf16", L.ptr(t.a), L.ptr(t.b), L.ptr(t.c), L.ptr(None), L.ptr(None), M, N, K, lda, ldb, ldc, ak,
            bk, 0, 1.0, 256, 1, L.stream_ptr())


def test_k_not_a_tile_multiple(t):
    _rejected(1, *_gemm(t, K=96))
    _rejected(1, "pa_gemm_bf16_pp", L.ptr(t.a), L.ptr(t.b), L.ptr(t.c), L.ptr(None), L.ptr(None), 64, 64, 96, 64, 64,
              64, 1, 0, 0, 1.0, L.ptr(None), L.stream_ptr())


def test_unaligned_lda(t):
    _rejected(1, *_gemm(t, lda=68))


def test_mn_major_a_needs_m_multiple_of_8(t):
    _rejected(1, *_gemm(t, M=60, ak=0))


def test_size_beyond_int(t):
    _rejected(1, *_gemm(t, M=2**31))


def test_pp_splitk_splits_must_divide_k_tiles(t):
    _rejected(1, "pa_gemm_bf16_pp_splitk", L.ptr(t.a), L.ptr(t.b), L.ptr(t.c), 64, 64, 128, 128, 64, 64, 1, 0, 0, 1.0,
              3, L.ptr(t.f32), L.stream_ptr())


def test_segs_at_most_four(t):
    tab = torch.zeros(5, 5, dtype=torch.int64)
    _rejected(1, "pa_gemm_bf16_pp_segs", tab.data_ptr(), 5, 1, L.ptr(t.a), L.ptr(t.b), L.ptr(t.c), L.ptr(None), 64, 64,
              64, 64, 64, 64, 1, 0, 0, 1.0, L.ptr(None), L.stream_ptr())


def test_dgelu_kernel_code(t):
    _rejected(1, "pa_gemm_bf16_dgelu", L.ptr(t.a), L.ptr(t.b), L.ptr(t.c), L.ptr(t.pre), L.ptr(t.f32), 64, 64, 64, 64,
              64, 64, 1, 0, 3, L.stream_ptr())


def test_residual_may_not_alias_output(t):
    _rejected(1, "pa_gemm_bf16_res", L.ptr(t.a), L.ptr(t.b), L.ptr(t.c), L.ptr(None), L.ptr(t.c), 64, 64, 64, 64, 64,
              64, 1, 0, L.ptr(None), L.stream_ptr())


def test_small_m_rows_and_stages(t):
    def small_m(M, stages):
        return ("pa_gemm_small_m", L.ptr(t.a), 64, L.ptr(t.b), 64, L.ptr(t.c), 64, L.ptr(None), L.ptr(t.f32), M, 64, 64,
                1, stages, L.stream_ptr())
    _rejected(1, *small_m(65, 4))
    _rejected(2, *small_m(64, 5))


def test_conv_wgrad_tile_width(t):
    # x [1, 8, 8, 8], dy [1, 8, 8, 8], 1x1 filter: 64 pixels, valid but for bn
    _rejected(2, "pa_conv2d_nhwc_wgrad", L.ptr(t.a), L.ptr(t.b), L.ptr(t.f32), L.ptr(t.pre), 1, 8, 8, 8, 8, 1, 1, 1, 0,
              0, 1, 8, 8, 1, 96, L.stream_ptr())
