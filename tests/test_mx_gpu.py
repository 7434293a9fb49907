"""MX kernels on the device (csrc/kernels/mx.hip): pa_mx_quant bit for bit against the torch rule, pa_gemm_mx and
pa_gemm_mx_small_m exactly (operands built from codes and scale bytes so that fp32 accumulation is exact in any order)
and on random data, and the MXFP4Linear layer."""
import pytest
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.incubate import nn as INN
from paddlepaddle_amd.ops import _loader as L
from paddlepaddle_amd.ops import mx as MX

pytestmark = pytest.mark.gpu
FMTS = ["mxfp8", "mxfp4"]


@pytest.mark.parametrize("shape", [(1, 32), (77, 160), (300, 4096)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("fmt", FMTS)
def test_mx_quant_bit_exact(fmt, dtype, shape):
    R, K = shape
    g = torch.Generator().manual_seed(R + K)
    p2 = 2.0 ** torch.randint(-20, 21, (R * K // 32, 1), generator=g)
    xb = torch.randn(R * K // 32, 32, generator=g) * p2
    # planted at fixed blocks (all values exact in bf16): midpoints between adjacent e2m1 codes and between adjacent
    # e4m3 codes under an amax of 5, values that saturate (7.5 -> 6; 7.5 * 64 -> 448), an all-zero block
    ties = torch.tensor([5.0, 2.5, 3.5, 0.25, 0.75, 1.25, 1.75, -2.5, 1.0625, 1.1875, 2.125, 2.375, -1.0625, -0.25])
    xb[0::5, :14] = ties * p2[0::5]
    xb[1::5, :2] = torch.tensor([7.5, -7.75]) * p2[1::5]
    xb[2::5] = 0
    x = xb.reshape(R, K).to(dtype)
    q_ref, s_ref = MX._quantize_torch(x, fmt)
    L.reset_calls()
    q, s = MX.quantize_mx(x.cuda(), fmt)
    assert L.calls("pa_mx_quant") == 1
    assert torch.equal(s.cpu(), s_ref)
    assert torch.equal(q.cpu().view(torch.uint8), q_ref.view(torch.uint8))


def _operand(R, K, fmt, g):
    """Codes and scale bytes drawn directly: every e2m1 code (mxfp8: the multiples of 0.5 up to 6), scales 2^-1 .. 2^2
    per (row, k-block). Every product term is a multiple of 2^-4 and a sum over K <= 640 stays under 2^19."""
    s = torch.randint(126, 130, (R, K // 32), generator=g, dtype=torch.uint8)
    if fmt == "mxfp4":
        c = torch.randint(0, 16, (R, K), generator=g, dtype=torch.uint8)
        return c[:, 0::2] | (c[:, 1::2] << 4), s
    return (torch.randint(-12, 13, (R, K), generator=g) * 0.5).to(torch.float8_e4m3fn), s


def _exact_case(a_fmt, M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N + K)
    a, b = _operand(M, K, a_fmt, g), _operand(N, K, "mxfp4", g)
    ref = MX.dequantize_mx(*a, a_fmt, torch.float64) @ MX.dequantize_mx(*b, "mxfp4", torch.float64).t()
    return [t.cuda() for t in a], [t.cuda() for t in b], ref


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (300, 272, 256), (77, 528, 384), (513, 784, 640)])
@pytest.mark.parametrize("a_fmt", FMTS)
def test_gemm_mx_tiled_exact(a_fmt, M, N, K):
    a, b, ref = _exact_case(a_fmt, M, N, K)
    L.reset_calls()
    c = MX.gemm_mx(*a, a_fmt, *b, out_dtype=torch.float32)
    assert L.calls("pa_gemm_mx") == 1 and L.calls("pa_gemm_mx_small_m") == 0
    torch.testing.assert_close(c.cpu().double(), ref, rtol=0, atol=0)


@pytest.mark.parametrize("splits", ["one", "helper"])
@pytest.mark.parametrize("N,K", [(48, 128), (4096, 640)])
@pytest.mark.parametrize("M", [1, 16, 17, 64])
@pytest.mark.parametrize("a_fmt", FMTS)
def test_gemm_mx_small_m_exact(a_fmt, M, N, K, splits):
    a, b, ref = _exact_case(a_fmt, M, N, K)
    n = 1 if splits == "one" else MX.small_m_splits(M, N, K)
    assert splits == "one" or (n > 1) == (K == 640)
    L.reset_calls()
    c = MX.gemm_mx(*a, a_fmt, *b, out_dtype=torch.float32, splits=n)
    assert L.calls("pa_gemm_mx_small_m") == 1 and L.calls("pa_gemm_mx") == 0
    torch.testing.assert_close(c.cpu().double(), ref, rtol=0, atol=0)


@pytest.mark.parametrize("M,N,K,launcher", [(300, 272, 256, "pa_gemm_mx"), (17, 4096, 640, "pa_gemm_mx_small_m")])
def test_gemm_mx_bf16_bias_exact(M, N, K, launcher):
    a, b, ref = _exact_case("mxfp8", M, N, K)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(5))
    L.reset_calls()
    c = MX.gemm_mx(*a, "mxfp8", *b, bias=bias.cuda(), out_dtype=torch.bfloat16)
    assert L.calls(launcher) == 1
    # the exact sum plus the fp32 bias, rounded to fp32 (the kernel's add) and then to bf16
    want = (ref + bias.double()).float().to(torch.bfloat16)
    torch.testing.assert_close(c.cpu(), want, rtol=0, atol=0)


@pytest.mark.parametrize("M,N,launcher", [(192, 320, "pa_gemm_mx"), (24, 512, "pa_gemm_mx_small_m")])
def test_gemm_mx_random(M, N, launcher):
    K = 2048
    g = torch.Generator().manual_seed(M)
    x, w = torch.randn(M, K, generator=g).bfloat16(), (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    a, b = MX.quantize_mx(x.cuda(), "mxfp8"), MX.quantize_mx(w.cuda(), "mxfp4")
    L.reset_calls()
    c = MX.gemm_mx(*a, "mxfp8", *b)
    assert L.calls(launcher) == 1 and c.dtype == torch.bfloat16
    ref = MX.dequantize_mx(a[0].cpu(), a[1].cpu(), "mxfp8") @ MX.dequantize_mx(b[0].cpu(), b[1].cpu(), "mxfp4").t()
    torch.testing.assert_close(c.cpu().float(), ref, rtol=2e-2, atol=4e-2)  # bf16 output rounding only


@pytest.mark.parametrize("fin,path", [(512, "hip"), (520, "fallback")])
def test_mxfp4_linear_layer(fin, path):
    prev = paddle.get_device()
    paddle.set_device("gpu:0")
    paddle.set_default_dtype("bfloat16")
    try:
        lin = INN.MXFP4Linear.from_linear(paddle.nn.Linear(fin, 384))
        assert lin.w_q._t.is_cuda and list(lin.w_q.shape) == [384, -(-fin // 32) * 16]
        x = torch.randn(2, 96, fin, generator=torch.Generator().manual_seed(2)).bfloat16()
        n0 = dict(MX.CALLS)
        y = lin(paddle.to_tensor(x.cuda()))._t
        assert MX.CALLS[path] == n0[path] + 1 and y.shape == (2, 96, 384) and y.dtype == torch.bfloat16
        emu = MX.mx_linear(x, lin.w_q._t.cpu(), lin.w_s._t.cpu(), lin.bias._t.detach().cpu())
        torch.testing.assert_close(y.cpu().float(), emu.float(), rtol=2e-2, atol=4e-2)
    finally:
        paddle.set_default_dtype("float32")
        paddle.set_device(prev)
