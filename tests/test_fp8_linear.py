"""fp8 training linear: ops.fp8.fp8_linear / incubate.nn.FP8Linear and the fp8 GEMM's device-side scales.

CPU: the torch emulation (same quantization, fp32 products of the dequantized operands) through the layer — shapes,
dtypes, shared parameters, state_dict round trip, fallback counter. GPU: pa_gemm_fp8_dscale against the host-alpha
path bit for bit; the HIP linear (pa_fp8_quant + pa_gemm_fp8_dscale) against that emulation run on the CPU from the
same inputs, its error against the unquantized fp32 linear, the delayed recipe's state machine, the weight cache and
the saved-tensor set."""
import functools

import pytest
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.incubate import nn as INN
from paddlepaddle_amd.ops import _loader as L
from paddlepaddle_amd.ops import fp8 as F8

E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2


def _inputs(M, K, N, dtype, lead=None, seed=0):
    """x ~ N(0, 1), w ~ 0.05 N(0, 1), b ~ 0.1 N(0, 1), dy ~ 1e-3 N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    xs = (M, K) if lead is None else (*lead, K)
    x = torch.randn(xs, generator=g).to(dtype)
    w = (0.05 * torch.randn(K, N, generator=g)).to(dtype)
    b = (0.1 * torch.randn(N, generator=g)).to(dtype)
    dy = (1e-3 * torch.randn(*xs[:-1], N, generator=g)).to(dtype)
    return x, w, b, dy


def _run(x, w, b, dy, states, emulate, device):
    """One forward + backward of ops.fp8.fp8_linear on ``device``: (y, dx, dw, db) on the CPU."""
    leaf = lambda t: t.detach().clone().to(device).requires_grad_()  # noqa: E731
    x, w, dy = leaf(x), leaf(w), dy.to(device)
    b = None if b is None else leaf(b)
    y = F8.fp8_linear(x, w, b, states, emulate=emulate)
    y.backward(dy)
    out = (y.detach(), x.grad, w.grad, None if b is None else b.grad)
    return tuple(None if t is None else t.cpu() for t in out)


# ------------------------------------------------------------------------------------------------- CPU
def _layer(K, N, recipe="delayed", bias=True, dtype="bfloat16", **kw):
    paddle.set_default_dtype(dtype)
    try:
        return INN.FP8Linear(K, N, bias_attr=None if bias else False, recipe=recipe, **kw)
    finally:
        paddle.set_default_dtype("float32")


def test_fp8_linear_layer_emulation_cpu():
    lin = _layer(128, 256, amax_history_len=4)
    assert list(lin.weight.shape) == [128, 256] and list(lin.bias.shape) == [256]
    assert sorted(k for k in lin.state_dict() if k.startswith("fp8_")) == sorted(
        f"fp8_{r}_{s}" for r in ("x", "w", "dy") for s in ("amax_history", "scale", "scale_inv"))
    n0 = dict(F8.CALLS)
    x = paddle.to_tensor(torch.randn(2, 64, 128), stop_gradient=False)  # fp32 input: cast to the weight dtype
    y = lin(x)
    assert list(y.shape) == [2, 64, 256] and y._t.dtype == torch.bfloat16
    y.sum().backward()
    assert F8.CALLS["emulated"] == n0["emulated"] + 1 and F8.CALLS["fallback"] == n0["fallback"]
    assert lin.weight.grad.shape == lin.weight.shape and lin.weight._t.grad.dtype == torch.bfloat16
    assert lin.bias._t.grad.dtype == torch.bfloat16 and list(x.grad.shape) == [2, 64, 128]
    # close to the bf16 linear (e4m3 carries 3 mantissa bits: a few percent)
    ref = x._t.to(torch.bfloat16).float().reshape(-1, 128) @ lin.weight._t.float() + lin.bias._t.float()
    err = (y._t.float().reshape(-1, 256) - ref).norm() / ref.norm()
    assert 1e-3 < err.item() < 0.08
    torch.testing.assert_close(lin.bias._t.grad.float(), torch.full((256,), 128.0))
    # every state has seen its tensor
    for r in ("x", "w", "dy"):
        assert getattr(lin, f"fp8_{r}_amax_history")._t[0].item() > 0
    assert lin.fp8_dy_amax_history._t[0].item() == 1.0  # the gradient of sum(): all ones
    assert lin.fp8_dy_scale._t.item() == 57344.0


def test_fp8_linear_from_linear_shares_parameters_cpu():
    paddle.set_default_dtype("bfloat16")
    try:
        base = paddle.nn.Linear(128, 128)
    finally:
        paddle.set_default_dtype("float32")
    lin = INN.FP8Linear.from_linear(base, recipe="current")
    assert lin.weight is base.weight and lin.bias is base.bias
    assert [id(p) for p in lin.parameters()] == [id(p) for p in base.parameters()]
    x = paddle.to_tensor(torch.randn(128, 128).to(torch.bfloat16))
    y0 = lin(x)._t.clone()
    with torch.no_grad():
        base.weight._t.mul_(2.0)
        base.bias._t.zero_()
    y1 = lin(x)._t
    assert not torch.equal(y0, y1)
    ref = x._t.float() @ base.weight._t.float()
    assert ((y1.float() - ref).norm() / ref.norm()).item() < 0.08


def test_fp8_linear_state_dict_round_trip_cpu():
    """A layer rebuilt from the state_dict continues exactly where the first one stands: same delayed scales, same
    next output and gradients, bit for bit."""
    g = torch.Generator().manual_seed(3)
    a = _layer(128, 128, amax_history_len=3)
    xs = [paddle.to_tensor((torch.randn(128, 128, generator=g) * (i + 1)).to(torch.bfloat16)) for i in range(3)]
    for x in xs[:2]:
        a(x).sum().backward()
        with torch.no_grad():  # the optimizer step between two calls
            a.weight._t.mul_(1.25)
    sd = {k: paddle.to_tensor(v._t.clone()) for k, v in a.state_dict().items()}
    b = _layer(128, 128, amax_history_len=3)
    missing, unexpected = b.set_state_dict(sd)
    assert not missing and not unexpected
    assert torch.equal(b.fp8_x_amax_history._t, a.fp8_x_amax_history._t) and b.fp8_x_amax_history._t[1].item() > 0
    outs = []
    for lay in (a, b):
        lay.clear_gradients()
        x = paddle.to_tensor(xs[2]._t.clone(), stop_gradient=False)
        y = lay(x)
        (y * y).sum().backward()
        outs.append((y._t, x._t.grad, lay.weight._t.grad, lay.bias._t.grad))
    for u, v in zip(*outs):
        assert torch.equal(u.view(torch.int16), v.view(torch.int16))
    for k, v in a.state_dict().items():
        assert torch.equal(v._t, b.state_dict()[k]._t), k


def test_fp8_linear_fallback_counter_cpu():
    lin = _layer(96, 128, recipe="current")  # K is no multiple of 128
    n0 = dict(F8.CALLS)
    x = paddle.to_tensor(torch.randn(128, 96).to(torch.bfloat16), stop_gradient=False)
    y = lin(x)
    y.sum().backward()
    assert F8.CALLS["fallback"] == n0["fallback"] + 1 and F8.CALLS["emulated"] == n0["emulated"]
    ref = x._t.float() @ lin.weight._t.float() + lin.bias._t.float()
    torch.testing.assert_close(y._t.float(), ref, rtol=2e-2, atol=2e-2)  # the plain bf16 linear
    assert lin.fp8_x_amax_history._t.abs().max().item() == 0.0 and list(x.grad.shape) == [128, 96]
    # rows that are no multiple of 128, and an fp32 layer, fall back as well
    lin2 = _layer(128, 128, recipe="current")
    lin2(paddle.to_tensor(torch.randn(100, 128).to(torch.bfloat16)))
    lin3 = _layer(128, 128, recipe="current", dtype="float32")
    lin3(paddle.to_tensor(torch.randn(128, 128)))
    assert F8.CALLS["fallback"] == n0["fallback"] + 3 and F8.CALLS["emulated"] == n0["emulated"]


# ------------------------------------------------------------------------------------------------- GPU: GEMM
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["auto", "generic"])
@pytest.mark.parametrize("shape", [(256, 256, 128), (300, 264, 384), (4096, 5120, 1024)])
def test_fp8_gemm_device_scales_gpu(shape, kernel):
    """alpha = 1 with device scales (sa, sb) == the host-alpha path at alpha = fp32(sa * sb), bit for bit; 4096 x 5120
    (320 tiles) at K = 1024, the smallest K the tail plan cuts into slices (two of four K-tiles), runs the ping-pong
    kernel's tail-reduce epilogue."""
    M, N, K = shape
    if M == 4096:
        assert int(L.lib().pa_gemm_fp8_ws_bytes(M, N, K)) > 0
    g = torch.Generator().manual_seed(7)
    a = torch.randn(M, K, generator=g).to(E4).cuda()
    b = torch.randn(N, K, generator=g).to(E5).cuda()
    bias = torch.randn(N, generator=g).to(torch.bfloat16).cuda()
    sa, sb = torch.tensor([0.37], dtype=torch.float32), torch.tensor([1.91], dtype=torch.float32)
    one = torch.ones(1)
    old = F8.set_kernel(kernel)
    try:
        for pa, pb in ((sa, sb), (sa, None), (None, sb)):
            alpha = ((one if pa is None else pa) * (one if pb is None else pb)).item()  # the product in fp32
            want = F8.gemm_fp8(a, b, bias, alpha, "identity", torch.bfloat16)
            n0 = L.calls("pa_gemm_fp8_dscale")
            got = F8.gemm_fp8(a, b, bias, 1.0, "identity", torch.bfloat16,
                              a_scale_inv=None if pa is None else pa.cuda(),
                              b_scale_inv=None if pb is None else pb.cuda())
            assert L.calls("pa_gemm_fp8_dscale") == n0 + 1
            assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        assert want.float().abs().max().item() > 1.0
    finally:
        F8.set_kernel(old)


# ------------------------------------------------------------------------------------------------- GPU: linear
CASES = [((128, 128, 128), None), ((256, 384, 128), None), ((256, 384, 128), (2, 128))]


@functools.lru_cache(maxsize=None)
def _reference(shape, lead, dtype, bias):
    """The inputs, the CPU emulation's (y, dx, dw, db) and the fp32 linear's (y, dx, dw), computed once."""
    M, K, N = shape
    x, w, b, dy = _inputs(M, K, N, dtype, lead)
    b = b if bias else None
    emu = _run(x, w, b, dy, F8.new_states("current"), True, "cpu")
    x32, w32, dy32 = x.float().reshape(-1, K), w.float(), dy.float().reshape(-1, N)
    y32 = x32 @ w32 + (b.float() if bias else 0.0)
    exact = (y32.reshape(dy.shape), (dy32 @ w32.t()).reshape(x.shape), x32.t() @ dy32)
    return (x, w, b, dy), emu, exact


def _rel(a, ref):
    return ((a.float() - ref).norm() / ref.norm()).item()


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape,lead", CASES)
def test_fp8_linear_matches_emulation_gpu(shape, lead, dtype, bias):
    (x, w, b, dy), emu, exact = _reference(shape, lead, dtype, bias)
    n0 = F8.CALLS["hip"]
    got = _run(x, w, b, dy, F8.new_states("current"), False, "cuda")
    assert F8.CALLS["hip"] == n0 + 1
    assert L.calls("pa_fp8_quant") == 3 and L.calls("pa_gemm_fp8_dscale") == 3 and L.calls("pa_fp8_amax") == 3
    assert L.calls("pa_colsum") + L.calls("pa_fold_partials") == (1 if bias else 0)
    tol = 1e-2 if dtype == torch.float16 else 2e-2
    for name, g_, e_ in zip(("y", "dx", "dw", "db"), got, emu):
        if e_ is None:
            assert g_ is None
            continue
        assert g_.dtype == dtype and g_.shape == e_.shape, name
        torch.testing.assert_close(g_.float(), e_.float(), rtol=tol, atol=2 * tol * e_.float().std().item(), msg=name)
    # against the unquantized fp32 linear: no worse than the emulation, up to the 16-bit output rounding
    for name, g_, e_, r_ in zip(("y", "dx", "dw"), got, emu, exact):
        eg, ee = _rel(g_, r_), _rel(e_, r_)
        print(f"{name}: fp8 HIP {eg:.4f} emulation {ee:.4f}")
        assert eg <= 1.25 * ee, (name, eg, ee)


@pytest.mark.gpu
def test_fp8_linear_delayed_recipe_gpu():
    """Three forward + backward calls with different inputs (and a weight update between them): the device states follow
    the CPU state machine, and the third call matches the emulation driven by the device's scales."""
    M, K, N = 256, 384, 128
    dev, cpu = F8.new_states("delayed", 4, 1, "cuda"), F8.new_states("delayed", 4, 1, "cpu")
    _, w, b, _ = _inputs(M, K, N, torch.bfloat16)
    wg = w.cuda()
    for i in range(3):
        x, _, _, dy = _inputs(M, K, N, torch.bfloat16, seed=10 + i)
        x, dy = x * (1.0 + i), dy * (3.0 - i)
        if i == 2:  # the third call quantizes with the scales of the history: give the emulation the device's own
            for r in ("x", "w", "dy"):
                cpu[r].scale.copy_(dev[r].scale.cpu())
                cpu[r].scale_inv.copy_(dev[r].scale_inv.cpu())
        got = _run(x, wg, b, dy, dev, False, "cuda")
        emu = _run(x, w, b, dy, cpu, True, "cpu")
        for r in ("x", "w", "dy"):
            torch.testing.assert_close(dev[r].amax_history.cpu(), cpu[r].amax_history, rtol=1e-6, atol=0)
            torch.testing.assert_close(dev[r].scale.cpu(), cpu[r].scale, rtol=1e-6, atol=0)
            torch.testing.assert_close(dev[r].scale_inv.cpu(), cpu[r].scale_inv, rtol=1e-6, atol=0)
            assert dev[r].amax_history[min(i, 3)].item() > 0 and dev[r].calls == i + 1
        with torch.no_grad():
            w = w * 1.5
            wg.mul_(1.5)
    # one amax pass per state (its first call); afterwards the amax comes out of the quantize kernel
    assert L.calls("pa_fp8_amax") == 3 and L.calls("pa_fp8_quant") == 9 and L.calls("pa_fp8_scale_update") == 9
    for name, g_, e_ in zip(("y", "dx", "dw", "db"), got, emu):
        torch.testing.assert_close(g_.float(), e_.float(), rtol=2e-2, atol=4e-2 * e_.float().std().item(), msg=name)


@pytest.mark.gpu
def test_fp8_linear_weight_cache_gpu():
    M, K, N = 128, 256, 128
    x, w, b, _ = _inputs(M, K, N, torch.bfloat16)
    st = F8.new_states("current", device="cuda")
    xg, wg, bg = x.cuda(), w.cuda().requires_grad_(), b.cuda()
    y1 = F8.fp8_linear(xg, wg, bg, st)
    assert L.calls("pa_fp8_quant") == 2  # x and the weight
    y2 = F8.fp8_linear(xg, wg, bg, st)
    assert L.calls("pa_fp8_quant") == 3 and st["w"].calls == 1  # x only: the weight's pair is reused
    assert torch.equal(y1, y2)
    with torch.no_grad():  # an optimizer's in-place update
        wg.mul_(-0.5)
    y3 = F8.fp8_linear(xg, wg, bg, st)
    assert L.calls("pa_fp8_quant") == 5 and st["w"].calls == 2
    emu = F8.fp8_linear(x, w * -0.5, b, F8.new_states("current"), emulate=True)
    torch.testing.assert_close(y3.float().cpu(), emu.float(), rtol=2e-2, atol=4e-2 * emu.float().std().item())
    assert not torch.allclose(y3.float(), y1.float(), rtol=0.1, atol=0.1)


@pytest.mark.gpu
def test_fp8_linear_saves_no_16bit_activation_gpu():
    M, K, N = 128, 256, 128
    x, w, b, dy = _inputs(M, K, N, torch.bfloat16)
    xg, wg = x.cuda().requires_grad_(), w.cuda().requires_grad_()
    y = F8.fp8_linear(xg, wg, b.cuda(), F8.new_states("current", device="cuda"))
    saved = [t for t in y.grad_fn.saved_tensors if t is not None]
    assert saved and L.calls("pa_gemm_fp8_dscale") == 1
    assert not any(t.dtype == xg.dtype and t.numel() == xg.numel() for t in saved)
    assert {(tuple(t.shape), t.dtype) for t in saved if t.numel() > 1} == {((K, M), E4), ((K, N), E4)}


@pytest.mark.gpu
def test_fp8_linear_layer_gpu():
    """The public layer on the device: HIP path for a multiple-of-128 shape, the fallback counter otherwise."""
    prev = paddle.get_device()
    paddle.set_device("gpu:0")
    try:
        lin = _layer(256, 128, recipe="delayed")
        assert lin.weight._t.is_cuda and lin.fp8_x_scale._t.is_cuda
        n0 = dict(F8.CALLS)
        x = paddle.to_tensor(torch.randn(2, 64, 256).cuda(), stop_gradient=False)
        y = lin(x)
        y.sum().backward()
        assert F8.CALLS["hip"] == n0["hip"] + 1 and L.calls("pa_gemm_fp8_dscale") == 3
        ref = x._t.to(torch.bfloat16).float().reshape(-1, 256) @ lin.weight._t.float() + lin.bias._t.float()
        assert _rel(y._t.reshape(-1, 128), ref) < 0.08
        assert lin.weight._t.grad.shape == (256, 128) and lin.fp8_dy_scale._t.item() == 57344.0
        lin(paddle.to_tensor(torch.randn(100, 256).cuda()))
        assert F8.CALLS["fallback"] == n0["fallback"] + 1
    finally:
        paddle.set_device(prev)
