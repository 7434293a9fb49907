"""MX (block-scaled fp4 / fp8) formats off the device: the torch definition of quantize_mx / dequantize_mx on
hand-written blocks, mx_linear against dequantise-then-matmul, and MXFP4Linear's state_dict."""
import pytest
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.incubate import nn as INN
from paddlepaddle_amd.ops import mx as MX


def _rows(*rows):
    x = torch.zeros(len(rows), 32)
    for r, vals in enumerate(rows):
        x[r, :len(vals)] = torch.tensor(vals)
    return x


# one 32-block per row: ties, a saturating amax, zeros, a power-of-two amax
_X = _rows([4.0, 2.5, 3.5, 0.25, 0.75, 1.25, 1.75, -2.5, 2.125], [7.9, -3.0], [], [2.0 ** -3, 3 * 2.0 ** -5])


@pytest.mark.parametrize("fmt,scales,want", [
    # e2m1 at scale 1: midpoints go to the even code (2.5 -> 2, 3.5 -> 4, 0.25 -> 0, 0.75 -> 1, ...); 7.9 saturates at 6
    ("mxfp4", [127, 127, 127, 122], _rows([4, 2, 4, 0, 1, 1, 2, -2, 2], [6, -3], [], [2.0 ** -3, 3 * 2.0 ** -5])),
    # e4m3 at 2^-6: row 0 is exact but 2.125 (136 / 64, midway 128 | 144 -> 128); 7.9 * 64 saturates at 448
    ("mxfp8", [121, 121, 127, 116], _rows([4, 2.5, 3.5, 0.25, 0.75, 1.25, 1.75, -2.5, 2], [7, -3], [],
                                          [2.0 ** -3, 3 * 2.0 ** -5])),
])
def test_quantize_reference_hand_blocks(fmt, scales, want):
    q, s = MX.quantize_mx(_X, fmt)
    assert s.dtype == torch.uint8 and s.flatten().tolist() == scales
    assert torch.equal(MX.dequantize_mx(q, s, fmt), want)
    if fmt == "mxfp4":  # element 2i in the low nibble: 4.0 (code 6) then 2.0 (code 4); -2.0 (code 12) then 2.0
        assert q.dtype == torch.uint8 and q.shape == (4, 16)
        assert q[0, 0].item() == 6 | (4 << 4) and q[0, 3].item() == 4 | (12 << 4) and not q[2].any()
    else:
        assert q.dtype == torch.float8_e4m3fn and q.shape == (4, 32)


@pytest.mark.parametrize("K,act_fmt", [(96, "mxfp8"), (96, "mxfp4"), (520, "mxfp8")])
def test_mx_linear_cpu_is_dequantise_then_matmul(K, act_fmt):
    g = torch.Generator().manual_seed(1)
    x, w, b = torch.randn(2, 5, K, generator=g), torch.randn(K, 24, generator=g) / K ** 0.5, torch.randn(24, generator=g)
    w_q, w_s = MX.quantize_weight(w)
    K32 = -(-K // 32) * 32
    assert w_q.shape == (24, K32 // 2) and w_s.shape == (24, K32 // 32)
    n0 = MX.CALLS["fallback"]
    y = MX.mx_linear(x, w_q, w_s, b, act_fmt)
    assert y.shape == (2, 5, 24) and y.dtype == torch.float32 and MX.CALLS["fallback"] == n0 + 1
    xq = MX.dequantize_mx(*MX.quantize_mx(MX.pad_k(x.reshape(10, K), K32), act_fmt), act_fmt)
    ref = xq @ MX.dequantize_mx(w_q, w_s, "mxfp4").t() + b
    torch.testing.assert_close(y.reshape(10, 24), ref, rtol=1e-6, atol=1e-6)
    # the format's own error stays in the expected range (e2m1 weights: about a tenth)
    full = x.reshape(10, K) @ w + b
    assert 0.01 < ((y.reshape(10, 24) - full).norm() / full.norm()).item() < 0.25
    with pytest.raises(RuntimeError, match="inference-only"):
        MX.mx_linear(x.clone().requires_grad_(), w_q, w_s, b, act_fmt)
    with torch.no_grad():
        MX.mx_linear(x.clone().requires_grad_(), w_q, w_s, b, act_fmt)


def test_mxfp4_linear_state_dict_round_trip_cpu():
    base = paddle.nn.Linear(64, 48)
    lin = INN.MXFP4Linear.from_linear(base, act_format="mxfp4")
    sd = lin.state_dict()
    assert {"w_q", "w_s", "bias"} <= set(sd) and sd["w_q"]._t.dtype == torch.uint8 and list(sd["w_s"].shape) == [48, 2]
    assert lin.bias is base.bias and "weight" not in sd
    new = INN.MXFP4Linear(64, 48, act_format="mxfp4")
    missing, unexpected = new.set_state_dict(dict(sd))
    assert not missing and not unexpected
    x = paddle.to_tensor(torch.randn(3, 64))
    assert torch.equal(new(x)._t, lin(x)._t) and new(x)._t.abs().sum() > 0
