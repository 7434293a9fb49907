"""OCP Microscaling (MX) inference linear on the gfx950 block-scaled MFMA (csrc/kernels/mx.hip).

Formats (the layout is public; the kernels and the torch code below implement the same rule):

* a tensor ``[R, K]`` is quantised along K in blocks of 32 (``K % 32 == 0``);
* ``scales``: ``uint8 [R, K / 32]`` row-major, an E8M0 exponent byte ``e`` with value ``2^(e - 127)``;
* ``"mxfp4"`` elements: e2m1 (0, 0.5, 1, 1.5, 2, 3, 4, 6 and their negatives; code = sign << 3 | index), packed two
  per byte, ``uint8 [R, K / 2]``: element ``2i`` is the low nibble of byte ``i``, element ``2i + 1`` the high nibble
  (the order the MFMA consumes);
* ``"mxfp8"`` elements: e4m3fn ``[R, K]`` (``torch.float8_e4m3fn``; a ``uint8`` view is accepted wherever one is read);
* rule (OCP MX v1.0) per block: ``amax = max|x|``; ``e = clamp(floor(log2 amax) - emax + 127, 0, 254)`` with
  ``emax`` 2 (e2m1) / 8 (e4m3); elements are ``x * 2^(127 - e)`` rounded to nearest even and saturated to +-6 /
  +-448; ``amax == 0`` gives ``e = 127`` and zero elements. An element keeps the sign bit of ``x``. Inputs are finite.

Inference only: no autograd. Every scale stays on the device (nothing here reads a device value on the host), so the
path can be captured in a hipGraph. Weights are mxfp4 stored K-major ``[out, in / 2]``; activations are quantised to
mxfp8 or mxfp4 just before the GEMM."""
from __future__ import annotations

import torch

from . import _loader as L

FMT_CODE = {"mxfp8": 0, "mxfp4": 4}  # the MFMA's format codes, which the launchers take
_EMAX = {"mxfp8": 8, "mxfp4": 2}
_OUT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
_FP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)

CALLS = {"hip": 0, "fallback": 0}  # which path gemm_mx took


def _check_fmt(fmt):
    if fmt not in FMT_CODE:
        raise ValueError(f"MX format must be 'mxfp4' or 'mxfp8', got {fmt!r}")


def _pow2(exp_field):
    """2^(exp_field - 127) in fp32 from the biased exponent (0 is the denormal 2^-127)."""
    bits = torch.where(exp_field == 0, torch.full_like(exp_field, 0x00400000), exp_field << 23)
    return bits.to(torch.int32).view(torch.float32)


def _quantize_torch(x2, fmt):
    R, K = x2.shape
    blk = x2.float().reshape(R, K // 32, 32)
    amax = blk.abs().amax(-1)
    # the fp32 exponent field is floor(log2 amax) + 127 (0 for a denormal, which clamps to 0 like its true value)
    e = ((amax.view(torch.int32) >> 23) - _EMAX[fmt]).clamp(0, 254)
    e = torch.where(amax == 0, torch.full_like(e, 127), e)
    v = blk * _pow2(254 - e).unsqueeze(-1)  # x * 2^(127 - e): exact
    if fmt == "mxfp8":
        q = v.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).reshape(R, K)  # round to nearest even
    else:
        a = v.abs().clamp(max=8.0)
        step = torch.where(a < 2, 0.5, torch.where(a < 4, 1.0, 2.0))  # spacing of e2m1 in [0, 2), [2, 4), [4, 6]
        r = (torch.round(a / step) * step).clamp(max=6.0)             # torch.round: half to even
        mag = torch.where(r < 2, r * 2, torch.where(r < 4, r + 2, r / 2 + 4)).to(torch.uint8)
        code = (mag | (torch.signbit(v).to(torch.uint8) << 3)).reshape(R, K)
        q = code[:, 0::2] | (code[:, 1::2] << 4)
    return q.contiguous(), e.to(torch.uint8)


def quantize_mx(x, fmt):
    """(q, scales) of ``x [..., K]`` viewed as ``[R, K]`` (K % 32 == 0): see the module docstring. On the device one
    pass of pa_mx_quant; the same rule in torch for CPU tensors."""
    _check_fmt(fmt)
    K = x.shape[-1]
    if K % 32 != 0:
        raise ValueError(f"quantize_mx: the last dimension ({K}) must be a multiple of 32")
    x2 = x.detach().reshape(-1, K)
    R = x2.shape[0]
    if L.hip_enabled_for(x2) and L.has("pa_mx_quant") and R > 0:
        if x2.dtype not in L._DT:
            x2 = x2.float()
        x2 = x2.contiguous()
        q = torch.empty(R, K // 2 if fmt == "mxfp4" else K, dtype=torch.uint8, device=x.device)
        s = torch.empty(R, K // 32, dtype=torch.uint8, device=x.device)
        L.call("pa_mx_quant", L.ptr(x2), L.ptr(q), L.ptr(s), R, K, L.dcode(x2), FMT_CODE[fmt], L.stream_ptr())
        return (q.view(torch.float8_e4m3fn) if fmt == "mxfp8" else q), s
    return _quantize_torch(x2, fmt)


def dequantize_mx(q, scales, fmt, dtype=torch.float32):
    """The values ``[R, K]`` that (q, scales) stand for, in ``dtype`` (exact in bf16 and wider: an element has at most
    4 significant bits and the scale is a power of two)."""
    _check_fmt(fmt)
    R, nb = scales.shape
    wide = torch.float64 if dtype == torch.float64 else torch.float32
    if fmt == "mxfp8":
        v = (q if q.dtype == torch.float8_e4m3fn else q.view(torch.float8_e4m3fn)).to(wide)
    else:
        lut = torch.tensor(_FP4_VALUES + tuple(-f for f in _FP4_VALUES), dtype=wide, device=q.device)
        codes = torch.stack([q & 15, q >> 4], dim=-1).reshape(R, nb * 32)
        v = lut[codes.long()]
    v = v.reshape(R, nb, 32) * _pow2(scales.to(torch.int32)).to(wide).unsqueeze(-1)
    return v.reshape(R, nb * 32).to(dtype)


def small_m_splits(M, N, K):
    """K splits the small-M kernel is launched with by default (pa_gemm_mx_small_m_splits)."""
    return int(L.lib().pa_gemm_mx_small_m_splits(M, N, K))


def _u8(t):
    return t if t.dtype == torch.uint8 else t.view(torch.uint8)


def gemm_mx(a_q, a_s, a_fmt, b_q, b_s, bias=None, out_dtype=torch.bfloat16, splits=None):
    """C [M, N] = A [M, K] . B [N, K]^T (+ bias): A in ``a_fmt`` ("mxfp8" / "mxfp4"), B mxfp4, both K-major with their
    scales. M <= 64 (and N % 16 == 0) runs pa_gemm_mx_small_m with ``splits`` K splits (None: the kernel's helper),
    other shapes with K % 128 == 0 and N % 4 == 0 the tiled pa_gemm_mx. What the kernels do not take (K % 128, N,
    non-contiguous operands, CPU tensors) multiplies the dequantised operands instead — on the device with the bf16
    linear, on the CPU in fp32 — and counts in CALLS["fallback"]."""
    _check_fmt(a_fmt)
    M, N, K = a_q.shape[0], b_q.shape[0], a_s.shape[1] * 32
    if b_s.shape[1] * 32 != K or b_q.shape[1] * 2 != K or a_q.shape[1] * (2 if a_fmt == "mxfp4" else 1) != K:
        raise ValueError("gemm_mx: operand and scale shapes disagree on K")
    ok = (L.hip_enabled_for(a_q) and L.has("pa_gemm_mx") and K % 128 == 0 and N % 4 == 0 and M > 0
          and out_dtype in _OUT and all(t.is_contiguous() for t in (a_q, a_s, b_q, b_s)))
    if not ok:
        CALLS["fallback"] += 1
        if a_q.is_cuda:
            from .linear import fused_linear
            x = dequantize_mx(a_q, a_s, a_fmt, torch.bfloat16)
            w = dequantize_mx(b_q, b_s, "mxfp4", torch.bfloat16)
            return fused_linear(x, w.t(), None if bias is None else bias.to(torch.bfloat16)).to(out_dtype)
        y = dequantize_mx(a_q, a_s, a_fmt) @ dequantize_mx(b_q, b_s, "mxfp4").t()
        return (y if bias is None else y + bias.float()).to(out_dtype)
    CALLS["hip"] += 1
    out = torch.empty(M, N, dtype=out_dtype, device=a_q.device)
    bias_f = None if bias is None else bias.detach().float().contiguous()
    args = (L.ptr(_u8(a_q)), L.ptr(a_s), L.ptr(b_q), L.ptr(b_s), L.ptr(out), L.ptr(bias_f))
    if M <= 64 and N % 16 == 0:
        if splits is None:
            splits = small_m_splits(M, N, K)
        ws = torch.empty(splits * M * N, dtype=torch.float32, device=a_q.device) if splits > 1 else None
        L.call("pa_gemm_mx_small_m", *args, L.ptr(ws), M, N, K, FMT_CODE[a_fmt], _OUT[out_dtype], int(splits),
               L.stream_ptr())
    else:
        L.call("pa_gemm_mx", *args, M, N, K, FMT_CODE[a_fmt], _OUT[out_dtype], L.stream_ptr())
    return out


def pad_k(x, K):
    """x [..., k] zero-padded along the last dimension to K (zeros leave every block's amax, so its scale, alone)."""
    return x if x.shape[-1] == K else torch.nn.functional.pad(x, (0, K - x.shape[-1]))


def quantize_weight(w_kn):
    """(w_q, w_s) of a linear's weight ``[in, out]``: the K-major mxfp4 image ``[out, in32 / 2]`` and its scales
    ``[out, in32 / 32]``, in32 = ``in`` rounded up to a multiple of 32 (zero padded), quantised where the weight is."""
    w_nk = w_kn.detach().t()
    return quantize_mx(pad_k(w_nk, -(-w_nk.shape[1] // 32) * 32).contiguous(), "mxfp4")


def mx_linear(x, w_q, w_s, bias=None, act_fmt="mxfp8"):
    """y = x @ W + bias with W given as quantize_weight's (w_q, w_s): x is flattened to rows, zero-padded to the
    weight's K when the layer's ``in`` is not a multiple of 32, quantised to ``act_fmt`` and multiplied by gemm_mx.
    The output has x's dtype (bf16 for other than fp32 / fp16 / bf16). Inference only."""
    _check_fmt(act_fmt)
    if torch.is_grad_enabled() and x.requires_grad:  # the weight is codes and a layer's bias a constant here
        raise RuntimeError("mx_linear is inference-only (no backward): call it under no_grad() or detach its inputs")
    K, N = w_s.shape[1] * 32, w_q.shape[0]
    if not K - 32 < x.shape[-1] <= K:
        raise ValueError(f"mx_linear: input features ({x.shape[-1]}) do not match the weight's ({K} after padding)")
    x2 = pad_k(x.detach().reshape(-1, x.shape[-1]), K)
    a_q, a_s = quantize_mx(x2, act_fmt)
    y = gemm_mx(a_q, a_s, act_fmt, w_q, w_s, None if bias is None else bias.detach(),
                x.dtype if x.dtype in _OUT else torch.bfloat16)
    return y.view(*x.shape[:-1], N)
