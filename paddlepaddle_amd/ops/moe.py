"""MoE building blocks on the device: token routing and the grouped (all-experts) linear layer.

Reference: paddle/phi/kernels/fusion/cutlass/fused_moe_kernel.cu, python/paddle/incubate/nn/functional/
fused_moe.py:20, python/paddle/incubate/distributed/models/moe/moe_layer.py.

``route(eid, E)`` turns the expert id of every (token, slot) entry into per-expert offsets and a stable
permutation (csrc/kernels/grouped_gemm.hip pa_moe_route — two small kernels, no host sync).
``grouped_linear(x, w, offs, bias)`` computes y[rows of e] = x[rows of e] . w[e] (+ bias[e]) for every expert
in one launch and has a backward made of the same grouped kernel (dX = dY . W_e^T, dW_e = X_e^T . dY_e);
bias gradients are per-expert segment sums. Everything is shape-static, so the MoE layer can be captured
in a hipGraph. On CPU (and for non-bf16 inputs) the same math runs per expert with torch.
"""
from __future__ import annotations

import torch

from . import _loader as L
from . import mx as MX

_ZERO = {}


def _zero_page(dev):
    z = _ZERO.get(dev)
    if z is None:
        z = _ZERO[dev] = torch.zeros(64, dtype=torch.uint8, device=dev)
    return z


def _hip(t):
    return L.hip_enabled_for(t) and L.has("pa_grouped_gemm")


def route(eid, num_experts):
    """eid [n] int (negative = dropped entry) -> (offs [E + 1] int32, perm [n] int64 whose first offs[E]
    entries list the kept entries grouped by expert, in entry order)."""
    eid = eid.reshape(-1)
    n = eid.numel()
    dev = eid.device
    if L.hip_enabled_for(eid) and L.has("pa_moe_route") and n > 0:
        e32 = eid.to(torch.int32).contiguous()
        counts = torch.empty(num_experts, dtype=torch.int32, device=dev)
        offs = torch.empty(num_experts + 1, dtype=torch.int32, device=dev)
        perm = torch.zeros(n, dtype=torch.int32, device=dev)
        L.call("pa_moe_route", L.ptr(e32), n, num_experts, L.ptr(counts), L.ptr(offs), L.ptr(perm), L.stream_ptr())
        return offs, perm.long()
    key = torch.where(eid < 0, torch.full_like(eid, num_experts), eid)
    perm = torch.argsort(key, stable=True)
    counts = torch.bincount(key, minlength=num_experts + 1)[:num_experts]
    offs = torch.zeros(num_experts + 1, dtype=torch.int32, device=dev)
    offs[1:] = torch.cumsum(counts, 0).to(torch.int32)
    return offs, perm


def expert_of_rows(offs, rows):
    """Expert index of every sorted row (rows past offs[-1] get E)."""
    r = torch.arange(rows, device=offs.device, dtype=torch.int32)
    return torch.searchsorted(offs[1:].contiguous(), r, right=True)


def _gg(mode, a, b, c, bias, offs, E, rows, M, N, K, lda, ldb, ldc, flags):
    L.call("pa_grouped_gemm", mode, L.ptr(a), L.ptr(b), L.ptr(c), L.ptr(bias), L.ptr(offs),
           L.ptr(_zero_page(a.device)), E, rows, M, N, K, lda, ldb, ldc, flags, L.stream_ptr())


def _fallback(x, w, offs, bias):
    out = x.new_zeros(x.shape[0], w.shape[2])
    o = offs.tolist()
    for e in range(w.shape[0]):
        s, t = o[e], o[e + 1]
        if t > s:
            y = x[s:t] @ w[e]
            if bias is not None:
                y = y + bias[e]
            out[s:t] = y
    return out


class _GroupedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, offs, bias):
        T, K = x.shape
        E, _, N = w.shape
        x, w = x.contiguous(), w.contiguous()
        b = bias.contiguous() if bias is not None else None
        y = torch.zeros(T, N, dtype=x.dtype, device=x.device)
        rows_alive = T  # rows past offs[E] are never written: zero them for a defined output
        _gg(0, x, w, y, b, offs, E, rows_alive, 0, N, K, K, N, N, 1 if b is not None else 0)
        ctx.save_for_backward(x, w, offs)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, offs = ctx.saved_tensors
        T, K = x.shape
        E, _, N = w.shape
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.zeros_like(x)
            _gg(1, dy, w, dx, None, offs, E, T, 0, K, N, N, N, K, 0)
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w)
            _gg(2, x, dy, dw, None, offs, E, T, K, N, 0, K, N, N, 0)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            eo = expert_of_rows(offs, T).long()
            db = torch.zeros(E + 1, N, dtype=torch.float32, device=dy.device)
            db.index_add_(0, eo, dy.float())
            db = db[:E].to(dy.dtype)
        return dx, dw, None, db


def grouped_linear(x, w, offs, bias=None):
    """x [T, K] rows sorted by expert (rows offs[e]:offs[e+1] -> expert e; rows past offs[E] give 0),
    w [E, K, N], bias [E, N] -> y [T, N]."""
    ok = (_hip(x) and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.shape[1] % 64 == 0
          and w.shape[2] % 64 == 0 and (bias is None or bias.dtype == torch.bfloat16))
    if not ok:
        return _fallback(x, w, offs, bias)
    y = _GroupedLinear.apply(x, w, offs.to(torch.int32).contiguous(), bias)
    return y


# ------------------------------------------------------------------------------------- decode (T <= 64)
# csrc/kernels/moe_decode.hip: gate + routing in one workgroup (pa_moe_decode_plan), then up projection with
# SwiGLU, K-split down projection and combine behind pa_moe_decode_ffn. Inference only.
DECODE_MAX_TOKENS, DECODE_MAX_EXPERTS, DECODE_MAX_TOPK = 64, 256, 8
# fused_moe takes the decode kernels up to this many tokens: measured ahead of the grouped path on every shape at
# 1 / 4 / 16 tokens; at 64 within +-6 % of it and behind on one shape (profiles/moe_decode.md)
DECODE_DISPATCH_TOKENS = 16
USE_DECODE = True  # False: fused_moe keeps the grouped path at every size (tools/bench_moe_decode.py's yardstick)


def _decode_plan_ok(logits, topk):
    return (logits.dim() == 2 and 1 <= logits.shape[0] <= DECODE_MAX_TOKENS
            and 1 <= logits.shape[1] <= DECODE_MAX_EXPERTS and 1 <= topk <= min(DECODE_MAX_TOPK, logits.shape[1])
            and L.hip_enabled_for(logits) and L.has("pa_moe_decode_plan"))


def decode_plan(logits, topk, norm=True):
    """Gate and routing of a decode step in one launch. logits [T, E] (T <= 64, E <= 256, topk <= min(8, E)) ->
    (val [T, topk] fp32, idx [T, topk] int32, offs [E + 1] int32, perm [n] int32 (sorted row -> entry, the stable
    order ``route`` gives), pos [n] int32 (entry -> sorted row), active [min(E, n)] int32 (the non-empty experts,
    ascending, -1 behind them), n_active [1] int32), n = T * topk: softmax in fp32, the topk largest (the lower
    expert index wins a tie), renormalised to sum 1 when ``norm``."""
    if not _decode_plan_ok(logits, topk):
        raise ValueError("decode_plan: needs a device tensor [T <= 64, E <= 256] and topk <= min(8, E)")
    if logits.dtype not in (torch.float32, torch.bfloat16):
        logits = logits.float()
    logits = logits.detach().contiguous()
    T, E = logits.shape
    n, slots = T * topk, min(E, T * topk)
    val = torch.empty(T, topk, dtype=torch.float32, device=logits.device)
    meta = torch.empty(3 * n + E + 1 + slots + 1, dtype=torch.int32, device=logits.device)
    idx, offs, perm, pos, active, n_active = meta.split([n, E + 1, n, n, slots, 1])
    L.call("pa_moe_decode_plan", L.ptr(logits), L.dcode(logits), T, E, topk, int(bool(norm)), L.ptr(val), L.ptr(idx),
           L.ptr(offs), L.ptr(perm), L.ptr(pos), L.ptr(active), L.ptr(n_active), L.stream_ptr())
    return val, idx.view(T, topk), offs, perm, pos, active, n_active


def decode_splits(n, E, d, f):
    """K splits the down projection of the decode FFN runs with by default (pa_moe_decode_splits)."""
    return int(L.lib().pa_moe_decode_splits(n, E, d, f))


def moe_decode_ffn(x, logits, w1, w2, b1=None, b2=None, topk=2, norm_topk_prob=True, splits=None):
    """SwiGLU expert FFN of a decode step: x [T, d], gate logits [T, E], w1 [E, d, 2f], w2 [E, f, d], b1 [E, 2f],
    b2 [E, d] -> [T, d] bf16, out[t] = sum_j val[t, j] (swiglu(x[t] w1[e] + b1[e]) w2[e] + b2[e]), e = idx[t, j].
    ``splits`` K splits of the down projection (None: decode_splits; must divide f / 64). Returns None when the
    shapes, dtypes or device are not the kernels' (T <= 64, E <= 256, topk <= min(8, E), d % 64 == f % 64 == 0,
    contiguous bf16 operands on the device): the caller keeps its own path."""
    bf = torch.bfloat16
    if x.dim() != 2 or logits.dim() != 2 or w1.dim() != 3 or w2.dim() != 3 or logits.shape[0] != x.shape[0]:
        return None
    (T, d), E, f = x.shape, w1.shape[0], w2.shape[1]
    ok = (_decode_plan_ok(logits, topk) and L.has("pa_moe_decode_ffn") and logits.shape[1] == E
          and tuple(w1.shape) == (E, d, 2 * f) and tuple(w2.shape) == (E, f, d) and d % 64 == 0 and f % 64 == 0
          and d > 0 and f > 0 and (b1 is None or tuple(b1.shape) == (E, 2 * f))
          and (b2 is None or tuple(b2.shape) == (E, d))
          and all(t is None or (t.dtype == bf and t.is_contiguous() and t.device == x.device)
                  for t in (x, w1, w2, b1, b2)))
    if not ok:
        return None
    n = T * topk
    if splits is None:
        splits = decode_splits(n, E, d, f)
    elif splits < 1 or (f // 64) % splits:
        raise ValueError(f"moe_decode_ffn: splits ({splits}) must divide f / 64 ({f // 64})")
    val, idx, offs, perm, pos, active, n_active = decode_plan(logits, topk, norm_topk_prob)
    h = torch.empty(n, f, dtype=bf, device=x.device)
    ws = torch.empty(splits, n, d, dtype=torch.float32, device=x.device)
    out = torch.empty(T, d, dtype=bf, device=x.device)
    L.call("pa_moe_decode_ffn", *(L.ptr(t.detach() if t is not None else None) for t in (x, w1, w2, b1, b2)),
           L.ptr(val), L.ptr(idx), L.ptr(offs), L.ptr(perm), L.ptr(pos), L.ptr(active), L.ptr(n_active), L.ptr(h),
           L.ptr(ws), L.ptr(out), T, E, topk, d, f, int(splits), L.stream_ptr())
    return out


# ------------------------------------------------------------------------------------- decode, MXFP4 experts
# The same plan and combine around two projections on the block-scaled MFMA (csrc/kernels/moe_decode.hip
# pa_moe_decode_up_mx / pa_moe_decode_down_mx): expert weights mxfp4, K-major per expert, activations mxfp8 at both
# projections (formats in ops/mx.py). Five launches: plan, quantise x, up, down, combine. Inference only.
CALLS = {"mx_fallback": 0}  # fused_moe(quant_method="mxfp4") calls that ran moe_ffn_mx_reference instead of the kernels


def quantize_experts_mx(w1, w2):
    """fused_moe's expert weights w1 [E, d, 2f], w2 [E, f, d] -> (w1_q [E, 2f, d / 2], w1_s [E, 2f, d / 32],
    w2_q [E, d, f / 2], w2_s [E, d, f / 32]) uint8: ``mx.quantize_weight(w[e])`` stacked over e (an expert at a time,
    so the transposed copy is one expert's), quantised where the weights are."""
    q1, s1 = zip(*(MX.quantize_weight(w1[e]) for e in range(w1.shape[0])))
    q2, s2 = zip(*(MX.quantize_weight(w2[e]) for e in range(w2.shape[0])))
    return torch.stack(q1), torch.stack(s1), torch.stack(q2), torch.stack(s2)


def moe_ffn_mx_reference(x, val, idx, w1_q, w1_s, w2_q, w2_s, b1=None, b2=None, dtype=torch.float32):
    """What the MXFP4 expert FFN computes, in plain torch with the arithmetic in ``dtype``, for any T, on CPU or device:
    x [T, d] is quantised to mxfp8 per row; entry (t, j) with e = idx[t, j] takes u = dq(xq[t]) . dq(w1_q[e])^T + b1[e],
    h = silu(value half) * gate half, h quantised to mxfp8 along f by the same rule, y = dq(hq) . dq(w2_q[e])^T + b2[e];
    out[t] = sum_j val[t, j] y. ``val`` / ``idx`` [T, topk] are the routing weights and experts. Returns [T, d] in
    ``dtype``. The CPU path and the fallback of fused_moe(quant_method="mxfp4")."""
    T, d = x.shape
    dq = lambda q, s, fmt: MX.dequantize_mx(q, s, fmt, dtype)
    xd = dq(*MX.quantize_mx(x, "mxfp8"), "mxfp8")
    out = torch.zeros(T, d, dtype=dtype, device=x.device)
    for e in torch.unique(idx).tolist():
        t, j = torch.nonzero(idx == e, as_tuple=True)
        u = xd[t] @ dq(w1_q[e], w1_s[e], "mxfp4").t()
        if b1 is not None:
            u = u + b1[e].to(dtype)
        a, g = u.chunk(2, -1)
        y = dq(*MX.quantize_mx(torch.nn.functional.silu(a) * g, "mxfp8"), "mxfp8") @ dq(w2_q[e], w2_s[e], "mxfp4").t()
        if b2 is not None:
            y = y + b2[e].to(dtype)
        out.index_add_(0, t, val[t, j].to(dtype).unsqueeze(1) * y)
    return out


def decode_splits_mx(n, E, d, f):
    """K splits the MXFP4 down projection runs with by default (pa_moe_decode_mx_splits; it counts 128-k steps)."""
    return int(L.lib().pa_moe_decode_mx_splits(n, E, d, f))


def _decode_up_mx(x_q, x_s, w1_q, w1_s, b1, plan, topk):
    """Up projection + SwiGLU + quantisation on a ``decode_plan``: x_q [T, d] e4m3fn / x_s [T, d / 32] -> (h_q [n, f]
    uint8 e4m3fn codes, h_s [n, f / 32]) in the plan's sorted row order."""
    _, _, offs, perm, _, active, n_active = plan
    (T, d), (E, f2) = x_q.shape, w1_q.shape[:2]
    n, f = T * topk, f2 // 2
    h_q = torch.empty(n, f, dtype=torch.uint8, device=x_q.device)
    h_s = torch.empty(n, f // 32, dtype=torch.uint8, device=x_q.device)
    L.call("pa_moe_decode_up_mx", L.ptr(MX._u8(x_q)), L.ptr(x_s), L.ptr(w1_q), L.ptr(w1_s), L.ptr(b1), L.ptr(offs),
           L.ptr(perm), L.ptr(active), L.ptr(n_active), L.ptr(h_q), L.ptr(h_s), T, E, topk, d, f, L.stream_ptr())
    return h_q, h_s


def _decode_down_mx(h_q, h_s, w2_q, w2_s, b2, plan, topk, splits=None):
    """Down projection (K = f split ``splits`` ways, None: decode_splits_mx) and combine on a ``decode_plan``:
    h_q [n, f] / h_s [n, f / 32] in sorted row order -> out [T, d] bf16."""
    val, idx, offs, _, pos, active, n_active = plan
    (n, f), (E, d) = h_q.shape, w2_q.shape[:2]
    T, steps = n // topk, f // 128
    if splits is None:
        splits = decode_splits_mx(n, E, d, f)
    elif not 1 <= splits <= steps or -(-steps // (-(-steps // splits))) != splits:  # ceil(steps / per) == splits
        raise ValueError(f"_decode_down_mx: splits ({splits}) must split {steps} k-steps with no empty split")
    ws = torch.empty(splits, n, d, dtype=torch.float32, device=h_q.device)
    out = torch.empty(T, d, dtype=torch.bfloat16, device=h_q.device)
    L.call("pa_moe_decode_down_mx", L.ptr(MX._u8(h_q)), L.ptr(h_s), L.ptr(w2_q), L.ptr(w2_s), L.ptr(b2), L.ptr(val),
           L.ptr(idx), L.ptr(offs), L.ptr(pos), L.ptr(active), L.ptr(n_active), L.ptr(ws), L.ptr(out), T, E, topk, d,
           f, int(splits), L.stream_ptr())
    return out


def moe_decode_ffn_mx(x, logits, w1_q, w1_s, w2_q, w2_s, b1=None, b2=None, topk=2, norm_topk_prob=True, splits=None):
    """SwiGLU expert FFN of a decode step over MXFP4 expert weights (``quantize_experts_mx``'s tensors): x [T, d] bf16,
    gate logits [T, E], b1 [E, 2f] / b2 [E, d] bf16 -> [T, d] bf16, the chain of ``moe_ffn_mx_reference`` on the plan's
    val / idx. ``splits``: K splits of the down projection (None: decode_splits_mx). Returns None when the shapes,
    dtypes or device are not the kernels' (T <= 64, E <= 256, topk <= min(8, E), d % 128 == f % 128 == 0, contiguous
    operands on the device): the caller keeps its own path."""
    u8, bf = torch.uint8, torch.bfloat16
    if x.dim() != 2 or logits.dim() != 2 or w1_q.dim() != 3 or w2_q.dim() != 3 or logits.shape[0] != x.shape[0]:
        return None
    (T, d), E, f = x.shape, w1_q.shape[0], w1_q.shape[1] // 2
    ok = (_decode_plan_ok(logits, topk) and L.has("pa_moe_decode_up_mx") and L.has("pa_mx_quant")
          and logits.shape[1] == E and d > 0 and f > 0 and d % 128 == 0 and f % 128 == 0
          and tuple(w1_q.shape) == (E, 2 * f, d // 2) and tuple(w1_s.shape) == (E, 2 * f, d // 32)
          and tuple(w2_q.shape) == (E, d, f // 2) and tuple(w2_s.shape) == (E, d, f // 32)
          and (b1 is None or tuple(b1.shape) == (E, 2 * f)) and (b2 is None or tuple(b2.shape) == (E, d))
          and all(t.dtype == u8 for t in (w1_q, w1_s, w2_q, w2_s))
          and all(t is None or t.dtype == bf for t in (x, b1, b2))
          and all(t is None or (t.is_contiguous() and t.device == x.device)
                  for t in (x, w1_q, w1_s, w2_q, w2_s, b1, b2)))
    if not ok:
        return None
    det = lambda t: None if t is None else t.detach()
    plan = decode_plan(logits, topk, norm_topk_prob)
    x_q, x_s = MX.quantize_mx(x, "mxfp8")
    h_q, h_s = _decode_up_mx(x_q, x_s, w1_q, w1_s, det(b1), plan, topk)
    return _decode_down_mx(h_q, h_s, w2_q, w2_s, det(b2), plan, topk, splits)


# ------------------------------------------------------------------------------------- weight-only int8 / int4 experts
# The reference's quant_method="weight_only_int8" / "weight_only_int4": expert weights in nn.quant.weight_quantize's
# layout, an expert at a time, per-channel scales (group_size = -1). bits 8: w1_q [E, 2f, d], w2_q [E, d, f] int8;
# bits 4: w1_q [E, f, d], w2_q [E, d / 2, f] (channels 2j / 2j + 1 in the low / high nibble, stored + 8: all 16 codes
# decode, code 0 is -8); w1_s [E, 2f], w2_s [E, d] fp32. Up to 64 tokens: the plan and the combine of the decode path
# around csrc/kernels/moe_decode_wo.hip's two projections (four launches, hipGraph-safe). More: ``moe_grouped_ffn_wo``.
# Inference only.
CALLS["wo_fallback"] = 0  # fused_moe(quant_method="weight_only_*") calls that ran moe_ffn_wo_reference
# fused_moe runs the weight-only decode kernels up to this many tokens, dequantise + grouped above and
# ``moe_prefill_ffn_wo`` from GROUPED_WO_MIN_TOKENS (profiles/moe_decode_wo.md)
WO_DECODE_DISPATCH_TOKENS = DECODE_MAX_TOKENS


def quantize_experts_wo(w1, w2, algo="weight_only_int8"):
    """fused_moe's expert weights w1 [E, d, 2f], w2 [E, f, d] -> (w1_q, w1_s, w2_q, w2_s) in the layout above:
    ``nn.quant.weight_quantize(w[e], algo)`` stacked over e, the scales as fp32."""
    from ..nn.quant import weight_quantize
    if algo not in ("weight_only_int8", "weight_only_int4"):
        raise ValueError(f"quantize_experts_wo: algo must be weight_only_int8 or weight_only_int4, got {algo!r}")
    q1, s1 = zip(*((q._t, s._t.float()) for q, s in (weight_quantize(w1[e], algo) for e in range(w1.shape[0]))))
    q2, s2 = zip(*((q._t, s._t.float()) for q, s in (weight_quantize(w2[e], algo) for e in range(w2.shape[0]))))
    return torch.stack(q1), torch.stack(s1), torch.stack(q2), torch.stack(s2)


def _dequant_wo(q, s, bits, dtype):
    """One expert's codes [N, K] (bits 4: pair-rows [N / 2, K]) and scales [N] -> [N, K] in ``dtype``."""
    if bits == 4:
        u = q.view(torch.uint8)
        q = torch.stack([u & 0xF, u >> 4], 1).reshape(-1, q.shape[-1]).to(torch.int16) - 8  # rows 2j (low), 2j + 1
    return q.to(dtype) * s.to(dtype)[:, None]


def moe_ffn_wo_reference(x, val, idx, w1_q, w1_s, w2_q, w2_s, b1=None, b2=None, bits=8, dtype=torch.float32):
    """What the weight-only expert FFN computes, in plain torch with the arithmetic in ``dtype``, for any T, on CPU or
    device: entry (t, j) with e = idx[t, j] takes u = x[t] . dq(w1_q[e])^T + b1[e], h = silu(value half) * gate half
    rounded to bf16 (the kernels keep h in bf16), y = h . dq(w2_q[e])^T + b2[e]; out[t] = sum_j val[t, j] y. Returns
    [T, d] in ``dtype``. The CPU path and the fallback of fused_moe(quant_method="weight_only_int8" | "..._int4")."""
    T, d = x.shape
    xd = x.to(dtype)
    out = torch.zeros(T, d, dtype=dtype, device=x.device)
    for e in torch.unique(idx).tolist():
        t, j = torch.nonzero(idx == e, as_tuple=True)
        u = xd[t] @ _dequant_wo(w1_q[e], w1_s[e], bits, dtype).t()
        if b1 is not None:
            u = u + b1[e].to(dtype)
        a, g = u.chunk(2, -1)
        y = (torch.nn.functional.silu(a) * g).bfloat16().to(dtype) @ _dequant_wo(w2_q[e], w2_s[e], bits, dtype).t()
        if b2 is not None:
            y = y + b2[e].to(dtype)
        out.index_add_(0, t, val[t, j].to(dtype).unsqueeze(1) * y)
    return out


def decode_splits_wo(n, E, d, f, bits):
    """K splits the weight-only down projection runs with by default (pa_moe_decode_wo_splits; it counts 64-chunks)."""
    return int(L.lib().pa_moe_decode_wo_splits(n, E, d, f, bits))


def _decode_up_wo(x, w1_q, w1_s, b1, plan, topk, bits):
    """Up projection + SwiGLU on a ``decode_plan``: x [T, d] bf16 -> h [n, f] bf16 in the plan's sorted row order."""
    _, _, offs, perm, _, active, n_active = plan
    (T, d), E, f = x.shape, w1_q.shape[0], w1_s.shape[1] // 2
    h = torch.empty(T * topk, f, dtype=torch.bfloat16, device=x.device)
    L.call("pa_moe_decode_up_wo", L.ptr(x), L.ptr(w1_q), L.ptr(w1_s), L.ptr(b1), L.ptr(offs), L.ptr(perm),
           L.ptr(active), L.ptr(n_active), L.ptr(h), T, E, topk, d, f, bits, L.stream_ptr())
    return h


def _decode_down_wo(h, w2_q, w2_s, b2, plan, topk, bits, splits=None):
    """Down projection (K = f split ``splits`` ways, None: decode_splits_wo) and combine on a ``decode_plan``:
    h [n, f] bf16 in sorted row order -> out [T, d] bf16."""
    val, idx, offs, _, pos, active, n_active = plan
    (n, f), (E, d) = h.shape, w2_s.shape
    T, chunks = n // topk, f // 64
    if splits is None:
        splits = decode_splits_wo(n, E, d, f, bits)
    elif not 1 <= splits <= chunks or -(-chunks // (-(-chunks // splits))) != splits:  # ceil(chunks / per) == splits
        raise ValueError(f"_decode_down_wo: splits ({splits}) must split {chunks} chunks with no empty split")
    ws = torch.empty(splits, n, d, dtype=torch.float32, device=h.device)
    out = torch.empty(T, d, dtype=torch.bfloat16, device=h.device)
    L.call("pa_moe_decode_down_wo", L.ptr(h), L.ptr(w2_q), L.ptr(w2_s), L.ptr(b2), L.ptr(val), L.ptr(idx), L.ptr(offs),
           L.ptr(pos), L.ptr(active), L.ptr(n_active), L.ptr(ws), L.ptr(out), T, E, topk, d, f, bits, int(splits),
           L.stream_ptr())
    return out


def _wo_operands_ok(x, logits, w1_q, w1_s, w2_q, w2_s, b1, b2, bits):
    """The operand checks the weight-only decode and grouped paths share; (E, d, f) or None."""
    bf = torch.bfloat16
    if (bits not in (8, 4) or x.dim() != 2 or logits.dim() != 2 or w1_q.dim() != 3 or w2_q.dim() != 3 or w1_s.dim() != 2
            or logits.shape[0] != x.shape[0]):
        return None
    (T, d), (E, f2) = x.shape, w1_s.shape
    f, pack = f2 // 2, 8 // bits
    ok = (L.hip_enabled_for(x) and logits.shape[1] == E and d > 0 and f > 0 and d % 64 == 0 and f % 64 == 0
          and f2 == 2 * f and tuple(w1_q.shape) == (E, 2 * f // pack, d) and tuple(w2_q.shape) == (E, d // pack, f)
          and tuple(w2_s.shape) == (E, d)
          and (b1 is None or tuple(b1.shape) == (E, 2 * f)) and (b2 is None or tuple(b2.shape) == (E, d))
          and all(t.dtype == torch.int8 for t in (w1_q, w2_q)) and all(t.dtype == torch.float32 for t in (w1_s, w2_s))
          and all(t is None or t.dtype == bf for t in (x, b1, b2))
          and all(t is None or (t.is_contiguous() and t.device == x.device)
                  for t in (x, w1_q, w1_s, w2_q, w2_s, b1, b2)))
    return (E, d, f) if ok else None


def moe_decode_ffn_wo(x, logits, w1_q, w1_s, w2_q, w2_s, b1=None, b2=None, topk=2, norm_topk_prob=True, bits=8,
                      splits=None):
    """SwiGLU expert FFN of a decode step over weight-only int8 / int4 expert weights (``quantize_experts_wo``'s
    tensors): x [T, d] bf16, gate logits [T, E], b1 [E, 2f] / b2 [E, d] bf16 -> [T, d] bf16, the chain of
    ``moe_ffn_wo_reference`` on the plan's val / idx. ``splits``: K splits of the down projection (None:
    decode_splits_wo). Returns None when the shapes, dtypes or device are not the kernels' (T <= 64, E <= 256,
    topk <= min(8, E), d % 64 == f % 64 == 0, int8 codes, fp32 scales, contiguous operands on the device): the caller
    keeps its own path."""
    if _wo_operands_ok(x, logits, w1_q, w1_s, w2_q, w2_s, b1, b2, bits) is None:
        return None
    if not (_decode_plan_ok(logits, topk) and L.has("pa_moe_decode_up_wo")):
        return None
    det = lambda t: None if t is None else t.detach()
    plan = decode_plan(logits, topk, norm_topk_prob)
    h = _decode_up_wo(x.detach(), w1_q, w1_s, det(b1), plan, topk, bits)
    return _decode_down_wo(h, w2_q, w2_s, det(b2), plan, topk, bits, splits)


def moe_grouped_ffn_wo(x, logits, w1_q, w1_s, w2_q, w2_s, b1=None, b2=None, topk=2, norm_topk_prob=True, bits=8):
    """The same FFN for any number of tokens with no kernel of its own: both weight stacks are dequantised to bf16 by
    pa_wo_dequant (an [E, N, K] stack with [E, N] scales is one [E N, K] matrix to it), pa_grouped_gemm multiplies the
    expert-sorted rows by the [E, N, K] images (its mode 1, which has no bias: the biases are added in torch) with
    ops.swiglu between the projections, and the token's experts are summed in fp32 in a fixed order. The transient
    images cost E * 2f * d * 2 bytes for w1 and half that for w2. Returns None when the operands are not the decode
    kernels' (apart from the token count)."""
    from . import quant as Q
    from .activation import swiglu
    shp = _wo_operands_ok(x, logits, w1_q, w1_s, w2_q, w2_s, b1, b2, bits)
    if shp is None or not (_hip(x) and L.has("pa_wo_dequant") and 1 <= topk <= logits.shape[1]):
        return None
    (E, d, f), T = shp, x.shape[0]
    n, dev = T * topk, x.device
    val, idx = torch.softmax(logits.detach().float(), -1).topk(topk, -1)
    if norm_topk_prob:
        val = val / val.sum(-1, keepdim=True)
    offs, perm = route(idx.reshape(-1), E)
    offs = offs.to(torch.int32).contiguous()
    pos = torch.empty(n, dtype=torch.long, device=dev)
    pos[perm] = torch.arange(n, device=dev)  # the inverse of perm: entry -> sorted row
    eo = expert_of_rows(offs, n).long()

    def project(rows, q, s, N, K, bias):
        img = Q.dequantize(q.view(-1, K), s.reshape(-1), bits, -1, K, E * N)  # [E N, K] = [E, N, K]
        y = torch.empty(n, N, dtype=torch.bfloat16, device=dev)
        _gg(1, rows, img, y, None, offs, E, n, 0, N, K, K, K, N, 0)
        return y if bias is None else y + bias.detach()[eo]

    u = project(x.detach()[perm // topk].contiguous(), w1_q, w1_s, 2 * f, d, b1)
    y = project(swiglu(u).contiguous(), w2_q, w2_s, d, f, b2)
    return (y[pos].float().view(T, topk, d) * val.unsqueeze(-1)).sum(1).to(torch.bfloat16)


# csrc/kernels/moe_grouped_wo.hip: the same FFN for any number of tokens as two grouped 128 x 256 GEMMs over the
# expert-sorted rows that read the codes themselves (pa_moe_grouped_up_wo gathers x by token and leaves h in bf16,
# pa_moe_grouped_down_wo ends in the decode path's combine): no bf16 image of the weights. Gate math in torch on the
# device, ``route`` for the sort, no host read. fused_moe(quant_method="weight_only_*") takes this path from
# GROUPED_WO_MIN_TOKENS tokens up. The decode kernels end at 64 tokens, so 65-127 tokens still run moe_grouped_ffn_wo
# (dequantise + grouped): the existing weight-only decode test pins a 65-token call to pa_wo_dequant == 2 and
# pa_grouped_gemm == 2, and this path is valid for any T >= 1, so a later change can close the gap by lowering the
# constant to 65 (profiles/moe_prefill_wo.md has the 128-token measurement behind the value).
GROUPED_WO_MIN_TOKENS = 128
GROUPED_WO_MAX_TOKENS = 65535


def moe_prefill_ffn_wo(x, logits, w1_q, w1_s, w2_q, w2_s, b1=None, b2=None, topk=2, norm_topk_prob=True, bits=8):
    """SwiGLU expert FFN over weight-only int8 / int4 expert weights (``quantize_experts_wo``'s tensors) for any number
    of tokens: x [T, d] bf16, gate logits [T, E], b1 [E, 2f] / b2 [E, d] bf16 -> [T, d] bf16, the chain of
    ``moe_ffn_wo_reference`` on val / idx = the top-k of the fp32 softmax (renormalised when ``norm_topk_prob``).
    Returns None when the shapes, dtypes or device are not the kernels' (1 <= T <= 65535, E <= 256, topk <= min(8, E),
    d % 64 == f % 64 == 0, int8 codes, fp32 scales, contiguous operands on the device): the caller keeps its own
    path."""
    shp = _wo_operands_ok(x, logits, w1_q, w1_s, w2_q, w2_s, b1, b2, bits)
    if shp is None:
        return None
    (E, d, f), T = shp, x.shape[0]
    if not (L.has("pa_moe_grouped_up_wo") and L.has("pa_moe_route") and 1 <= T <= GROUPED_WO_MAX_TOKENS
            and 1 <= E <= DECODE_MAX_EXPERTS and 1 <= topk <= min(DECODE_MAX_TOPK, E)):
        return None
    n, dev = T * topk, x.device
    det = lambda t: None if t is None else t.detach()
    val, idx = torch.softmax(logits.detach().float(), -1).topk(topk, -1)
    if norm_topk_prob:
        val = val / val.sum(-1, keepdim=True)
    val, idx = val.contiguous(), idx.to(torch.int32).contiguous()
    offs, perm = route(idx.reshape(-1), E)
    pos = torch.empty(n, dtype=torch.int32, device=dev)
    pos[perm] = torch.arange(n, dtype=torch.int32, device=dev)  # the inverse of perm: entry -> sorted row
    perm = perm.to(torch.int32)
    h = torch.empty(n, f, dtype=torch.bfloat16, device=dev)
    L.call("pa_moe_grouped_up_wo", L.ptr(x.detach()), L.ptr(w1_q), L.ptr(w1_s), L.ptr(det(b1)), L.ptr(offs),
           L.ptr(perm), L.ptr(h), T, E, topk, d, f, bits, L.stream_ptr())
    return _prefill_down_wo(h, w2_q, w2_s, det(b2), val, idx, offs, pos, bits)


def _prefill_down_wo(h, w2_q, w2_s, b2, val, idx, offs, pos, bits):
    """Down projection and combine on expert-sorted rows: h [n, f] bf16, val [T, topk] fp32, idx [T, topk] /
    offs [E + 1] / pos [n] int32 -> out [T, d] bf16 (y [n, d] fp32 of workspace, each row written once)."""
    (n, f), (E, d), (T, topk) = h.shape, w2_s.shape, val.shape
    y = torch.empty(n, d, dtype=torch.float32, device=h.device)
    out = torch.empty(T, d, dtype=torch.bfloat16, device=h.device)
    L.call("pa_moe_grouped_down_wo", L.ptr(h), L.ptr(w2_q), L.ptr(w2_s), L.ptr(b2), L.ptr(val), L.ptr(idx),
           L.ptr(offs), L.ptr(pos), L.ptr(y), L.ptr(out), T, E, topk, d, f, bits, L.stream_ptr())
    return out


# ------------------------------------------------------------------------------------- prefill, MXFP4 experts
# csrc/kernels/moe_grouped_mx.hip: the same FFN for any number of tokens as two grouped 128 x 256 block-scaled GEMMs
# over the expert-sorted rows (pa_moe_grouped_up_mx gathers x_q by token and leaves h as mxfp8, pa_moe_grouped_down_mx
# ends in the decode path's combine). Gate math in torch on the device, ``route`` for the sort, no host read.
# fused_moe(quant_method="mxfp4") takes this path from GROUPED_MX_MIN_TOKENS tokens up. The decode kernels end at
# DECODE_MAX_TOKENS = 64, so 65-127 tokens still run moe_ffn_mx_reference: the existing MX decode test pins a 65-token
# call to that fallback, and this path is valid for any T >= 1, so a later change can close the gap by lowering the
# constant to DECODE_MAX_TOKENS + 1 (profiles/moe_prefill_mx.md has the 128-token measurement behind the value).
GROUPED_MX_MIN_TOKENS = 128
GROUPED_MX_MAX_TOKENS = 65535


def moe_grouped_ffn_mx(x, logits, w1_q, w1_s, w2_q, w2_s, b1=None, b2=None, topk=2, norm_topk_prob=True):
    """SwiGLU expert FFN over MXFP4 expert weights (``quantize_experts_mx``'s tensors) for any number of tokens:
    x [T, d] bf16, gate logits [T, E], b1 [E, 2f] / b2 [E, d] bf16 -> [T, d] bf16, the chain of
    ``moe_ffn_mx_reference`` on val / idx = the top-k of the fp32 softmax (renormalised when ``norm_topk_prob``).
    Returns None when the shapes, dtypes or device are not the kernels' (1 <= T <= 65535, E <= 256, topk <= min(8, E),
    d % 128 == f % 128 == 0, d f < 2^31, T topk max(d, f) < 2^36, contiguous operands on the device): the caller keeps
    its own path."""
    u8, bf = torch.uint8, torch.bfloat16
    if x.dim() != 2 or logits.dim() != 2 or w1_q.dim() != 3 or w2_q.dim() != 3 or logits.shape[0] != x.shape[0]:
        return None
    (T, d), E, f = x.shape, w1_q.shape[0], w1_q.shape[1] // 2
    n = T * topk
    ok = (L.hip_enabled_for(x) and L.has("pa_moe_grouped_up_mx") and L.has("pa_mx_quant") and L.has("pa_moe_route")
          and 1 <= T <= GROUPED_MX_MAX_TOKENS and 1 <= E <= DECODE_MAX_EXPERTS and 1 <= topk <= min(DECODE_MAX_TOPK, E)
          and logits.shape[1] == E and d > 0 and f > 0 and d % 128 == 0 and f % 128 == 0
          and d * f < 2 ** 31 and n * max(d, f) < 2 ** 36
          and tuple(w1_q.shape) == (E, 2 * f, d // 2) and tuple(w1_s.shape) == (E, 2 * f, d // 32)
          and tuple(w2_q.shape) == (E, d, f // 2) and tuple(w2_s.shape) == (E, d, f // 32)
          and (b1 is None or tuple(b1.shape) == (E, 2 * f)) and (b2 is None or tuple(b2.shape) == (E, d))
          and all(t.dtype == u8 for t in (w1_q, w1_s, w2_q, w2_s))
          and all(t is None or t.dtype == bf for t in (x, b1, b2))
          and all(t is None or (t.is_contiguous() and t.device == x.device)
                  for t in (x, logits, w1_q, w1_s, w2_q, w2_s, b1, b2)))
    if not ok:
        return None
    dev = x.device
    det = lambda t: None if t is None else t.detach()
    val, idx = torch.softmax(logits.detach().float(), -1).topk(topk, -1)
    if norm_topk_prob:
        val = val / val.sum(-1, keepdim=True)
    val, idx = val.contiguous(), idx.to(torch.int32).contiguous()
    offs, perm = route(idx.reshape(-1), E)
    pos = torch.empty(n, dtype=torch.int32, device=dev)
    pos[perm] = torch.arange(n, dtype=torch.int32, device=dev)  # the inverse of perm: entry -> sorted row
    perm = perm.to(torch.int32)
    x_q, x_s = MX.quantize_mx(x, "mxfp8")
    h_q = torch.empty(n, f, dtype=u8, device=dev)
    h_s = torch.empty(n, f // 32, dtype=u8, device=dev)
    L.call("pa_moe_grouped_up_mx", L.ptr(MX._u8(x_q)), L.ptr(x_s), L.ptr(w1_q), L.ptr(w1_s), L.ptr(det(b1)),
           L.ptr(offs), L.ptr(perm), L.ptr(h_q), L.ptr(h_s), T, E, topk, d, f, L.stream_ptr())
    return _grouped_down_mx(h_q, h_s, w2_q, w2_s, det(b2), val, idx, offs, pos)


def _grouped_down_mx(h_q, h_s, w2_q, w2_s, b2, val, idx, offs, pos):
    """Down projection and combine on expert-sorted rows: h_q [n, f] e4m3fn codes / h_s [n, f / 32], val [T, topk]
    fp32, idx [T, topk] / offs [E + 1] / pos [n] int32 -> out [T, d] bf16 (y [n, d] fp32 of workspace, each row
    written once)."""
    (n, f), (E, d), (T, topk) = h_q.shape, w2_q.shape[:2], val.shape
    y = torch.empty(n, d, dtype=torch.float32, device=h_q.device)
    out = torch.empty(T, d, dtype=torch.bfloat16, device=h_q.device)
    L.call("pa_moe_grouped_down_mx", L.ptr(MX._u8(h_q)), L.ptr(h_s), L.ptr(w2_q), L.ptr(w2_s), L.ptr(b2), L.ptr(val),
           L.ptr(idx), L.ptr(offs), L.ptr(pos), L.ptr(y), L.ptr(out), T, E, topk, d, f, L.stream_ptr())
    return out
