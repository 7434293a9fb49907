"""fp8 GEMM with a fused bias / activation epilogue on the gfx950 block-scaled MFMA (csrc/kernels/gemm_fp8.hip).

Reference: python/paddle/tensor/linalg.py fp8_fp8_half_gemm_fused, paddle/phi/kernels/fusion/fp8_gemm/.
OCP e4m3fn / e5m2 operands (gfx950's native encodings, not the fnuz variants), fp32 accumulation,
fp16 / bf16 output: out = act(alpha * x @ y + bias)."""
from __future__ import annotations

import weakref

import torch

from . import _loader as L

_FMT = {torch.float8_e4m3fn: 0, torch.float8_e5m2: 1}
_ACT = {"identity": 0, "none": 0, "gelu": 1, "relu": 2}


def _ref(a, b_nk, bias, alpha, act, out_dtype):
    return _ref_epilogue(alpha * (a.float() @ b_nk.float().t()), bias, act, out_dtype)


def _ref_epilogue(y, bias, act, out_dtype):
    if bias is not None:
        y = y + bias.float()
    if act == "gelu":
        y = torch.nn.functional.gelu(y)
    elif act == "relu":
        y = torch.relu(y)
    return y.to(out_dtype)


def hip_ok(a, b_nk, bias, out_dtype):
    return (L.hip_enabled_for(a) and L.has("pa_gemm_fp8") and a.dtype in _FMT and b_nk.dtype in _FMT
            and a.dim() == 2 and b_nk.dim() == 2 and a.shape[1] % 128 == 0 and b_nk.shape[0] % 4 == 0
            and out_dtype in (torch.float16, torch.bfloat16) and a.stride(1) == 1 and b_nk.stride(1) == 1
            and a.stride(0) % 16 == 0 and b_nk.stride(0) % 16 == 0 and a.data_ptr() % 16 == 0
            and b_nk.data_ptr() % 16 == 0 and (bias is None or bias.is_contiguous()))


def set_kernel(kind):
    """fp8 GEMM kernel choice: "auto" (the ping-pong 256x256 schedule when N % 8 == 0, else the generic kernel) or
    "generic"; returns the previous choice (A/B measurements and tests)."""
    global _KERNEL
    old, _KERNEL = _KERNEL, kind
    L.call("pa_gemm_fp8_set_kernel", {"auto": 0, "generic": 1}[kind])
    return old


_KERNEL = "auto"


def gemm_fp8(a, b_nk, bias=None, alpha=1.0, act="identity", out_dtype=torch.float16, a_scale_inv=None,
             b_scale_inv=None):
    """a [M, K] and b_nk [N, K] fp8 (both K-major) -> [M, N] in out_dtype. ``a_scale_inv`` / ``b_scale_inv``:
    one-element fp32 tensors on a's device (or None = 1) that the kernel multiplies ``alpha`` by in its epilogue, so a
    scale that was computed on the device is never read back."""
    if act not in _ACT:
        raise ValueError(f"fp8 GEMM: unsupported activation {act!r} (identity / relu / gelu)")
    M, K = a.shape
    N = b_nk.shape[0]
    if b_nk.shape[1] != K:
        raise ValueError(f"fp8 GEMM: inner dimensions differ ({K} vs {b_nk.shape[1]})")
    if not hip_ok(a, b_nk, bias, out_dtype):
        if a.is_cuda and L.hip_enabled_for(a) and a.dtype in _FMT and a.shape[1] % 128 == 0 \
                and b_nk.shape[0] % 4 == 0:
            a, b_nk = a.contiguous(), b_nk.contiguous()
            if hip_ok(a, b_nk, bias, out_dtype):
                return gemm_fp8(a, b_nk, bias, alpha, act, out_dtype, a_scale_inv, b_scale_inv)
        y = _ref(a, b_nk, None, alpha, "identity", torch.float32)
        for sc in (a_scale_inv, b_scale_inv):
            if sc is not None:
                y = y * sc.float().reshape(())
        return _ref_epilogue(y, bias, act, out_dtype)
    out = torch.empty(M, N, dtype=out_dtype, device=a.device)
    bias_c = None if bias is None else bias.to(out_dtype).contiguous()
    if a_scale_inv is not None or b_scale_inv is not None:
        for sc in (a_scale_inv, b_scale_inv):
            if sc is not None and (sc.dtype != torch.float32 or sc.numel() != 1 or sc.device != a.device):
                raise ValueError("fp8 GEMM: a_scale_inv / b_scale_inv must be one-element fp32 tensors on the device")
        nb = int(L.lib().pa_gemm_fp8_ws_bytes(M, N, K))
        ws = torch.empty(nb // 4, dtype=torch.float32, device=a.device) if nb else None
        L.call("pa_gemm_fp8_dscale", L.ptr(a), L.ptr(b_nk), L.ptr(out), L.ptr(bias_c), M, N, K, a.stride(0),
               b_nk.stride(0), out.stride(0), _FMT[a.dtype], _FMT[b_nk.dtype], float(alpha), _ACT[act],
               1 if out_dtype == torch.float16 else 0, L.ptr(ws), L.ptr(a_scale_inv), L.ptr(b_scale_inv),
               L.stream_ptr())
        return out
    if L.has("pa_gemm_fp8_ws"):  # the ping-pong kernel's balanced tail: K-sliced last wave of tiles
        nb = int(L.lib().pa_gemm_fp8_ws_bytes(M, N, K))
        ws = torch.empty(nb // 4, dtype=torch.float32, device=a.device) if nb else None
        L.call("pa_gemm_fp8_ws", L.ptr(a), L.ptr(b_nk), L.ptr(out), L.ptr(bias_c), M, N, K, a.stride(0),
               b_nk.stride(0), out.stride(0), _FMT[a.dtype], _FMT[b_nk.dtype], float(alpha), _ACT[act],
               1 if out_dtype == torch.float16 else 0, L.ptr(ws), L.stream_ptr())
        return out
    L.call("pa_gemm_fp8", L.ptr(a), L.ptr(b_nk), L.ptr(out), L.ptr(bias_c), M, N, K, a.stride(0), b_nk.stride(0),
           out.stride(0), _FMT[a.dtype], _FMT[b_nk.dtype], float(alpha), _ACT[act],
           1 if out_dtype == torch.float16 else 0, L.stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------
# fp8 training linear (csrc/kernels/quant_fp8.hip + the GEMM above).
# Reference recipe: per-tensor amax scaling, current or delayed over an amax history ("FP8 Formats for Deep
# Learning", Micikevicius et al. 2022); activations and weights e4m3fn, gradients e5m2.
# Paddle 3.0 itself publishes only fp8_fp8_half_gemm_fused (python/paddle/tensor/linalg.py); the quantise /
# linear / layer names under paddle.incubate.nn are this project's own.
#
# A linear's three products read every tensor once as stored and once transposed (the GEMM reads both operands
# K-major):  y = x . W   as qx [M, K] x qw^T [N, K];   dx = dy . W^T as qd [M, N] x qw [K, N];
#            dW = x^T . dy as qx^T [K, M] x qd^T [N, M].
# pa_fp8_quant writes q and q^T from one read of the 16-bit tensor, with the scale read from device memory, and the
# GEMM epilogue multiplies by the two scale inverses it reads from device memory: no value crosses to the host.
FMAX = {torch.float8_e4m3fn: 448.0, torch.float8_e5m2: 57344.0}
_N_PARTS = []  # [slots of an amax partials buffer]
_ONES = {}


def _fmt_of(fmt):
    if isinstance(fmt, str):
        fmt = {"float8_e4m3fn": torch.float8_e4m3fn, "e4m3": torch.float8_e4m3fn, "float8_e5m2": torch.float8_e5m2,
               "e5m2": torch.float8_e5m2}.get(fmt, fmt)
    if fmt not in FMAX:
        raise ValueError(f"fp8 quantize: unsupported format {fmt!r} (float8_e4m3fn / float8_e5m2)")
    return fmt


def n_parts():
    """Slots of an amax partials buffer: what the kernels fill (pa_fp8_nparts()); 1024 without the library."""
    if not _N_PARTS:
        _N_PARTS.append(int(L.lib().pa_fp8_nparts()) if L.has("pa_fp8_nparts") else 1024)
    return _N_PARTS[0]


def new_parts(device):
    return torch.zeros(n_parts(), dtype=torch.float32, device=device)


def _quant_hip_ok(x):
    return L.hip_enabled_for(x) and L.has("pa_fp8_quant") and x.dtype in L._DT


def _one(device):
    t = _ONES.get(device)
    if t is None:
        t = _ONES[device] = torch.ones(1, dtype=torch.float32, device=device)
    return t


def amax_parts(x, parts):
    """parts[:] = partial absolute maxima of x (their maximum is |x|max; non-finite if x holds an inf or a NaN)."""
    if _quant_hip_ok(x):
        x = x if x.is_contiguous() else x.contiguous()
        L.call("pa_fp8_amax", L.ptr(x), x.numel(), L.dcode(x), L.ptr(parts), L.stream_ptr())
    else:
        parts.zero_()
        parts[0] = x.detach().abs().max().float()  # torch's max propagates a NaN
    return parts


def quantize_fp8(x, fmt, scale=None, transpose=False, amax_parts=None):
    """(q, qT): q = sat(x * scale) in ``fmt`` with x's shape, qT = its transpose [C, R] over x viewed as [R, C]
    (C = the last dimension) when ``transpose``, else None. ``scale``: one-element fp32 tensor on x's device (None =
    1). ``amax_parts``: an fp32 buffer of n_parts() slots that receives the partial absolute maxima of x."""
    fmt = _fmt_of(fmt)
    C = x.shape[-1] if x.dim() else 1
    R = x.numel() // max(C, 1)
    if scale is None:
        scale = _one(x.device)
    if _quant_hip_ok(x) and x.numel() > 0:
        x = x if x.is_contiguous() else x.contiguous()
        q = torch.empty(x.shape, dtype=fmt, device=x.device)
        qT = torch.empty(C, R, dtype=fmt, device=x.device) if transpose else None
        L.call("pa_fp8_quant", L.ptr(x), R, C, L.dcode(x), _FMT[fmt], L.ptr(scale), L.ptr(q), L.ptr(qT),
               L.ptr(amax_parts), L.stream_ptr())
        return q, qT
    xf = x.detach().float()
    q = (xf * scale.reshape(())).clamp(-FMAX[fmt], FMAX[fmt]).to(fmt)
    if amax_parts is not None:
        amax_parts.zero_()
        if x.numel():
            amax_parts[0] = xf.abs().max()
    return q, (q.reshape(R, C).t().contiguous() if transpose else None)


class _Box:
    """Holder of one tensor (``_t``), the shape a Layer buffer has: a state built on a layer's buffers follows the
    layer's ``.to()`` and ``set_state_dict``."""
    __slots__ = ("_t",)

    def __init__(self, t):
        self._t = t


class Fp8TensorState:
    """Scaling state of one quantized role (a linear's input, weight or output gradient).

    ``scale`` maps the tensor onto the fp8 range: scale = (fmax / amax) * 2^-margin, ``scale_inv`` = 1 / scale.
    recipe "current": amax is that of the tensor being quantized (one extra read of it). recipe "delayed": amax is
    the maximum of ``amax_history`` (newest first), the tensor is quantized with the scale of the calls before it
    and its own amax, taken by the quantize kernel in the same pass, enters the history afterwards; a state's first
    call has no history yet and runs the current recipe. A zero or non-finite amax leaves the scale as it is, and a
    non-finite one stays out of the history. Everything is computed on the tensor's device (pa_fp8_amax /
    pa_fp8_scale_update, or the same rule in torch ops elsewhere): nothing here reads a device value on the host.
    """

    def __init__(self, fmt=torch.float8_e4m3fn, recipe="delayed", amax_history_len=16, margin=0, device="cpu",
                 buffers=None):
        if recipe not in ("current", "delayed"):
            raise ValueError(f"fp8 recipe must be 'current' or 'delayed', got {recipe!r}")
        if not 1 <= int(amax_history_len) <= 1024:
            raise ValueError("amax_history_len must be in [1, 1024]")
        if abs(int(margin)) > 64:
            raise ValueError("margin must be in [-64, 64]")
        self.fmt, self.recipe, self.margin = _fmt_of(fmt), recipe, int(margin)
        if buffers is None:
            buffers = (_Box(torch.zeros(int(amax_history_len), dtype=torch.float32, device=device)),
                       _Box(torch.ones(1, dtype=torch.float32, device=device)),
                       _Box(torch.ones(1, dtype=torch.float32, device=device)))
        self._h, self._s, self._si = buffers
        self._parts = None
        self.calls = 0      # host-side: 0 = the next call is the state's first
        self.cache = None   # (weakref, (data_ptr, version), q, qT, scale_inv) of the tensor last quantized by cached()

    amax_history = property(lambda self: self._h._t)
    scale = property(lambda self: self._s._t)
    scale_inv = property(lambda self: self._si._t)

    @property
    def parts(self):
        return self._parts

    def _on(self, device):
        """The state's tensors on ``device`` as fp32 (a layer cast or moved as a whole takes its buffers along)."""
        for b in (self._h, self._s, self._si):
            if b._t.device != device or b._t.dtype != torch.float32:
                b._t = b._t.to(device=device, dtype=torch.float32)
        if self._parts is None or self._parts.device != device:
            self._parts = new_parts(device)

    def update(self, mode=None):
        """Fold ``parts`` into the scale (mode 0 current, 1 delayed; default: the recipe's)."""
        mode = (1 if self.recipe == "delayed" else 0) if mode is None else mode
        h, s, si, parts = self.amax_history, self.scale, self.scale_inv, self._parts
        fmax = FMAX[self.fmt]
        if L.hip_enabled_for(parts) and L.has("pa_fp8_scale_update"):
            L.call("pa_fp8_scale_update", L.ptr(parts), parts.numel(), L.ptr(h), h.numel(), L.ptr(s), L.ptr(si),
                   fmax, self.margin, mode, L.stream_ptr())
            return
        a_new = parts.max()
        a = a_new
        if mode == 1:
            h.copy_(torch.where(torch.isfinite(a_new), torch.cat([a_new.reshape(1), h[:-1]]), h))
            a = torch.where(torch.isfinite(a_new), h.max(), a_new)
        ok = torch.isfinite(a) & (a > 0)
        new = (torch.full_like(a, fmax) / a) * torch.full_like(a, 2.0 ** -self.margin)
        s.copy_(torch.where(ok, new, s.reshape(())).reshape(1))
        si.copy_(torch.where(ok, 1.0 / new, si.reshape(())).reshape(1))

    def quantize(self, x, transpose=True):
        """(q, qT, scale_inv): x quantized by the recipe; ``scale_inv`` is a copy of the inverse of the scale that q
        was made with (the state's own tensor moves on with the next call)."""
        self._on(x.device)
        first = self.calls == 0
        self.calls += 1
        if self.recipe == "current" or first:
            amax_parts(x, self._parts)
            self.update()
            q, qT = quantize_fp8(x, self.fmt, self.scale, transpose)
            return q, qT, self.scale_inv.clone()
        sinv = self.scale_inv.clone()
        q, qT = quantize_fp8(x, self.fmt, self.scale, transpose, amax_parts=self._parts)
        self.update()
        return q, qT, sinv

    def cached(self, w):
        """quantize(w) once per value of ``w``: keyed on (data_ptr, version), so the micro-batches of a gradient
        accumulation window share one quantization and an in-place optimizer update renews it."""
        key = (w.data_ptr(), w._version)
        ent = self.cache
        if ent is None or ent[0]() is not w or ent[1] != key:  # identity too: a freed weight's address can come back
            ent = self.cache = (weakref.ref(w), key, *self.quantize(w, True))
        return ent[2:]


def new_states(recipe="current", amax_history_len=16, margin=0, device="cpu"):
    """The three states of a linear: input and weight in e4m3fn, output gradient in e5m2."""
    mk = lambda fmt: Fp8TensorState(fmt, recipe, amax_history_len, margin, device)  # noqa: E731
    return {"x": mk(torch.float8_e4m3fn), "w": mk(torch.float8_e4m3fn), "dy": mk(torch.float8_e5m2)}


CALLS = {"hip": 0, "emulated": 0, "fallback": 0}  # which path fp8_linear took


def _mm_deq(a, b_nk, sa, sb, bias, out_dtype):
    """The GEMM's arithmetic in torch: fp32 product of the fp8 operands, times both scale inverses, plus bias."""
    y = (a.float() @ b_nk.float().t()) * (sa.reshape(()) * sb.reshape(()))
    if bias is not None:
        y = y + bias.float()
    return y.to(out_dtype)


class _Fp8LinearFn(torch.autograd.Function):
    """y = x W (+ b) with all three products on fp8 operands. Saved for backward: qx^T, qw and the scale
    inverses — not x."""

    @staticmethod
    def forward(ctx, x, w, b, states, hip):
        shape = x.shape
        x2 = x.reshape(-1, shape[-1])
        mm = (lambda a, bn, sa, sb, bias, dt: gemm_fp8(a, bn, bias, 1.0, "identity", dt, sa, sb)) if hip else _mm_deq
        need_w_grad = ctx.needs_input_grad[1]
        qx, qxT, sx = states["x"].quantize(x2, transpose=need_w_grad)
        qw, qwT, sw = states["w"].cached(w)
        y = mm(qx, qwT, sx, sw, b, x.dtype)
        ctx.save_for_backward(qxT, qw, sx, sw)
        ctx.states, ctx.mm, ctx.hip = states, mm, hip
        ctx.shape, ctx.w_dtype, ctx.has_b = shape, w.dtype, b is not None
        return y.view(*shape[:-1], w.shape[1])

    @staticmethod
    def backward(ctx, dy):
        qxT, qw, sx, sw = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        if dy2.dtype != ctx.w_dtype:
            dy2 = dy2.to(ctx.w_dtype)
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        qd, qdT, sd = ctx.states["dy"].quantize(dy2, transpose=need_w)
        dx = ctx.mm(qd, qw, sd, sw, None, dy2.dtype).view(ctx.shape) if need_x else None
        dw = ctx.mm(qxT, qdT, sx, sd, None, ctx.w_dtype) if need_w else None
        db = None
        if ctx.has_b and need_b:
            if ctx.hip:
                from .linear import colsum
                db = colsum(dy2)
            else:
                db = dy2.float().sum(0).to(dy2.dtype)
        return dx, dw, db, None, None


def fp8_shapes_ok(x, w):
    """What the three fp8 products take: 16-bit x and w of one dtype, and M, K, N multiples of 128 (the GEMM's
    K % 128 and 16-byte row strides, applied to y = x W, dx = dy W^T and dW = x^T dy)."""
    if not (x.dtype in (torch.bfloat16, torch.float16) and w.dtype == x.dtype and w.dim() == 2 and x.dim() >= 1
            and x.shape[-1] == w.shape[0] and x.numel() > 0):
        return False
    M, K, N = x.numel() // x.shape[-1], w.shape[0], w.shape[1]
    return M % 128 == 0 and K % 128 == 0 and N % 128 == 0


def fp8_hip_ok(x, w):
    """The HIP path's condition: fp8_shapes_ok on a plain device tensor."""
    return x.is_cuda and fp8_shapes_ok(x, w) and L.hip_enabled_for(x) and L.has("pa_fp8_quant") \
        and L.has("pa_gemm_fp8_dscale")


def fp8_linear(x, w_kn, bias=None, states=None, emulate=False):
    """y = x @ w_kn + bias, w_kn [K, N] (the Paddle layout), forward and backward on the fp8 GEMM.

    ``states``: {"x", "w", "dy"} -> Fp8TensorState (new_states(); None = current scaling, nothing kept). Shapes or
    dtypes the fp8 GEMM does not take (fp8_shapes_ok) run ops.linear.fused_linear in the input dtype and count in
    CALLS["fallback"]. ``emulate=True`` runs the same quantization with fp32 matmuls of the dequantized operands in
    torch instead of the HIP kernels (any device; the reference of the tests)."""
    ok = fp8_shapes_ok(x, w_kn)
    hip = ok and not emulate and fp8_hip_ok(x, w_kn)
    if not (hip or (ok and emulate)):
        from .linear import fused_linear
        CALLS["fallback"] += 1
        return fused_linear(x, w_kn, bias)
    if states is None:
        states = new_states("current", device=x.device)
    CALLS["hip" if hip else "emulated"] += 1
    if bias is not None and bias.dtype != x.dtype:
        bias = bias.to(x.dtype)
    return _Fp8LinearFn.apply(x, w_kn, bias, states, hip)
