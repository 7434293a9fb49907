"""Needle inputs, fp64 references and tolerances for the attention kernels (flash forward/backward, paged and
dense decode). Plain helper module, imported by the tests like ``op_test``.

Why needles: with ``randn`` inputs a softmax row over n keys gives every key ~1/n of the weight, so one wrong
key at a block / tile / mask / sequence boundary moves the output by less than any usable tolerance. Here each
query's logit toward one chosen boundary key is raised by g = ln(Sk) + 1, so that key holds ~0.65 of its row:

* a *needle* row aims at the last key still visible at a boundary (losing it changes the row by O(1));
* a *trap* row aims at the first key just beyond the boundary, which the reference masks (a kernel that is off
  by one lets it dominate the row);
* every fourth row stays plain random.

Boundaries are read off the visibility matrix itself: every key whose visibility differs from a neighbour's
along the key axis (causal diagonal / diagonal + 1, bool-mask edges, -inf entries, varlen sequence ends) or
along the row axis (flashmask bound rows LTS - 1 / LTS, LTE - 1 / LTE), plus keys 0, 63, 64, 127, 128, Sk - 1.

``reference`` is fp64 math on the rounded inputs (gradients by autograd); ``rounding_model`` is the same math
with only the roundings a correct kernel must make. The tolerances in ``TOL`` are derived from the rounding
model's measured error (``python tests/attn_needles.py`` prints the table; profiles/attention_needle_tests.md
records it), not from any kernel output.
"""
from __future__ import annotations

import math

import torch

INF = float("inf")

# ------------------------------------------------------------------------------------------------ tolerances
# check(): |got - ref| <= atol + rtol |ref| per element.
# rtol: two ulps of the storage type (ulp = machine epsilon: 2^-7 bf16, 2^-10 fp16).
# atol: 4 x the rounding model's worst error that rtol does not cover, max(|model - ref| - rtol |ref|), over every
# case below (measure(); the 4 is headroom for fp32 accumulation order, the hardware exp2 and the deferred
# rescale, not a fit to the kernel). For o it is absolute; for dq / dk / dv it is a fraction of max|ref| of the
# tensor, since gradient magnitudes grow with the number of rows summed. Neither may exceed what the older
# attention tests allow (3e-2 absolute forward, 2.5e-2 of max for gradients): bf16 dq and dk are capped there.
# The plain max|model - ref| is not used: needle outputs reach |o| ~ 4, where one bf16 rounding of O is already
# 0.016, and 4 x that would be above the older tests' bound.
FWD_CAP, GRAD_CAP = 3e-2, 2.5e-2
MEASURED = {   # uncovered rounding-model error (python tests/attn_needles.py), see profiles/attention_needle_tests.md
    torch.bfloat16: {"o": 5.084e-3, "dq": 1.234e-2, "dk": 1.731e-2, "dv": 1.604e-3},
    torch.float16: {"o": 4.629e-4, "dq": 1.334e-3, "dk": 3.252e-3, "dv": 1.735e-4},
}
TOL = {dt: {n: min(4 * e, FWD_CAP if n == "o" else GRAD_CAP) for n, e in d.items()} for dt, d in MEASURED.items()}
RTOL = {torch.bfloat16: 2 * 2.0 ** -7, torch.float16: 2 * 2.0 ** -10}
# LSE (fp32): 8 x the worst error of an fp32 QK^T + logsumexp against fp64 (6.24e-6), absolute.
LSE_MEASURED = 6.24e-6
LSE_ATOL = 8 * LSE_MEASURED
# Decode output (bf16, all math fp32 in the kernel): an fp32 model of the op is inside rtol on every element, so the
# measurement gives no absolute term; outputs near zero (cancelling p v terms) still carry the fp32 error of the
# scores. Bound from the formats: a 128-term fp32 dot has |ds| <= 130 * 2^-24 * scale * sum|q_i k_i|, p moves by
# <= 2 |ds| relative, so |do| <= 2 |ds| max|v|: 9.4e-4 at most over the cases (measure() prints it).
DECODE_ATOL = 1e-3


def tolerances(dtype, name, ref):
    """(atol, rtol) of output ``name`` ('o', 'dq', 'dk', 'dv', 'lse') for a reference tensor."""
    if name == "lse":
        return LSE_ATOL, 0.0
    a = TOL[dtype][name]
    if name != "o":
        fin = ref[torch.isfinite(ref)]
        a = a * (float(fin.abs().max()) if fin.numel() else 0.0)
    return a, RTOL[dtype]


def excess(got, ref, atol, rtol):
    """max over elements of |got - ref| / (atol + rtol |ref|) and its index; NaN or a wrong infinity -> inf."""
    got, ref = got.detach().double(), ref.double()
    same_inf = torch.isinf(ref) & (got == ref)
    diff = (got - ref).abs()
    err = diff / (atol + rtol * ref.abs())
    err = torch.where(same_inf | (diff == 0), torch.zeros_like(err), err)   # (an exact match passes a zero tolerance)
    err = torch.where(torch.isnan(err) | (torch.isinf(ref) & ~same_inf), torch.full_like(err, INF), err)
    if err.numel() == 0:
        return 0.0, ()
    flat = int(err.reshape(-1).argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), err.shape))
    return float(err.reshape(-1)[flat]), idx


def check(got, ref, atol, rtol, what=""):
    """Elementwise |got - ref| <= atol + rtol |ref|; NaN fails; reports the worst element."""
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    r, idx = excess(got, ref, atol, rtol)
    if r > 1.0:
        g, e = float(got[idx]), float(ref[idx])
        raise AssertionError(f"{what}: worst element {idx}: got {g:.6g}, want {e:.6g}, |diff| {abs(g - e):.3g} = "
                             f"{r:.3g} x (atol {atol:.3g} + rtol {rtol:.3g} |ref|)")


# --------------------------------------------------------------------------------------------- visibility
def causal_keep(Sq, Sk):
    """Bottom-right aligned causal mask [Sq, Sk]: row i sees keys <= i + Sk - Sq."""
    return torch.arange(Sk)[None] <= torch.arange(Sq)[:, None] + (Sk - Sq)


def flashmask_keep(se, Sq, Sk, causal):
    """Dense keep mask [B, H|1, Sq, Sk] of startend_row_indices [B, H|1, Sk, 1|2|4]: key j is masked for rows in
    [LTS, LTE) (LTE = inf when absent) and, non-causal, in [UTS, UTE) (UTS = 0 when absent)."""
    se = se.long()
    n = se.shape[-1]
    rows = torch.arange(Sq).view(1, 1, Sq, 1)
    big = torch.full_like(se[..., 0], 1 << 40).unsqueeze(2)
    lts = se[..., 0].unsqueeze(2)
    if causal:
        lte = se[..., 1].unsqueeze(2) if n >= 2 else big
        return ~((rows >= lts) & (rows < lte)) & causal_keep(Sq, Sk)
    if n == 1:
        return ~(rows >= lts)
    if n == 2:
        lte, uts, ute = big, torch.zeros_like(lts), se[..., 1].unsqueeze(2)
    else:
        lte, uts, ute = (se[..., i].unsqueeze(2) for i in (1, 2, 3))
    return ~(((rows >= lts) & (rows < lte)) | ((rows >= uts) & (rows < ute)))


def varlen_keep(lens_q, lens_k, causal):
    """Packed sequences as one [Tq, Tk] block-diagonal mask (each block bottom-right causal when ``causal``)."""
    keep = torch.zeros(sum(lens_q), sum(lens_k), dtype=torch.bool)
    a = c = 0
    for lq, lk in zip(lens_q, lens_k):
        keep[a:a + lq, c:c + lk] = causal_keep(lq, lk) if causal else True
        a, c = a + lq, c + lk
    return keep


# -------------------------------------------------------------------------------------------- needle inputs
def needle_targets(vis):
    """vis bool [B, H, Sq, Sk] -> (target key [B, H, Sq] or -1 for a plain row, role [B, H, Sq]: 0 needle, 1 trap,
    2 needle, 3 plain). Role = (row + head) % 4, so one row plays different roles in the heads of a GQA group and
    the candidate picked cycles with row, head and batch."""
    B, H, Sq, Sk = vis.shape
    edge = torch.zeros_like(vis)
    if Sk > 1:
        d = vis[..., 1:] != vis[..., :-1]
        edge[..., 1:] |= d
        edge[..., :-1] |= d
    if Sq > 1:
        d = vis[..., 1:, :] != vis[..., :-1, :]
        edge[..., 1:, :] |= d
        edge[..., :-1, :] |= d
    for kf in (0, 63, 64, 127, 128, Sk - 1):
        if 0 <= kf < Sk:
            edge[..., kf] = True
    rows = torch.arange(Sq).view(1, 1, Sq)
    heads = torch.arange(H).view(1, H, 1)
    batch = torch.arange(B).view(B, 1, 1)
    role = ((rows + heads) % 4).expand(B, H, Sq)
    want_vis = (role != 1).unsqueeze(-1)
    cand = edge & (vis == want_vis)
    cnt = cand.sum(-1)
    pick = ((rows // 4) * 5 + heads * 3 + batch * 7) % cnt.clamp(min=1)
    hit = cand & (cand.cumsum(-1) == (pick + 1).unsqueeze(-1))
    tgt = hit.int().argmax(-1)
    tgt = torch.where((cnt > 0) & (role != 3), tgt, torch.full_like(tgt, -1))
    return tgt, role


def needle_inputs(B, Sq, Sk, H, Hk, D, dtype, vis, seed=0, scale=None):
    """q [B, Sq, H, D], k, v [B, Sk, Hk, D] and a cotangent do [B, Sq, H, D] in ``dtype`` (CPU tensors).
    k, v, do ~ N(0, 1); q = 0.5 N(0, 1) + g k[target] / (scale D) with g = ln(Sk) + 1: with the default scale
    1/sqrt(D) that is g k[t] / sqrt(D); |k|^2 ~ D, so the target's logit is raised by ~g at any scale."""
    gen = torch.Generator().manual_seed(1000 + seed)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    k = torch.randn(B, Sk, Hk, D, generator=gen)
    v = torch.randn(B, Sk, Hk, D, generator=gen)
    q = 0.5 * torch.randn(B, Sq, H, D, generator=gen)
    do = torch.randn(B, Sq, H, D, generator=gen)
    tgt, _ = needle_targets(vis.expand(B, H, Sq, Sk))
    g = math.log(Sk) + 1.0
    kh = k.repeat_interleave(H // Hk, 2).permute(0, 2, 1, 3)                       # [B, H, Sk, D]
    kt = torch.gather(kh, 2, tgt.clamp(min=0).unsqueeze(-1).expand(B, H, Sq, D))  # [B, H, Sq, D]
    kt = kt * (tgt >= 0).unsqueeze(-1)
    q = q + (g / (scale * D)) * kt.permute(0, 2, 1, 3)
    return q.to(dtype), k.to(dtype), v.to(dtype), do.to(dtype)


# ------------------------------------------------------------------------------------------- fp64 reference
def _heads(q, k, v):
    H, Hk = q.shape[2], k.shape[2]
    qh = q.permute(0, 2, 1, 3)
    kh = k.repeat_interleave(H // Hk, 2).permute(0, 2, 1, 3)
    vh = v.repeat_interleave(H // Hk, 2).permute(0, 2, 1, 3)
    return qh, kh, vh


def _scores(qh, kh, vis, bias, scale):
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias.to(s.dtype)
    s = s.masked_fill(~vis, -INF)
    dead = torch.isneginf(s).all(-1, keepdim=True)
    return s.masked_fill(dead, 0.0), dead


def reference(q, k, v, do, vis, bias=None, scale=None, keep=None, drop_p=0.0):
    """fp64 attention of the rounded inputs. q, do [B, Sq, H, D]; k, v [B, Sk, Hk, D]; vis bool and bias (additive,
    may hold -inf) broadcastable to [B, H, Sq, Sk]; keep: dropout keep mask applied to P after the row sum, scaled
    by 1 / (1 - drop_p). Returns dict o [B, Sq, H, D], lse [B, H, Sq], dq, dk, dv. Rows without a visible key:
    o = 0, zero gradient contributions, lse = +inf (the kernel's value)."""
    D = q.shape[-1]
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    q, k, v = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    qh, kh, vh = _heads(q, k, v)
    s, dead = _scores(qh, kh, vis, bias, scale)
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse).masked_fill(dead, 0.0)
    if keep is not None:
        p = p * keep.to(p.dtype) / (1.0 - drop_p)
    o = torch.matmul(p, vh).permute(0, 2, 1, 3)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), do.double())
    lse = lse.detach().masked_fill(dead, INF).squeeze(-1)
    return {"o": o.detach(), "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def lse_fp32(q, k, vis, bias=None, scale=None):
    """LSE as a correct fp32 implementation gives it (fp32 QK^T + logsumexp): its distance from ``reference`` sets
    the LSE tolerance."""
    D = q.shape[-1]
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    qh, kh, _ = _heads(q.float(), k.float(), k.float())
    s, dead = _scores(qh, kh, vis, None if bias is None else bias.float(), scale)
    return torch.logsumexp(s, -1).masked_fill(dead.squeeze(-1), INF)


def rounding_model(q, k, v, do, vis, bias=None, scale=None, keep=None, drop_p=0.0):
    """``reference`` with only the roundings a correct kernel must make, all else fp64: P rounded to the storage
    type before PV, O rounded; backward: P and dS rounded before their GEMMs, delta from the rounded O, dq / dk /
    dv rounded (dk / dv after the GQA group sum)."""
    dt, D = q.dtype, q.shape[-1]
    H, Hk = q.shape[2], k.shape[2]
    scale = 1.0 / math.sqrt(D) if scale is None else scale

    def rnd(x):
        return x.to(dt).double()

    qh, kh, vh = _heads(q.double(), k.double(), v.double())
    doh = do.double().permute(0, 2, 1, 3)
    s, dead = _scores(qh, kh, vis, bias, scale)
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse).masked_fill(dead, 0.0)
    kf = 1.0 if keep is None else keep.double() / (1.0 - drop_p)
    o = rnd(torch.matmul(rnd(p * kf), vh))
    delta = (o * doh).sum(-1, keepdim=True)
    dv = torch.matmul(rnd(p * kf).transpose(-1, -2), doh)
    dp = torch.matmul(doh, vh.transpose(-1, -2)) * kf
    ds = rnd(p * (dp - delta))
    dq = rnd(torch.matmul(ds, kh) * scale)
    dk = torch.matmul(ds.transpose(-1, -2), qh) * scale
    B, _, Sk, _ = dk.shape
    dk = rnd(dk.view(B, Hk, H // Hk, Sk, D).sum(2))
    dv = rnd(dv.view(B, Hk, H // Hk, Sk, D).sum(2))
    return {"o": o.permute(0, 2, 1, 3), "lse": lse.masked_fill(dead, INF).squeeze(-1), "dq": dq.permute(0, 2, 1, 3),
            "dk": dk.permute(0, 2, 1, 3), "dv": dv.permute(0, 2, 1, 3)}


# ------------------------------------------------------------------------------------------------ flash cases
GEOMS = [(1, 1, 1, 1, 1), (1, 1, 129, 2, 1), (2, 130, 130, 2, 2), (1, 65, 200, 2, 1), (1, 257, 193, 4, 2),
         (1, 384, 384, 8, 8), (1, 512, 512, 2, 2)]
FEATURE_GEOMS = [(1, 257, 193, 4, 2), (2, 130, 130, 2, 2)]
ROUTE_GEOMS = [(1, 1, 129, 2, 1), (2, 130, 130, 2, 2), (1, 65, 200, 2, 1), (1, 257, 193, 4, 2)]
FEATURES = ["bool", "add_bf16", "add_f32", "fm1", "fm2", "fm4", "varlen"]
VARLEN_LENS = [1, 64, 65, 127]
_DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


class Case:
    """One attention problem: inputs (CPU, storage dtype), the kernel's optional arguments and the dense (vis, bias)
    form the reference evaluates. Varlen cases hold packed [1, T, H, D] tensors; ``kernel_args`` unpacks them."""

    def __init__(self, geom, D, dtype="bf16", causal=False, feature=None, scale=None, seed=0):
        self.id = f"{'x'.join(map(str, geom))}-D{D}-{dtype}-{'causal' if causal else 'full'}" + \
                  (f"-{feature}" if feature else "") + (f"-scale{scale}" if scale else "") + f"-s{seed}"
        self.dtype, self.D, self.causal, self.feature, self.scale = _DT[dtype], D, causal, feature, scale
        self._geom, self._seed, self._built = geom, seed, False

    def __getattr__(self, name):   # tensors are built on first use (test collection only needs the ids)
        if name.startswith("_") or self.__dict__.get("_built", True):
            raise AttributeError(name)
        self._build()
        return getattr(self, name)

    def _build(self):
        self._built = True
        (B, Sq, Sk, H, Hk), D, causal, feature, scale, seed = self._geom, self.D, self.causal, self.feature, \
            self.scale, self._seed
        self.mask = self.startend = self.bias = self.lens = None
        gen = torch.Generator().manual_seed(77 + seed)
        if feature == "varlen":
            B, Sq, Sk = 1, sum(VARLEN_LENS), sum(VARLEN_LENS)
            self.lens = VARLEN_LENS
            vis = varlen_keep(VARLEN_LENS, VARLEN_LENS, causal).view(1, 1, Sq, Sk)
        else:
            vis = (causal_keep(Sq, Sk) if causal else torch.ones(Sq, Sk, dtype=torch.bool)).view(1, 1, Sq, Sk)
        self.B, self.Sq, self.Sk, self.H, self.Hk = B, Sq, Sk, H, Hk
        r = torch.arange(Sq).view(1, 1, Sq, 1)
        h = torch.arange(H).view(1, H, 1, 1)
        j = torch.arange(Sk).view(1, 1, 1, Sk)
        if feature == "bool":
            # per (batch, head, row) one masked key range of 1..70 keys, the last key masked on every third row,
            # row 5 (and, causal, the rows causality kills) fully masked
            b = torch.arange(B).view(B, 1, 1, 1)
            a0 = (r * 37 + h * 11 + b * 5) % Sk
            m = ~((j >= a0) & (j < a0 + 1 + r % 70))
            m &= ~((j == Sk - 1) & (r % 3 == 0))
            m &= r != min(5, Sq - 1)
            self.mask = m
            vis = vis & m
        elif feature in ("add_bf16", "add_f32"):
            # per-head bias [1, H, Sq, Sk]: N(0, 0.5) with a -inf range and a -1e4 range on every row
            mdt = torch.bfloat16 if feature == "add_bf16" else torch.float32
            bias = 0.5 * torch.randn(1, H, Sq, Sk, generator=gen)
            a0 = (r * 29 + h * 7) % Sk
            bias = bias.masked_fill((j >= a0) & (j < a0 + 1 + r % 50), -INF)
            a1 = (r * 13 + h * 17 + Sk // 2) % Sk
            bias = bias.masked_fill((j >= a1) & (j < a1 + 1 + r % 9) & ~torch.isinf(bias), -1e4)
            self.mask = bias.to(mdt)
            self.bias = self.mask.double()
        elif feature in ("fm1", "fm2", "fm4"):
            def ri(lo, hi):
                return torch.randint(lo, hi + 1, (B, H, Sk, 1), generator=gen, dtype=torch.int32)
            if feature == "fm1":                      # LTS (causal): key j masked from row LTS on
                se = ri(0, Sq)
            elif feature == "fm2" and causal:         # LTS, LTE
                a, b = ri(0, Sq), ri(0, Sq)
                se = torch.cat([torch.minimum(a, b), torch.maximum(a, b)], -1)
            elif feature == "fm2":                    # LTS, UTE
                se = torch.cat([ri(Sq // 2, Sq), ri(0, Sq // 4)], -1)
            else:                                     # LTS, LTE, UTS, UTE
                a, b = ri(Sq // 2, Sq), ri(Sq // 2, Sq)
                c, d = ri(0, Sq // 3), ri(0, Sq // 3)
                se = torch.cat([torch.minimum(a, b), torch.maximum(a, b), torch.minimum(c, d), torch.maximum(c, d)], -1)
            self.startend = se
            vis = flashmask_keep(se, Sq, Sk, causal)
        self.vis = vis.expand(B, H, Sq, Sk)
        aim = self.vis if self.bias is None else self.vis & (self.bias > -1e3)   # -inf / -1e4 entries are traps
        self.q, self.k, self.v, self.do = needle_inputs(B, Sq, Sk, H, Hk, D, self.dtype, aim, seed, scale)

    def dense(self, device="cpu"):
        """Arguments of reference / rounding_model on ``device``."""
        t = [x.to(device) for x in (self.q, self.k, self.v, self.do)]
        return t, dict(vis=self.vis.to(device), bias=None if self.bias is None else self.bias.to(device),
                       scale=self.scale)

    def kernel_args(self, device):
        """(q, k, v, do, kwargs) for ops.attention.attention on ``device``."""
        q, k, v, do = (x.to(device) for x in (self.q, self.k, self.v, self.do))
        kw = dict(causal=self.causal, scale=self.scale)
        if self.lens is not None:
            cu = torch.tensor([0] + list(torch.tensor(self.lens).cumsum(0)), dtype=torch.int32, device=device)
            kw.update(cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=max(self.lens), max_seqlen_k=max(self.lens))
            q, k, v, do = q[0], k[0], v[0], do[0]
        if self.mask is not None:
            kw["mask"] = self.mask.to(device)
        if self.startend is not None:
            kw["startend_row_indices"] = self.startend.to(device)
        return q, k, v, do, kw


def tile_edge_case(which, D=128, dtype="bf16"):
    """Flashmask bounds constant over each 64-key tile and equal to q_lo, q_lo + 1, q_hi, q_hi + 1 of the 128-row
    block 1 (rows 128..255) of a 384 x 384 problem: the exact transitions of fm_tile_class between 2 (every row
    masked: skip), 1 (test per element) and 0 (no bound touches the block). ``which``: 'causal' (LTS, LTE), 'lower'
    or 'upper' (4 columns, the intervals in the lower resp. upper pair)."""
    Sq = Sk = 384
    iv = [(128, 256), (129, 256), (128, 255), (256, 384), (0, 128), (255, 257)]   # [lo, hi) per 64-key tile
    lo = torch.tensor([a for a, _ in iv], dtype=torch.int32).repeat_interleave(64).view(1, 1, Sk, 1)
    hi = torch.tensor([b for _, b in iv], dtype=torch.int32).repeat_interleave(64).view(1, 1, Sk, 1)
    none_lo, none_hi = torch.full_like(lo, Sq), torch.full_like(lo, Sq)
    zero = torch.zeros_like(lo)
    c = Case.__new__(Case)
    c._built = True
    c.id = f"tile-edges-{which}-D{D}-{dtype}"
    c.dtype, c.D, c.causal, c.feature, c.scale = _DT[dtype], D, which == "causal", "tile", None
    c.mask = c.bias = c.lens = None
    c.B, c.Sq, c.Sk, c.H, c.Hk = 1, Sq, Sk, 2, 1
    if which == "causal":
        se = torch.cat([lo, hi], -1)
    elif which == "lower":
        se = torch.cat([lo, hi, zero, zero], -1)
    else:
        se = torch.cat([none_lo, none_hi, lo, hi], -1)
    c.startend = se
    c.vis = flashmask_keep(se, Sq, Sk, c.causal).expand(1, 2, Sq, Sk)
    c.q, c.k, c.v, c.do = needle_inputs(1, Sq, Sk, 2, 1, D, c.dtype, c.vis, 5)
    return c


def plain_cases():
    return [Case(g, 128, causal=c) for g in GEOMS for c in (False, True)]


def route_cases():
    return [Case(g, 128, causal=c, seed=1) for g in ROUTE_GEOMS for c in (False, True)]


def feature_causal(feature, gi):
    """Causal flag of a feature case: the 257 x 193 geometry runs causal (64 dead rows under every mask kind), the
    130 x 130 one full; fm1 is causal by definition and fm4 non-causal."""
    return True if feature == "fm1" else False if feature == "fm4" else gi == 0


def feature_cases():
    return [Case(g, D, dt, feature_causal(f, gi), f, seed=2)
            for f in FEATURES for gi, g in enumerate(FEATURE_GEOMS) for D in (64, 128, 256) for dt in ("bf16", "fp16")]


def misc_cases():
    out = [Case((2, 130, 130, 2, 2), 80, causal=True, seed=3), Case((1, 257, 193, 4, 2), 80, causal=False, seed=3)]
    for sc in (0.05, 0.3):
        out += [Case((1, 257, 193, 4, 2), 128, causal=True, scale=sc, seed=4),
                Case((2, 130, 130, 2, 2), 128, causal=False, feature="add_f32", scale=sc, seed=4),
                Case((1, 257, 193, 4, 2), 64, causal=True, feature="add_bf16", scale=sc, seed=4)]
    out += [tile_edge_case(w, D) for w in ("causal", "lower", "upper") for D in (64, 128)]
    return out


def bhsd_cases():
    return [Case((2, 130, 130, 2, 2), 128, causal=f is None, feature=f, seed=8) for f in (None, "bool", "add_f32")]


def dead_row_cases():
    """257 x 193 causal: the first 64 rows see no key."""
    return [Case((1, 257, 193, 4, 2), D, causal=True, seed=7) for D in (64, 128, 256)]


def dropout_cases():
    return [Case((2, 257, 193, 4, 2), D, causal=c, seed=6) for D in (128, 256) for c in (False, True)]


def dropout_keep(case, p=0.3, seed=9):
    """A stand-in keep mask for CPU measurements of the dropout cases (the GPU test recovers the kernel's own)."""
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(case.B, case.H, case.Sq, case.Sk, generator=gen) >= p


# ----------------------------------------------------------------------------------------------- decode cases
def decode_splits(N, Hkv, max_len, bs):
    """The split count ops.attention._decode_splits derives from the max_len hint (kept in step by a CPU test)."""
    nblk = max(1, (max_len + bs - 1) // bs)
    want = max(1, -(-1024 // max(1, N * Hkv)))
    return int(max(1, min(want, nblk // 4, 64)))


def decode_targets(length, bs, splits):
    """Needle keys of one sequence, most telling first: the last key, key 0, the first and last key of every split
    range (ranges of ceil(nblk / splits) blocks, as the kernel cuts them), and the edges of the first four 16-key
    chunks of each range (one per wave) and of its last chunk."""
    if length <= 0:
        return []
    nblk = (length + bs - 1) // bs
    per = (nblk + splits - 1) // splits
    out = [length - 1, 0]
    ranges = []
    for sp in range(splits):
        b0, b1 = sp * per, min(nblk, sp * per + per)
        k0, k1 = b0 * bs, min(b1 * bs, length)
        if k0 < k1:
            ranges.append((k0, k1))
            out += [k0, k1 - 1]
    for k0, k1 in ranges:
        for c in range(4):
            out += [k0 + 16 * c + 15, k0 + 16 * c + 16]
        last = k0 + (k1 - 1 - k0) // 16 * 16
        out += [last - 1, last]
    seen, uniq = set(), []
    for t in out:
        if 0 <= t < length and t not in seen:
            seen.add(t)
            uniq.append(t)
    return uniq


def _fp32_bound(q, keys, vals, G):
    """2 |ds| max|v| with |ds| = 130 * 2^-24 * scale * max sum_i |q_i k_i|: the fp32 score error carried to o."""
    worst, vmax = 0.0, 0.0
    for n, (K, V) in enumerate(zip(keys, vals)):
        if K.shape[1] == 0:
            continue
        qn = q[n].double().abs().view(K.shape[0], G, -1)
        worst = max(worst, float(torch.einsum("kgd,kld->kgl", qn, K.double().abs()).max()))
        vmax = max(vmax, float(V.double().abs().max()))
    return 2 * 130 * 2.0 ** -24 * worst / math.sqrt(q.shape[-1]) * vmax


class DecodeCase:
    """Paged decode problem with NaN poison everywhere a correct kernel never reads: slots >= len of the last used
    block, whole blocks no table entry of a used position names, and the table entries past the used ones, which
    point at a poison block (a valid index of the cache). q [N, H, D]; every head of a sequence aims at another
    needle key (``decode_targets``); every fourth head stays plain."""

    def __init__(self, G, bs, lens, max_len=None, H=16, D=128, seed=0):
        N = len(lens)
        Hkv = H // G
        self.G, self.bs, self.lens_list, self.max_len = G, bs, lens, max_len
        self.N, self.H, self.Hkv, self.D = N, H, Hkv, D
        self.id = f"G{G}-bs{bs}-lens{'_'.join(map(str, lens))}-hint{max_len}"
        gen = torch.Generator().manual_seed(500 + seed)
        max_blocks = max(1, max((l + bs - 1) // bs for l in lens)) + 2
        self.splits = decode_splits(N, Hkv, max_blocks * bs if max_len is None else max_len, bs)
        nb = N * max_blocks + 4
        perm = torch.randperm(nb, generator=gen)
        poison_blocks = perm[N * max_blocks:]
        tab = perm[:N * max_blocks].view(N, max_blocks).clone()
        kc = torch.full((nb, Hkv, bs, D), float("nan"))
        vc = torch.full((nb, Hkv, bs, D), float("nan"))
        self.keys, self.vals = [], []      # valid keys per sequence [Hkv, len, D], bf16-rounded
        for n, ln in enumerate(lens):
            used = (ln + bs - 1) // bs
            K = torch.randn(Hkv, ln, D, generator=gen).bfloat16()
            V = torch.randn(Hkv, ln, D, generator=gen).bfloat16()
            self.keys.append(K)
            self.vals.append(V)
            for b in range(used):
                m = min(bs, ln - b * bs)
                kc[tab[n, b], :, :m] = K[:, b * bs:b * bs + m].float()
                vc[tab[n, b], :, :m] = V[:, b * bs:b * bs + m].float()
            tab[n, used:] = poison_blocks[n % len(poison_blocks)]
        q = 0.5 * torch.randn(N, H, D, generator=gen)
        self.targets = torch.full((N, H), -1, dtype=torch.long)
        for n, ln in enumerate(lens):
            cand = decode_targets(ln, bs, self.splits)
            rot = 5 * seed % max(1, len(cand) - 2)   # len - 1 and key 0 always; other cases start the rest elsewhere
            cand = cand[:2] + cand[2 + rot:] + cand[2:2 + rot]
            nxt = 0
            for h in range(H):
                if not cand or (h + n) % 4 == 3:
                    continue
                t = cand[nxt % len(cand)]
                nxt += 1
                self.targets[n, h] = t
                q[n, h] += (math.log(ln) + 1.0) / math.sqrt(D) * self.keys[n][h // G, t].float()
        self.q, self.kc, self.vc = q.bfloat16(), kc.bfloat16(), vc.bfloat16()
        self.tables, self.lens = tab.int(), torch.tensor(lens, dtype=torch.int32)

    def fp32_bound(self):
        return _fp32_bound(self.q, self.keys, self.vals, self.G)

    def reference(self, drop=None, stale=None, dt=torch.float64):
        """fp64 softmax over the valid keys only, gathered per sequence: [N, H, D]; zeros for len 0. ``drop``:
        mutant hook, (n, keys to lose); ``stale``: mutant hook, n: also read slot ``len`` of the cache. ``dt`` =
        float32 gives the model of a correct fp32 kernel that sets the absolute tolerance."""
        out = torch.zeros(self.N, self.H, self.D, dtype=dt)
        for n, ln in enumerate(self.lens_list):
            if ln == 0:
                continue
            K, V = self.keys[n].to(dt), self.vals[n].to(dt)
            if stale == n:
                blk, off = self.tables[n, ln // self.bs], ln % self.bs
                K = torch.cat([K, self.kc[blk, :, off:off + 1].to(dt)], 1)
                V = torch.cat([V, self.vc[blk, :, off:off + 1].to(dt)], 1)
            if drop is not None and drop[0] == n:
                sel = torch.ones(K.shape[1], dtype=torch.bool)
                sel[drop[1]] = False
                K, V = K[:, sel], V[:, sel]
            qn = self.q[n].to(dt).view(self.Hkv, self.G, self.D)
            p = torch.softmax(torch.einsum("kgd,kld->kgl", qn, K) / math.sqrt(self.D), -1)
            out[n] = torch.einsum("kgl,kld->kgd", p, V).reshape(self.H, self.D)
        return out


class DenseDecodeCase:
    """Dense-cache decode [B, Hkv, Lc, D]: positions >= len NaN-filled, needles at key 0, len - 1 and the 16-key
    chunk / 64-key virtual block edges."""

    def __init__(self, G, Lc, lens, H=16, D=128, seed=0):
        N, Hkv = len(lens), H // G
        self.G, self.Lc, self.lens_list, self.N, self.H, self.Hkv, self.D = G, Lc, lens, N, H, Hkv, D
        self.id = f"dense-G{G}-Lc{Lc}"
        self.splits = decode_splits(N, Hkv, Lc, 64)
        gen = torch.Generator().manual_seed(900 + seed)
        kc = torch.randn(N, Hkv, Lc, D, generator=gen).bfloat16()
        vc = torch.randn(N, Hkv, Lc, D, generator=gen).bfloat16()
        q = 0.5 * torch.randn(N, H, D, generator=gen)
        for n, ln in enumerate(lens):
            cand = decode_targets(ln, 64, self.splits)
            nxt = 0
            for h in range(H):
                if (h + n) % 4 == 3:
                    continue
                t = cand[nxt % len(cand)]
                nxt += 1
                q[n, h] += (math.log(ln) + 1.0) / math.sqrt(D) * kc[n, h // G, t].float()
            kc[n, :, ln:] = float("nan")
            vc[n, :, ln:] = float("nan")
        self.q, self.kc, self.vc, self.lens = q.bfloat16(), kc, vc, torch.tensor(lens, dtype=torch.int32)

    def fp32_bound(self):
        ks = [self.kc[n, :, :ln] for n, ln in enumerate(self.lens_list)]
        return _fp32_bound(self.q, ks, [self.vc[n, :, :ln] for n, ln in enumerate(self.lens_list)], self.G)

    def reference(self, dt=torch.float64):
        out = torch.zeros(self.N, self.H, self.D, dtype=dt)
        for n, ln in enumerate(self.lens_list):
            K, V = self.kc[n, :, :ln].to(dt), self.vc[n, :, :ln].to(dt)
            qn = self.q[n].to(dt).view(self.Hkv, self.G, self.D)
            p = torch.softmax(torch.einsum("kgd,kld->kgl", qn, K) / math.sqrt(self.D), -1)
            out[n] = torch.einsum("kgl,kld->kgd", p, V).reshape(self.H, self.D)
        return out


def decode_specs():
    """(G, block size, lens, max_len hint, seed): G x block size, each with lens mixing 0, 1, bs - 1, bs, bs + 1, 63,
    64, 65, 1025, under three hints: one split, two, and the maximum the table capacity allows (there the short
    sequences leave splits empty)."""
    out = []
    for i, (G, bs) in enumerate([(1, 8), (2, 16), (4, 64), (8, 128), (2, 128), (8, 8), (1, 64), (4, 16)]):
        lens = [0, 1, bs - 1, bs, bs + 1, 63, 64, 65, 1025]
        out += [(G, bs, lens, hint, i) for hint in (4 * bs, 8 * bs, None)]
    return out


def dense_decode_specs():
    """(G, Lc, lens, seed); lens 1, 64, 65, Lc (33 for 65 where Lc = 64)."""
    return [(G, Lc, [1, 64, 65 if Lc > 64 else 33, Lc], G) for G in (1, 2, 4, 8) for Lc in (64, 512)]


def decode_cases():
    return [DecodeCase(G, bs, lens, hint, seed=i) for G, bs, lens, hint, i in decode_specs()]


def dense_decode_cases():
    return [DenseDecodeCase(G, Lc, lens, seed=sd) for G, Lc, lens, sd in dense_decode_specs()]


# ------------------------------------------------------------------------------------------------ measurement
def uncovered(got, ref, rtol):
    """Worst error the rtol term does not cover: max(|got - ref| - rtol |ref|), the least atol that passes."""
    return float(((got.double() - ref).abs() - rtol * ref.abs()).max())


def measure(verbose=True):
    """Least atol with which the rounding model passes ``check`` against the fp64 reference (``uncovered``), worst
    over every case of the GPU files, per dtype and output (o: absolute; dq / dk / dv: as a fraction of max|ref|);
    the error of the fp32 LSE; and the same for an fp32 model of decode (bf16 output)."""
    worst = {dt: {n: (0.0, "") for n in ("o", "dq", "dk", "dv")} for dt in (torch.bfloat16, torch.float16)}
    lse_w = (0.0, "")
    groups = [plain_cases(), route_cases(), feature_cases(), misc_cases(), dropout_cases(), bhsd_cases(),
              dead_row_cases()]
    for gi, cases in enumerate(groups):
        for c in cases:
            t, kw = c.dense()
            if gi == 4:
                kw.update(keep=dropout_keep(c), drop_p=0.3)
            ref, mod = reference(*t, **kw), rounding_model(*t, **kw)
            for n in ("o", "dq", "dk", "dv"):
                e = uncovered(mod[n], ref[n], RTOL[c.dtype])
                if n != "o":
                    e /= max(float(ref[n].abs().max()), 1e-30)
                if e > worst[c.dtype][n][0]:
                    worst[c.dtype][n] = (e, c.id)
            l32 = lse_fp32(t[0], t[1], kw["vis"], kw["bias"], kw["scale"]).double()
            fin = torch.isfinite(ref["lse"])
            assert torch.equal(torch.isfinite(l32), fin)
            e = float((l32 - ref["lse"])[fin].abs().max()) if fin.any() else 0.0
            if e > lse_w[0]:
                lse_w = (e, c.id)
    dec_w, dec_bound = (0.0, ""), 0.0
    for c in decode_cases() + dense_decode_cases():
        dec_bound = max(dec_bound, c.fp32_bound())
        e = uncovered(c.reference(dt=torch.float32).bfloat16(), c.reference(), RTOL[torch.bfloat16])
        if e > dec_w[0]:
            dec_w = (e, c.id)
    if verbose:
        for dt, d in worst.items():
            for n, (e, cid) in d.items():
                print(f"{str(dt):16s} {n:3s} uncovered {e:.4g}  x4 = {4 * e:.4g}   ({cid})")
        print(f"lse fp32 vs fp64 worst {lse_w[0]:.4g}  x8 = {8 * lse_w[0]:.4g}   ({lse_w[1]})")
        print(f"decode fp32 model uncovered {dec_w[0]:.4g} ({dec_w[1]}); fp32 bound 2 |ds| max|v| = {dec_bound:.4g}")
    return worst, lse_w, dec_w, dec_bound


if __name__ == "__main__":
    measure()
