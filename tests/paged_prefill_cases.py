"""One batch builder for the paged prefill attention tests (CPU and GPU), on tests/attn_needles.py inputs.

Per sequence (start, n): ``A.needle_inputs(1, n, start + n, ..., A.causal_keep(n, start + n))``, so the needle and trap
rows sit on the causal diagonal: the chunk's own later tokens are in the cache and dominate a row if the limit is off
by one. K / V go into a paged cache through a shuffled block table (or a dense [B, Hkv, Lc, D] cache). Everything a
correct kernel never reads is poison: unreferenced blocks, slots at or past ctx_len, the block the spare table entries
name. Float caches: NaN. uint8 caches: K byte 0, V byte 255, and K = round(32 k), V = round(16 v) clamped to +-127 with
dequant scales 1/32 and 1/16, so the dequantised cache is the exact input of the fp64 reference.
"""
from types import SimpleNamespace

import torch

import attn_needles as A

D, HKV = 128, 2


def batch(G):
    """(start, n): crosses a query tile with a first row that sees one key; start inside a block past a 64-key tile;
    an empty chunk in the middle; a decode-like single token."""
    return [(0, 128 // G + 2), (70, 37), (5, 0), (130, 1)]


def build(G, bs, quant=False, dense_lc=None, dtype=torch.bfloat16, seqs=None, pad=3):
    seqs = batch(G) if seqs is None else seqs
    H, B = G * HKV, len(seqs)
    qs, ks, vs, refs, mods = [], [], [], [], []
    for b, (start, n) in enumerate(seqs):
        m = max(n, 1)   # an empty chunk still has its history in the cache
        q, k, v, do = A.needle_inputs(1, m, start + m, H, HKV, D, dtype, A.causal_keep(m, start + m), seed=b)
        if quant:
            k = ((32 * k.float()).round().clamp(-127, 127) / 32).to(dtype)
            v = ((16 * v.float()).round().clamp(-127, 127) / 16).to(dtype)
        q, k, v, do = q[:, :n], k[:, :start + n], v[:, :start + n], do[:, :n]
        qs.append(q[0])
        ks.append(k[0].transpose(0, 1))   # [Hkv, ctx, D]
        vs.append(v[0].transpose(0, 1))
        for fn, dst in ((A.reference, refs), (A.rounding_model, mods)):
            dst.append(fn(q, k, v, do, A.causal_keep(n, start + n))["o"][0] if n else torch.zeros(0, H, D).double())
    ctx = [s + n for s, n in seqs]
    cdt = torch.uint8 if quant else dtype
    kpoison, vpoison = (0, 255) if quant else (float("nan"), float("nan"))

    def stored(t, mul):
        return (mul * t.float() + 128).to(torch.uint8) if quant else t

    if dense_lc is not None:
        kc = torch.full((B, HKV, dense_lc, D), kpoison, dtype=cdt)
        vc = torch.full((B, HKV, dense_lc, D), vpoison, dtype=cdt)
        for b in range(B):
            kc[b, :, :ctx[b]], vc[b, :, :ctx[b]] = stored(ks[b], 32), stored(vs[b], 16)
        tables = None
    else:
        gen = torch.Generator().manual_seed(31 + G + bs)
        max_blocks = max((c + bs - 1) // bs for c in ctx) + 2
        perm = torch.randperm(B * max_blocks + 4, generator=gen)
        tables = perm[:B * max_blocks].view(B, max_blocks).clone()
        kc = torch.full((perm.numel(), HKV, bs, D), kpoison, dtype=cdt)
        vc = torch.full((perm.numel(), HKV, bs, D), vpoison, dtype=cdt)
        for b in range(B):
            used = (ctx[b] + bs - 1) // bs
            for j in range(used):
                m = min(bs, ctx[b] - j * bs)
                kc[tables[b, j], :, :m] = stored(ks[b][:, j * bs:j * bs + m], 32)
                vc[tables[b, j], :, :m] = stored(vs[b][:, j * bs:j * bs + m], 16)
            tables[b, used:] = perm[B * max_blocks + b % 4]
        tables = tables.int()
    junk = torch.randn(pad, H, D, generator=torch.Generator().manual_seed(3)).to(dtype)   # rows past cu_q[B]
    zeros = torch.zeros(pad, H, D).double()
    kw = dict(k_dequant=torch.full((HKV,), 1 / 32), v_dequant=torch.full((HKV,), 1 / 16)) if quant else {}
    ns = [n for _, n in seqs]
    return SimpleNamespace(
        q=torch.cat(qs + [junk]), kc=kc, vc=vc, tables=tables, kw=kw, H=H, max_q=max(ns), pad=pad,
        cu=torch.tensor([0] + list(torch.tensor(ns).cumsum(0)), dtype=torch.int32),
        ctx=torch.tensor(ctx, dtype=torch.int32), ref=torch.cat(refs + [zeros]), model=torch.cat(mods + [zeros]))


def run(op_paged, op_dense, c, device="cpu", **extra):
    """The op on case ``c`` (the dense form when the case has no tables)."""
    t = {k: v.to(device) for k, v in dict(q=c.q, kc=c.kc, vc=c.vc, cu=c.cu, ctx=c.ctx).items()}
    kw = {k: v.to(device) for k, v in c.kw.items()}
    if c.tables is None:
        return op_dense(t["q"], t["kc"], t["vc"], t["cu"], t["ctx"], **kw, **extra)
    return op_paged(t["q"], t["kc"], t["vc"], c.tables.to(device), t["cu"], t["ctx"], **kw, **extra)
