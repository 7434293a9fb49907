"""Decode-attention problems over an int8 KV cache (uint8 storage = int8 + 128) on which the quantised cache is the
exact input, so no quantisation error can hide a kernel bug. Plain helper module like ``attn_needles``, whose
needle targets, split rule, ``check`` / ``excess`` and decode tolerance it reuses unchanged.

* K and V are the integers round(32 N(0, 1)) clamped to +-127, stored + 128. A cached element means
  (u - 128) * dq[kv head] with distinct, non-power-of-two per-head scales that differ between K and V.
* The reference is fp64 softmax over the valid dequantised keys, gathered per sequence. Needle queries are built
  from the dequantised keys exactly as ``attn_needles.DecodeCase`` builds them.
* uint8 has no NaN, so the poison is content: every slot a correct kernel never reads (slots >= len, unreferenced
  blocks, the block the spare table entries name) holds K = that kv head's first needle key and V = 255. A kernel
  that reads one gives the needle's weight to the value 127 * dq.
* ``cur=True`` adds k_cur / v_cur (bf16 [N, Hkv, D]) that replace key len - 1 of every sequence; the cache slot
  len - 1 is then poisoned too.

``reference(mutant=...)`` gives deliberately wrong references (what a kernel with that bug would compute); the CPU
test asserts that each is far outside the tolerance, i.e. that these cases can see the bug.
"""
from __future__ import annotations

import math

import torch

import attn_needles as A

MUTANTS = ["no_offset", "head_scale", "swap_scales", "drop_last", "stale", "cur_ignored"]
LOG2E = 1.4426950408889634


def dequant_scales(Hkv):
    """(k_dequant, v_dequant) fp32 [Hkv]: distinct per head, no powers of two, K and V different."""
    h = torch.arange(Hkv, dtype=torch.float64)
    return ((1 + 0.173 * h) / 32).float(), ((0.7 + 0.291 * h) / 32).float()


def _ints(gen, *shape):
    return torch.round(32 * torch.randn(*shape, generator=gen)).clamp(-127, 127)


class _Q8Case:
    """Shared by the paged and the dense form. After ``_finish``: q bf16 [N, H, D]; kq / vq: per sequence the valid
    cached integers [Hkv, len, D] (fp64); k_cur / v_cur bf16 [N, Hkv, D] or None; k_dq / v_dq fp32 [Hkv]."""

    def _init_common(self, G, lens, H, D, cur, gen):
        self.G, self.lens_list, self.N, self.H, self.Hkv, self.D, self.cur = G, lens, len(lens), H, H // G, D, cur
        self.k_dq, self.v_dq = dequant_scales(self.Hkv)
        self.kq = [_ints(gen, self.Hkv, ln, D).double() for ln in lens]
        self.vq = [_ints(gen, self.Hkv, ln, D).double() for ln in lens]
        self.k_cur = self.v_cur = None
        if cur:
            self.k_cur = torch.randn(self.N, self.Hkv, D, generator=gen).bfloat16()
            self.v_cur = torch.randn(self.N, self.Hkv, D, generator=gen).bfloat16()

    def keys(self, n):
        """Dequantised valid keys / values of sequence n in fp64 [Hkv, len, D], key len - 1 from k_cur when given."""
        K = self.kq[n] * self.k_dq.double().view(-1, 1, 1)
        V = self.vq[n] * self.v_dq.double().view(-1, 1, 1)
        if self.cur and self.lens_list[n] > 0:
            K[:, -1], V[:, -1] = self.k_cur[n].double(), self.v_cur[n].double()
        return K, V

    def _needles(self, gen, bs, seed):
        """q and the needle targets, as attn_needles.DecodeCase; also the poison key bytes pk [N, Hkv, D] (uint8):
        per kv head the first needle key of the sequence (for a k_cur target its nearest int8 image)."""
        N, H, D, G = self.N, self.H, self.D, self.G
        q = 0.5 * torch.randn(N, H, D, generator=gen)
        self.targets = torch.full((N, H), -1, dtype=torch.long)
        pk = torch.full((N, self.Hkv, D), 128.0, dtype=torch.float64)
        for n, ln in enumerate(self.lens_list):
            cand = A.decode_targets(ln, bs, self.splits)
            rot = 5 * seed % max(1, len(cand) - 2)
            cand = cand[:2] + cand[2 + rot:] + cand[2:2 + rot]
            K, _ = self.keys(n)
            nxt, first = 0, {}
            for h in range(H):
                if not cand or (h + n) % 4 == 3:
                    continue
                t = cand[nxt % len(cand)]
                nxt += 1
                self.targets[n, h] = t
                first.setdefault(h // G, t)
                q[n, h] += (math.log(ln) + 1.0) / math.sqrt(D) * K[h // G, t].float()
            for hk in range(self.Hkv):
                if ln == 0:
                    continue
                t = first.get(hk, ln - 1)
                img = torch.round(K[hk, t] / self.k_dq[hk].double()).clamp(-127, 127)
                pk[n, hk] = img + 128
        self.q = q.bfloat16()
        self.pk = pk.to(torch.uint8)
        self.lens = torch.tensor(self.lens_list, dtype=torch.int32)

    def slot(self, n, pos):
        """Cache bytes (K, V) uint8 [Hkv, D] of sequence n at position pos (subclasses)."""
        raise NotImplementedError

    def applies(self, mutant):
        if mutant == "head_scale":
            return self.Hkv > 1
        if mutant == "cur_ignored":
            return self.cur
        if mutant == "stale":   # a slot ``len`` must exist in the sequence's table row / dense row
            return any(self.has_slot(n, ln) for n, ln in enumerate(self.lens_list) if ln > 0)
        return True

    def reference(self, mutant=None, dt=torch.float64, kernel_model=False):
        """Softmax over the valid dequantised keys per sequence: [N, H, D] in ``dt``; zeros for len 0.
        ``dt=float32`` is the fp32 model of the op. ``kernel_model`` (fp32): the arithmetic of the HIP kernel: q
        times scale * log2(e), dotted with the integers u - 128, the reduced score times k_dq; exp2 weights times
        v_dq, times the integer values; normalised at the end. ``mutant``: one of MUTANTS, applied to every sequence
        it can apply to."""
        out = torch.zeros(self.N, self.H, self.D, dtype=dt)
        Hkv, G, D = self.Hkv, self.G, self.D
        kdq, vdq = self.k_dq.double(), self.v_dq.double()
        if mutant == "head_scale":
            kdq, vdq = kdq.roll(-1), vdq.roll(-1)
        if mutant == "swap_scales":
            kdq, vdq = vdq, kdq
        off = 0.0 if mutant == "no_offset" else 128.0
        for n, ln in enumerate(self.lens_list):
            if ln == 0:
                continue
            Ki, Vi = self.kq[n] + 128.0 - off, self.vq[n] + 128.0 - off            # the integers as (mis)read
            ks = kdq.view(-1, 1).expand(Hkv, ln).clone()
            vs = vdq.view(-1, 1).expand(Hkv, ln).clone()
            if self.cur and mutant != "cur_ignored":
                Ki, Vi = Ki.clone(), Vi.clone()
                Ki[:, -1], Vi[:, -1] = self.k_cur[n].double(), self.v_cur[n].double()
                ks[:, -1], vs[:, -1] = 1.0, 1.0
            elif self.cur:   # the bug: the cache slot len - 1 is read instead of k_cur / v_cur
                kb, vb = self.slot(n, ln - 1)
                Ki, Vi = Ki.clone(), Vi.clone()
                Ki[:, -1], Vi[:, -1] = kb.double() - off, vb.double() - off
            if mutant == "stale" and self.has_slot(n, ln):
                kb, vb = self.slot(n, ln)
                Ki = torch.cat([Ki, (kb.double() - off).unsqueeze(1)], 1)
                Vi = torch.cat([Vi, (vb.double() - off).unsqueeze(1)], 1)
                ks = torch.cat([ks, kdq.view(-1, 1)], 1)
                vs = torch.cat([vs, vdq.view(-1, 1)], 1)
            if mutant == "drop_last":
                Ki, Vi, ks, vs = Ki[:, :-1], Vi[:, :-1], ks[:, :-1], vs[:, :-1]
                if Ki.shape[1] == 0:
                    continue
            qn = self.q[n].to(dt).view(Hkv, G, D)
            if kernel_model:
                assert dt == torch.float32
                s = torch.einsum("kgd,kld->kgl", qn * (LOG2E / math.sqrt(D)), Ki.float()) * ks.float()[:, None]
                p = torch.exp2(s - s.amax(-1, keepdim=True))
                o = torch.einsum("kgl,kld->kgd", p * vs.float()[:, None], Vi.float()) / p.sum(-1, keepdim=True)
            else:
                K, V = (Ki * ks.unsqueeze(-1)).to(dt), (Vi * vs.unsqueeze(-1)).to(dt)
                p = torch.softmax(torch.einsum("kgd,kld->kgl", qn, K) / math.sqrt(D), -1)
                o = torch.einsum("kgl,kld->kgd", p, V)
            out[n] = o.reshape(self.H, D)
        return out

    def cur_kwargs(self, device="cpu"):
        kw = dict(k_dequant=self.k_dq.to(device), v_dequant=self.v_dq.to(device))
        if self.cur:
            kw.update(k_cur=self.k_cur.to(device), v_cur=self.v_cur.to(device))
        return kw


class PagedCase(_Q8Case):
    """Paged form: kc / vc uint8 [nb, Hkv, bs, D], tables int32 [N, max_blocks] with two spare entries per row that
    name a poison block, four unreferenced blocks."""

    def __init__(self, G, bs, lens, max_len=None, H=16, D=128, seed=0, cur=False):
        gen = torch.Generator().manual_seed(7500 + seed)
        self._init_common(G, lens, H, D, cur, gen)
        N, Hkv = self.N, self.Hkv
        self.bs, self.max_len = bs, max_len
        self.id = f"G{G}-bs{bs}-hint{max_len}-{'cur' if cur else 'nocur'}"
        max_blocks = max(1, max((l + bs - 1) // bs for l in lens)) + 2
        self.splits = A.decode_splits(N, Hkv, max_blocks * bs if max_len is None else max_len, bs)
        nb = N * max_blocks + 4
        perm = torch.randperm(nb, generator=gen)
        poison_blocks = perm[N * max_blocks:]
        tab = perm[:N * max_blocks].view(N, max_blocks).clone()
        self._needles(gen, bs, seed)
        nref = max(range(N), key=lambda n: lens[n])          # whole poison blocks: the longest sequence's needle keys
        kc = self.pk[nref].view(1, Hkv, 1, D).expand(nb, Hkv, bs, D).clone()
        vc = torch.full((nb, Hkv, bs, D), 255, dtype=torch.uint8)
        for n, ln in enumerate(lens):
            used = (ln + bs - 1) // bs
            for b in range(used):
                m = min(bs, ln - b * bs)
                kc[tab[n, b], :, :m] = (self.kq[n][:, b * bs:b * bs + m] + 128).to(torch.uint8)
                vc[tab[n, b], :, :m] = (self.vq[n][:, b * bs:b * bs + m] + 128).to(torch.uint8)
                kc[tab[n, b], :, m:] = self.pk[n].unsqueeze(1)
            if cur and ln > 0:
                kc[tab[n, (ln - 1) // bs], :, (ln - 1) % bs] = self.pk[n]
                vc[tab[n, (ln - 1) // bs], :, (ln - 1) % bs] = 255
            tab[n, used:] = poison_blocks[n % len(poison_blocks)]
        self.kc, self.vc, self.tables = kc, vc, tab.int()

    def has_slot(self, n, pos):
        return pos // self.bs < self.tables.shape[1]

    def slot(self, n, pos):
        blk = int(self.tables[n, pos // self.bs])
        return self.kc[blk, :, pos % self.bs], self.vc[blk, :, pos % self.bs]


class DenseCase(_Q8Case):
    """Dense form: kc / vc uint8 [N, Hkv, Lc, D], positions >= len poisoned; needles on the 64-key virtual blocks."""

    def __init__(self, G, Lc, lens, H=16, D=128, seed=0, cur=False):
        gen = torch.Generator().manual_seed(7900 + seed)
        self._init_common(G, lens, H, D, cur, gen)
        N, Hkv = self.N, self.Hkv
        self.Lc = Lc
        self.id = f"dense-G{G}-Lc{Lc}-{'cur' if cur else 'nocur'}"
        self.splits = A.decode_splits(N, Hkv, Lc, 64)
        self._needles(gen, 64, 0)
        kc = self.pk.view(N, Hkv, 1, D).expand(N, Hkv, Lc, D).clone()
        vc = torch.full((N, Hkv, Lc, D), 255, dtype=torch.uint8)
        for n, ln in enumerate(lens):
            kc[n, :, :ln] = (self.kq[n] + 128).to(torch.uint8)
            vc[n, :, :ln] = (self.vq[n] + 128).to(torch.uint8)
            if cur and ln > 0:
                kc[n, :, ln - 1] = self.pk[n]
                vc[n, :, ln - 1] = 255
        self.kc, self.vc = kc, vc

    def has_slot(self, n, pos):
        return pos < self.Lc

    def slot(self, n, pos):
        return self.kc[n, :, pos], self.vc[n, :, pos]


def paged_specs():
    """(G, bs, lens, hint, seed, cur): every geometry of attn_needles.decode_specs(), with and without k_cur."""
    return [s + (cur,) for s in A.decode_specs() for cur in (False, True)]


def dense_specs():
    return [s + (cur,) for s in A.dense_decode_specs() for cur in (False, True)]


def spec_id(s):
    return (f"G{s[0]}-bs{s[1]}-hint{s[3]}-{'cur' if s[5] else 'nocur'}" if len(s) == 6
            else f"G{s[0]}-Lc{s[1]}-{'cur' if s[4] else 'nocur'}")


def make(spec):
    if len(spec) == 6:
        G, bs, lens, hint, seed, cur = spec
        return PagedCase(G, bs, lens, hint, seed=seed, cur=cur)
    G, Lc, lens, seed, cur = spec
    return DenseCase(G, Lc, lens, seed=seed, cur=cur)


def measure():
    """Prints, per case, the fp32 models' excess over the tolerance and each mutant's (python tests/kv8_cases.py)."""
    atol, rtol = A.DECODE_ATOL, A.RTOL[torch.bfloat16]
    for spec in paged_specs() + dense_specs():
        c = make(spec)
        ref = c.reference()
        row = [f"{c.id:34s}"]
        for km in (False, True):
            row.append(f"fp32{'k' if km else ' '} {A.excess(c.reference(dt=torch.float32, kernel_model=km).bfloat16(), ref, atol, rtol)[0]:.3f}")
        for m in MUTANTS:
            if c.applies(m):
                row.append(f"{m} {A.excess(c.reference(mutant=m).bfloat16(), ref, atol, rtol)[0]:.3g}")
        print("  ".join(row))


if __name__ == "__main__":
    measure()
