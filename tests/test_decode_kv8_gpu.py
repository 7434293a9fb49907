"""int8 KV cache on the GPU: the flash-decoding kernel reading uint8 caches (pa_paged_decode_attn_q8) on the exact
needle cases of tests/kv8_cases.py, the quantising RoPE + cache write (pa_decode_rope_cache_q8) bit for bit against
the torch formula, block_multihead_attention's decode phase on the uint8 caches against its math path, and LLaMA
generation on an int8 cache (graph replay, teacher-forced logits against the fallbacks)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_needles as A  # noqa: E402
import kv8_cases as C  # noqa: E402
import paddlepaddle_amd as paddle  # noqa: E402
import paddlepaddle_amd.incubate.nn.functional as IF  # noqa: E402
from paddlepaddle_amd import ops  # noqa: E402
from paddlepaddle_amd.framework import flags  # noqa: E402
from paddlepaddle_amd.ops import _loader as L  # noqa: E402
from paddlepaddle_amd.ops.rope import rope_tables  # noqa: E402

DEV = "cuda"
Q8 = "pa_paged_decode_attn_q8"


def _check(case, got, before):
    ref = case.reference().to(DEV)
    r, idx = A.excess(got, ref, A.DECODE_ATOL, A.RTOL[torch.bfloat16])
    print(f"[kv8] {case.id} splits {case.splits}: {r:.3f} x tol at {idx}")
    A.check(got, ref, A.DECODE_ATOL, A.RTOL[torch.bfloat16], what=case.id)
    for n, ln in enumerate(case.lens_list):
        if ln == 0:
            assert float(got[n].abs().max()) == 0.0, "an empty sequence gives zeros"
    assert L.calls(Q8) == before + 1


@pytest.mark.parametrize("spec", C.paged_specs(), ids=C.spec_id)
def test_paged_decode_q8_needles(spec):
    case = C.make(spec)
    hint = spec[3]
    want_splits = 1 if hint == 4 * case.bs else 2 if hint == 8 * case.bs else None
    assert case.splits == want_splits or (want_splits is None and case.splits >= 2)
    assert int(case.tables.max()) < case.kc.shape[0] and int(case.tables.min()) >= 0
    q, kc, vc, tab, ln = (t.to(DEV) for t in (case.q, case.kc, case.vc, case.tables, case.lens))
    before = L.calls(Q8)
    _check(case, ops.paged_decode_attention(q, kc, vc, tab, ln, max_len=hint, **case.cur_kwargs(DEV)), before)


@pytest.mark.parametrize("spec", C.dense_specs(), ids=C.spec_id)
def test_dense_decode_q8_needles(spec):
    case = C.make(spec)
    q, kc, vc, ln = (t.to(DEV) for t in (case.q, case.kc, case.vc, case.lens))
    before = L.calls(Q8)
    _check(case, ops.dense_decode_attention(q, kc, vc, ln, **case.cur_kwargs(DEV)), before)


def _quant_formula(x, scale):
    z = x.float() * scale.float().view(-1, 1)
    z = torch.sign(z) * torch.floor(z.abs() + 0.5)
    return (z.clamp(-127, 127) + 128).to(torch.uint8)


@pytest.mark.parametrize("p", [0, 41])   # position 0: cos 1, sin 0, the rotated K is the input (exact ties reach K)
@pytest.mark.parametrize("H,Hkv,D", [(32, 32, 128), (8, 2, 128), (4, 4, 64)])
def test_decode_rope_cache_q8_hip(H, Hkv, D, p):
    g = torch.Generator().manual_seed(H + D + p)
    B, Bc, Lc = 3, 4, 64
    qkv = torch.randn(B, H + 2 * Hkv, D, generator=g)
    # kv head 0 of K and V: scale 16 and values (2m + 1) / 32, so x * scale = m + 0.5 exactly; plus values that clamp
    m = torch.randint(-100, 100, (B, D), generator=g).float()
    tie = (2 * m + 1) / 32
    tie[:, :4] = torch.tensor([20.0, -20.0, 7.96875, -7.96875])   # 320 -> 127, -320 -> -127, +-127.5 -> +-127
    qkv[:, H], qkv[:, H + Hkv] = tie, tie.flip(0)
    qkv = qkv.reshape(B, -1).to(DEV, torch.bfloat16)
    ks = (torch.rand(Hkv, generator=g) * 60 + 20).to(DEV)
    vs = (torch.rand(Hkv, generator=g) * 60 + 20).to(DEV)
    ks[0], vs[0] = 16.0, 16.0
    cos, sin = rope_tables(Lc, D, device=DEV)
    pos = torch.tensor([p], device=DEV)
    cs, sn = cos.index_select(0, pos), sin.index_select(0, pos)
    kf = torch.zeros(Bc, Hkv, Lc, D, device=DEV, dtype=torch.bfloat16)
    vf = torch.zeros_like(kf)
    q_ref = ops.decode_rope_cache(qkv, H, Hkv, D, cs, sn, pos, kf, vf)
    kc = torch.randint(0, 256, (Bc, Hkv, Lc, D), generator=g, dtype=torch.uint8).to(DEV)
    vc = torch.randint(0, 256, (Bc, Hkv, Lc, D), generator=g, dtype=torch.uint8).to(DEV)
    kc0, vc0 = kc.clone(), vc.clone()
    before = L.calls("pa_decode_rope_cache_q8")
    q = ops.decode_rope_cache(qkv, H, Hkv, D, cs, sn, pos, kc, vc, k_scale=ks, v_scale=vs)
    assert L.calls("pa_decode_rope_cache_q8") == before + 1
    assert torch.equal(q, q_ref), "q is the bf16 kernel's, bit for bit"
    want_k, want_v = _quant_formula(kf[:B, :, p], ks), _quant_formula(vf[:B, :, p], vs)
    assert torch.equal(kc[:B, :, p], want_k) and torch.equal(vc[:B, :, p], want_v)
    # the ties and the clamps were there: V of kv head 0 is z = m + 0.5 -> sign(z) * (|m + 0.5| + 0.5)
    zt = tie.flip(0).to(DEV) * 16
    assert torch.equal(vc[:B, 0, p].float() - 128, (torch.sign(zt) * torch.floor(zt.abs() + 0.5)).clamp(-127, 127))
    assert int((vc[:B, 0, p] == 255).sum()) >= 2 and int((vc[:B, 0, p] == 1).sum()) >= 2
    if p == 0:
        assert torch.equal(kc[:B, 0, p], _quant_formula(tie.to(DEV), ks[:1]))
    kc[:B, :, p], vc[:B, :, p] = kc0[:B, :, p], vc0[:B, :, p]
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0), "every other cache byte is untouched"


def _blha(dynamic):
    """A prefill step fills four sequences; then a mixed step (three decode, the fourth prefills a new prompt) and a
    decode-only step, each run on the uint8 caches through the q8 kernel and, with tgt_mask = zeros, through the
    math path over the dequantised view."""
    H, Hk, D, bs, B = 4, 2, 128, 16, 4
    W = (H + 2 * Hk) * D
    gen = torch.Generator().manual_seed(17 + dynamic)
    tol = 3e-2   # the tolerance of test_serving_ops.py::test_block_mha_static_int8_cache_gpu_bf16
    kq = torch.full((B * 3 + 1, Hk, bs, D), 128, dtype=torch.uint8, device=DEV)
    vq = kq.clone()
    tables = torch.arange(B * 3, dtype=torch.int32, device=DEV).view(B, 3)
    if dynamic:
        sc = [torch.zeros(B, Hk, device=DEV) for _ in range(4)]
    else:
        ksc, vsc = torch.tensor([40.0, 60.0], device=DEV), torch.tensor([50.0, 30.0], device=DEV)
        sc = [ksc, vsc, 1.0 / ksc, 1.0 / vsc]
    P = paddle.to_tensor
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731

    def call(per_seq, caches, tgt=False, hints=None):
        toks = torch.cat([t for _, _, t in per_seq]).to(DEV, torch.bfloat16)
        n = [t.shape[0] for _, _, t in per_seq]
        cu = i32(np.concatenate([[0], np.cumsum(n)]).tolist())
        extra = dict(cache_k_quant_scales=P(sc[0]), cache_v_quant_scales=P(sc[1]), cache_k_dequant_scales=P(sc[2]),
                     cache_v_dequant_scales=P(sc[3]), use_dynamic_cachekv_quant=bool(dynamic))
        if tgt:
            extra["tgt_mask"] = P(torch.zeros(len(per_seq), 1, 1, 3 * bs, device=DEV, dtype=torch.bfloat16))
        if hints is not None:
            extra.update(max_enc_len_this_time=paddle.to_tensor(np.array([hints[0]], "int32"), place=paddle.CPUPlace()),
                         max_dec_len_this_time=paddle.to_tensor(np.array([hints[1]], "int32"), place=paddle.CPUPlace()))
        out = IF.block_multihead_attention(
            P(toks), P(caches[0]), P(caches[1]), P(i32([e for e, _, _ in per_seq])), P(i32([d for _, d, _ in per_seq])),
            P(i32(n)), None, None, P(cu), P(cu), P(tables[:len(per_seq)]), block_size=bs, **extra)[0]
        return out._t.float()

    rnd = lambda n: torch.randn(n, W, generator=gen) * 0.5  # noqa: E731
    call([(21, 0, rnd(21)), (16, 0, rnd(16)), (5, 0, rnd(5)), (3, 0, rnd(3))], (kq, vq))
    assert int((kq != 128).sum()) > 0
    steps = [([(0, 21, rnd(1)), (0, 16, rnd(1)), (0, 5, rnd(1)), (7, 0, rnd(7))], None),     # mixed, no hints
             ([(0, 22, rnd(1)), (0, 17, rnd(1)), (0, 6, rnd(1)), (0, 7, rnd(1))], (0, 22))]  # decode only, hints
    for per_seq, hints in steps:
        snap = (kq.clone(), vq.clone())
        sc_snap = [t.clone() for t in sc]
        before = L.calls(Q8)
        got = call(per_seq, (kq, vq), hints=hints)
        assert L.calls(Q8) == before + 1, "the decode phase ran the q8 kernel on the uint8 caches"
        for t, s in zip(sc, sc_snap):     # (the dynamic variant rewrites the scale rows: same start for the twin)
            t.copy_(s)
        want = call(per_seq, snap, tgt=True, hints=hints)
        assert L.calls(Q8) == before + 1
        assert torch.equal(snap[0], kq) and torch.equal(snap[1], vq)
        print(f"[kv8] blha dynamic={dynamic} hints={hints}: max |diff| {float((got - want).abs().max()):.4g}")
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=tol, atol=tol)


def test_block_mha_int8_static_scales():
    _blha(False)


def test_block_mha_int8_dynamic_scales():
    _blha(True)


def _tiny_llama():
    from paddlepaddle_amd.models.llama import LlamaConfig, LlamaForCausalLM
    paddle.set_device("gpu")
    paddle.seed(23)
    # The config's own initializer_range (0.02): logits reach ~1.1. Turning the HIP kernels off swaps every GEMM and
    # norm of the model for its fallback, and that noise grows with the weight scale: measured on the bf16 cache
    # (the path that existed before), HIP against fallback logits differ by 0.26 x the tolerance below at 0.02,
    # 0.98 x at 0.05 and 2.05 x at 0.1; the int8 cache: 0.30 x, 1.01 x, 1.95 x. Larger weights would test the GEMMs.
    cfg = LlamaConfig.tiny(num_hidden_layers=2, hidden_size=256, intermediate_size=512, num_attention_heads=2,
                           num_key_value_heads=1, vocab_size=512)
    model = LlamaForCausalLM(cfg)
    model.to(dtype="bfloat16")
    model.eval()
    return cfg, model


def test_llama_int8_cache_graph_and_logits():
    prev = paddle.get_device()
    try:
        _llama_int8_cache_graph_and_logits()
    finally:
        paddle.set_device(prev)   # _tiny_llama selects the GPU: leave the process's device as it was


def _llama_int8_cache_graph_and_logits():
    from paddlepaddle_amd.models.llama import Int8KVCache
    cfg, model = _tiny_llama()
    Ly = cfg.num_hidden_layers
    prompt = torch.randint(3, cfg.vocab_size, (2, 5), generator=torch.Generator().manual_seed(2))
    ids = paddle.to_tensor(prompt.numpy(), place=paddle.CUDAPlace(0))
    before = L.calls(Q8)
    eager, _ = model.generate(ids, max_new_tokens=6, eos_token_id=-1, kv_cache_dtype="int8", use_graph=False)
    assert L.calls(Q8) == before + Ly * 5, "one q8 decode launch per layer per step after the prefill"
    graph, _ = model.generate(ids, max_new_tokens=6, eos_token_id=-1, kv_cache_dtype="int8", use_graph=True)
    assert tuple(graph._t.shape) == (2, 6)
    assert torch.equal(graph._t, eager._t), "the captured int8 decode step replays to the eager ids"

    # teacher-forced decode: the same prefilled int8 caches, HIP kernels against the ops fallbacks
    forced = torch.randint(3, cfg.vocab_size, (2, 6), generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        caches = model.new_cache(2, 5 + 6, kv_dtype="int8")
        model(ids, caches, 0)
        assert all(isinstance(c, Int8KVCache) and c.k.dtype == torch.uint8 and c.v.dtype == torch.uint8
                   for c in caches)
        assert bool((caches[0].k[:, :, :5] != 128).any()) and bool((caches[0].k[:, :, 5:] == 128).all())
        twin = copy.deepcopy(caches)
        bf16_caches = model.new_cache(2, 5 + 6)
        model(ids, bf16_caches, 0)
        pos_t = torch.zeros(1, dtype=torch.int64, device=DEV)
        worst = 0.0
        for t in range(6):
            pos_t.fill_(5 + t)
            tok = forced[:, t:t + 1].contiguous()
            before = L.calls(Q8)
            hip = model._decode_logits(tok, caches, pos_t)
            assert L.calls(Q8) == before + Ly
            flags.set_flags({"FLAGS_use_hip_kernels": False})
            try:
                ref = model._decode_logits(tok, twin, pos_t)
            finally:
                flags.set_flags({"FLAGS_use_hip_kernels": True})
            assert L.calls(Q8) == before + Ly
            worst = max(worst, float((hip - ref).abs().max()))
            # the tolerance tests/test_decode_attn.py uses for HIP against the reference
            torch.testing.assert_close(hip, ref, rtol=2e-2, atol=2e-2)
            # and against the same model on its bf16 cache: the plumbing (which scale goes where) is shared by the
            # HIP and the fallback run above. A stored element is off by at most amax / 254; 10 % of the largest
            # logit is a loose bound on what that does (tests/test_decode_kv8_cpu.py shows swapped scales miss it)
            full = model._decode_logits(tok, bf16_caches, pos_t)
            assert float((hip - full).abs().max()) <= 0.1 * float(full.abs().max()), (t, float((hip - full).abs().max()))
        print(f"[kv8] llama int8 teacher-forced logits: max |hip - fallback| {worst:.4g}, max |logit| "
              f"{float(ref.abs().max()):.3g}")
        assert bool((caches[0].k[:, :, 5:11] != 128).any()) and bool((caches[0].k[:, :, 11:] == 128).all())
