"""int8 KV cache, CPU side: the yardstick of tests/kv8_cases.py can see (an fp32 model of the op and of the HIP
kernel's own arithmetic pass, every mutant reference fails by far), the ops fallbacks on uint8 caches match the
reference, the argument checks, the quantising cache write's rounding rule, and LLaMA generation on an int8 cache.

Measured on the CPU with this construction (python tests/kv8_cases.py): fp32 models <= 0.25 x the tolerance;
mutants at least: no offset 3900 x, neighbouring head's scale 67 x, K / V scales swapped 100 x, last key dropped
210 x, slot ``len`` read 1800 x, k_cur ignored 3200 x."""
import functools

import pytest
import torch

import attn_needles as A
import kv8_cases as C
from paddlepaddle_amd import ops
from paddlepaddle_amd.ops.rope import rope_tables

ATOL, RTOL = A.DECODE_ATOL, A.RTOL[torch.bfloat16]
SPECS = C.paged_specs() + C.dense_specs()


@functools.lru_cache(maxsize=None)
def _case(i):
    c = C.make(SPECS[i])
    return c, c.reference()


@pytest.mark.parametrize("i", range(len(SPECS)), ids=[C.spec_id(s) for s in SPECS])
def test_yardstick_sees(i):
    c, ref = _case(i)
    for km in (False, True):   # the op in fp32, and the kernel's arithmetic (scales applied after the reductions)
        got = c.reference(dt=torch.float32, kernel_model=km).bfloat16()
        r, idx = A.excess(got, ref, ATOL, RTOL)
        print(f"[kv8] {c.id} fp32 model (kernel arithmetic: {km}): {r:.3f} x tol")
        A.check(got, ref, ATOL, RTOL, what=f"{c.id} fp32 model (kernel {km})")
    for m in C.MUTANTS:
        if not c.applies(m):
            continue
        r, _ = A.excess(c.reference(mutant=m).bfloat16(), ref, ATOL, RTOL)
        print(f"[kv8] {c.id} mutant {m}: {r:.3g} x tol")
        assert r > 10.0, f"{c.id}: the mutant '{m}' is only {r:.3g} x the tolerance away"


def test_mutants_apply():
    """Each mutant applies somewhere, the head-scale one needs Hkv > 1, the k_cur one a case with k_cur."""
    def first(pred):
        return C.make(next(s for s in SPECS if pred(s)))
    paged, dense = (lambda s: len(s) == 6), (lambda s: len(s) == 5)
    cases = [first(lambda s: paged(s) and not s[-1] and 16 // s[0] > 1), first(lambda s: paged(s) and s[-1]),
             first(lambda s: dense(s) and not s[-1]), first(lambda s: dense(s) and s[-1] and 16 // s[0] > 1)]
    assert [c.cur for c in cases] == [False, True, False, True] and cases[0].Hkv > 1 and cases[3].Hkv > 1
    for c in cases:   # every mutant applies wherever its precondition holds, paged and dense
        for m in C.MUTANTS:
            want = {"head_scale": c.Hkv > 1, "cur_ignored": c.cur}.get(m, True)
            assert c.applies(m) == want, (c.id, m)
    g8 = C.PagedCase(16, 8, [1, 9], H=16)   # one kv head
    assert not g8.applies("head_scale") and not g8.applies("cur_ignored")


@pytest.mark.parametrize("i", range(len(SPECS)), ids=[C.spec_id(s) for s in SPECS])
def test_ops_fallback_uint8(i):
    """CPU: the wrappers dequantise the gathered blocks only and apply k_cur / v_cur."""
    c, ref = _case(i)
    if isinstance(c, C.PagedCase):
        got = ops.paged_decode_attention(c.q, c.kc, c.vc, c.tables, c.lens, max_len=c.max_len, **c.cur_kwargs())
    else:
        got = ops.dense_decode_attention(c.q, c.kc, c.vc, c.lens, **c.cur_kwargs())
    assert got.dtype == torch.bfloat16
    A.check(got, ref, ATOL, RTOL, what=c.id)
    for n, ln in enumerate(c.lens_list):
        if ln == 0:
            assert float(got[n].abs().max()) == 0.0


def test_argument_checks():
    c = C.PagedCase(2, 16, [5, 17], H=4)
    kw = c.cur_kwargs()
    with pytest.raises(ValueError):   # uint8 caches without scales
        ops.paged_decode_attention(c.q, c.kc, c.vc, c.tables, c.lens)
    with pytest.raises(ValueError):
        ops.paged_decode_attention(c.q, c.kc, c.vc, c.tables, c.lens, k_dequant=kw["k_dequant"])
    with pytest.raises(ValueError):   # scales with a float cache
        ops.paged_decode_attention(c.q, c.kc.bfloat16(), c.vc.bfloat16(), c.tables, c.lens, **kw)
    with pytest.raises(ValueError):   # k_cur without v_cur
        ops.paged_decode_attention(c.q, c.kc, c.vc, c.tables, c.lens, k_cur=torch.zeros(2, 2, 128).bfloat16(), **kw)
    with pytest.raises(ValueError):   # k_cur with a float cache
        ops.paged_decode_attention(c.q, c.kc.bfloat16(), c.vc.bfloat16(), c.tables, c.lens,
                                   k_cur=torch.zeros(2, 2, 128).bfloat16(), v_cur=torch.zeros(2, 2, 128).bfloat16())
    d = C.DenseCase(2, 64, [5, 64], H=4)
    with pytest.raises(ValueError):
        ops.dense_decode_attention(d.q, d.kc, d.vc, d.lens)
    with pytest.raises(ValueError):
        ops.dense_decode_attention(d.q, d.kc.bfloat16(), d.vc.bfloat16(), d.lens, **d.cur_kwargs())
    with pytest.raises(ValueError):   # decode_rope_cache: scales and uint8 caches go together
        ops.decode_rope_cache(torch.zeros(1, 4 * 16), 2, 1, 16, torch.ones(1, 16), torch.zeros(1, 16),
                              torch.tensor([0]), torch.zeros(1, 1, 4, 16, dtype=torch.uint8),
                              torch.zeros(1, 1, 4, 16, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.decode_rope_cache(torch.zeros(1, 4 * 16), 2, 1, 16, torch.ones(1, 16), torch.zeros(1, 16),
                              torch.tensor([0]), torch.zeros(1, 1, 4, 16), torch.zeros(1, 1, 4, 16),
                              k_scale=torch.ones(1), v_scale=torch.ones(1))


def test_bf16_calls_unaffected():
    """Float caches and no new arguments: the results of the reference path, bit for bit."""
    case = A.DecodeCase(2, 16, [0, 1, 17, 65], 64, H=4)
    got = ops.paged_decode_attention(case.q, case.kc, case.vc, case.tables, case.lens, max_len=64)
    want = ops.attention.paged_decode_reference(case.q, case.kc, case.vc, case.tables, case.lens)
    assert torch.equal(got, want)
    A.check(got, case.reference(), ATOL, RTOL, what="bf16 paged")
    dense = A.DenseDecodeCase(2, 64, [1, 64, 33, 64], H=4)
    got = ops.dense_decode_attention(dense.q, dense.kc, dense.vc, dense.lens)
    A.check(got, dense.reference(), ATOL, RTOL, what="bf16 dense")


def _quant_formula(x, scale):
    z = x.float() * scale.float().view(-1, 1)
    z = torch.sign(z) * torch.floor(z.abs() + 0.5)
    return (z.clamp(-127, 127) + 128).to(torch.uint8)


def test_quantize_kv_int8_rule():
    """Ties go away from zero (quant_round_type 1), the range clamps to +-127, zero stays 128."""
    x = torch.tensor([[0.5, -0.5, 1.5, -1.5, 2.5, 126.5, 127.5, -127.5, 300.0, -300.0, 0.0, 0.49, -0.49, 1e-30]])
    got = ops.quantize_kv_int8(x, torch.ones(1))
    want = torch.tensor([[1, -1, 2, -2, 3, 127, 127, -127, 127, -127, 0, 0, 0, 0]]) + 128
    assert torch.equal(got.long(), want)
    assert torch.equal(got, _quant_formula(x, torch.ones(1)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_decode_rope_cache_fallback_bytes(dtype):
    g = torch.Generator().manual_seed(3)
    B, Bc, H, Hkv, D, Lc, p = 3, 4, 4, 2, 32, 16, 5
    qkv = torch.randn(B, (H + 2 * Hkv) * D, generator=g).to(dtype)
    cos, sin = rope_tables(Lc, D)
    pos = torch.tensor([p])
    cs, sn = cos.index_select(0, pos), sin.index_select(0, pos)
    kf, vf = torch.zeros(Bc, Hkv, Lc, D, dtype=dtype), torch.zeros(Bc, Hkv, Lc, D, dtype=dtype)
    q_ref = ops.decode_rope_cache(qkv, H, Hkv, D, cs, sn, pos, kf, vf)
    ks, vs = torch.tensor([40.0, 90.0]), torch.tensor([55.0, 25.0])    # the second K scale clamps
    kc = torch.full((Bc, Hkv, Lc, D), 7, dtype=torch.uint8)
    vc = torch.full((Bc, Hkv, Lc, D), 9, dtype=torch.uint8)
    q = ops.decode_rope_cache(qkv, H, Hkv, D, cs, sn, pos, kc, vc, k_scale=ks, v_scale=vs)
    assert torch.equal(q, q_ref)
    assert torch.equal(kc[:B, :, p], _quant_formula(kf[:B, :, p], ks))
    assert torch.equal(vc[:B, :, p], _quant_formula(vf[:B, :, p], vs))
    assert int((kc[:B, :, p] == 255).sum()) + int((kc[:B, :, p] == 1).sum()) > 0, "some values clamp"
    kc[:B, :, p], vc[:B, :, p] = 7, 9
    assert bool((kc == 7).all()) and bool((vc == 9).all()), "every other byte untouched"


def _tiny():
    import paddlepaddle_amd as paddle
    from paddlepaddle_amd.models.llama import LlamaConfig, LlamaForCausalLM
    paddle.seed(11)
    cfg = LlamaConfig.tiny(num_hidden_layers=2, hidden_size=64, intermediate_size=128, num_attention_heads=2,
                           num_key_value_heads=1, vocab_size=128, initializer_range=0.2)
    return paddle, LlamaForCausalLM(cfg)


def test_llama_generate_int8_cpu():
    from paddlepaddle_amd.models.llama import Int8KVCache
    paddle, model = _tiny()
    model.eval()
    ids = paddle.to_tensor(torch.tensor([[5, 9, 33, 7, 100], [4, 8, 15, 16, 23]]))
    out8, sc8 = model.generate(ids, max_new_tokens=6, eos_token_id=-1, kv_cache_dtype="int8")
    out, sc = model.generate(ids, max_new_tokens=6, eos_token_id=-1)
    assert tuple(out8._t.shape) == (2, 6) and tuple(sc8._t.shape) == (2, 6)
    assert torch.isfinite(sc8._t).all()
    assert torch.equal(out8._t[:, 0], out._t[:, 0])   # the prefill attends to the unquantised prompt
    torch.testing.assert_close(sc8._t[:, 0], sc._t[:, 0])
    # the cache: bytes and per-kv-head scales from the prompt, decode steps written behind it
    caches = model.new_cache(2, 11, kv_dtype="int8")
    assert all(isinstance(c, Int8KVCache) for c in caches) and caches[0].k.dtype == torch.uint8
    assert tuple(caches[0].k.shape) == (2, 1, 64, 32) and tuple(caches[0].k_scale.shape) == (1,)
    with torch.no_grad():
        model(ids, caches, 0)
        c = caches[0]
        torch.testing.assert_close(c.k_scale * c.k_dequant, torch.ones(1))
        assert int(c.k[:, :, :5].min()) == 1 or int(c.k[:, :, :5].max()) == 255   # amax maps to +-127
        assert bool((c.k[:, :, 5:] == 128).all())
        model(paddle.to_tensor(torch.tensor([[3], [6]])), caches, 5)
        assert bool((c.k[:, :, 5] != 128).any()) and bool((c.k[:, :, 6:] == 128).all())
        with pytest.raises(NotImplementedError):
            model(ids, caches, 6)
    with pytest.raises(ValueError):
        model.new_cache(2, 11, kv_dtype="fp8")
    kc, vc = model.new_cache(2, 11)[0]    # the default stays a (k, v) pair in the parameters' dtype
    assert kc.dtype == torch.float32 and vc.shape == kc.shape


def test_llama_int8_decode_logits_track_float_cache_cpu():
    """Teacher-forced decode on the int8 cache against the same model on its float cache, at every step: the check
    of the plumbing from the model to the ops (which scale goes where), which a comparison of the HIP kernels with
    their fallbacks on one cache object cannot see. V's projection is scaled by 3 so that the K and V scales differ.
    Bound: a stored element is off by at most half a step, amax / 254 (0.4 % of its head's largest value), the
    errors of the ~100s of elements of a dot product are independent, and the model is linear in V and smooth in K:
    10 % of the largest logit is loose. The same step with the K and V dequant scales swapped must miss it."""
    import copy
    paddle, model = _tiny()
    model.eval()
    cfg = model.config
    kvw = cfg.num_key_value_heads * cfg.head_dim
    with torch.no_grad():
        for layer in model.llama.layers:
            layer.self_attn.qkv_proj.weight._t[:, -kvw:] *= 3.0
        ids = paddle.to_tensor(torch.tensor([[5, 9, 33, 7, 100], [4, 8, 15, 16, 23]]))
        forced = torch.tensor([[11, 2, 90, 41, 7, 64], [3, 77, 120, 9, 50, 1]])
        c8, cf = model.new_cache(2, 11, kv_dtype="int8"), model.new_cache(2, 11)
        model(ids, c8, 0)
        model(ids, cf, 0)
        assert float((c8[0].k_dequant / c8[0].v_dequant - 1).abs()) > 0.3, "K and V scales differ"
        for t in range(6):
            tok = paddle.to_tensor(forced[:, t:t + 1])
            swapped = copy.deepcopy(c8)
            for c in swapped:
                c.k_dequant, c.v_dequant = c.v_dequant, c.k_dequant
            want = model(tok, cf, 5 + t)._t[:, -1]
            got = model(tok, c8, 5 + t)._t[:, -1]
            bad = model(tok, swapped, 5 + t)._t[:, -1]
            bound = 0.1 * float(want.abs().max())
            err, err_bad = float((got - want).abs().max()), float((bad - want).abs().max())
            print(f"[kv8] step {t}: max |logit| {bound * 10:.3f}, int8 - float {err:.4f}, scales swapped {err_bad:.4f}")
            assert err <= bound, (t, err, bound)
            assert err_bad > bound, (t, err_bad, bound)
