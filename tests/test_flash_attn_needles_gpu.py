"""HIP flash attention (forward, LSE, backward) against the fp64 reference of tests/attn_needles.py on needle
inputs: every case checks o, LSE, dq, dk and dv elementwise, so one lost or leaked key at a block, tile, mask,
bound or sequence edge fails (tests/test_attn_needles_cpu.py proves that on reference mutants). Every case asserts
the HIP launchers ran and the ATen fallback did not. Tolerances: attn_needles.TOL (from the rounding model)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_needles as A  # noqa: E402
from paddlepaddle_amd.ops import _loader as L  # noqa: E402
from paddlepaddle_amd.ops.attention import attention, attention_bhsd  # noqa: E402

DEV = "cuda"
_REF = {}


def _reference(case, **extra):
    """fp64 reference of a case on the GPU, computed once and shared (the route tests reuse the cases)."""
    key = (case.id, tuple(sorted(extra)))
    if key not in _REF:
        t, kw = case.dense(DEV)
        kw.update(extra)
        _REF[key] = A.reference(*t, **kw)
    return _REF[key]


def _compare(case, got, ref, names):
    """check() every output after printing its error as a multiple of the tolerance."""
    fails = []
    for n in names:
        atol, rtol = A.tolerances(case.dtype, n, ref[n])
        r, idx = A.excess(got[n], ref[n], atol, rtol)
        print(f"[needle] {case.id} {n}: {r:.3f} x tol at {idx}")
        try:
            A.check(got[n], ref[n], atol, rtol, what=f"{case.id} {n}")
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)


def _assert_hip_ran():
    assert L.calls("pa_flash_attn_fwd_ex") > 0
    assert L.calls("pa_flash_attn_bwd_ex") + L.calls("pa_flash_attn_bwd_ds") > 0
    assert L.calls("attn_aten_fallback") == 0


def _run(case, **extra):
    q, k, v, do, kw = case.kernel_args(DEV)
    for t in (q, k, v):
        t.requires_grad_(True)
    o, lse = attention(q, k, v, return_lse=True, **kw, **{a: b for a, b in extra.items() if a in ("dropout", "seed")})
    o.backward(do)
    ref = _reference(case, **{a: b for a, b in extra.items() if a in ("keep", "drop_p")})
    got = {"o": o.detach(), "lse": lse, "dq": q.grad, "dk": k.grad, "dv": v.grad}
    if case.lens is not None:       # packed varlen: [T, H, D] and LSE [H, T]
        got = {n: t[None] for n, t in got.items()}
    _compare(case, got, ref, ("o", "lse", "dq", "dk", "dv"))
    dead = torch.isposinf(ref["lse"])                      # [B, H, Sq]: rows without a visible key
    if bool(dead.any()):
        rows = dead.permute(0, 2, 1)                       # [B, Sq, H]
        assert bool((got["o"][rows] == 0).all()) and bool((got["dq"][rows] == 0).all()), "dead rows must be exactly 0"
        assert bool(torch.isposinf(got["lse"][dead]).all())
    _assert_hip_ran()
    return got


_ids = {"ids": lambda c: c.id}


@pytest.mark.parametrize("case", A.plain_cases(), **_ids)
def test_plain(case):
    """Every geometry, causal and full, D = 128 bf16 (default backward: the dS route)."""
    _run(case)
    assert L.calls("flash_attn_bwd_ds") > 0 and L.calls("pa_flash_attn_bwd_ex") == 0


@pytest.mark.parametrize("route", ["ds", "atomics16", "atomics4"])
@pytest.mark.parametrize("case", A.route_cases(), **_ids)
def test_backward_routes(monkeypatch, case, route):
    """The three D = 128 backward routes on the ragged and Sq != Sk geometries."""
    if route == "atomics16":
        monkeypatch.setenv("PA_FA_BWD_DS", "0")
        monkeypatch.setenv("PA_FA_BWD16", "1")
    elif route == "atomics4":
        monkeypatch.setenv("PA_FA_BWD16", "0")
    else:
        monkeypatch.delenv("PA_FA_BWD_DS", raising=False)
        monkeypatch.delenv("PA_FA_BWD16", raising=False)
    _run(case)
    if route == "ds":
        assert L.calls("flash_attn_bwd_ds") > 0 and L.calls("pa_flash_attn_bwd_ex") == 0
    else:
        assert L.calls("flash_attn_bwd_ds") == 0 and L.calls("pa_flash_attn_bwd_ex") > 0


@pytest.mark.parametrize("case", A.feature_cases(), **_ids)
def test_features(case):
    """Bool / additive masks, flashmask with 1, 2 and 4 columns, varlen: D 64 / 128 / 256, bf16 and fp16."""
    _run(case)


@pytest.mark.parametrize("case", A.misc_cases(), **_ids)
def test_padded_dim_scale_and_tile_class_edges(case):
    """Head dim 80 (padded to 128), scale 0.05 / 0.3 (plain and additive mask), and flashmask bounds that sit
    exactly on the transitions of the kernel's per-tile classes (skip / per-element test / untouched)."""
    _run(case)


@pytest.mark.parametrize("case", A.bhsd_cases(), **_ids)
def test_attention_bhsd_transposed_views(case):
    """attention_bhsd hands the kernel non-contiguous [B, S, H, D] views of [B, H, S, D] tensors."""
    q, k, v, do, kw = case.kernel_args(DEV)
    q, k, v, do = (t.transpose(1, 2).contiguous() for t in (q, k, v, do))
    for t in (q, k, v):
        t.requires_grad_(True)
    o = attention_bhsd(q, k, v, scale=kw["scale"], mask=kw.get("mask"), causal=kw["causal"])
    assert o.shape == q.shape
    o.backward(do)
    got = {"o": o.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}
    _compare(case, {n: t.transpose(1, 2) for n, t in got.items()}, _reference(case), ("o", "dq", "dk", "dv"))
    _assert_hip_ran()


@pytest.mark.parametrize("case", A.dropout_cases(), **_ids)
def test_dropout_mask_over_tiles_blocks_and_heads(case):
    """The kernel's keep mask read off exactly: V = identity on one chunk of D keys makes O = P' on that chunk, so
    ceil(Sk / D) passes with one seed give the whole mask (3 Q blocks x 4 key tiles x 4 heads x 2 batches). It must
    be reproducible, keep 1 - p of the visible entries, differ between (batch, head) pairs, match the reference
    forward, and be the mask the backward regenerates (checked through dq / dk / dv with random V)."""
    p, seed = 0.3, 4321
    q, k, v, do, kw = case.kernel_args(DEV)
    B, Sq, Sk, H, Hk, D = case.B, case.Sq, case.Sk, case.H, case.Hk, case.D
    vis = case.vis.to(DEV)
    keep = torch.zeros(B, H, Sq, Sk, dtype=torch.bool, device=DEV)
    pprime = torch.zeros(B, H, Sq, Sk, dtype=torch.float64, device=DEV)
    for c0 in range(0, Sk, D):
        n = min(D, Sk - c0)
        vid = torch.zeros(B, Sk, Hk, D, dtype=case.dtype, device=DEV)
        vid[:, c0:c0 + n] = torch.eye(D, dtype=case.dtype, device=DEV)[:n].view(1, n, 1, D)
        o = attention(q, k, vid, dropout=p, seed=seed, **kw)
        if c0 == 0:
            assert torch.equal(o, attention(q, k, vid, dropout=p, seed=seed, **kw)), "same seed, same mask"
        pprime[..., c0:c0 + n] = o.double().permute(0, 2, 1, 3)[..., :n]
        keep[..., c0:c0 + n] = o.permute(0, 2, 1, 3)[..., :n] != 0
    assert not bool((keep & ~vis).any()), "a masked key got weight"
    frac = float(keep[vis].float().mean())
    print(f"[needle] {case.id} keep fraction {frac:.4f}")
    assert abs(frac - (1 - p)) < 0.01, frac
    flat = keep.view(B * H, Sq, Sk)
    both = vis.reshape(B * H, Sq, Sk)
    for a in range(B * H):
        for b in range(a + 1, B * H):
            m = both[a] & both[b]
            assert float((flat[a] != flat[b])[m].float().mean()) > 0.3, f"(b, h) pairs {a} and {b} share a mask"
    # forward: O = P' with the recovered mask
    t, dkw = case.dense(DEV)
    qh, kh, _ = A._heads(t[0].double(), t[1].double(), t[1].double())
    s, dead = A._scores(qh, kh, dkw["vis"], None, D ** -0.5)
    want = (torch.softmax(s, -1).masked_fill(dead, 0.0) * keep / (1 - p))
    A.check(pprime, want, *A.tolerances(case.dtype, "o", want), what=f"{case.id} P'")
    # backward (and forward with random V) against the reference with that mask
    _run(case, dropout=p, seed=seed, keep=keep, drop_p=p)


@pytest.mark.parametrize("case", A.dead_row_cases(), **_ids)
def test_dead_rows_exact_zero(case):
    """257 x 193 causal: the first 64 rows see no key. o and dq rows exactly 0, LSE +inf, dk / dv as the reference
    (checked in _run), in all three head dims."""
    got = _run(case)
    assert bool((got["o"][:, :64] == 0).all()) and bool((got["dq"][:, :64] == 0).all())
    assert bool(torch.isposinf(got["lse"][:, :, :64]).all()) and bool(torch.isfinite(got["lse"][:, :, 64:]).all())
