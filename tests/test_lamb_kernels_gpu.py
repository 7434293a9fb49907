"""Multi-tensor LAMB (csrc/kernels/lamb.hip: lamb_stage1_k, lamb_trust_k, lamb_stage2_k) driven through
``paddle.optimizer.Lamb``, against a float64 reference on the device, in the style of test_optim_kernels_gpu.py.

The reference is the documented update in float64, started from the same rounded inputs as the kernel (the bf16/fp16
parameter and gradient upcast exactly), with ``g`` already multiplied by ``inv_scale``::

    m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g
    r = (m/(1-b1^t)) / (sqrt(v/(1-b2^t)) + eps) + wd*p
    trust = ||p||/||r|| if (wd != 0 or always_adapt) and ||p|| > 0 and ||r|| > 0 else 1      (per tensor)
    p -= lr*mult * trust * r

Tolerances are not chosen by hand: next to the float64 reference every test runs the same update in fp32 torch eager
(every operand, the hyper-parameters included, held in fp32), and the constants below are 4x the error of that eager run
against float64, measured on an MI355X over all cases of this file. Eager fp32 is the accuracy the formula itself
allows; 4x covers differences in summation order. Measures, each where it is well defined:

* parameters and first moments are signed sums that cancel: largest absolute error divided by the largest
  ``|reference|`` of the same tensor.
* second moments are sums of non-negative terms: largest elementwise relative error, exact zeros where the reference
  is zero.
* a trust ratio is one positive number: relative error.

Low-precision shadows are checked bitwise against ``master.to(dtype)``. The trust ratios of the last step are read from
the group's table entry, ``opt._tables[id(group)].extra[-1].trust`` (one per fused parameter, in the group's order).
"""
import math

import pytest
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.ops import _loader as L
from paddlepaddle_amd.optimizer.optimizer import L2Decay

pytestmark = pytest.mark.gpu

CHUNK = 16384
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
F32, F64 = torch.float32, torch.float64

# 4x the error of the fp32 eager update against float64 (measured values on the right; "kernel" is what the HIP kernels
# showed in the same run, for orientation only)
TOL_LAMB_P = 4 * 1.89e-7       # scaled abs; eager 1.888e-07, kernel 1.888e-07
TOL_LAMB_M = 4 * 1.38e-7       # scaled abs; eager 1.380e-07, kernel 1.577e-07
RTOL_LAMB_V = 4 * 4.75e-7      # max rel;    eager 4.747e-07, kernel 4.220e-07
RTOL_LAMB_TRUST = 4 * 3.86e-7  # rel;        eager 3.855e-07, kernel 2.616e-07

HYPER = dict(lr=1e-2, b1=0.8, b2=0.95, eps=1e-6, wd=0.1)
SEEN = {}  # quantity -> [largest eager error, largest kernel error] over the tests run so far (printed by each test)


def _randn(n, seed, dtype=F32, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(n, device="cuda", generator=g) * scale).to(dtype)


def _s(x, dtype):
    return torch.tensor(x, dtype=dtype, device="cuda")


def _bits(t):
    return t.contiguous().view(_INT[t.dtype])


def _scaled_err(got, ref):
    if ref.numel() == 0 or float(ref.abs().max()) == 0.0:
        assert bool((got == 0).all()), "non-zero where the whole reference is zero"
        return 0.0
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _rel_err(got, ref):
    """Largest elementwise relative error of a non-negative quantity; where the reference is 0 so must ``got`` be."""
    got = got.double()
    zero = ref == 0
    assert bool((got[zero] == 0).all()), "non-zero where the reference is exactly zero"
    if bool(zero.all()):
        return 0.0
    return float(((got - ref).abs()[~zero] / ref[~zero]).max())


def _check(key, what, got, eager, ref, tol, err=_scaled_err):
    e_eager, e_got = err(eager, ref), err(got, ref)
    s = SEEN.setdefault(key, [0.0, 0.0])
    s[0], s[1] = max(s[0], e_eager), max(s[1], e_got)
    assert e_got <= tol, f"{key} {what}: kernel error {e_got:.3e} > {tol:.3e} (fp32 eager: {e_eager:.3e})"


def _report():
    for k in ("lamb.p", "lamb.m", "lamb.v", "lamb.trust"):
        if k in SEEN:
            print(f"[lamb-kernels] {k}: fp32-eager max err {SEEN[k][0]:.3e}, kernel max err {SEEN[k][1]:.3e}")


class _Ent:
    """One parameter with its gradient tensor: separately allocated, or (``offset``) views into one flat parameter
    buffer and one flat gradient buffer with guard elements on both sides. Weights are N(0, scale), exactly zero for
    scale 0."""

    def __init__(self, name, shape, dtype, seed, offset=None, lr_mult=1.0, scale=1.0, gscale=1.0):
        n = math.prod(shape)
        self.name, self.n, self.dtype, self.gscale, self.lr_mult = name, n, dtype, gscale, lr_mult
        self.guards = []
        if offset is None:
            w = _randn(n, seed, dtype, scale).view(shape) if scale else torch.zeros(shape, dtype=dtype, device="cuda")
            g = torch.zeros(shape, dtype=dtype, device="cuda")
        else:
            pbuf, gbuf = _randn(offset + n + 3, seed, dtype, scale), _randn(offset + n + 3, seed + 1, dtype)
            w, g = pbuf[offset:offset + n], gbuf[offset:offset + n]
            for buf in (pbuf, gbuf):
                for sl in (slice(0, offset), slice(offset + n, None)):
                    self.guards.append((buf, sl, buf[sl].clone()))
            assert w.is_contiguous() and g.is_contiguous()
        self.param = paddle.Parameter(w, name=name, optimize_attr={"learning_rate": lr_mult})
        self.param._t.grad = g
        self.grad = g
        assert self.param._t.data_ptr() == w.data_ptr() and self.param._t.grad.data_ptr() == g.data_ptr()
        self.w0 = w.detach().clone()

    def new_grad(self, seed, premul):
        """Fresh N(0, gscale) gradient, stored pre-multiplied by ``premul``, written in place (same pointer)."""
        self.grad.copy_(_randn(self.n, seed, F32, self.gscale * premul).view(self.grad.shape))

    def state(self, dtype):
        return [self.w0.to(dtype), torch.zeros(self.w0.shape, dtype=dtype, device="cuda"),
                torch.zeros(self.w0.shape, dtype=dtype, device="cuda")]

    def check_guards(self):
        for buf, sl, before in self.guards:
            assert torch.equal(_bits(buf[sl]), _bits(before)), f"{self.name}: element next to the view was written"


def _geometry(dtype):
    """Chunk edges, misaligned contiguous views (whole chunks on the scalar branch) and one empty parameter. Weight
    scales 0.02, 5, 0.02, 1, 5, 0.02, 5: with N(0, 1) gradients the trust ratios are far from 1 on both sides. t3 has
    optimize_attr lr 0.5."""
    shapes = [(7,), (33, 17), (CHUNK,), (CHUNK + 1,), (2 * CHUNK + 3,)]
    scales = [0.02, 5.0, 0.02, 1.0, 5.0, 0.02, 5.0]
    ents = [_Ent(f"t{i}", shape, dtype, 100 + i, lr_mult=0.5 if i == 3 else 1.0, scale=scales[i])
            for i, shape in enumerate(shapes)]
    size = torch.empty(0, dtype=dtype).element_size()
    for off in ((1,) if dtype == F32 else (1, 2)):
        e = _Ent(f"view{off}", (CHUNK + 5,), dtype, 200 + 10 * off, offset=off, scale=scales[len(ents)])
        for t in (e.param._t, e.grad):
            assert t.is_contiguous() and t.data_ptr() % 16 == off * size
            assert t.data_ptr() % (16 if dtype == F32 else 8) != 0
        ents.append(e)
    ents.insert(2, _Ent("empty", (0,), dtype, 99))  # between two tensors that own items
    return ents


def _fp32_of(opt, e):
    return opt._master_weights[id(e.param)] if e.dtype != F32 else e.param._t.detach()


def _check_shadow(opt, e):
    if e.dtype != F32:
        master = opt._master_weights[id(e.param)]
        assert master.dtype == F32 and master.data_ptr() % 16 == 0
        assert torch.equal(_bits(e.param._t.detach()), _bits(master.to(e.dtype))), f"{e.name}: shadow != RNE(master)"


def _buffers(opt):
    return opt._tables[id(opt._param_groups[0])].extra[-1]


def _lamb_math(st, g, mult, wd, t, adapt, lr=HYPER["lr"], rows=False):
    """One documented LAMB update of state [p, m, v] in the dtype of the state; ``g`` is the effective gradient.
    Returns the new state and the trust ratio(s): one per tensor, or one per row of a 2-D state with ``rows``."""
    dt = st[0].dtype
    lr, mult, wd, b1, b2, eps, one = (_s(x, dt) for x in (lr, mult, wd, HYPER["b1"], HYPER["b2"], HYPER["eps"], 1.0))
    p, m, v = st
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * g * g
    r = (m / (one - b1 ** t)) / ((v / (one - b2 ** t)).sqrt() + eps) + wd * p
    dim = 1 if rows else None
    wn = torch.linalg.vector_norm(p, dim=dim, keepdim=rows)
    rn = torch.linalg.vector_norm(r, dim=dim, keepdim=rows)
    trust = torch.ones_like(wn)
    if adapt:
        trust = torch.where((wn > 0) & (rn > 0), wn / rn, trust)
    p = p - lr * mult * trust * r
    return [p, m, v], trust


def _trust_err(got, ref):
    return float(((got.double() - ref).abs() / ref).max())


def _run_lamb(opt, ents, steps=3, wd_of=lambda name: HYPER["wd"], always_adapt=False, l2_of=lambda name: 0.0,
              premul=1.0, inv=None, seed0=1000, fused=None):
    """``steps`` optimizer steps on fresh gradients, each checked against the float64 reference. ``fused``: names of
    the parameters expected on the fused path (default all); ``l2_of``: coefficient of an L2Decay regularizer folded
    into the gradient (per-parameter path). Returns the float64 trust ratios per name, one per step."""
    fused = [e.name for e in ents] if fused is None else fused
    ref = {e.name: e.state(F64) for e in ents}
    eag = {e.name: e.state(F32) for e in ents}
    trusts = {e.name: [] for e in ents}
    L.reset_calls()
    for t in range(1, steps + 1):
        for i, e in enumerate(ents):
            e.new_grad(seed0 + 100 * t + i, premul)
        opt.step()
        assert L.calls("pa_lamb_multi") == t, "one multi-tensor call per group per step"
        buf = _buffers(opt)
        assert buf.trust.dtype == F32 and buf.trust.shape == (len(fused),)
        for e in ents:
            wd = wd_of(e.name)
            tr = {}
            for states, dt in ((ref, F64), (eag, F32)):
                scale = _s(1.0, dt) if inv is None else inv.to(dt).reshape(())
                g = e.grad.to(dt) * scale + _s(l2_of(e.name), dt) * states[e.name][0]
                states[e.name], tr[dt] = _lamb_math(states[e.name], g, e.lr_mult, wd, t, bool(wd) or always_adapt)
            trusts[e.name].append(float(tr[F64]))
            m1, m2 = opt._accumulators["moment1"][id(e.param)], opt._accumulators["moment2"][id(e.param)]
            assert m1.dtype == F32 and m2.dtype == F32
            what = f"{e.name} step {t}"
            _check("lamb.p", what, _fp32_of(opt, e), eag[e.name][0], ref[e.name][0], TOL_LAMB_P)
            _check("lamb.m", what, m1, eag[e.name][1], ref[e.name][1], TOL_LAMB_M)
            _check("lamb.v", what, m2, eag[e.name][2], ref[e.name][2], RTOL_LAMB_V, err=_rel_err)
            if e.name in fused:
                got = buf.trust[fused.index(e.name)].reshape(1)
                _check("lamb.trust", what, got, tr[F32].reshape(1), tr[F64].reshape(1), RTOL_LAMB_TRUST, err=_trust_err)
            _check_shadow(opt, e)
            e.check_guards()
    _report()
    return trusts


def _lamb(ents, **kw):
    return paddle.optimizer.Lamb(HYPER["lr"], lamb_weight_decay=HYPER["wd"], beta1=HYPER["b1"], beta2=HYPER["b2"],
                                 epsilon=HYPER["eps"], parameters=[e.param for e in ents], **kw)


@pytest.mark.parametrize("dtype", list(_DTYPES), ids=list(_DTYPES))
def test_lamb_geometry(dtype):
    """Chunk edges, the scalar branch on misaligned views, an empty parameter, fp32 / bf16 / fp16 with masters, a
    per-row lr multiplier and the inv_scale pointer on gradients stored 1024x. The trust ratios of the reference are
    far from 1 (else a kernel that ignored them, or took one norm for the whole group, would pass)."""
    dt = _DTYPES[dtype]
    ents = _geometry(dt)
    opt = _lamb(ents, multi_precision=dt != F32)
    inv = torch.full((1,), 1.0 / 1024, dtype=F32, device="cuda")
    opt._inv_scale_tensor = inv
    trusts = _run_lamb(opt, ents, premul=1024.0, inv=inv)
    far = [n for n, tr in trusts.items() if all(x < 0.5 or x > 2.0 for x in tr)]
    assert len(far) >= 4 and min(min(trusts[n]) for n in far) < 0.5 and max(max(trusts[n]) for n in far) > 2.0, trusts
    assert trusts["empty"] == [1.0, 1.0, 1.0]
    assert float(_buffers(opt).trust[[e.name for e in ents].index("empty")]) == 1.0
    assert _buffers(opt).offsets.tolist()[-1] == opt._tables[id(opt._param_groups[0])].n_items


def test_lamb_more_items_than_reducing_threads():
    """One tensor of 257 work items: lamb_trust_k's 256 threads take a second partial."""
    ents = [_Ent("big", (257 * CHUNK + 3,), F32, 300, scale=0.02)]
    opt = _lamb(ents)
    trusts = _run_lamb(opt, ents, seed0=3000)
    assert opt._tables[id(opt._param_groups[0])].n_items == 258
    assert all(x < 0.5 for x in trusts["big"])


def test_lamb_grid_wrap_4100_tensors():
    """4100 five-element parameters, consecutive views of one flat fp32 buffer: 4100 work items on the 4096-workgroup
    grids of the two stages and 4100 tensors on the 1024-workgroup grid of lamb_trust_k, weight scale alternating
    0.02 and 5. Reference norms are row norms of the (4100, 5) reshape; every trust ratio is checked."""
    n_p, k = 4100, 5
    scale = torch.tensor([0.02, 5.0], device="cuda").repeat(n_p // 2).repeat_interleave(k)
    flat_p, flat_g = _randn(n_p * k, 400) * scale, torch.zeros(n_p * k, device="cuda")
    w0 = flat_p.clone()
    ps = []
    for i in range(n_p):
        p = paddle.Parameter(flat_p[i * k:(i + 1) * k], name=f"w{i}")
        p._t.grad = flat_g[i * k:(i + 1) * k]
        ps.append(p)
    assert {p._t.data_ptr() % 16 for p in ps} == {0, 4, 8, 12} == {p._t.grad.data_ptr() % 16 for p in ps}
    assert all(p._t.data_ptr() == flat_p.data_ptr() + 4 * k * i for i, p in enumerate(ps))
    opt = paddle.optimizer.Lamb(HYPER["lr"], lamb_weight_decay=HYPER["wd"], beta1=HYPER["b1"], beta2=HYPER["b2"],
                                epsilon=HYPER["eps"], parameters=ps)
    ref = [w0.double().view(n_p, k)] + [torch.zeros(n_p, k, dtype=F64, device="cuda") for _ in range(2)]
    eag = [w0.clone().view(n_p, k)] + [torch.zeros(n_p, k, device="cuda") for _ in range(2)]
    L.reset_calls()
    for t in range(1, 4):
        flat_g.copy_(_randn(n_p * k, 410 + t))
        opt.step()
        assert L.calls("pa_lamb_multi") == t
        ref, tr_ref = _lamb_math(ref, flat_g.double().view(n_p, k), 1.0, HYPER["wd"], t, True, rows=True)
        eag, tr_eag = _lamb_math(eag, flat_g.view(n_p, k), 1.0, HYPER["wd"], t, True, rows=True)
        m1 = torch.cat([opt._accumulators["moment1"][id(p)] for p in ps])
        m2 = torch.cat([opt._accumulators["moment2"][id(p)] for p in ps])
        what = f"flat step {t}"
        _check("lamb.p", what, flat_p, eag[0].reshape(-1), ref[0].reshape(-1), TOL_LAMB_P)
        _check("lamb.m", what, m1, eag[1].reshape(-1), ref[1].reshape(-1), TOL_LAMB_M)
        _check("lamb.v", what, m2, eag[2].reshape(-1), ref[2].reshape(-1), RTOL_LAMB_V, err=_rel_err)
        got = _buffers(opt).trust
        assert got.shape == (n_p,)
        _check("lamb.trust", what, got, tr_eag.reshape(-1), tr_ref.reshape(-1), RTOL_LAMB_TRUST, err=_trust_err)
        # per tensor, not per group: the two halves sit on opposite sides of 1
        assert float(tr_ref[0::2].max()) < 0.5 and float(tr_ref[1::2].median()) > 2.0
    assert opt._tables[id(opt._param_groups[0])].n_items == n_p
    _report()


@pytest.mark.parametrize("always_adapt", [False, True], ids=["plain", "always_adapt"])
def test_lamb_trust_gating(always_adapt):
    """A parameter excluded from weight decay has trust exactly 1 unless ``always_adapt``; an all-zero parameter has
    trust exactly 1 and moves with a non-zero gradient, and stays exactly zero with a zero one."""
    ents = [_Ent("dec", (33, 17), F32, 500, scale=5.0), _Ent("excl", (CHUNK + 1,), F32, 501, scale=0.02),
            _Ent("zero_w", (300,), F32, 502, scale=0.0), _Ent("zero_wg", (300,), F32, 503, scale=0.0, gscale=0.0)]
    opt = _lamb(ents, exclude_from_weight_decay_fn=lambda p: p.name == "excl", always_adapt=always_adapt)
    trusts = _run_lamb(opt, ents, steps=1, wd_of=lambda name: 0.0 if name == "excl" else HYPER["wd"],
                       always_adapt=always_adapt, seed0=5000)
    got = _buffers(opt).trust.tolist()
    assert trusts["dec"][0] > 2.0 and got[0] > 2.0
    if always_adapt:
        assert trusts["excl"][0] < 0.5 and got[1] < 0.5  # ||p|| / ||r||, checked against the reference above
    else:
        assert got[1] == 1.0
    assert got[2] == 1.0 and got[3] == 1.0
    zw, zwg = ents[2].param._t.detach(), ents[3].param._t.detach()
    assert float(zw.abs().min()) > 0.0, "the all-zero parameter did not move"
    assert bool((zwg == 0).all()) and bool(zwg.isfinite().all())
    for acc in ("moment1", "moment2"):
        a = opt._accumulators[acc][id(ents[3].param)]
        assert bool((a == 0).all()) and bool(a.isfinite().all())


def test_lamb_mixed_paths_and_state_dict():
    """One parameter carries an L2Decay regularizer and takes ``_update_param``; the others are fused. Both match the
    reference, the beta powers advance on both paths, and a fresh optimizer loaded from ``state_dict()`` takes the same
    next step bit for bit."""
    b1, b2 = HYPER["b1"], HYPER["b2"]
    ents = [_Ent("fa", (33, 17), F32, 600, scale=5.0), _Ent("reg", (CHUNK + 1,), F32, 601, scale=0.02),
            _Ent("fb", (2 * CHUNK + 3,), F32, 602, scale=0.02, lr_mult=0.5)]
    ents[1].param.regularizer = L2Decay(0.05)
    opt = _lamb(ents)
    _run_lamb(opt, ents, l2_of=lambda name: 0.05 if name == "reg" else 0.0, seed0=6000, fused=["fa", "fb"])
    for e in ents:
        assert opt._param_step[id(e.param)] == 3
        for acc, b in (("beta1_pow_acc", b1), ("beta2_pow_acc", b2)):
            torch.testing.assert_close(opt._accumulators[acc][id(e.param)].cpu(), torch.tensor([b ** 3]),
                                       rtol=1e-6, atol=0)

    twins = [_Ent(e.name, tuple(e.param._t.shape), F32, 0, lr_mult=e.lr_mult) for e in ents]
    for e, tw in zip(ents, twins):
        tw.param._t.detach().copy_(e.param._t.detach())
    twins[1].param.regularizer = L2Decay(0.05)
    opt2 = _lamb(twins)
    opt2.set_state_dict(opt.state_dict())
    assert [opt2._param_step[id(tw.param)] for tw in twins] == [3, 3, 3] and not opt2._tables
    for i, (e, tw) in enumerate(zip(ents, twins)):
        e.new_grad(6900 + i, 1.0)
        tw.grad.copy_(e.grad)
    before = L.calls("pa_lamb_multi")
    opt.step()
    opt2.step()
    assert L.calls("pa_lamb_multi") == before + 2
    for e, tw in zip(ents, twins):
        assert torch.equal(_bits(e.param._t.detach()), _bits(tw.param._t.detach())), e.name
        for acc in ("moment1", "moment2", "beta1_pow_acc", "beta2_pow_acc"):
            assert torch.equal(_bits(opt._accumulators[acc][id(e.param)]),
                               _bits(opt2._accumulators[acc][id(tw.param)])), (e.name, acc)
    assert torch.equal(_bits(_buffers(opt).trust), _bits(_buffers(opt2).trust))


def test_lamb_is_deterministic():
    """Two optimizers on cloned inputs are bit-identical after three steps: parameters, shadows, moments and trust
    ratios (no atomics, every sum in a fixed order)."""
    runs = []
    for _ in range(2):
        ents = _geometry(torch.bfloat16) + [_Ent("many", (5 * CHUNK + 77,), torch.bfloat16, 700, scale=0.02)]
        opt = _lamb(ents, multi_precision=True)
        for t in range(1, 4):
            for i, e in enumerate(ents):
                e.new_grad(7000 + 100 * t + i, 1.0)
            opt.step()
        assert L.calls("pa_lamb_multi") == 3 * (len(runs) + 1)
        out = [_buffers(opt).trust.clone()]
        for e in ents:
            out += [e.param._t.detach(), opt._master_weights[id(e.param)]]
            out += [opt._accumulators[a][id(e.param)] for a in ("moment1", "moment2")]
        runs.append(out)
    assert len(runs[0]) == len(runs[1])
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))
