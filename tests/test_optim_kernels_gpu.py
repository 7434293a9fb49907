"""Multi-tensor optimizer kernels (csrc/kernels/adamw.hip: adamw_multi_k, momentum_multi_k, sq_norm_multi_k) driven
through the public optimizers and ``ops.optim.global_sq_norm``, against a float64 reference on the device.

The reference is the documented update in float64, started from the same rounded inputs as the kernel (the bf16/fp16
parameter and gradient upcast exactly). AdamW, with ``g`` already multiplied by ``inv_scale`` (and the clip coefficient)::

    m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g
    p = p*(1 - lr*mult*wd) - lr*mult/(1-b1^t) * m / (sqrt(v/(1-b2^t)) + eps)

Momentum::

    g = grad*rescale*inv_scale + wd*p;  vel = mu*vel + g;  p -= lr*mult * (g + mu*vel if nesterov else vel)

Tolerances are not chosen by hand: next to the float64 reference every test runs the same update in fp32 torch eager
(every operand, the hyper-parameters included, held in fp32 as the kernel receives them), and the constants below are
4x the error of that eager run against float64, measured on an MI355X over all cases of this file. Three error measures
are used, each where it is well defined:

* parameters, first moments and velocities are signed sums that cancel, so an element's relative error is unbounded;
  they are compared by the largest absolute error divided by the largest ``|reference|`` of the same tensor (an
  ``atol`` scaled to the tensor, ``rtol = 0``). With ``|p| < 6`` this is far inside the ``atol=2e-5, rtol=1e-5``
  (AdamW) and ``1e-5`` (Momentum) that the older tests ask of the masters.
* second moments are sums of non-negative terms: largest elementwise relative error, no absolute term, exact zeros
  where the reference is zero.
* the squared norm is one positive number: relative error (older test: ``rtol=1e-4``).

Low-precision shadows are checked bitwise against ``master.to(dtype)``: both sides do one round-to-nearest-even convert
of the fp32 value just written.
"""
import math

import pytest
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.ops import _loader as L
from paddlepaddle_amd.ops import optim as O
from paddlepaddle_amd.ops.optim import global_sq_norm

pytestmark = pytest.mark.gpu

CHUNK = 16384
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
F32, F64 = torch.float32, torch.float64

# 4x the error of the fp32 eager update against float64 (measured values on the right; "kernel" is what the HIP kernel
# showed in the same run, for orientation only)
TOL_ADAMW_P = 4 * 2.20e-7   # scaled abs; eager 2.196e-07, kernel 1.622e-07
TOL_ADAMW_M = 4 * 2.06e-7   # scaled abs; eager 2.056e-07, kernel 2.056e-07
RTOL_ADAMW_V = 4 * 6.37e-7  # max rel;    eager 6.365e-07, kernel 6.022e-07 (1 - fp32(0.95) is 2.4e-7 off 0.05)
TOL_MOM_P = 4 * 1.50e-7     # scaled abs; eager 1.499e-07, kernel 1.499e-07
TOL_MOM_VEL = 4 * 1.33e-7   # scaled abs; eager 1.330e-07, kernel 1.006e-07
RTOL_SQ_NORM = 4 * 3.62e-8  # rel;        eager 3.624e-08, kernel 8.275e-08

SEEN = {}  # quantity -> [largest eager error, largest kernel error] over the tests run so far (printed by each test)


def _randn(n, seed, dtype=F32, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(n, device="cuda", generator=g) * scale).to(dtype)


def _s(x, dtype):
    return torch.tensor(x, dtype=dtype, device="cuda")


def _bits(t):
    return t.contiguous().view(_INT[t.dtype])


def _scaled_err(got, ref):
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


def _report(*keys):
    for k in keys:
        if k in SEEN:
            print(f"[optim-kernels] {k}: fp32-eager max err {SEEN[k][0]:.3e}, kernel max err {SEEN[k][1]:.3e}")


class _Ent:
    """One parameter with its gradient tensor: separately allocated, or (``offset``) views into one flat parameter
    buffer and one flat gradient buffer with guard elements on both sides."""

    def __init__(self, name, shape, dtype, seed, offset=None, lr_mult=1.0, gscale=1.0):
        n = math.prod(shape)
        self.name, self.n, self.dtype, self.gscale, self.lr_mult = name, n, dtype, gscale, lr_mult
        self.guards = []
        if offset is None:
            w = _randn(n, seed, dtype).view(shape)
            g = torch.zeros(shape, dtype=dtype, device="cuda")
        else:
            pbuf, gbuf = _randn(offset + n + 3, seed, dtype), _randn(offset + n + 3, seed + 1, dtype)
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


def _geometry(dtype, tiny=None, half_lr=None):
    """The shared geometry set. ``tiny``: index of the tensor whose grads are scaled by 1e-6; ``half_lr``: index of
    the tensor with lr multiplier 0.5."""
    shapes = [(7,), (33, 17), (CHUNK,), (CHUNK + 1,), (2 * CHUNK + 3,)]
    ents = []
    for i, shape in enumerate(shapes):
        ents.append(_Ent(f"t{i}", shape, dtype, 100 + i, lr_mult=0.5 if i == half_lr else 1.0,
                         gscale=1e-6 if i == tiny else 1.0))
    size = torch.empty(0, dtype=dtype).element_size()
    for off in ((1,) if dtype == F32 else (1, 2)):
        e = _Ent(f"view{off}", (CHUNK + 5,), dtype, 200 + 10 * off, offset=off)
        # contiguous, but not on the 16-byte (fp32) / 8-byte (16-bit) boundary of the vector branch: whole chunks of
        # these tensors take the scalar loop (fp32: P and G; 16-bit: G and the shadow LP)
        for t in (e.param._t, e.grad):
            assert t.is_contiguous() and t.data_ptr() % 16 == off * size
            assert t.data_ptr() % (16 if dtype == F32 else 8) != 0
        ents.append(e)
    return ents


def _fp32_of(opt, e):
    return opt._master_weights[id(e.param)] if e.dtype != F32 else e.param._t.detach()


def _check_shadow(opt, e):
    if e.dtype != F32:
        master = opt._master_weights[id(e.param)]
        assert master.dtype == F32 and master.data_ptr() % 16 == 0
        assert torch.equal(_bits(e.param._t.detach()), _bits(master.to(e.dtype))), f"{e.name}: shadow != RNE(master)"


# ---------------------------------------------------------------------------------------------------------- AdamW


def _adamw_math(st, g, lr, mult, wd, b1, b2, eps, t):
    """One documented AdamW update of state [p, m, v] in the dtype of the state; ``g`` is the effective gradient."""
    dt = st[0].dtype
    lr, mult, wd, b1, b2, eps, one = (_s(x, dt) for x in (lr, mult, wd, b1, b2, eps, 1.0))
    p, m, v = st
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * g * g
    plr = lr * mult
    bc1, bc2 = one - b1 ** t, one - b2 ** t
    p = p * (one - plr * wd) - plr / bc1 * m / ((v / bc2).sqrt() + eps)
    return [p, m, v]


def _clip_coef(grads, dtype, clip_norm=1.0):
    """clip_norm / max(global norm of the gradients as stored, clip_norm), computed in ``dtype``."""
    sq = torch.stack([g.to(dtype).pow(2).sum() for g in grads]).sum()
    return _s(clip_norm, dtype) / torch.clamp(sq.sqrt(), min=clip_norm)


def _run_adamw(opt, ents, wd_of, ratio_of=None, steps=3, lr=1e-2, b1=0.8, b2=0.95, eps=1e-6, premul=1.0, inv=None,
               clip=False, seed0=1000, after_step=None):
    ref = {e.name: e.state(F64) for e in ents}
    eag = {e.name: e.state(F32) for e in ents}
    L.reset_calls()
    for t in range(1, steps + 1):
        for i, e in enumerate(ents):
            e.new_grad(seed0 + 100 * t + i, premul)
        scale = {}
        for dt in (F64, F32):
            s = _s(1.0, dt) if inv is None else inv.to(dt).reshape(())
            if clip:
                s = _clip_coef([e.grad for e in ents], dt) * s
            scale[dt] = s
        opt.step()
        assert L.calls("pa_adamw_multi") == t, "one multi-tensor launch per group per step"
        assert L.calls("pa_sq_norm_multi") == (t if clip else 0)
        if clip:
            assert opt._clip_coef is not None, "the clip was not folded into the fused kernel"
        for e in ents:
            mult = e.lr_mult * (1.0 if ratio_of is None else ratio_of(e.name))
            for states, dt in ((ref, F64), (eag, F32)):
                states[e.name] = _adamw_math(states[e.name], e.grad.to(dt) * scale[dt], lr, mult, wd_of(e.name), b1,
                                             b2, eps, t)
            m1, m2 = opt._accumulators["moment1"][id(e.param)], opt._accumulators["moment2"][id(e.param)]
            assert m1.dtype == F32 and m2.dtype == F32
            what = f"{e.name} step {t}"
            _check("adamw.p", what, _fp32_of(opt, e), eag[e.name][0], ref[e.name][0], TOL_ADAMW_P)
            _check("adamw.m", what, m1, eag[e.name][1], ref[e.name][1], TOL_ADAMW_M)
            _check("adamw.v", what, m2, eag[e.name][2], ref[e.name][2], RTOL_ADAMW_V, err=_rel_err)
            _check_shadow(opt, e)
            e.check_guards()
        if after_step is not None:
            after_step(t)
    _report("adamw.p", "adamw.m", "adamw.v")


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("dtype", list(_DTYPES), ids=list(_DTYPES))
def test_adamw_geometry(dtype, clip):
    """Chunk edges, the scalar branch on misaligned views, fp32 / bf16 / fp16, non-default betas and eps, per-row
    weight decay and lr multiplier, the inv_scale pointer alone and multiplied with the folded clip coefficient.
    The clip coefficient is taken over the gradients as stored (1024x), as ``_apply_clip`` sees them."""
    dt = _DTYPES[dtype]
    ents = _geometry(dt, tiny=2, half_lr=3)  # t2: grads ~1e-6, so sqrt(v^) ~ eps; t3: optimize_attr lr 0.5
    opt = paddle.optimizer.AdamW(1e-2, beta1=0.8, beta2=0.95, epsilon=1e-6, parameters=[e.param for e in ents],
                                 weight_decay=0.1, apply_decay_param_fun=lambda name: name != "t1",
                                 multi_precision=dt != F32,
                                 grad_clip=paddle.nn.ClipGradByGlobalNorm(1.0) if clip else None)
    inv = torch.full((1,), 1.0 / 1024, dtype=F32, device="cuda")
    opt._inv_scale_tensor = inv
    _run_adamw(opt, ents, wd_of=lambda name: 0.0 if name == "t1" else 0.1, premul=1024.0, inv=inv, clip=clip)
    moved = (ents[1].param._t.detach().float() - ents[1].w0.float()).abs().max()
    assert float(moved) > 1e-3  # the parameter without decay is still updated


def test_adamw_grid_wrap_4100_items():
    """4100 five-element parameters, consecutive views of one flat fp32 buffer: 4100 work items on the 4096-workgroup
    grid (four workgroups take a second item), pointers cycling through 0/4/8/12 bytes past a 16-byte boundary."""
    n_p, k = 4100, 5
    flat_p, flat_g = _randn(n_p * k, 300), torch.zeros(n_p * k, device="cuda")
    w0 = flat_p.clone()
    ps = []
    for i in range(n_p):
        p = paddle.Parameter(flat_p[i * k:(i + 1) * k], name=f"w{i}")
        p._t.grad = flat_g[i * k:(i + 1) * k]
        ps.append(p)
    assert {p._t.data_ptr() % 16 for p in ps} == {0, 4, 8, 12} == {p._t.grad.data_ptr() % 16 for p in ps}
    assert all(p._t.data_ptr() == flat_p.data_ptr() + 4 * k * i for i, p in enumerate(ps))
    opt = paddle.optimizer.AdamW(1e-2, beta1=0.8, beta2=0.95, epsilon=1e-6, parameters=ps, weight_decay=0.1)
    ref = [w0.double(), torch.zeros_like(w0, dtype=F64), torch.zeros_like(w0, dtype=F64)]
    eag = [w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0)]
    L.reset_calls()
    for t in range(1, 4):
        flat_g.copy_(_randn(n_p * k, 310 + t))
        opt.step()
        assert L.calls("pa_adamw_multi") == t
        ref = _adamw_math(ref, flat_g.double(), 1e-2, 1.0, 0.1, 0.8, 0.95, 1e-6, t)
        eag = _adamw_math(eag, flat_g, 1e-2, 1.0, 0.1, 0.8, 0.95, 1e-6, t)
        m1 = torch.cat([opt._accumulators["moment1"][id(p)] for p in ps])
        m2 = torch.cat([opt._accumulators["moment2"][id(p)] for p in ps])
        _check("adamw.p", f"flat step {t}", flat_p, eag[0], ref[0], TOL_ADAMW_P)
        _check("adamw.m", f"flat step {t}", m1, eag[1], ref[1], TOL_ADAMW_M)
        _check("adamw.v", f"flat step {t}", m2, eag[2], ref[2], RTOL_ADAMW_V, err=_rel_err)
    assert opt._tables[id(opt._param_groups[0])].n_items == n_p  # work items
    _report("adamw.p", "adamw.m", "adamw.v")


def test_adam_fused_without_decay():
    """Adam (not decoupled, no weight decay) takes the same fused launch with a zero decay column."""
    ents = [_Ent("a0", (33, 17), F32, 400), _Ent("a1", (CHUNK + 1,), F32, 401)]
    opt = paddle.optimizer.Adam(1e-2, beta1=0.8, beta2=0.95, epsilon=1e-6, parameters=[e.param for e in ents])
    _run_adamw(opt, ents, wd_of=lambda name: 0.0, seed0=4000)
    assert not getattr(opt, "_host_path", False)


def test_adamw_lr_ratio_gpu():
    """lr_ratio(param) multiplies the row's lr_mult: ratio 0 leaves the parameter bit-identical while m and v advance,
    0.5 halves both the update and the decoupled decay; it composes with optimize_attr's learning rate."""
    ratios = {"frozen": 0.0, "half": 0.5, "full": 1.0}
    ents = [_Ent("frozen", (CHUNK + 1,), F32, 500), _Ent("half", (33, 17), F32, 501, lr_mult=0.5),
            _Ent("full", (7,), F32, 502)]
    seen = []

    def ratio(p):
        seen.append(p)
        return ratios[p.name]

    opt = paddle.optimizer.AdamW(1e-2, beta1=0.8, beta2=0.95, epsilon=1e-6, parameters=[e.param for e in ents],
                                 weight_decay=0.1, lr_ratio=ratio)

    def frozen(t):
        assert torch.equal(_bits(ents[0].param._t.detach()), _bits(ents[0].w0)), "lr_ratio 0 moved the parameter"

    _run_adamw(opt, ents, wd_of=lambda name: 0.1, ratio_of=ratios.get, seed0=5000, after_step=frozen)
    assert seen and all(isinstance(p, paddle.Parameter) for p in seen)  # the callable receives the parameter
    assert float(opt._accumulators["moment2"][id(ents[0].param)].min()) > 0.0


def test_adamw_table_follows_a_replaced_moment():
    """The group's device table is keyed on every pointer in its rows: a ``moment1`` accumulator replaced by a fresh
    tensor of ones (new address; parameter and gradient addresses unchanged) is the one the next step reads and
    writes, and the orphaned tensor is left alone. With N(0, 1) gradients the step-2 parameter computed from the
    orphaned moment is 4e-2 of max|p| (7 elements) away from the one computed from the ones, 4e4 x ``TOL_ADAMW_P``
    (float64 on the CPU, median over seeds 0..99; smallest 1.0e-2, largest 0.2). A table keyed on the parameter
    and gradient pointers alone fails the parameter, the moment and the orphan check."""
    lr, wd, b1, b2, eps = 1e-2, 0.1, 0.8, 0.95, 1e-6
    ents = [_Ent("s0", (7,), F32, 800), _Ent("s1", (CHUNK + 1,), F32, 801)]
    opt = paddle.optimizer.AdamW(lr, beta1=b1, beta2=b2, epsilon=eps, parameters=[e.param for e in ents],
                                 weight_decay=wd)
    ref = {e.name: e.state(F64) for e in ents}

    def step(t):
        for i, e in enumerate(ents):
            e.new_grad(8000 + 100 * t + i, 1.0)
        opt.step()

    step(1)
    for e in ents:
        ref[e.name] = _adamw_math(ref[e.name], e.grad.double(), lr, 1.0, wd, b1, b2, eps, 1)
    m1 = opt._accumulators["moment1"]
    old = m1[id(ents[0].param)]
    fresh = torch.ones(7, dtype=F32, device="cuda")
    assert fresh.data_ptr() != old.data_ptr()
    m1[id(ents[0].param)] = fresh
    old_bits = _bits(old).clone()
    ptrs = [(e.param._t.data_ptr(), e.grad.data_ptr()) for e in ents]

    step(2)
    assert ptrs == [(e.param._t.data_ptr(), e.param._t.grad.data_ptr()) for e in ents]
    orphan = _adamw_math(ref["s0"], ents[0].grad.double(), lr, 1.0, wd, b1, b2, eps, 2)
    ref["s0"][1] = torch.ones(7, dtype=F64, device="cuda")
    for e in ents:
        ref[e.name] = _adamw_math(ref[e.name], e.grad.double(), lr, 1.0, wd, b1, b2, eps, 2)
        assert _scaled_err(e.param._t.detach(), ref[e.name][0]) <= TOL_ADAMW_P, e.name
        assert _scaled_err(m1[id(e.param)], ref[e.name][1]) <= TOL_ADAMW_M, e.name
    assert _scaled_err(orphan[0], ref["s0"][0]) > 1000 * TOL_ADAMW_P  # the check above tells the two tables apart
    assert m1[id(ents[0].param)] is fresh and not bool((fresh == 1).all()), "the new moment was not written"
    assert torch.equal(_bits(old), old_bits), "the orphaned moment was written"

    from paddlepaddle_amd.ops import multi_tensor as MT
    assert L.lib().pa_multi_tensor_chunk() == MT.CHUNK == CHUNK


# ------------------------------------------------------------------------------------------------------- Momentum


def _momentum_math(st, g, lr, mult, wd, mu, gs, nesterov):
    dt = st[0].dtype
    lr, mult, wd, mu, gs = (_s(x, dt) for x in (lr, mult, wd, mu, gs))
    p, vel = st
    g = g * gs + wd * p
    vel = mu * vel + g
    p = p - lr * mult * (g + mu * vel if nesterov else vel)
    return [p, vel]


@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
@pytest.mark.parametrize("dtype", list(_DTYPES), ids=list(_DTYPES))
def test_momentum_geometry(dtype, nesterov):
    """The AdamW geometry set through momentum_multi_k: L2 decay folded into the gradient, rescale_grad * inv_scale,
    a per-row lr multiplier, both Nesterov settings."""
    dt = _DTYPES[dtype]
    lr, mu, wd, rescale = 0.05, 0.9, 1e-2, 0.5
    ents = _geometry(dt, half_lr=3)
    opt = paddle.optimizer.Momentum(lr, mu, parameters=[e.param for e in ents], use_nesterov=nesterov,
                                    weight_decay=wd, rescale_grad=rescale, multi_precision=dt != F32)
    inv = torch.full((1,), 1.0 / 1024, dtype=F32, device="cuda")
    opt._inv_scale_tensor = inv
    ref = {e.name: e.state(F64)[:2] for e in ents}
    eag = {e.name: e.state(F32)[:2] for e in ents}
    L.reset_calls()
    for t in range(1, 4):
        for i, e in enumerate(ents):
            e.new_grad(6000 + 100 * t + i, 1024.0)
        opt.step()
        assert L.calls("pa_momentum_multi") == t, "one multi-tensor launch per group per step"
        for e in ents:
            for states, d in ((ref, F64), (eag, F32)):
                # the kernel receives rescale and reads inv_scale as fp32 and multiplies them first
                states[e.name] = _momentum_math(states[e.name], e.grad.to(d), lr, e.lr_mult, wd, mu,
                                                rescale * (1.0 / 1024), nesterov)
            vel = opt._accumulators["velocity"][id(e.param)]
            assert vel.dtype == F32
            what = f"{e.name} step {t}"
            _check("momentum.p", what, _fp32_of(opt, e), eag[e.name][0], ref[e.name][0], TOL_MOM_P)
            _check("momentum.vel", what, vel, eag[e.name][1], ref[e.name][1], TOL_MOM_VEL)
            _check_shadow(opt, e)
            e.check_guards()
    _report("momentum.p", "momentum.vel")


# ------------------------------------------------------------------------------------------------ global_sq_norm


def _check_norm(tensors, what):
    before = L.calls("pa_sq_norm_multi")
    got = global_sq_norm(tensors)
    assert L.calls("pa_sq_norm_multi") == before + 1, "one launch per call"
    assert got.dtype == F32 and got.dim() == 0
    ref = torch.stack([t.double().pow(2).sum() for t in tensors]).sum()
    eager = torch.stack([t.float().pow(2).sum() for t in tensors]).sum()
    _check("sq_norm", what, got, eager, ref, RTOL_SQ_NORM)  # one positive number: scaled error == relative error
    return got


def test_sq_norm_mixed_dtypes_edges_and_views():
    lengths = (7, 333, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
    tensors = [_randn(n, 700 + 10 * j + i, dt) for j, dt in enumerate(_DTYPES.values()) for i, n in enumerate(lengths)]
    bview = _randn(CHUNK + 6, 740, torch.bfloat16)[1:]
    fview = _randn(CHUNK + 6, 741, F32)[1:]
    assert bview.is_contiguous() and bview.data_ptr() % 16 == 2  # the 16-byte vector path is not taken
    assert fview.is_contiguous() and fview.data_ptr() % 16 == 4
    tensors += [bview, fview, torch.empty(0, dtype=F32, device="cuda")]
    _check_norm(tensors, "mixed list")
    n_cached = len(O._SQ_CACHE)
    _check_norm(tensors, "mixed list, second call")  # unchanged list: the cached table is reused
    assert len(O._SQ_CACHE) == n_cached
    _report("sq_norm")


def test_sq_norm_grid_wrap_1026_items():
    x = _randn(1026 * CHUNK + 5, 750, torch.bfloat16)  # 1027 items on the 1024-workgroup grid
    _check_norm([x], "1026*CHUNK+5 bf16")
    _report("sq_norm")


def test_sq_norm_cache_is_keyed_on_length_and_dtype():
    """Same address, then a shorter length, then another dtype: each call gets its own table. The order (long before
    short, f32 before bf16) keeps even a stale table inside ``buf``. ``buf`` is made of 8192 bf16 normal deviates read
    as 4096 fp32 values, so that both views of it hold finite numbers of ordinary size (the low halves of fp32
    normal deviates, read as bf16, would hold infinities and NaNs)."""
    buf = _randn(8192, 760, torch.bfloat16).view(F32)
    assert buf.numel() == 4096 and bool(buf.isfinite().all()) and float(buf.abs().max()) < 16.0
    a = _check_norm([buf[:1000]], "f32[:1000]")
    b = _check_norm([buf[:500]], "f32[:500] at the same address")
    c = _check_norm([buf.view(torch.bfloat16)[:1000]], "bf16[:1000] at the same address")
    assert float(b) < float(a) and float(c) != float(a)
    _check_norm([buf[:1000]], "f32[:1000] again")
    _report("sq_norm")
