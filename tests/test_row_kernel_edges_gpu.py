"""Row kernels (csrc/kernels/softmax.hip, norm.hip) at the inputs and geometries where they can go wrong:
-inf inside softmax / cross-entropy rows, LayerNorm rows whose first element is an outlier, every branch of the
norm dispatch (lanes per row, padded lanes, row counts around the 4-rows-per-workgroup and 512-partials limits),
the 2048-column revisit of the softmax kernels, the vocabulary-slice cross entropy called directly, and inputs
with no rows.

Inputs are built in fp32 from a fixed seed and rounded to the dtype under test; the reference is the plain torch
op in float64 on those rounded values. Tolerances are those of the matching test in test_hip_kernels.py (`_tol`
with that test's multipliers; fp16, where that test has no fp16 case, takes `_tol(torch.float16)` with the same
multipliers; the cross-entropy values are test_softmax_cross_entropy's, whose non-fp32 branch also serves fp16)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from paddlepaddle_amd import ops  # noqa: E402
from paddlepaddle_amd.ops import _loader as L  # noqa: E402
from paddlepaddle_amd.ops.loss import ce_slice_grad, ce_slice_stats  # noqa: E402
from paddlepaddle_amd.ops.norm import layer_norm_residual, rms_norm_residual  # noqa: E402

DEV = "cuda"
NINF = float("-inf")
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IGNORE = -100


def _ran(*launchers):
    assert L._LIB is not None, "HIP kernel library not loaded"
    for n in launchers:
        assert L.calls(n) > 0, f"{n} did not run (calls: {dict(L.CALLS)})"


def _tol(dt):
    return {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 2e-3}[dt]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, g, scale=1.0):
    return torch.randn(shape, device=DEV, generator=g) * scale


def _close(name, got, ref, atol, rtol):
    """assert_close in float64 that first prints the largest absolute error and the largest ratio of error to
    allowance (atol + rtol * |ref|), so that a run with -s records how far inside the tolerance each case is."""
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if got.numel():
        err = (got - ref).abs()
        fin = torch.isfinite(err)
        if fin.any():
            ratio = (err / (atol + rtol * ref.abs()))[fin].max().item()
            print(f"ERR {name}: max_abs={err[fin].max().item():.3e} max_ratio={ratio:.3f} atol={atol:g} rtol={rtol:g}")
    torch.testing.assert_close(got, ref, atol=atol, rtol=rtol)


# tolerance multipliers (atol, rtol) in units of _tol(dt), from test_softmax / test_layer_norm / test_rms_norm
SM_Y, SM_DX = (1, 2), (2, 4)
NORM_TOL = {"layer_norm": {"y": (8, 1), "dx": (10, 2), "dw": (60, 4), "db": (60, 4)},
            "rms_norm": {"y": (4, 1), "dx": (8, 2), "dw": (40, 4)}}


def _ce_tol(dt):
    """(loss/lse atol, rtol), (gradient atol, rtol) of test_softmax_cross_entropy."""
    f32 = dt == torch.float32
    return (1e-3 if f32 else 3e-2, 1e-3), (1e-5 if f32 else 3e-3, 1e-3 if f32 else 3e-2)


# ---------------------------------------------------------------------------------------------------------------
# A. -inf inputs


def _softmax_check(x32, dt, tag, masked=None):
    """ops.softmax forward + backward on x32 rounded to dt against torch.softmax in float64; `masked` (bool, x's
    shape) marks the -inf positions, which must come out as exact zeros in y and dx."""
    x = x32.to(dt).requires_grad_(True)
    y = ops.softmax(x, -1)
    _ran("pa_softmax_fwd")
    x64 = x.detach().double().requires_grad_(True)
    y64 = torch.softmax(x64, -1)
    g = torch.randn(x32.shape, device=DEV, generator=_gen(99)).to(dt)
    y.backward(g)
    _ran("pa_softmax_bwd")
    y64.backward(g.double())
    assert torch.isfinite(y).all(), f"{tag}: y has NaN/Inf"
    assert torch.isfinite(x.grad).all(), f"{tag}: dx has NaN/Inf"
    t = _tol(dt)
    _close(f"{tag} y", y, y64, t * SM_Y[0], t * SM_Y[1])
    _close(f"{tag} dx", x.grad, x64.grad, t * SM_DX[0], t * SM_DX[1])
    if masked is not None:
        assert (y.detach()[masked] == 0).all(), f"{tag}: y is not exactly 0 at masked positions"
        assert (x.grad[masked] == 0).all(), f"{tag}: dx is not exactly 0 at masked positions"


CAUSAL_K = [0, 7, 8, 2047, 2048, 2055, 4087]


def _neg_inf_mask(case):
    """bool [rows, cols]: True where the input is -inf."""
    if case == "tail_group_2056":     # one all--inf 8-group right after the 2048-column revisit
        m = torch.zeros(5, 2056, dtype=torch.bool, device=DEV)
        m[:, 2048:2056] = True
    elif case == "causal_4096":       # row i: everything after column CAUSAL_K[i]
        k = torch.tensor(CAUSAL_K, device=DEV).unsqueeze(1)
        m = torch.arange(4096, device=DEV).unsqueeze(0) > k
    else:                             # "leading_4096": leading all--inf groups, finite tail
        m = torch.zeros(5, 4096, dtype=torch.bool, device=DEV)
        m[:, :2048] = True
    return m


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ["tail_group_2056", "causal_4096", "leading_4096"])
def test_softmax_neg_inf(case, dt):
    """A thread that has merged a finite 8-group and then meets an all--inf group 2048 columns later must add 0
    for it (with exp(-inf - -inf) = NaN as that group's sum the whole row became NaN). Leading -inf groups were
    always hidden by the -inf running maximum and must stay right."""
    m = _neg_inf_mask(case)
    x32 = _randn(m.shape, _gen(10), 4.0).masked_fill(m, NINF)
    _softmax_check(x32, dt, f"A softmax {case} {dt}", masked=m)


def test_softmax_mask_fuse_upper_triangle_long_sequence():
    """Causal softmax over 2304 > 2048 positions: rows 0 .. 2303 mask everything above the diagonal with -inf."""
    from paddlepaddle_amd.framework.tensor import _wrap
    from paddlepaddle_amd.incubate.operators import softmax_mask_fuse_upper_triangle
    S, dt = 2304, torch.bfloat16
    x = _randn((1, 1, S, S), _gen(11), 4.0).to(dt)
    y = softmax_mask_fuse_upper_triangle(_wrap(x))._t
    _ran("pa_softmax_fwd")
    up = torch.ones(S, S, dtype=torch.bool, device=DEV).triu(1)
    y64 = torch.softmax(x.double().masked_fill(up, NINF), -1)
    assert torch.isfinite(y).all()
    _close("A mask_fuse_upper_triangle bf16 y", y, y64, _tol(dt) * SM_Y[0], _tol(dt) * SM_Y[1])
    assert (y[0, 0][up] == 0).all()


def _banned_mask(V):
    """Banned-token columns: two 8-aligned runs at columns >= 2048 (one directly at the revisit, one at the end
    of the row) and one run that starts and ends inside 8-groups."""
    b = torch.zeros(V, dtype=torch.bool, device=DEV)
    b[2048:2064] = True
    b[V - 8:V] = True
    b[3003:3030] = True
    return b


def _finite_labels(banned, rows, g):
    ok = (~banned).nonzero().squeeze(1)
    lab = ok[torch.randint(0, ok.numel(), (rows,), device=DEV, generator=g)]
    lab[0], lab[1], lab[2] = 2047, 2064, 3002   # finite neighbours of the banned runs
    return lab


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("V", [4096, 50304])
def test_softmax_cross_entropy_banned_tokens(V, dt):
    """Banned tokens (-inf logits) in a vocabulary row: loss and gradient stay finite and match F.cross_entropy in
    float64; the gradient at a banned token is exactly 0."""
    g = _gen(12)
    rows = 9
    banned = _banned_mask(V)
    logits = _randn((rows, V), g, 3.0).masked_fill(banned, NINF).to(dt).requires_grad_(True)
    labels = _finite_labels(banned, rows, g)
    labels[5] = IGNORE
    loss = ops.softmax_cross_entropy(logits, labels, IGNORE)
    _ran("pa_softmax_ce_fwd")
    l64 = logits.detach().double().requires_grad_(True)
    ref = F.cross_entropy(l64, labels, ignore_index=IGNORE, reduction="none")
    dl = torch.rand(rows, device=DEV, generator=g)
    loss.backward(dl)
    _ran("pa_softmax_ce_bwd")
    ref.backward(dl.double())
    assert torch.isfinite(loss).all() and torch.isfinite(logits.grad).all()
    (la, lr), (ga, gr) = _ce_tol(dt)
    _close(f"A ce banned V={V} {dt} loss", loss, ref, la, lr)
    _close(f"A ce banned V={V} {dt} grad", logits.grad, l64.grad, ga, gr)
    assert loss[5] == 0 and (logits.grad[5] == 0).all()
    assert (logits.grad[:, banned] == 0).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_ce_slice_stats_banned_tokens(dt):
    """The slice kernel shares row_stats: banned runs inside each 2056-wide slice (one all--inf group at the
    slice's columns 2048 .. 2055, one unaligned run)."""
    g = _gen(13)
    rows, S, n = 9, 2056, 3
    banned = torch.zeros(S * n, dtype=torch.bool, device=DEV)
    for s in range(n):
        banned[s * S + 2048:s * S + 2056] = True
        banned[s * S + 100:s * S + 117] = True
    full = _randn((rows, S * n), g, 3.0).masked_fill(banned, NINF).to(dt)
    labels = _finite_labels(banned, rows, g)
    (la, lr), _ = _ce_tol(dt)
    lses, tgts = [], []
    for s in range(n):
        sl = full[:, s * S:(s + 1) * S].contiguous()
        lse, tgt = ce_slice_stats(sl, labels, s * S)
        assert torch.isfinite(lse).all()
        _close(f"A ce_slice banned {dt} lse[{s}]", lse, torch.logsumexp(sl.double(), -1), la, lr)
        lses.append(lse)
        tgts.append(tgt)
    _ran("pa_ce_slice_fwd")
    loss = torch.logsumexp(torch.stack(lses), 0) - torch.stack(tgts).sum(0)
    _close(f"A ce_slice banned {dt} loss", loss, F.cross_entropy(full.double(), labels, reduction="none"), la, lr)


# ---------------------------------------------------------------------------------------------------------------
# B. ce_slice_stats / ce_slice_grad called directly


def _slice_labels(S, n):
    """11 labels: first and last column of every slice (each is also the column just outside a neighbouring
    slice, and owned by another slice from that neighbour's point of view), ignore_index, interior columns."""
    lab = []
    for s in range(n):
        lab += [s * S, (s + 1) * S - 1]
    lab.append(IGNORE)
    k = 0
    while len(lab) < 11:
        lab.append((k % n) * S + S // 2 + k)
        k += 1
    return torch.tensor(lab, device=DEV, dtype=torch.int64)


SLICE_GEOM = [(24, 3), (6168, 3), (50304, 4)]
_slice_cache = {}


def _slice_problem(V, n, dt):
    """Logits rounded to dt, labels, dloss and the float64 reference (per-slice lse and label logit, per-row loss,
    global lse, gradient), computed once per (V, dt) and shared by the tests below; nothing in it is modified."""
    key = (V, dt)
    if key not in _slice_cache:
        g = _gen(20)
        S = V // n
        rows = 11
        full = _randn((rows, V), g, 3.0).to(dt)
        labels = _slice_labels(S, n)
        dloss = torch.rand(rows, device=DEV, generator=g) + 0.25
        f64 = full.double().requires_grad_(True)
        loss64 = F.cross_entropy(f64, labels, ignore_index=IGNORE, reduction="none")
        loss64.backward(dloss.double())
        _slice_cache[key] = dict(S=S, n=n, rows=rows, full=full, labels=labels, dloss=dloss,
                                 loss64=loss64.detach(), grad64=f64.grad,
                                 lse64=torch.logsumexp(full.double(), -1))
    return _slice_cache[key]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("V,n", SLICE_GEOM)
def test_ce_slice_stats_direct(V, n, dt):
    p = _slice_problem(V, n, dt)
    S, labels, full = p["S"], p["labels"], p["full"]
    (la, lr), _ = _ce_tol(dt)
    lses, tgts = [], []
    for s in range(n):
        sl = full[:, s * S:(s + 1) * S].contiguous()
        lse, tgt = ce_slice_stats(sl, labels, s * S)
        _close(f"B stats V={V} {dt} lse[{s}]", lse, torch.logsumexp(sl.double(), -1), la, lr)
        local = labels - s * S
        inside = (local >= 0) & (local < S)
        want = torch.where(inside, sl.double().gather(1, local.clamp(0, S - 1).unsqueeze(1)).squeeze(1),
                           torch.zeros(p["rows"], dtype=torch.float64, device=DEV))
        assert torch.equal(tgt.double(), want), f"slice {s}: label logit {tgt.tolist()} vs {want.tolist()}"
        assert (tgt[~inside] == 0).all()
        lses.append(lse)
        tgts.append(tgt)
    _ran("pa_ce_slice_fwd")
    assert L.calls("pa_ce_slice_fwd") == n
    loss = torch.logsumexp(torch.stack(lses), 0) - torch.stack(tgts).sum(0)
    valid = labels != IGNORE   # the caller zeroes ignored rows; F.cross_entropy returns 0 for them
    _close(f"B stats V={V} {dt} combined loss", loss[valid], p["loss64"][valid], la, lr)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("V,n", SLICE_GEOM)
def test_ce_slice_grad_direct(V, n, dt):
    p = _slice_problem(V, n, dt)
    S, labels, full, dloss = p["S"], p["labels"], p["full"], p["dloss"]
    lse = p["lse64"].float()   # the global logsumexp, as the caller hands it over
    _, (ga, gr) = _ce_tol(dt)
    ign = labels == IGNORE
    for s in range(n):
        sl = full[:, s * S:(s + 1) * S].contiguous()
        keep = sl.clone()
        out = ce_slice_grad(sl, labels, s * S, lse, dloss, IGNORE)
        assert torch.equal(sl, keep), "the out-of-place call changed its input"
        _close(f"B grad V={V} {dt} slice {s}", out, p["grad64"][:, s * S:(s + 1) * S], ga, gr)
        assert (out[ign] == 0).all()
        inplace = sl.clone()
        res = ce_slice_grad(inplace, labels, s * S, lse, dloss, IGNORE, out=inplace)
        assert res.data_ptr() == inplace.data_ptr()
        assert torch.equal(inplace, out), "in-place gradient differs from the out-of-place one"
    _ran("pa_ce_slice_bwd")
    assert L.calls("pa_ce_slice_bwd") == 2 * n


@pytest.mark.parametrize("kind", ["int32", "strided"])
def test_ce_slice_label_layouts(kind):
    """int32 labels and a strided labels[::2] view give bitwise the results of contiguous int64 labels (the
    kernels read a dense int64 vector; the wrappers convert)."""
    p = _slice_problem(6168, 3, torch.bfloat16)
    S, labels, full, dloss = p["S"], p["labels"], p["full"], p["dloss"]
    if kind == "int32":
        alt = labels.to(torch.int32)
    else:
        buf = torch.full((2 * labels.numel(),), 3, dtype=torch.int64, device=DEV)
        buf[::2] = labels
        alt = buf[::2]
        assert not alt.is_contiguous()
    lse = p["lse64"].float()
    for s in range(p["n"]):
        sl = full[:, s * S:(s + 1) * S].contiguous()
        a, b = ce_slice_stats(sl, labels, s * S), ce_slice_stats(sl, alt, s * S)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        ga = ce_slice_grad(sl, labels, s * S, lse, dloss, IGNORE)
        gb = ce_slice_grad(sl, alt, s * S, lse, dloss, IGNORE)
        assert torch.equal(ga, gb)
    _ran("pa_ce_slice_fwd", "pa_ce_slice_bwd")


# ---------------------------------------------------------------------------------------------------------------
# C. geometry of the norm and softmax kernels


def _norm_ref(op, x, w, b):
    if op == "layer_norm":
        return F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6)
    return y if w is None else y * w


def _norm_hip(op, x, w, b):
    return ops.layer_norm(x, w, b, 1e-5) if op == "layer_norm" else ops.rms_norm(x, w, 1e-6)


def _norm_check(op, dt, rows, cols, tag, w_dt=None, affine=True, x32=None, seed=30):
    """Forward, dx, dw (and db) of a norm op against float64 autograd of the same formula on the rounded inputs."""
    g = _gen(seed)
    w_dt = w_dt or dt
    ln = op == "layer_norm"
    x = (_randn((rows, cols), g) if x32 is None else x32).to(dt).requires_grad_(True)
    w = (torch.rand(cols, device=DEV, generator=g) + 0.5).to(w_dt).requires_grad_(True) if affine else None
    b = _randn((cols,), g).to(w_dt).requires_grad_(True) if affine and ln else None
    y = _norm_hip(op, x, w, b)
    _ran(f"pa_{op}_fwd")
    x64, w64, b64 = (None if t is None else t.detach().double().requires_grad_(True) for t in (x, w, b))
    y64 = _norm_ref(op, x64, w64, b64)
    gy = _randn((rows, cols), g).to(dt)
    y.backward(gy)
    _ran(f"pa_{op}_bwd")
    y64.backward(gy.double())
    t, m = _tol(dt), NORM_TOL[op]
    assert y.dtype == dt and x.grad.dtype == dt
    _close(f"{tag} y", y, y64, t * m["y"][0], t * m["y"][1])
    _close(f"{tag} dx", x.grad, x64.grad, t * m["dx"][0], t * m["dx"][1])
    if affine:
        assert w.grad.dtype == w_dt and w.grad.shape == (cols,)
        _close(f"{tag} dw", w.grad, w64.grad, t * m["dw"][0], t * m["dw"][1])
        if ln:
            assert b.grad.dtype == w_dt
            _close(f"{tag} db", b.grad, b64.grad, t * m["db"][0], t * m["db"][1])


NORM_COLS = [8, 504, 512, 520, 1024, 1032, 1536, 1544, 2048, 2056, 2560, 3072, 3080, 4096]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cols", NORM_COLS)
@pytest.mark.parametrize("op", ["layer_norm", "rms_norm"])
def test_norm_widths(op, cols, dt):
    """Every lanes-per-row instantiation (1, 2, 3, 4, 6 vectors per lane) at its upper limit and 8 columns past
    it, widths whose last vector slot is padded (520 under 2, 2560 under 6, ...), and the workgroup-per-row
    kernels from 3080 columns; 5 rows leave the second workgroup with one live wave."""
    _norm_check(op, dt, 5, cols, f"C {op} {dt} 5x{cols}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cols", [8, 520, 3080])
@pytest.mark.parametrize("rows", [1, 4, 8200])
@pytest.mark.parametrize("op", ["layer_norm", "rms_norm"])
def test_norm_row_counts(op, rows, cols, dt):
    """One row, one exactly full workgroup, and 8200 rows: more than 512 * 16, where the number of weight-gradient
    partials saturates at 512 and each partial strides over 16 or 17 rows."""
    _norm_check(op, dt, rows, cols, f"C {op} {dt} {rows}x{cols}")


@pytest.mark.parametrize("cols", [520, 3080])
@pytest.mark.parametrize("op", ["layer_norm", "rms_norm"])
def test_norm_fp32_weight_on_bf16_input(op, cols):
    """fp32 parameters with bf16 activations: the weight (and bias) gradient comes back in fp32."""
    _norm_check(op, torch.bfloat16, 5, cols, f"C {op} bf16 x, fp32 w 5x{cols}", w_dt=torch.float32)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("op", ["layer_norm", "rms_norm"])
def test_norm_without_affine_wide(op, dt):
    _norm_check(op, dt, 5, 4096, f"C {op} {dt} no affine 5x4096", affine=False)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cols", [520, 2560, 3080])
@pytest.mark.parametrize("op", ["layer_norm", "rms_norm"])
def test_norm_residual_backward(op, cols, dt):
    """(x, norm(x)) with the residual branch's gradient added inside the backward kernel; that gradient arrives
    as a non-contiguous (transposed) view."""
    g = _gen(31)
    rows = 5
    ln = op == "layer_norm"
    x = _randn((rows, cols), g).to(dt).requires_grad_(True)
    w = (torch.rand(cols, device=DEV, generator=g) + 0.5).to(dt).requires_grad_(True)
    b = _randn((cols,), g).to(dt).requires_grad_(True) if ln else None
    xres, y = layer_norm_residual(x, w, b, 1e-5) if ln else rms_norm_residual(x, w, 1e-6)
    gy = _randn((rows, cols), g).to(dt)
    gz = _randn((cols, rows), g).to(dt)       # gradient of xres.t(): reaches xres as the view gz.t()
    torch.autograd.backward([xres.t(), y], [gz, gy])
    _ran(f"pa_{op}_fwd", "pa_layer_norm_bwd" if ln else "pa_rms_norm_bwd_res")
    x64, w64, b64 = (None if t is None else t.detach().double().requires_grad_(True) for t in (x, w, b))
    torch.autograd.backward([x64.t(), _norm_ref(op, x64, w64, b64)], [gz.double(), gy.double()])
    t, m = _tol(dt), NORM_TOL[op]
    tag = f"C {op}_residual {dt} 5x{cols}"
    _close(f"{tag} dx", x.grad, x64.grad, t * m["dx"][0], t * m["dx"][1])
    _close(f"{tag} dw", w.grad, w64.grad, t * m["dw"][0], t * m["dw"][1])
    if ln:
        _close(f"{tag} db", b.grad, b64.grad, t * m["db"][0], t * m["db"][1])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("cols", [8, 2040, 2048, 2056, 65536])
def test_softmax_widths(cols, rows, dt):
    """Widths straddling the 2048-column revisit of a thread, the narrowest row and the 65536-column limit of the
    HIP path."""
    _softmax_check(_randn((rows, cols), _gen(32), 4.0), dt, f"C softmax {dt} {rows}x{cols}")


def test_softmax_large_fp32_logits():
    """fp32 logits with a spread of 30: exp overflows without the max subtraction."""
    _softmax_check(_randn((5, 2056), _gen(33), 30.0), torch.float32, "C softmax fp32 x30 5x2056")


def test_softmax_fp16_near_range_limit():
    """fp16 values near +-6e4 (fp16 max is 65504)."""
    g = _gen(34)
    sign = torch.where(torch.rand((5, 2056), device=DEV, generator=g) < 0.5, -1.0, 1.0)
    x32 = sign * 60000.0 + _randn((5, 2056), g, 64.0)
    assert x32.abs().max() < 65504
    _softmax_check(x32, torch.float16, "C softmax fp16 +-6e4 5x2056")


def test_softmax_transposed_input():
    """A non-contiguous input whose softmax axis is last only after transpose."""
    dt = torch.bfloat16
    base = _randn((2056, 5), _gen(35), 4.0).to(dt).requires_grad_(True)
    x = base.transpose(0, 1)
    assert not x.is_contiguous()
    y = ops.softmax(x, -1)
    _ran("pa_softmax_fwd")
    b64 = base.detach().double().requires_grad_(True)
    y64 = torch.softmax(b64.transpose(0, 1), -1)
    gy = _randn((5, 2056), _gen(36)).to(dt)
    y.backward(gy)
    y64.backward(gy.double())
    t = _tol(dt)
    _close("C softmax transposed bf16 y", y, y64, t * SM_Y[0], t * SM_Y[1])
    _close("C softmax transposed bf16 dx", base.grad, b64.grad, t * SM_DX[0], t * SM_DX[1])


# ---------------------------------------------------------------------------------------------------------------
# D. LayerNorm rows with an outlier


OUTLIERS = [50.0, -50.0, 1000.0, -1000.0, 1e4, -1e4]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("cols", [3072, 3080, 4096, 16384])
def test_layer_norm_outlier(cols, where, dt):
    """x ~ N(0, 1) with one outlier per row (+-50, +-1000, +-1e4: six rows) at the first or the last column. The
    first element is the shift of the kernels' mean sums: one-pass moments about it, var = s2/n - md^2, lost the
    variance of the wide kernel (> 3072 columns) when that element was the outlier. Forward and dx against float64
    at test_layer_norm's tolerances; torch's own fp32 LayerNorm is within 2.5e-5 of float64 on these inputs."""
    x32 = _randn((6, cols), _gen(40))
    x32[:, 0 if where == "first" else cols - 1] = torch.tensor(OUTLIERS, device=DEV)
    g = _gen(41)
    x = x32.to(dt).requires_grad_(True)
    w = _randn((cols,), g).to(dt)
    b = _randn((cols,), g).to(dt)
    y = ops.layer_norm(x, w, b, 1e-5)
    _ran("pa_layer_norm_fwd")
    x64 = x.detach().double().requires_grad_(True)
    y64 = F.layer_norm(x64, (cols,), w.double(), b.double(), 1e-5)
    gy = _randn((6, cols), g).to(dt)
    y.backward(gy)
    _ran("pa_layer_norm_bwd")
    y64.backward(gy.double())
    t, m = _tol(dt), NORM_TOL["layer_norm"]
    tag = f"D layer_norm outlier {where} {dt} 6x{cols}"
    _close(f"{tag} y", y, y64, t * m["y"][0], t * m["y"][1])
    _close(f"{tag} dx", x.grad, x64.grad, t * m["dx"][0], t * m["dx"][1])


# ---------------------------------------------------------------------------------------------------------------
# E. inputs without rows


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(0, 512), (2, 0, 512)])
@pytest.mark.parametrize("op", ["softmax", "softmax_cross_entropy", "layer_norm", "rms_norm", "gelu"])
def test_empty_input(op, shape, dt):
    """No rows (an expert that received no tokens): the launchers return without launching an empty grid, outputs
    keep the input's shape, dx is empty and the parameter gradients are exact zeros, not uninitialised memory."""
    cols = shape[-1]
    x = torch.empty(shape, device=DEV, dtype=dt, requires_grad=True)
    w = torch.ones(cols, device=DEV, dtype=dt, requires_grad=True)
    b = torch.zeros(cols, device=DEV, dtype=dt, requires_grad=True)
    if op == "softmax":
        y, names = ops.softmax(x, -1), ("pa_softmax_fwd", "pa_softmax_bwd")
    elif op == "softmax_cross_entropy":
        labels = torch.empty(shape[:-1], device=DEV, dtype=torch.int64)
        y, names = ops.softmax_cross_entropy(x, labels, IGNORE), ("pa_softmax_ce_fwd", "pa_softmax_ce_bwd")
    elif op == "layer_norm":
        y, names = ops.layer_norm(x, w, b, 1e-5), ("pa_layer_norm_fwd", "pa_layer_norm_bwd")
    elif op == "rms_norm":
        y, names = ops.rms_norm(x, w, 1e-6), ("pa_rms_norm_fwd", "pa_rms_norm_bwd")
    else:
        y, names = ops.gelu(x), ("pa_gelu_fwd", "pa_gelu_bwd")
    assert y.shape == (shape[:-1] if op == "softmax_cross_entropy" else shape)
    y.backward(torch.empty_like(y))
    torch.cuda.synchronize()
    _ran(*names)
    assert x.grad is not None and x.grad.shape == shape and x.grad.dtype == dt
    params = {"layer_norm": (w, b), "rms_norm": (w,)}.get(op, ())
    for p in params:
        assert p.grad is not None and p.grad.dtype == dt and p.grad.shape == (cols,)
        assert (p.grad == 0).all(), "parameter gradient of an input without rows must be zero"
