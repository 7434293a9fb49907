"""Fused non-finite check + unscale of gradients (csrc/kernels/amp.hip, ops/amp.py) against torch on the device.

The reference is ``(x.float() * inv).to(x.dtype)``: one correctly rounded fp32 multiply and one round-to-nearest-even
convert on both sides, so the written values are expected bitwise equal (NaNs compared by position). Inputs are
``randn * 1024`` and ``inv = 1 / 1024``.
"""
import pytest
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.ops import _loader as L
from paddlepaddle_amd.ops.amp import check_finite_and_unscale_

pytestmark = pytest.mark.gpu

NAME = "pa_amp_check_unscale_multi"
CHUNK = 16384
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def _rand(n, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(n, device="cuda", generator=g) * 1024).to(dtype)


def _ref(x, inv):
    return (x.float() * inv).to(x.dtype)


def _assert_bitwise(got, ref, msg=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, msg
    nan = ref.isnan()
    assert torch.equal(got.isnan(), nan), f"{msg}: NaN positions differ"
    keep = ~nan
    assert torch.equal(got[keep].view(_INT[got.dtype]), ref[keep].view(_INT[ref.dtype])), f"{msg}: values differ"


def _run(tensors, inv_value=1.0 / 1024, found_init=0.0):
    inv = torch.full((1,), inv_value, dtype=torch.float32, device="cuda")
    found = torch.full((1,), found_init, dtype=torch.float32, device="cuda")
    refs = [_ref(t, inv) for t in tensors]
    L.reset_calls()
    check_finite_and_unscale_(tensors, inv, found)
    assert L.calls(NAME) > 0
    return refs, float(found.item())


def test_mixed_dtypes_and_shapes_one_launch():
    odd = _rand(CHUNK + 1, torch.float32, 6)
    tensors = [_rand(100000, torch.float32, 0), _rand(333, torch.bfloat16, 1), _rand(70000, torch.float16, 2),
               _rand(7, torch.bfloat16, 3), _rand(CHUNK, torch.float32, 4), _rand(2 * CHUNK + 3, torch.bfloat16, 5),
               odd[1:],  # contiguous, 4-byte aligned: the scalar path
               torch.empty(0, dtype=torch.float32, device="cuda")]
    assert tensors[6].is_contiguous() and tensors[6].data_ptr() % 16 == 4
    refs, found = _run(tensors)
    assert L.calls(NAME) == 1  # one launch for all dtypes
    for i, (t, r) in enumerate(zip(tensors, refs)):
        _assert_bitwise(t, r, f"tensor {i}")
    assert found == 0.0
    assert torch.equal(odd[:1], _rand(CHUNK + 1, torch.float32, 6)[:1])  # the element in front of the view: untouched


def test_workgroup_walks_two_items():
    n = 1024 * CHUNK + CHUNK + 5  # 1026 items on a 1024-workgroup grid
    x = _rand(n, torch.bfloat16, 7)
    refs, found = _run([x])
    _assert_bitwise(x, refs[0])
    assert found == 0.0
    y = _rand(n, torch.bfloat16, 7)
    y[-1] = float("inf")
    refs, found = _run([y])
    _assert_bitwise(y, refs[0])
    assert found == 1.0


_SIZES = (CHUNK + 2048 + 3, 333, 4099)  # two items with a vector body and a scalar tail; one small; one odd


@pytest.mark.parametrize("where", ["first", "body", "tail_last", "last_tensor"])
@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")], ids=["inf", "ninf", "nan"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_non_finite_placement(dtype, value, where):
    tensors = [_rand(n, dtype, 10 + i) for i, n in enumerate(_SIZES)]
    ti, idx = {"first": (0, 0), "body": (0, 5000), "tail_last": (0, _SIZES[0] - 1), "last_tensor": (2, 1234)}[where]
    tensors[ti][idx] = value
    refs, found = _run(tensors)
    assert found == 1.0
    for i, (t, r) in enumerate(zip(tensors, refs)):
        _assert_bitwise(t, r, f"tensor {i}")
    got = tensors[ti][idx].float()
    assert bool(got.isnan()) if value != value else float(got) == value


def test_found_inf_accumulates_and_inv_scale_is_read_on_device():
    x = _rand(3 * CHUNK + 9, torch.bfloat16, 20)
    _, found = _run([x], found_init=1.0)  # clean call: a set flag stays set
    assert found == 1.0
    # same buffer, same cached table: only the device value of inv_scale changes between the two calls
    x = _rand(40000, torch.float32, 21)
    x0 = x.clone()
    inv = torch.full((1,), 0.5, dtype=torch.float32, device="cuda")
    found = torch.zeros(1, dtype=torch.float32, device="cuda")
    L.reset_calls()
    check_finite_and_unscale_([x], inv, found)
    _assert_bitwise(x, _ref(x0, inv))
    inv.fill_(0.125)
    check_finite_and_unscale_([x], inv, found)
    _assert_bitwise(x, _ref(_ref(x0, torch.tensor(0.5, device="cuda")), inv))
    assert L.calls(NAME) == 2 and float(found.item()) == 0.0


def test_grad_scaler_round_trip():
    paddle.seed(3)
    lin = paddle.nn.Linear(96, 64)
    lin.weight._t.data = lin.weight._t.data.bfloat16()  # bf16 weight, fp32 bias
    params = list(lin.parameters())
    opt = paddle.optimizer.AdamW(1e-2, parameters=params)
    scaler = paddle.amp.GradScaler(init_loss_scaling=1024)
    for i, p in enumerate(params):
        p._t.grad = _rand(p._t.numel(), p._t.dtype, 30 + i).view(p._t.shape)
    # torch's foreach kernel has no bf16 instantiation on the GPU ("not implemented for 'BFloat16'"): it runs on the
    # exact fp32 upcast, and its result is rounded to the gradient's dtype (round to nearest even)
    exp32 = [p._t.grad.float() for p in params]
    found = torch.zeros(1, device="cuda")
    inv = torch.full((1,), 1.0 / 1024, device="cuda")
    torch._amp_foreach_non_finite_check_and_unscale_(exp32, found, inv)
    exp = [e.to(p._t.dtype) for e, p in zip(exp32, params)]
    assert float(found.item()) == 0.0
    L.reset_calls()
    scaler.unscale_(opt)
    assert L.calls(NAME) > 0
    for i, (p, e) in enumerate(zip(params, exp)):
        _assert_bitwise(p._t.grad, e, f"param {i}")
    scaler.update()
    assert scaler.get_loss_scaling() == 1024
    # a NaN gradient: the step is skipped and the scale halves
    for i, p in enumerate(params):
        p._t.grad = _rand(p._t.numel(), p._t.dtype, 40 + i).view(p._t.shape)
    params[0]._t.grad.view(-1)[17] = float("nan")
    before = [p._t.detach().clone() for p in params]
    scaler.step(opt)
    scaler.update()
    assert scaler.get_loss_scaling() == 512
    for p, b in zip(params, before):
        assert torch.equal(p._t.detach().view(_INT[b.dtype]), b.view(_INT[b.dtype]))
