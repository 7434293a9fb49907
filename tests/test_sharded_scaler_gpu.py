"""GradScaler through group_sharded_parallel on the GPU (degree 1: the gradients are the flat bf16 grad buffers).
Reference: python/paddle/distributed/fleet/meta_parallel/sharding/group_sharded_utils.py (GroupShardedScaler)."""
import numpy as np
import pytest
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.ops import _loader as L

pytestmark = pytest.mark.gpu


class _Net(paddle.nn.Layer):
    def __init__(self, d=256, n=3):
        super().__init__()
        self.blocks = paddle.nn.LayerList([paddle.nn.Linear(d, d) for _ in range(n)])
        self.head = paddle.nn.Linear(d, 1)

    def forward(self, x):
        for b in self.blocks:
            x = paddle.nn.functional.gelu(b(x))
        return self.head(x)


def _build(scale):
    from paddlepaddle_amd.distributed.sharding import group_sharded_parallel
    paddle.seed(7)
    net = _Net()
    for p in net.parameters():
        p._t.data = p._t.data.bfloat16()  # full_grad is bf16
    opt = paddle.optimizer.SGD(0.05, parameters=net.parameters())
    scaler = paddle.amp.GradScaler(init_loss_scaling=scale) if scale else None
    model, opt, scaler = group_sharded_parallel(net, opt, level="os_g", scaler=scaler)
    rng = np.random.RandomState(0)
    x = paddle.Tensor(torch.from_numpy(rng.randn(32, 256).astype("float32")).cuda().bfloat16())
    y = paddle.Tensor(torch.from_numpy(rng.randn(32, 1).astype("float32")).cuda())
    return model, opt, scaler, x, y


def _loss(model, x, y):
    return ((model(x).astype("float32") - y) ** 2).mean()


def _params(model):
    return [p._t.detach().clone() for p in model.parameters()]


def _train(scale, steps=4):
    model, opt, scaler, x, y = _build(scale)
    assert (scaler is None) == (not scale)
    losses = []
    for _ in range(steps):
        loss = _loss(model, x, y)
        if scaler is None:
            loss.backward()
            opt.step()
        else:
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        opt.clear_grad()
        losses.append(float(loss))
    return losses, [p.float().cpu().numpy() for p in _params(model)]


def test_scaled_run_matches_unscaled_run():
    ref_losses, ref_params = _train(0)
    L.reset_calls()
    losses, params = _train(1024)
    assert L.calls("pa_amp_check_unscale_multi") == 4  # one launch per step: the flat grads really were unscaled
    assert ref_losses[-1] != ref_losses[0]  # the steps moved the model
    # a power-of-two scale commutes with every rounding of the backward: same-code parity tolerance
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-5, atol=1e-6)
    for i, (a, b) in enumerate(zip(params, ref_params)):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=f"param {i}")


def test_overflow_skips_the_step_and_halves_the_scale():
    model, opt, scaler, x, y = _build(1024)
    scaler.scale(_loss(model, x, y)).backward()
    scaler.step(opt)
    scaler.update()
    opt.clear_grad()
    scaler.scale(_loss(model, x, y)).backward()
    opt._engine.shard_grads()[0][0] = float("inf")
    before = _params(model)
    scaler.step(opt)
    scaler.update()
    opt.clear_grad()
    for b, a in zip(before, _params(model)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert scaler.get_loss_scaling() == 512
