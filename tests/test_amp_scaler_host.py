"""GradScaler host logic (no device needed): the fallback of ops.amp, one host read of found_inf per step, the
found_inf group set, and the reference module path of GroupShardedScaler."""
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.amp.grad_scaler import add_found_inf_groups
from paddlepaddle_amd.ops.amp import check_finite_and_unscale_


def test_cpu_fallback_unscales_mixed_dtypes_and_accumulates():
    g = torch.Generator().manual_seed(0)
    xs = [torch.randn(1000, generator=g) * 1024, (torch.randn(77, generator=g) * 1024).bfloat16(),
          torch.empty(0)]
    refs = [(x.float() * (1.0 / 1024)).to(x.dtype) for x in xs]
    inv, found = torch.full((1,), 1.0 / 1024), torch.zeros(1)
    check_finite_and_unscale_(xs, inv, found)
    for x, r in zip(xs, refs):
        assert torch.equal(x, r)
    assert float(found) == 0.0
    xs[1][5] = float("nan")
    check_finite_and_unscale_(xs, inv, found)
    assert float(found) == 1.0
    check_finite_and_unscale_(xs[:1], inv, found)  # a clean call leaves the flag set
    assert float(found) == 1.0
    check_finite_and_unscale_([], inv, found)


class _CountingFlag:
    """Stands in for the device flag: counts the host reads."""

    def __init__(self, value):
        self.value, self.reads = value, 0

    def item(self):
        self.reads += 1
        return self.value


def test_found_inf_is_read_on_the_host_once_per_step():
    lin = paddle.nn.Linear(3, 2)
    opt = paddle.optimizer.SGD(0.1, parameters=lin.parameters())
    scaler = paddle.amp.GradScaler(init_loss_scaling=1024)
    for value, want in ((0.0, 1024), (1.0, 512)):
        flag = _CountingFlag(value)

        def unscale_(optimizer, _flag=flag):  # a patched unscale_ (MixPrecisionScaler, shard_scaler) only sets the flag
            scaler._found_inf = _flag
        scaler.unscale_ = unscale_
        lin(paddle.to_tensor(torch.ones(1, 3))).sum().backward()
        before = lin.weight._t.detach().clone()
        scaler.step(opt)
        scaler.update()
        opt.clear_grad()
        assert flag.reads == 1
        assert scaler.get_loss_scaling() == want
        assert torch.equal(lin.weight._t.detach(), before) == bool(value)
    # update() without step(): one lazy read
    flag = _CountingFlag(1.0)
    scaler._found_inf = flag
    scaler.update()
    assert flag.reads == 1 and scaler.get_loss_scaling() == 256


class _G:
    def __init__(self, ranks):
        self.ranks, self.nranks, self.process_group = list(ranks), len(ranks), object()


def test_found_inf_groups_unite_and_skip_single_rank_groups():
    scaler = paddle.amp.GradScaler()
    assert scaler._found_inf_groups == ()
    a, b = _G([0, 1]), _G([0, 2])
    add_found_inf_groups(scaler, [a, _G([0]), b])
    add_found_inf_groups(scaler, [_G([0, 1]), _G([0, 4])])  # (0, 1) is already there
    assert [r for r, _ in scaler._found_inf_groups] == [(0, 1), (0, 2), (0, 4)]
    assert scaler._found_inf_groups[0][1] is a.process_group
    assert paddle.amp.GradScaler()._found_inf_groups == ()  # per object, not shared


def test_group_sharded_scaler_reference_path_and_degree_one():
    from paddlepaddle_amd.distributed.fleet.meta_parallel.sharding.group_sharded_utils import GroupShardedScaler
    from paddlepaddle_amd.distributed.sharding import group_sharded_parallel
    from paddlepaddle_amd.parallel import sharding
    assert GroupShardedScaler is sharding.GroupShardedScaler
    net = paddle.nn.Linear(4, 4)
    opt = paddle.optimizer.SGD(0.1, parameters=net.parameters())
    scaler = paddle.amp.GradScaler(init_loss_scaling=1024)
    model, opt, got = group_sharded_parallel(net, opt, level="os_g", scaler=scaler)
    assert got is scaler and scaler._found_inf_groups == ()  # one rank: nothing to reduce over
    x = paddle.to_tensor(torch.ones(2, 4))
    scaler.scale(model(x).sum()).backward()
    grads = opt._amp_grads()
    assert [g.data_ptr() for g in grads] == [g.data_ptr() for g in opt._engine.shard_grads()] and grads
    scaled = [g.clone() for g in grads]
    assert any(float(g.abs().max()) > 0 for g in scaled)
    scaler.step(opt)
    scaler.update()
    for g, s in zip(grads, scaled):  # unscaled in place, exactly (power of two)
        assert torch.equal(g, s / 1024)
