"""Loss scaling under sharding / tensor parallel / pipeline parallel (gloo, world_size=2, CPU).

A power-of-two loss scale commutes with every rounding of a linear backward, so a run through a GradScaler must
reproduce the same run without one; an overflow seen by one rank must skip the step on every rank (a rank that
stepped alone would issue all-gathers nobody joins) and halve the scale everywhere.
Reference: fleet/meta_parallel/sharding/group_sharded_utils.py GroupShardedScaler, fleet/scaler.py distributed_scaler.
"""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


# ----------------------------------------------------------------------------- spawn helper (test_distributed_cpu.py)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _setup(rank, world, port):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), PADDLE_AMD_FORCE_CPU="1")
    import paddlepaddle_amd as paddle
    paddle.distributed.init_parallel_env(backend="gloo")
    return paddle


def _spawn(fn, *args, world=2):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=fn, args=(r, world, port, *args, q)) for r in range(world)]
    for p in procs:
        p.start()
    import queue
    import time
    res = []
    try:
        deadline = time.time() + 240
        while len(res) < world:
            try:
                res.append(q.get(timeout=1))
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                if dead or time.time() > deadline:
                    raise RuntimeError(f"worker failed (exit codes {dead})" if dead else "workers timed out")
    finally:
        for p in procs:
            p.join(timeout=10)
            if p.is_alive():
                p.kill()
    for p in procs:
        p.join(timeout=60)
    return sorted(res, key=lambda x: x[0])


def _make_model(paddle):
    from paddlepaddle_amd.models.gpt import GPTConfig, GPTForPretraining, GPTPretrainingCriterion
    paddle.seed(11)
    cfg = GPTConfig.tiny(num_hidden_layers=3, hidden_dropout_prob=0.0)
    return cfg, GPTForPretraining(cfg), GPTPretrainingCriterion(cfg)


def _data(cfg):
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, cfg.vocab_size, (4, 17), generator=g)


def _step(scaler, opt, loss, poke=None):
    """backward (+ ``poke()`` on the finished gradients) + optimizer step, through ``scaler`` when there is one"""
    if scaler is None:
        loss.backward()
        opt.step()
    else:
        scaler.scale(loss).backward()
        if poke is not None:
            poke()
        scaler.step(opt)
        scaler.update()
    opt.clear_grad()


# ----------------------------------------------------------------------------- sharding: parity
def _sharded_parity_worker(rank, world, port, level, q):
    paddle = _setup(rank, world, port)
    from paddlepaddle_amd.distributed.sharding import group_sharded_parallel
    out = []
    for scale in (None, 1024):
        cfg, model, crit = _make_model(paddle)
        ids = paddle.Tensor(_data(cfg)[rank * 2:(rank + 1) * 2])
        opt = paddle.optimizer.SGD(0.1, parameters=model.parameters())
        scaler = paddle.amp.GradScaler(init_loss_scaling=scale) if scale else None
        model, opt, got = group_sharded_parallel(model, opt, level=level, scaler=scaler)
        assert got is scaler  # the user's own object, patched in place (None stays None)
        losses = []
        for _ in range(3):
            loss = crit(model(ids[:, :-1]), ids[:, 1:])
            _step(scaler, opt, loss)
            losses.append(float(loss))
        out.append((losses, {k: v.numpy() for k, v in model.state_dict().items()}))
        if scaler is not None:
            assert scaler.get_loss_scaling() == 1024
    q.put((rank, out[0], out[1]))
    paddle.distributed.barrier()


@pytest.mark.parametrize("level", ["os", "os_g", "p_g_os"])
def test_sharded_scaler_matches_unscaled_run(level):
    res = _spawn(_sharded_parity_worker, level)
    for rank, (ref_losses, ref_sd), (losses, sd) in res:
        np.testing.assert_allclose(losses, ref_losses, rtol=1e-5, atol=1e-6, err_msg=f"{level} rank {rank}")
        assert ref_losses[-1] < ref_losses[0]
        for k in ref_sd:
            np.testing.assert_allclose(sd[k], ref_sd[k], rtol=1e-5, atol=1e-6, err_msg=f"{level} rank {rank}: {k}")
    for k in res[0][2][1]:
        np.testing.assert_allclose(res[1][2][1][k], res[0][2][1][k], rtol=0, atol=0, err_msg=f"{k} replicas differ")


# ----------------------------------------------------------------------------- sharding: overflow on one rank
def _sharded_overflow_worker(rank, world, port, level, q):
    paddle = _setup(rank, world, port)
    from paddlepaddle_amd.distributed.collective_check import check_collectives, enable_collective_check
    from paddlepaddle_amd.distributed.sharding import group_sharded_parallel
    enable_collective_check()
    cfg, model, crit = _make_model(paddle)
    ids = paddle.Tensor(_data(cfg)[rank * 2:(rank + 1) * 2])
    opt = paddle.optimizer.AdamW(1e-2, parameters=model.parameters(), grad_clip=paddle.nn.ClipGradByGlobalNorm(0.5))
    model, opt, scaler = group_sharded_parallel(model, opt, level=level,
                                                scaler=paddle.amp.GradScaler(init_loss_scaling=1024))
    eng = opt._engine

    def state():
        shards = [f.shard for u in eng.units for f in u.flats]
        m1 = opt._inner._accumulators.get("moment1", {})  # created by the first step
        return [s._t.detach().clone() for s in shards] + [m1[id(s)].clone() for s in shards if id(s) in m1]

    def poke():
        if rank == 0:
            eng.shard_grads()[1][0] = INF

    same, scales = None, []
    for step in (1, 2, 3):
        before = state()
        loss = crit(model(ids[:, :-1]), ids[:, 1:])
        _step(scaler, opt, loss, poke if step == 2 else None)
        after = state()
        unchanged = len(after) == len(before) and all(torch.equal(a, b) for a, b in zip(after, before))
        if step == 2:
            assert len(after) == 2 * len(eng.shard_grads())  # every shard and its moment1 were compared
            same = unchanged
        else:
            assert not unchanged, f"step {step} did not run"
        if step >= 2:
            check_collectives(f"after step {step}")  # no rank issued a collective its peer did not
        scales.append(scaler.get_loss_scaling())
    finite = all(bool(torch.isfinite(t).all()) for t in state())
    sd = {k: v.numpy() for k, v in model.state_dict().items()}
    q.put((rank, same, scales, finite, sd))
    paddle.distributed.barrier()


@pytest.mark.parametrize("level", ["os_g", "p_g_os"])
def test_sharded_overflow_on_one_rank_skips_everywhere(level):
    res = _spawn(_sharded_overflow_worker, level)
    for rank, same, scales, finite, _ in res:
        assert same, f"rank {rank}: parameters / moment1 changed in the overflow step"
        assert scales == [1024, 512, 512], f"rank {rank}: {scales}"
        assert finite, f"rank {rank}: non-finite state"
    for k in res[0][4]:
        np.testing.assert_allclose(res[1][4][k], res[0][4][k], rtol=0, atol=0, err_msg=f"{k} replicas differ")


# ----------------------------------------------------------------------------- fleet: tensor parallel
def _fleet_init(paddle, **hc):
    from paddlepaddle_amd.distributed import fleet
    s = fleet.DistributedStrategy()
    cfg = dict(dp_degree=1, mp_degree=1, pp_degree=1)
    cfg.update(hc)
    s.hybrid_configs = cfg
    s.pipeline_configs = {"accumulate_steps": 2, "micro_batch_size": 2, "schedule_mode": "1F1B"}
    fleet.init(is_collective=True, strategy=s)
    return fleet


def _tp_worker(rank, world, port, q):
    paddle = _setup(rank, world, port)
    from paddlepaddle_amd.models.gpt import GPTConfig, GPTForPretraining, GPTPretrainingCriterion
    fleet = _fleet_init(paddle, mp_degree=2)
    paddle.seed(11)
    cfg = GPTConfig.tiny(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                         tensor_parallel_degree=2)
    model, crit = GPTForPretraining(cfg), GPTPretrainingCriterion(cfg)
    params = list(model.parameters())
    opt = paddle.optimizer.AdamW(1e-2, parameters=params)
    model = fleet.distributed_model(model)
    opt = fleet.distributed_optimizer(opt)
    scaler = fleet.distributed_scaler(paddle.amp.GradScaler(init_loss_scaling=1024))
    assert [ranks for ranks, _ in scaler._found_inf_groups] == [(0, 1)]
    ids = paddle.Tensor(_data(cfg))

    def poke():
        if rank == 0:
            g = next(p._t.grad for p in params if p._t.grad is not None)
            g.view(-1)[0] = INF

    flags, scales = [], []
    for step in (1, 2):
        before = [p._t.detach().clone() for p in params]
        _step(scaler, opt, crit(model(ids[:, :-1]), ids[:, 1:]), poke if step == 2 else None)
        flags.append(all(torch.equal(p._t.detach(), b) for p, b in zip(params, before)))
        scales.append(scaler.get_loss_scaling())
    q.put((rank, flags, scales))
    paddle.distributed.barrier()


def test_tensor_parallel_overflow_on_one_rank_skips_both():
    for rank, unchanged, scales in _spawn(_tp_worker):
        assert unchanged == [False, True], f"rank {rank}: {unchanged}"
        assert scales == [1024, 512], f"rank {rank}: {scales}"


# ----------------------------------------------------------------------------- fleet: pipeline parallel
def _mlp_descs(paddle):
    from paddlepaddle_amd.parallel.pipeline import LayerDesc
    nn = paddle.nn
    return [LayerDesc(nn.Linear, 16, 32), LayerDesc(nn.Tanh), LayerDesc(nn.Linear, 32, 32), LayerDesc(nn.GELU),
            LayerDesc(nn.Linear, 32, 32), LayerDesc(nn.Tanh), LayerDesc(nn.Linear, 32, 8)]


def _mse(out, label):
    return ((out - label) ** 2).mean()


def _pp_worker(rank, world, port, q):
    paddle = _setup(rank, world, port)
    from paddlepaddle_amd.parallel.pipeline import PipelineLayer
    fleet = _fleet_init(paddle, pp_degree=2)
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(8, 16, generator=g), torch.randn(8, 8, generator=g)
    runs = []
    for scale in (None, 1024):
        paddle.seed(7)
        pl = PipelineLayer(_mlp_descs(paddle), num_stages=2, loss_fn=_mse)
        opt = paddle.optimizer.SGD(0.1, parameters=pl.parameters())
        model = fleet.distributed_model(pl)
        opt = fleet.distributed_optimizer(opt)
        scaler = paddle.amp.GradScaler(init_loss_scaling=scale) if scale else None
        losses = [float(model.train_batch([paddle.Tensor(x), paddle.Tensor(y)], opt, scaler=scaler))
                  for _ in range(3)]
        runs.append((losses, [p._t.detach().clone().numpy() for p in pl.parameters()]))
    # overflow on stage 0 only: its first parameter's gradient starts the batch at inf (backward accumulates into it)
    params = list(pl.parameters())
    if rank == 0:
        params[0]._t.grad = torch.full_like(params[0]._t, INF)
    before = [p._t.detach().clone() for p in params]
    loss = float(model.train_batch([paddle.Tensor(x), paddle.Tensor(y)], opt, scaler=scaler))
    unchanged = all(torch.equal(p._t.detach(), b) for p, b in zip(params, before))
    q.put((rank, runs[0], runs[1], unchanged, scaler.get_loss_scaling(), loss))
    paddle.distributed.barrier()


def test_pipeline_train_batch_with_scaler():
    for rank, (ref_losses, ref_params), (losses, params), unchanged, scale, loss in _spawn(_pp_worker):
        np.testing.assert_allclose(losses, ref_losses, rtol=1e-5, atol=1e-6, err_msg=f"stage {rank}")
        assert ref_losses[-1] < ref_losses[0]
        for i, (a, b) in enumerate(zip(params, ref_params)):
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=f"stage {rank} param {i}")
        assert unchanged, f"stage {rank} stepped in the overflow batch"
        assert scale == 512, f"stage {rank}: {scale}"
        assert np.isfinite(loss) and loss < ref_losses[0]  # the returned loss is the unscaled one
