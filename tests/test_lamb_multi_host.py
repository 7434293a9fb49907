"""Host side of the fused LAMB update (ops/multi_tensor.py item_offsets, optimizer/others.py Lamb) without a device:
the per-tensor item ranges that lamb_trust_k walks agree with the work list, and on the CPU ``Lamb`` still takes the
per-parameter path and computes the documented update."""
import torch

import paddlepaddle_amd as paddle
from paddlepaddle_amd.ops import _loader as L
from paddlepaddle_amd.ops import multi_tensor as MT

CHUNK = MT.CHUNK


def test_offsets_agree_with_items():
    numels = [7, 0, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
    rows = [(0, n, 0) for n in numels]
    _, items, n_items, _ = MT.build_tables(rows, numels, torch.device("cpu"))
    off = MT.item_offsets(numels)
    assert off.dtype == torch.int64 and off.tolist() == [0, 1, 1, 2, 4, 7]
    assert n_items == int(off[-1]) == items.shape[0] and items.shape[1] == 2
    for i, n in enumerate(numels):
        mine = items[int(off[i]):int(off[i + 1])]
        assert mine[:, 0].tolist() == [i] * len(mine), "a tensor's range holds another tensor's item"
        assert mine[:, 1].tolist() == [k * CHUNK for k in range(len(mine))]
        assert len(mine) == -(-n // CHUNK)  # covers [0, n) and nothing more; none for the empty tensor
    assert int(off[1]) == int(off[2])
    assert MT.item_offsets([]).tolist() == [0]


def test_lamb_on_cpu_takes_the_per_parameter_path():
    """Three steps against a float64 loop of
    m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;  r = (m/bc1)/(sqrt(v/bc2)+eps) + wd*p;  p -= lr*mult*trust*r
    with one excluded parameter (trust 1, no decay) and one lr multiplier. fp32 against float64: 1e-5 of max|p| is two
    orders above the rounding of the ~15 fp32 operations per element."""
    lr, wd, b1, b2, eps = 1e-2, 0.1, 0.8, 0.95, 1e-6
    g = torch.Generator().manual_seed(0)
    shapes = {"a": (7,), "b": (33, 17), "nodecay": (65,)}
    ps = [paddle.Parameter(torch.randn(s, generator=g) * sc, name=n,
                           optimize_attr={"learning_rate": 0.5 if n == "b" else 1.0})
          for (n, s), sc in zip(shapes.items(), (0.02, 5.0, 1.0))]
    opt = paddle.optimizer.Lamb(lr, lamb_weight_decay=wd, beta1=b1, beta2=b2, epsilon=eps, parameters=ps,
                                exclude_from_weight_decay_fn=lambda p: p.name == "nodecay")
    ref = {p.name: [p._t.detach().double(), torch.zeros(p._t.shape, dtype=torch.float64),
                    torch.zeros(p._t.shape, dtype=torch.float64)] for p in ps}
    L.reset_calls()
    for t in range(1, 4):
        for p in ps:
            p._t.grad = torch.randn(p._t.shape, generator=g)
        opt.step()
        assert L.calls("pa_lamb_multi") == 0 and not opt._tables
        for p in ps:
            w, m, v = ref[p.name]
            gd = p._t.grad.double()
            m = b1 * m + (1 - b1) * gd
            v = b2 * v + (1 - b2) * gd * gd
            pwd = 0.0 if p.name == "nodecay" else wd
            r = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps) + pwd * w
            trust = float(w.norm() / r.norm()) if pwd else 1.0
            w = w - lr * (0.5 if p.name == "b" else 1.0) * trust * r
            ref[p.name] = [w, m, v]
            err = float((p._t.detach().double() - w).abs().max() / w.abs().max())
            assert err < 1e-5, (p.name, t, err)
            assert opt._param_step[id(p)] == t
            torch.testing.assert_close(opt._accumulators["beta1_pow_acc"][id(p)], torch.tensor([b1 ** t]))
