"""Host side of the multi-tensor launches (ops/multi_tensor.py): the work-item builder against the nested loop it
replaces, and the key of the table cache. CPU only."""
import torch

from paddlepaddle_amd.ops import multi_tensor as MT

CPU = torch.device("cpu")
CHUNK = 16384
NUMELS = (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)


def _update_keys(numels=NUMELS, state=0x3000, dtypes=0 | (3 << 8)):
    """The 7 key columns of update rows with made-up addresses (nothing dereferences them on the CPU)."""
    return [(0x1000 + 64 * i, 0x2000 + 64 * i, state + 64 * i, 0x4000 + 64 * i, 0, n, dtypes)
            for i, n in enumerate(numels)]


def _scalars(wd=0.1):
    return [(MT.f32_bits(wd), MT.f32_bits(1.0))] * len(NUMELS)


def test_items_match_the_nested_loop():
    assert MT.CHUNK == CHUNK
    rows = [list(k + s) for k, s in zip(_update_keys(), _scalars())]
    table, items, n_items, hosts = MT.build_tables(rows, list(NUMELS), CPU)
    naive = [[i, s] for i, n in enumerate(NUMELS) for s in range(0, n, CHUNK)]
    assert len(naive) == 0 + 1 + 1 + 1 + 2 + 3
    assert n_items == len(naive)
    assert table.dtype == torch.int64 and tuple(table.shape) == (len(NUMELS), 9) and table.tolist() == rows
    assert items.dtype == torch.int64 and tuple(items.shape) == (n_items, 2) and items.tolist() == naive
    assert 0 not in items[:, 0].tolist()  # the empty tensor has a row and no item
    assert len(hosts) == 2

    t3 = [[0x1000 * (i + 1), n, 2] for i, n in enumerate(NUMELS)]
    table, items, n_items, _ = MT.build_tables(t3, list(NUMELS), CPU)
    assert table.dtype == torch.int64 and tuple(table.shape) == (len(NUMELS), 3)
    assert tuple(items.shape) == (n_items, 2) and items.tolist() == naive

    table, items, n_items, _ = MT.build_tables([[0x1000, 0, 0]], [0], CPU)  # nothing to do
    assert n_items == 0 and items.dtype == torch.int64 and tuple(items.shape) == (0, 2)


def test_cache_key_is_pointers_numel_and_dtype():
    cache = {}

    def get(keys, wd=0.1):
        return MT.cached_tables(cache, "group", keys, CPU, scalars=lambda: _scalars(wd))

    first = get(_update_keys())
    assert tuple(first.table.shape) == (len(NUMELS), 9)
    assert first.table[0].tolist() == list(_update_keys()[0] + _scalars()[0])
    assert get(_update_keys()) is first, "same rows: hit"
    shorter = get(_update_keys(numels=NUMELS[:-1] + (CHUNK,)))
    assert shorter is not first and shorter.n_items == first.n_items - 2, "same pointers, another numel: miss"
    first = get(_update_keys())
    assert get(_update_keys(dtypes=2 | (3 << 8))) is not first, "same pointers, another dtype word: miss"
    first = get(_update_keys())
    moved = get(_update_keys(state=0x5000))
    assert moved is not first and moved.table[:, 2].tolist() != first.table[:, 2].tolist(), "a new state pointer: miss"
    assert len(cache) == 1  # one entry per slot

    # scalar columns are not part of the key (a weight decay edited later keeps the old table)
    first = get(_update_keys())
    assert get(_update_keys(), wd=0.5) is first


def test_module_level_cache_clears_at_65th_key():
    cache = {}

    def get(k):
        return MT.cached_tables(cache, None, [(0x1000 + 16 * k, 5, 0)], CPU, extra=lambda: k)

    for k in range(64):
        get(k)
    assert len(cache) == 64
    e0 = get(0)
    assert len(cache) == 64 and e0.extra == 0 and get(0) is e0  # a hit adds nothing
    assert get(64).extra == 64
    assert len(cache) == 1  # the 65th distinct key cleared the other 64
