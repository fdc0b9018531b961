"""Host side of per-query filters (no GPU): RowFilterBatch stacking, deduplication, None -> -1, per-rank slicing at a first row
that is not a multiple of 32, generation staleness, and the validation and deduplication of Embeddings.batchsearch(filters=)."""
import numpy as np
import pytest
import torch

from vietnamese_qa_system_amd.rowfilter import RowFilter, RowFilterBatch
from vietnamese_qa_system_amd.sharded import shard_bounds


def _rf(n, seed, p=0.3):
    return RowFilter.from_mask(np.random.default_rng(seed).random(n) < p)


def test_stacking_dedup_and_none():
    n = 1000
    a, b, c = _rf(n, 1), _rf(n, 2), _rf(n, 3)
    batch = RowFilterBatch([a, None, b, a, c, None, b])
    assert len(batch) == 7 and batch.F == 3 and batch.n == n
    assert batch.bits.dtype == torch.int32 and tuple(batch.bits.shape) == (3, (n + 31) // 32)
    assert batch.query_filter.dtype == torch.int32
    assert batch.query_filter.tolist() == [0, -1, 1, 0, 2, -1, 1]
    for f, row in zip((a, b, c), batch.bits):
        assert torch.equal(row, f.bits)


def test_equal_contents_are_distinct_objects():
    """Deduplication is by identity: two equal filters built separately are stored twice (Embeddings dedupes by value first)."""
    m = np.zeros(100, bool)
    m[:10] = True
    batch = RowFilterBatch([RowFilter.from_mask(m), RowFilter.from_mask(m)])
    assert batch.F == 2 and batch.query_filter.tolist() == [0, 1]


def test_all_none_batch():
    batch = RowFilterBatch([None, None, None])
    assert batch.n is None and batch.F == 1 and batch.query_filter.tolist() == [-1, -1, -1]


def test_bad_entries():
    with pytest.raises(ValueError):
        RowFilterBatch([])
    with pytest.raises(ValueError):
        RowFilterBatch([_rf(100, 1), "rows"])
    with pytest.raises(ValueError):
        RowFilterBatch([_rf(100, 1), _rf(101, 1)])  # two shards


@pytest.mark.parametrize("world", [2, 3])
def test_slice_at_a_rank_boundary(world):
    n = 1000 + world
    fs = [_rf(n, 10 + j) for j in range(3)]
    batch = RowFilterBatch([fs[0], None, fs[2], fs[1], fs[0]])
    got = [[] for _ in fs]
    for r in range(world):
        lo, hi = shard_bounds(n, world, r)
        part = batch.slice(lo, hi)
        assert part.n == hi - lo and part.F == 3
        assert part.query_filter.tolist() == batch.query_filter.tolist()
        for j in range(3):
            got[j].append(RowFilter(part.bits[j].clone(), hi - lo).mask().numpy())
    assert any(shard_bounds(n, world, r)[0] % 32 for r in range(world))
    assert [id(f) for f in batch.filters] == [id(fs[0]), id(fs[2]), id(fs[1])]  # stored in order of first use
    for j, f in enumerate(batch.filters):
        assert np.array_equal(np.concatenate(got[j]), f.mask().numpy())


def test_generation_carried_and_mixed_generations_refused():
    a, b = _rf(500, 1), _rf(500, 2)
    a.generation = 3
    batch = RowFilterBatch([a, b, None])  # b has none: built from a mask, it fits any generation of the shard
    assert batch.generation == 3
    assert batch.slice(7, 300).generation == 3
    b.generation = 4
    with pytest.raises(ValueError):
        RowFilterBatch([a, b])


def _emb(n=4):
    from vietnamese_qa_system_amd.embeddings import Embeddings
    e = Embeddings()
    e.n = n
    e._index = object()  # batchsearch validates filters= before it touches the index
    return e


def test_filters_argument_validation():
    e = _emb()
    q = np.zeros((2, 8), np.float32)
    with pytest.raises(ValueError, match="either"):
        e.batchsearch(q, 3, filter=[1, 2], filters=[[1], None])
    with pytest.raises(ValueError, match="entries"):
        e.batchsearch(q, 3, filters=[[1]])
    with pytest.raises(ValueError, match="entries"):
        e.batchsearch(["a", "b", "c"], 3, filters=[None, None])
    with pytest.raises(ValueError, match="list"):
        e.batchsearch(q, 3, filters={"source": "x"})


def test_filter_keys_resolve_equal_entries_once():
    from vietnamese_qa_system_amd.embeddings import Embeddings
    key = Embeddings._filter_key
    assert key({"source": ["x", "y"], "lang": "vi"}) == key({"lang": ["vi"], "source": ("y", "x")})
    assert key({"source": "x"}) != key({"source": "y"})
    assert key([1, 2, 3]) == key(np.array([1, 2, 3])) == key((1, 2, 3))
    assert key([1, 2, 3]) != key([1, 2])
    assert key(["a", "b"]) == key(["a", "b"])
    rf = _rf(10, 1)
    assert key(rf) == key(rf) and key(rf) != key(_rf(10, 1))
