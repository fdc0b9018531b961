"""Host side of filtered search (no GPU): the bitmap layout and RowFilter construction, id -> row mapping of Embeddings filters for
the three kinds of ids, per-rank slicing at an odd first row, and the keyword half's row mask."""
import numpy as np
import pytest
import torch

from vietnamese_qa_system_amd.rowfilter import RowFilter, bits_to_mask, mask_to_bits
from vietnamese_qa_system_amd.sharded import shard_bounds
from vietnamese_qa_system_amd.sparse import BM25Index


def _ref_words(mask):
    n = mask.size
    w = np.zeros((n + 31) // 32, dtype=np.uint32)
    for p in np.flatnonzero(mask):
        w[p >> 5] |= np.uint32(1) << np.uint32(p & 31)
    return w.view(np.int32)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 255, 256, 257, 1000, 4097])
def test_bitmap_layout(n):
    rng = np.random.default_rng(n)
    mask = rng.random(n) < 0.3
    mask[n - 1] = True  # the bit of the last row, inside a partial last word
    bits = mask_to_bits(torch.from_numpy(mask))
    assert bits.dtype == torch.int32 and bits.numel() == (n + 31) // 32
    assert np.array_equal(bits.numpy(), _ref_words(mask))
    assert np.array_equal(bits_to_mask(bits, n).numpy(), mask)


def test_row_filter_from_positions_and_masks():
    n = 1000
    pos = np.array([999, 0, 256, 256, 511, 512])
    a = RowFilter.from_positions(n, pos)
    m = np.zeros(n, bool)
    m[pos] = True
    assert a.allowed == 5 and a.tiles == 4  # rows 0, 256, 511, 512, 999 lie in tiles 0, 1, 1, 2, 3
    assert np.array_equal(a.mask().numpy(), m)
    for src in (m, m.astype(np.uint8), torch.from_numpy(m), torch.from_numpy(m.astype(np.uint8))):
        b = RowFilter.from_mask(src)
        assert torch.equal(b.bits, a.bits) and b.allowed == a.allowed
    assert RowFilter.from_positions(n, []).allowed == 0 and RowFilter.from_positions(n, []).tiles == 0
    with pytest.raises(ValueError):
        RowFilter.from_positions(n, [n])
    with pytest.raises(ValueError):
        RowFilter.from_positions(n, [-1])
    with pytest.raises(ValueError):
        RowFilter.from_mask(np.zeros(n, np.float32))


def test_tiles_counted():
    n = 70001
    m = np.zeros(n, bool)
    m[255:257] = True      # straddles tiles 0 / 1
    m[n - 1] = True        # the ragged last tile
    rf = RowFilter.from_mask(m)
    assert rf.tiles == 3 and rf.allowed == 3


@pytest.mark.parametrize("world", [2, 3, 5])
def test_per_rank_slices_at_odd_first_rows(world):
    n = 1000 + world  # shard_bounds gives rows that start at odd positions
    rng = np.random.default_rng(world)
    m = rng.random(n) < 0.4
    rf = RowFilter.from_mask(m)
    got = []
    for r in range(world):
        lo, hi = shard_bounds(n, world, r)
        part = rf.slice(lo, hi)
        assert part.n == hi - lo
        assert np.array_equal(part.bits.numpy(), _ref_words(m[lo:hi]))
        got.append(part.mask().numpy())
    assert np.array_equal(np.concatenate(got), m)
    with pytest.raises(ValueError):
        rf.slice(5, n + 1)


def _host_embeddings(ids, n):
    """An Embeddings object in the state index_vectors leaves for `ids` (no device index: the id mapping is host logic)."""
    from vietnamese_qa_system_amd.embeddings import Embeddings

    class Shard:  # what the mapping reads of a DeviceIndex
        def __init__(self, n, id_base, has_ids):
            self.n, self.id_base, self.has_ids = n, id_base, has_ids

    e = Embeddings()
    e.n = n
    if ids is None:
        e._index = Shard(n, 1, False)  # contiguous ids from 1 (sqlite rowids): no id vector
    elif all(isinstance(i, int) for i in ids):
        e._index = Shard(n, 0, True)
        e._shard_ids = np.asarray(ids, dtype=np.int64)
    else:
        e._host_ids = list(ids)
        e._index = Shard(n, 0, False)
    return e


def test_id_mapping_contiguous():
    e = _host_embeddings(None, 10)
    m = e._shard_mask(e._device_ids_of([1, 5, 10, 11, 0, -3]))
    assert np.array_equal(np.flatnonzero(m), [0, 4, 9])


def test_id_mapping_id_vector():
    ids = [100, 7, 55, 3, 900]
    e = _host_embeddings(ids, 5)
    m = e._shard_mask(e._device_ids_of([3, 900, 12345, 100]))
    assert np.array_equal(np.flatnonzero(m), [0, 3, 4])


def test_id_mapping_string_ids():
    ids = ["a", "b", "c", "d"]
    e = _host_embeddings(ids, 4)
    m = e._shard_mask(e._device_ids_of(["d", "zz", "b"]))
    assert np.array_equal(np.flatnonzero(m), [1, 3])


def test_field_filter_in_memory():
    e = _host_embeddings(None, 4)
    e._docs_rows = [(1, {"text": "a", "source": "x"}), (2, {"text": "b", "source": "y"}), (3, {"text": "c", "source": "x"}),
                    (4, {"text": "d", "source": "z"})]
    assert np.array_equal(np.flatnonzero(e._shard_mask(e._device_ids_of({"source": "x"}))), [0, 2])
    assert np.array_equal(np.flatnonzero(e._shard_mask(e._device_ids_of({"source": ["y", "z"]}))), [1, 3])
    with pytest.raises(ValueError):
        e._device_ids_of({"author": "x"})


def test_bm25_allow_mask():
    texts = ["alpha beta", "alpha gamma", "beta beta", "delta", "alpha alpha alpha"]
    bm = BM25Index().index(texts)
    plain = bm.search("alpha beta", 10)
    assert plain == bm.search("alpha beta", 10, allow=None)
    allow = np.array([False, True, True, True, False])
    got = bm.search("alpha beta", 10, allow=allow)
    rows = [r for r, _ in got]
    assert rows and all(allow[r] for r in rows)
    assert set(rows) == {r for r, _ in plain if allow[r]}
    assert bm.search("alpha beta", 10, allow=np.zeros(5, bool)) == []
    with pytest.raises(ValueError):
        bm.search("alpha", 3, allow=np.ones(4, bool))
