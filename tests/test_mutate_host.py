"""Host side of in-place index updates, no GPU: the compaction rule against a brute-force model, argument errors of the two C entry
points, the BM25 half following moved rows, and sharded Embeddings refusing updates."""
import ctypes

import numpy as np
import pytest


def _brute(n, positions):
    """The removal rule stated naively: holes below n' in ascending order take the survivors at >= n' in ascending order."""
    removed = set(int(p) for p in positions)
    n1 = n - len(removed)
    holes = sorted(p for p in removed if p < n1)
    survivors = [p for p in range(n1, n) if p not in removed]
    rows = list(range(n))
    for h, s in zip(holes, survivors):
        rows[h] = s
    return survivors, holes, rows[:n1]


def test_compaction_moves_matches_a_brute_force_model():
    from vietnamese_qa_system_amd.index import compaction_moves
    rng = np.random.default_rng(0)
    cases = [(1, [0]), (5, []), (5, [4]), (5, [0, 1, 2, 3, 4]), (10, [9, 0]), (300, list(range(100, 200)))]
    for _ in range(300):
        n = int(rng.integers(1, 600))
        c = int(rng.integers(0, n + 1))
        cases.append((n, rng.choice(n, c, replace=False).tolist()))
    for n, pos in cases:
        src, dst = compaction_moves(n, np.asarray(pos, dtype=np.int64))
        bs, bd, rows = _brute(n, pos)
        assert src.tolist() == bs and dst.tolist() == bd
        mirror = np.arange(n)
        mirror[dst] = mirror[src]
        assert mirror[:n - len(pos)].tolist() == rows
        assert not set(rows) & set(pos)


def test_compaction_moves_rejects_bad_positions():
    from vietnamese_qa_system_amd.index import compaction_moves
    for bad in ([5], [-1], [1, 1]):
        with pytest.raises(ValueError):
            compaction_moves(5, bad)


def test_entry_points_reject_null_handles_and_bad_arguments(native_lib):
    from vietnamese_qa_system_amd import _native as N
    lib = N.load()
    pos = np.arange(3, dtype=np.int64)
    rows = np.zeros((3, 8), np.float16)
    assert lib.vqa_index_capacity(None) == -1
    assert lib.vqa_index_remove_rows(None, pos.ctypes.data, 3) == -1
    assert b"null" in lib.vqa_last_error()
    assert lib.vqa_index_append_rows(None, 3, rows.ctypes.data, N.VQA_F16, None) == -1
    assert b"null" in lib.vqa_last_error()
    o = N.index_options(0, capacity=7)
    assert o.capacity == 7 and ctypes.sizeof(o) == o.struct_size
    assert N.index_options().capacity == 0


def test_bm25_update_equals_a_fresh_index():
    from vietnamese_qa_system_amd.sparse import BM25Index
    rng = np.random.default_rng(1)
    vocab = [f"w{i}" for i in range(40)]
    texts = [" ".join(rng.choice(vocab, int(rng.integers(1, 12)))) for _ in range(300)]
    ix = BM25Index().index(texts)
    # delete 30 rows by compaction, overwrite 10, append 5 (one with a word no row had)
    from vietnamese_qa_system_amd.index import compaction_moves
    gone = rng.choice(300, 30, replace=False)
    src, dst = compaction_moves(300, gone)
    keep = np.ones(300, bool)
    keep[gone] = False
    pmap = np.full(300, -1, np.int64)
    pmap[keep] = np.flatnonzero(keep)
    pmap[src] = dst
    ix.update(pmap, 270)
    rows = np.arange(300)
    rows[dst] = rows[src]
    now = [texts[r] for r in rows[:270]]
    over = [3, 50, 269]
    pm = np.arange(270)
    pm[over] = -1
    add_texts = ["w1 w1 w2", "w7", "w39 w3"] + ["zz w5", "w0 w0 w0", "novel", "w2", "w3 w4"]
    ix.update(pm, 275, added=(np.asarray(over + list(range(270, 275))), add_texts))
    for p, t in zip(over + list(range(270, 275)), add_texts):
        if p < 270:
            now[p] = t
        else:
            now.append(t)
    ref = BM25Index().index(now)
    assert set(ix.vocab) == set(ref.vocab)
    for qtext in ["w1", "w7 w3", "novel w0", "w39", "zz", "w12 w13 w14"]:
        a, b = ix.search(qtext, 20), ref.search(qtext, 20)
        assert [r for r, _ in a] == [r for r, _ in b]
        assert np.allclose([s for _, s in a], [s for _, s in b], rtol=1e-6, atol=1e-7)


def test_sharded_embeddings_refuse_updates_before_the_device():
    from vietnamese_qa_system_amd.embeddings import Embeddings
    e = Embeddings()
    e.world, e._index, e.d = 2, object(), 4  # a rank of a two-rank index (no device is touched)
    with pytest.raises(NotImplementedError):
        e.upsert_vectors([1], np.zeros((1, 4), np.float32))
    with pytest.raises(NotImplementedError):
        e.delete([1])
    with pytest.raises(NotImplementedError):
        e.upsert([{"id": 1, "text": "x"}])
