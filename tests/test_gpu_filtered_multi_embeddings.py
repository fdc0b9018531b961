"""Embeddings.batchsearch(filters=[...]): one filter per query in one batched search -- by ids (contiguous, an id vector, string
ids), by a document field in memory and after save() / load(), None entries, text queries, hybrid, after upsert / delete, and a
two-rank sharded merge -- each query held to the exact top-k over its own rows, or to the single-filter call -- needs an MI355X."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from oracle import retrieval as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _unit(n, d, seed):
    rng = np.random.default_rng(seed)
    return R.l2_normalize(rng.standard_normal((n, d)).astype(np.float32))


def _want(x, q, rows, limit):
    """Exact top-limit positions among `rows` for one query (fp16 stored values, score desc, position asc), scores > 0 only."""
    full = q.astype(np.float64) @ x.astype(np.float16).astype(np.float64).T
    rows = np.asarray(sorted(rows), dtype=np.int64)
    sc = full[rows]
    o = rows[np.lexsort((rows, -sc))][:limit]
    return [int(p) for p in o if full[p] > 0]


def _emb(**kw):
    from vietnamese_qa_system_amd.embeddings import Embeddings
    return Embeddings(**kw)


@pytest.mark.parametrize("kind", ["contiguous", "vector", "string"])
def test_filters_by_ids(native_lib, kind):
    n, d, b, limit = 3000, 64, 6, 10
    x, q = _unit(n, d, 1), _unit(b, d, 2).astype(np.float16)
    ids = {"contiguous": list(range(1, n + 1)), "vector": [int(v) for v in np.random.default_rng(3).permutation(10 * n)[:n]],
           "string": [f"doc-{p}" for p in range(n)]}[kind]
    e = _emb()
    e.index_vectors(ids, x)
    rows = [list(range(700, 1300)) + [5, 2999], list(range(0, 40)), None, list(range(700, 1300)) + [5, 2999], [1234], []]
    filters = [None if r is None else [ids[p] for p in r] for r in rows]
    got = e.batchsearch(q, limit, filters=filters)
    for j in range(b):
        want = _want(x, q[j], range(n) if rows[j] is None else rows[j], limit)
        assert [i for i, _ in got[j]] == [ids[p] for p in want], j
        assert got[j] == e.batchsearch(q[j:j + 1], limit, filter=filters[j])[0] if filters[j] is not None else True


def test_filters_by_source_in_memory_and_after_load(native_lib, tmp_path):
    n, d, b, limit = 2000, 64, 5, 8
    x, q = _unit(n, d, 4), _unit(b, d, 5).astype(np.float16)
    sources = ["wiki", "news", "blog"]
    docs = [{"id": p + 1, "text": f"text {p}", "source": sources[(p // 100) % 3]} for p in range(n)]
    e = _emb(content=True)
    e.index_vectors([doc["id"] for doc in docs], x, documents=docs)
    filters = [{"source": "news"}, None, {"source": ["wiki", "blog"]}, {"source": ("blog", "wiki")}, {"source": "nowhere"}]

    def rows_of(f):
        if f is None:
            return range(n)
        vals = {f["source"]} if isinstance(f["source"], str) else set(f["source"])
        return [p for p in range(n) if docs[p]["source"] in vals]

    for emb in (e, None):
        if emb is None:
            e.save(str(tmp_path))
            emb = _emb().load(str(tmp_path))
        got = emb.batchsearch(q, limit, filters=filters)
        for j in range(b):
            assert [h["id"] for h in got[j]] == [p + 1 for p in _want(x, q[j], rows_of(filters[j]), limit)], j
        assert got[4] == []
        with pytest.raises(ValueError):
            emb.batchsearch(q, limit, filters=[{"author": "x"}] + [None] * (b - 1))


def test_text_queries_and_hybrid(native_lib):
    """Text queries through an encoder, dense only and hybrid: each query's result equals the single-filter call with its filter
    (whose hybrid path is held to a numpy recomputation in test_gpu_filtered_embeddings.py)."""
    n, d, limit = 600, 32, 5
    x = _unit(n, d, 6)
    words = ["alpha", "beta", "gamma", "delta", "omega"]
    texts = [" ".join(words[(p * 7 + j) % 5] for j in range(1 + p % 4)) for p in range(n)]
    queries = ["alpha beta", "gamma", "omega delta", "beta"]
    qv = _unit(len(queries), d, 7).astype(np.float16)

    def encoder(t):
        import torch
        return torch.from_numpy(qv[[queries.index(s) for s in t]]).cuda()
    filters = [list(range(100, 400)), None, list(range(500, 600)), list(range(100, 400))]
    for hybrid in (False, True):
        e = _emb(hybrid=hybrid, encoder=encoder)
        e.index([{"id": p, "text": texts[p]} for p in range(n)], vectors=x)
        got = e.batchsearch(queries, limit, filters=filters)
        for j, text in enumerate(queries):
            single = e.batchsearch([text], limit, filter=filters[j])[0] if filters[j] is not None else None
            if single is not None:
                assert got[j] == single, (hybrid, j)
                assert all(i in set(filters[j]) for i, _ in got[j])
        # the None entry: the whole corpus, as an unfiltered batch of the same queries
        assert got[1] == e.batchsearch(queries, limit, filter=list(range(n)))[1]


def test_after_upsert_and_delete(native_lib):
    from vietnamese_qa_system_amd.rowfilter import RowFilterBatch
    n, d, b, limit = 1500, 64, 4, 6
    x, q = _unit(n, d, 8), _unit(b, d, 9).astype(np.float16)
    e = _emb()
    e.index_vectors(list(range(n)), x)
    e.delete([10, 11, 950])  # the first update (the shard may be rebuilt for its id vector): the handle below is the one that stays
    ix = e._index
    stale = RowFilterBatch([ix.row_filter(positions=np.arange(0, 300)), None, ix.row_filter(positions=np.arange(900, 1400)), None])
    import torch
    qd = torch.from_numpy(q).cuda()
    ix.search(qd, limit, allow=stale)
    newv = _unit(2, d, 10)
    e.upsert_vectors([5, 1000], newv)  # (rows overwritten in place: the positions, and with them the filters, stay valid)
    ix.search(qd, limit, allow=stale)
    e.delete([20])  # a removal moves rows: the batch is stale
    with pytest.raises(ValueError, match="generation"):
        ix.search(qd, limit, allow=stale)
    # a rebuilt batch (by ids through Embeddings) is exact over the updated rows
    cur = {i: x[i] for i in range(n)}
    cur[5], cur[1000] = newv[0], newv[1]
    for i in (10, 11, 950, 20):
        del cur[i]
    filters = [list(range(0, 300)), None, list(range(900, 1500)), [10, 11, 20, 5, 1000]]
    got = e.batchsearch(q, limit, filters=filters)
    keys = np.array(sorted(cur))
    mat = np.stack([cur[i] for i in keys])
    for j in range(b):
        allowed = keys if filters[j] is None else np.array([i for i in keys if i in set(filters[j])])
        full = q[j].astype(np.float64) @ mat.astype(np.float16).astype(np.float64).T
        sc = {int(i): full[np.searchsorted(keys, i)] for i in allowed}
        want = sorted(sc, key=lambda i: -sc[i])[:limit]
        want = [i for i in want if sc[i] > 0]
        assert sorted(i for i, _ in got[j]) == sorted(want), j
        assert np.allclose([s for _, s in got[j]], [sc[i] for i in (i for i, _ in got[j])], atol=1e-5)


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_per_query_filters_merge(native_lib, tmp_path):
    world = 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "filtered_multi_sharded_worker.py"), "--out", str(tmp_path)]
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-4000:] + "\n" + r.stderr[-6000:])
    for rank in range(world):
        with open(tmp_path / f"rank{rank}.json") as f:
            rec = json.load(f)
        assert rec["world"] == world and rec["checks"] == ["merged_fp16"], rec
