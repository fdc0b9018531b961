"""Filtered search with one bitmap per query (vqa_index_search_filtered_multi, DeviceIndex.search(allow=RowFilterBatch)): each query's
exact top-k among the rows of its own bitmap, against the oracle restricted to those rows, and bit for bit against the shared-filter
call -- needs an MI355X."""
import numpy as np
import pytest
import torch

from oracle import retrieval as R

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-5
TIE_TOL = 2e-6
FP8_SCALE = 16.0


def _unit(n, d, seed):
    rng = np.random.default_rng(seed)
    return R.l2_normalize(rng.standard_normal((n, d)).astype(np.float32))


def _masks(n, seed, count):
    """``count`` bool [n] masks of different shapes: ranges over tile boundaries, random densities, one row, the last row, none, all."""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(count):
        kind = j % 7
        m = np.zeros(n, bool)
        if kind == 0:
            lo = int(rng.integers(0, n))
            m[lo:lo + max(1, n // 50)] = True
        elif kind == 1:
            m = rng.random(n) < 0.01
        elif kind == 2:
            m = rng.random(n) < 0.5
        elif kind == 3:
            m[int(rng.integers(0, n))] = True
        elif kind == 4:
            m[n - 1] = True
        elif kind == 5:
            pass
        else:
            m[:] = True
        out.append(m)
    return out


def _bits_past_n(rf, n):
    """Set every bit of the last word past n (the library must ignore them)."""
    if n % 32:
        w = rf.bits[-1:].to(torch.int64) & 0xFFFFFFFF
        w |= (0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF
        rf.bits[-1:] = torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)


def _check_row(s, i, p, full_row, mask, k, id_base, score_tol=SCORE_TOL, tie_tol=TIE_TOL):
    allowed = np.flatnonzero(mask)
    kk = min(k, allowed.size)
    if kk:
        assert np.all(mask[p[:kk]]), "a returned row is outside the query's filter"
        R.check_topk(s[None, :kk], np.searchsorted(allowed, p[None, :kk]), full_row[None, allowed], k, score_tol=score_tol,
                     tie_tol=tie_tol)
        assert np.array_equal(i[:kk], p[:kk] + id_base)
    assert np.all(np.isneginf(s[kk:])) and np.all(i[kk:] == -1) and np.all(p[kk:] == -1)


def _index(x, dtype, **kw):
    from vietnamese_qa_system_amd.index import DeviceIndex
    return DeviceIndex(x, dtype=dtype, device=0, **kw)


def _search(ix, q, k, allow=None):
    s, i, p = ix.search(torch.from_numpy(q).cuda(), k, return_positions=True, allow=allow)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy(), p.cpu().numpy()


def _per_query(ix, n, b, seed, distinct):
    """A batch of b queries over ``distinct`` masks (query j -> mask j % distinct, every fifth query None = all rows)."""
    from vietnamese_qa_system_amd.rowfilter import RowFilterBatch
    masks = _masks(n, seed, distinct)
    rfs = [ix.row_filter(mask=m) for m in masks]
    for rf in rfs:
        _bits_past_n(rf, n)
    entries = [None if j % 5 == 4 else rfs[j % distinct] for j in range(b)]
    qmasks = [np.ones(n, bool) if e is None else masks[j % distinct] for j, e in enumerate(entries)]
    return RowFilterBatch(entries), qmasks


@pytest.mark.parametrize("n,d,b,k", [
    (1000, 768, 256, 10), (1, 64, 3, 1), (4097, 100, 5, 13), (70001, 64, 257, 10), (2000, 33, 300, 12), (9000, 64, 5, 100),
    (5000, 64, 3, 1024), (1500, 64, 1, 10),
])
def test_matches_oracle_fp16(native_lib, n, d, b, k):
    x = _unit(n, d, n + d).astype(np.float16)
    q = _unit(b, d, b + 1).astype(np.float16)
    full = R.full_scores(q.astype(np.float32), x, R.DTYPE_F16)
    ix = _index(x, "fp16", id_base=1)
    for distinct in (1, 7, b):
        batch, qmasks = _per_query(ix, n, b, n + distinct, distinct)
        s, i, p = _search(ix, q, k, batch)
        for r in range(b):
            _check_row(s[r], i[r], p[r], full[r], qmasks[r], k, 1)
    ix.close()


@pytest.mark.parametrize("n,d,b,k", [(5000, 128, 9, 10), (70001, 64, 257, 13)])
def test_matches_oracle_fp32(native_lib, n, d, b, k):
    x = _unit(n, d, n).astype(np.float32)
    q = _unit(b, d, b).astype(np.float32)
    full = R.full_scores(q, x, R.DTYPE_F32)
    ix = _index(x, "fp32")
    batch, qmasks = _per_query(ix, n, b, n + 1, 11)
    s, i, p = _search(ix, q, k, batch)
    for r in range(b):
        _check_row(s[r], i[r], p[r], full[r], qmasks[r], k, 0)
    ix.close()


@pytest.mark.parametrize("n,d,b,k", [(5000, 128, 9, 10), (3001, 768, 256, 12), (3001, 128, 300, 40)])
def test_matches_oracle_fp8(native_lib, n, d, b, k):
    x = _unit(n, d, n)
    q = _unit(b, d, b)
    codes = R.e4m3_encode(x * FP8_SCALE)
    qd = R.e4m3_decode(R.e4m3_encode(q * FP8_SCALE)).astype(np.float64)
    full = qd @ R.e4m3_decode(codes).astype(np.float64).T / (FP8_SCALE * FP8_SCALE)
    ix = _index(x, "fp8")
    batch, qmasks = _per_query(ix, n, b, n + 2, 13)
    s, i, p = _search(ix, q, k, batch)
    for r in range(b):
        _check_row(s[r], i[r], p[r], full[r], qmasks[r], k, 0, score_tol=5e-5, tie_tol=1e-4)
    ix.close()


def _bit_equal(a, b):
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("k", [1, 10, 30])
def test_one_bitmap_equals_the_shared_filter_call(native_lib, k):
    n, d, b = 70001, 128, 300
    x = _unit(n, d, 61).astype(np.float16)
    q = _unit(b, d, 62).astype(np.float16)
    ix = _index(x, "fp16", id_base=2)
    m = np.zeros(n, bool)
    m[5000:12000] = True
    rf = ix.row_filter(mask=m)
    _bit_equal(_search(ix, q, k, rf), _search(ix, q, k, [rf] * b))
    ix.close()


@pytest.mark.parametrize("n,opts", [(20000, {}), (300_000, {"stage_min_tiles": 2, "final_rescore": 1})])
def test_distinct_filters_equal_single_query_calls(native_lib, n, opts):
    """F = B distinct bitmaps: every query returns the bits of a B = 1 shared-filter call with its own bitmap (the second shard ends
    in the final re-scoring, the first does not)."""
    d, b, k = 128, 24, 10
    x = _unit(n, d, 71).astype(np.float16)
    q = _unit(b, d, 72).astype(np.float16)
    ix = _index(x, "fp16", options=opts)
    masks = _masks(n, 73, b)
    rfs = [ix.row_filter(mask=m) for m in masks]
    s, i, p = _search(ix, q, k, rfs)
    for r in range(b):
        s1, i1, p1 = _search(ix, q[r:r + 1], k, rfs[r])
        assert np.array_equal(s[r], s1[0]) and np.array_equal(i[r], i1[0]) and np.array_equal(p[r], p1[0]), r
    ix.close()


def test_all_rows_entry_equals_the_all_ones_call(native_lib):
    from vietnamese_qa_system_amd.rowfilter import RowFilterBatch
    n, d, b, k = 70001, 64, 40, 12
    x = _unit(n, d, 81).astype(np.float16)
    q = _unit(b, d, 82).astype(np.float16)
    ix = _index(x, "fp16")
    ones = ix.row_filter(mask=np.ones(n, bool))
    some = ix.row_filter(mask=(np.arange(n) % 3) == 0)
    a = _search(ix, q, k, ones)
    entries = [None if r % 2 == 0 else some for r in range(b)]
    s, i, p = _search(ix, q, k, RowFilterBatch(entries))
    for r in range(0, b, 2):
        assert np.array_equal(s[r], a[0][r]) and np.array_equal(i[r], a[1][r]) and np.array_equal(p[r], a[2][r])
    _bit_equal(a, _search(ix, q, k, [None] * b))
    ix.close()


def _raw_multi(ix, q, k, bits, qf, F):
    from vietnamese_qa_system_amd import _native as N
    b = q.shape[0]
    s = torch.empty((b, k), dtype=torch.float32, device="cuda")
    i = torch.empty((b, k), dtype=torch.int64, device="cuda")
    p = torch.empty((b, k), dtype=torch.int64, device="cuda")
    rc = N.load().vqa_index_search_filtered_multi(ix._handle, q.data_ptr(), N.VQA_F16, b, k, bits.data_ptr(), F, qf.data_ptr(),
                                                  s.data_ptr(), i.data_ptr(), p.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy(), p.cpu().numpy()


def test_out_of_range_entries_and_empty_bitmaps_give_padding(native_lib):
    n, d, b, k = 9000, 64, 8, 10
    x = _unit(n, d, 91).astype(np.float16)
    q = torch.from_numpy(_unit(b, d, 92).astype(np.float16)).cuda()
    full = R.full_scores(q.cpu().numpy().astype(np.float32), x, R.DTYPE_F16)
    ix = _index(x, "fp16")
    some = np.zeros(n, bool)
    some[100:900] = True
    bits = torch.stack([ix.row_filter(mask=some).bits, ix.row_filter(mask=np.zeros(n, bool)).bits]).contiguous()
    qf = torch.tensor([0, 1, 2, -2, 1 << 30, -(1 << 31), 0, -1], dtype=torch.int32, device="cuda")
    s, i, p = _raw_multi(ix, q, k, bits, qf, 2)
    for r in range(b):
        mask = some if r in (0, 6) else np.ones(n, bool) if r == 7 else np.zeros(n, bool)
        _check_row(s[r], i[r], p[r], full[r], mask, k, 0)
    ix.close()


def test_empty_shard_gives_padding(native_lib):
    from vietnamese_qa_system_amd.rowfilter import RowFilter
    ix = _index(np.zeros((0, 64), np.float16), "fp16")
    rf = RowFilter.from_mask(np.zeros(0, bool), device=0)
    s, i, p = _search(ix, _unit(3, 64, 5).astype(np.float16), 7, [rf, None, rf])
    assert np.all(np.isneginf(s)) and np.all(i == -1) and np.all(p == -1)
    ix.close()


@pytest.mark.parametrize("k", [10, 40])
def test_golden_ties_bit_exact_under_per_query_masks(native_lib, golden_dir, k):
    g = np.load(f"{golden_dir}/retr_ties.npz")
    x, q, ids = g["x"].astype(np.float16), g["q"].astype(np.float16), g["ids"]
    n = x.shape[0]
    full = q.astype(np.float64) @ x.astype(np.float64).T
    ix = _index(x, "fp16", ids=ids)
    masks = [(np.arange(n) % 3) != 1, np.arange(n) >= 37, np.arange(n) < 64, np.ones(n, bool)]
    rfs = [ix.row_filter(mask=m) for m in masks]
    s, i, p = _search(ix, q, k, [rfs[r % 4] for r in range(q.shape[0])])
    for r in range(q.shape[0]):
        allowed = np.flatnonzero(masks[r % 4])
        kk = min(k, allowed.size)
        order = allowed[np.lexsort((allowed, -full[r, allowed]))][:kk]
        assert np.array_equal(p[r, :kk], order)
        assert np.array_equal(i[r, :kk], ids[order])
        assert np.array_equal(s[r, :kk], full[r, order].astype(np.float32))
        assert np.all(p[r, kk:] == -1) and np.all(i[r, kk:] == -1) and np.all(np.isneginf(s[r, kk:]))
    ix.close()


def test_sketch_state_unchanged(native_lib):
    n, d, b = 300_000, 128, 32
    x = _unit(n, d, 101).astype(np.float16)
    q = _unit(b, d, 102).astype(np.float16)
    ix = _index(x, "fp16", sketch=True, options={"stage_min_tiles": 2, "final_rescore": 1})
    assert ix.sketch_state() == 0, "the test needs a shard that keeps a sketch"
    a = _search(ix, q, 10)
    state = ix.sketch_state()
    rfs = [ix.row_filter(mask=m) for m in _masks(n, 103, 8)]
    for _ in range(10):
        _search(ix, q, 10, [rfs[r % 8] for r in range(b)])
    assert ix.sketch_state() == state
    _bit_equal(a, _search(ix, q, 10))
    ix.close()


def test_poisoned_workspace(native_lib):
    n, d, b, k = 9000, 64, 260, 30
    x = _unit(n, d, 111).astype(np.float16)
    q = _unit(b, d, 112).astype(np.float16)
    full = R.full_scores(q.astype(np.float32), x, R.DTYPE_F16)
    ix = _index(x, "fp16", options={"poison_workspace": 0xA5})
    batch, qmasks = _per_query(ix, n, b, 113, 9)
    s, i, p = _search(ix, q, k, batch)
    for r in range(b):
        _check_row(s[r], i[r], p[r], full[r], qmasks[r], k, 0)
    ix.close()


def test_hip_graph_replay_follows_both_arrays(native_lib):
    from vietnamese_qa_system_amd.rowfilter import RowFilterBatch
    n, d, b, k = 20000, 64, 16, 10
    x = _unit(n, d, 121).astype(np.float16)
    q = _unit(b, d, 122).astype(np.float16)
    full = R.full_scores(q.astype(np.float32), x, R.DTYPE_F16)
    ix = _index(x, "fp16")
    m0, m1, m2 = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    m0[:3000] = True
    m1[12345:13045] = True
    m2[19000:] = True
    f0, f1 = ix.row_filter(mask=m0), ix.row_filter(mask=m1)
    batch = RowFilterBatch([f0 if r % 2 else f1 for r in range(b)])
    dev = torch.device("cuda", 0)
    q_buf = torch.from_numpy(q).to(dev)
    out_s = torch.empty((b, k), dtype=torch.float32, device=dev)
    out_i = torch.empty((b, k), dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        ix.search(q_buf, k, out=(out_s, out_i), allow=batch)  # warm-up outside the capture: one-time kernel attributes
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ix.search(q_buf, k, out=(out_s, out_i), allow=batch)
    bitmaps = {0: m1, 1: m0}  # (stored in order of first use: query 0 takes f1)
    for assign, rewrite in (([1, 0] * (b // 2), None), ([0] * b, None), ([-1, 1, 0, 5] * (b // 4), (1, m2))):
        if rewrite is not None:
            batch.bits[rewrite[0]].copy_(ix.row_filter(mask=rewrite[1]).bits)
            bitmaps[rewrite[0]] = rewrite[1]
        batch.query_filter.copy_(torch.tensor(assign, dtype=torch.int32))
        out_s.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        s, i = out_s.cpu().numpy(), out_i.cpu().numpy()
        for r in range(b):
            a = assign[r]
            mask = bitmaps[a] if a in bitmaps else np.ones(n, bool) if a == -1 else np.zeros(n, bool)
            _check_row(s[r], i[r], i[r], full[r], mask, k, 0)
    ix.close()


def test_errors(native_lib):
    from vietnamese_qa_system_amd import _native as N
    n, d = 1000, 64
    x = _unit(n, d, 131).astype(np.float16)
    ix = _index(x, "fp16")
    lib = N.load()
    q = torch.from_numpy(_unit(2, d, 132).astype(np.float16)).cuda()
    s = torch.empty((2, 1024), dtype=torch.float32, device="cuda")
    i = torch.empty((2, 1024), dtype=torch.int64, device="cuda")
    bits = ix.row_filter(mask=np.ones(n, bool)).bits
    bits_host = np.full((n + 31) // 32, -1, dtype=np.int32)
    qf = torch.zeros(2, dtype=torch.int32, device="cuda")
    qf_host = np.zeros(2, dtype=np.int32)
    stream = torch.cuda.current_stream().cuda_stream
    cases = [
        (N.VQA_F16, 2, 10, None, 1, qf.data_ptr()),
        (N.VQA_F16, 2, 10, bits_host.ctypes.data, 1, qf.data_ptr()),
        (N.VQA_F16, 2, 10, bits.data_ptr(), 1, None),
        (N.VQA_F16, 2, 10, bits.data_ptr(), 1, qf_host.ctypes.data),
        (N.VQA_F16, 2, 10, bits.data_ptr(), 0, qf.data_ptr()),
        (N.VQA_F16, 2, 10, bits.data_ptr(), -3, qf.data_ptr()),
        (N.VQA_F16, 0, 10, bits.data_ptr(), 1, qf.data_ptr()),
        (N.VQA_F16, 2, 0, bits.data_ptr(), 1, qf.data_ptr()),
        (N.VQA_F16, 2, 1025, bits.data_ptr(), 1, qf.data_ptr()),
        (N.VQA_FP8_E4M3, 2, 10, bits.data_ptr(), 1, qf.data_ptr()),
    ]
    for dt, b, k, allow, F, qfp in cases:
        rc = lib.vqa_index_search_filtered_multi(ix._handle, q.data_ptr(), dt, b, k, allow, F, qfp, s.data_ptr(), i.data_ptr(), None, stream)
        assert rc == -1, (dt, b, k, allow, F, qfp)
    with pytest.raises(ValueError):
        ix.search(q, 10, allow=[None])  # one entry for two queries
    ix.close()
