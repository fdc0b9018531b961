"""Filtered search (vqa_index_search_filtered, DeviceIndex.search(allow=...)): the exact top-k among the rows a bitmap allows,
against the oracle restricted to those rows -- needs an MI355X."""
import ctypes

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


def _masks(n, seed):
    """name -> bool [n]: none; one row; the last row (partial last tile); a range over tile boundaries; every other row;
    random 1 %; random 50 %; all rows."""
    rng = np.random.default_rng(seed)
    out = {}
    out["none"] = np.zeros(n, bool)
    m = np.zeros(n, bool)
    m[n // 2] = True
    out["one"] = m
    m = np.zeros(n, bool)
    m[n - 1] = True
    out["last"] = m
    m = np.zeros(n, bool)
    m[n // 5: n // 5 + max(1, n // 3)] = True
    out["range"] = m
    out["every_other"] = (np.arange(n) % 2) == 0
    out["rand1"] = rng.random(n) < 0.01
    out["rand50"] = rng.random(n) < 0.5
    out["all"] = np.ones(n, bool)
    return out


def _bits_past_n(rf, n):
    """Set every bit of the last word past n (the library must ignore them)."""
    if n % 32:
        w = rf.bits[-1:].to(torch.int64) & 0xFFFFFFFF
        w |= (0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF
        rf.bits[-1:] = torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)


def _check(s, i, p, full, mask, k, id_base, score_tol=SCORE_TOL, tie_tol=TIE_TOL):
    allowed = np.flatnonzero(mask)
    kk = min(k, allowed.size)
    if kk:
        assert np.all(mask[p[:, :kk]]), "a returned row is outside the filter"
        R.check_topk(s[:, :kk], np.searchsorted(allowed, p[:, :kk]), full[:, allowed], k, score_tol=score_tol, tie_tol=tie_tol)
        assert np.array_equal(i[:, :kk], p[:, :kk] + id_base)
    assert np.all(np.isneginf(s[:, kk:])) and np.all(i[:, kk:] == -1) and np.all(p[:, kk:] == -1)


def _index(x, dtype, **kw):
    from vietnamese_qa_system_amd.index import DeviceIndex
    return DeviceIndex(x, dtype=dtype, device=0, **kw)


def _search(ix, q, k, rf=None):
    s, i, p = ix.search(torch.from_numpy(q).cuda(), k, return_positions=True, allow=rf)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy(), p.cpu().numpy()


@pytest.mark.parametrize("n,d,b,k", [
    (1000, 768, 256, 10), (1, 64, 3, 1), (7, 64, 1, 10), (257, 128, 5, 10), (4097, 100, 9, 3),
    (70001, 64, 300, 10), (2000, 33, 259, 5), (1500, 64, 777, 3),
])
def test_filtered_matches_oracle_fp16(native_lib, n, d, b, k):
    x = _unit(n, d, n + d).astype(np.float16)
    q = _unit(b, d, b + 1).astype(np.float16)
    full = R.full_scores(q.astype(np.float32), x, R.DTYPE_F16)
    ix = _index(x, "fp16", id_base=1)
    for name, mask in _masks(n, n).items():
        rf = ix.row_filter(mask=mask)
        assert rf.allowed == int(mask.sum())
        _bits_past_n(rf, n)
        s, i, p = _search(ix, q, k, rf)
        _check(s, i, p, full, mask, k, 1)
    ix.close()


@pytest.mark.parametrize("n,d,b,k", [(5000, 128, 9, 10), (70001, 64, 40, 3)])
def test_filtered_matches_oracle_fp32(native_lib, n, d, b, k):
    x = _unit(n, d, n).astype(np.float32)
    q = _unit(b, d, b).astype(np.float32)
    full = R.full_scores(q, x, R.DTYPE_F32)
    ix = _index(x, "fp32")
    for name, mask in _masks(n, n + 1).items():
        s, i, p = _search(ix, q, k, ix.row_filter(mask=mask))
        _check(s, i, p, full, mask, k, 0)
    ix.close()


@pytest.mark.parametrize("n,d,b,k", [(5000, 128, 9, 10), (3001, 768, 33, 12)])
def test_filtered_matches_oracle_fp8(native_lib, n, d, b, k):
    x = _unit(n, d, n)
    q = _unit(b, d, b)
    codes = R.e4m3_encode(x * FP8_SCALE)
    qd = R.e4m3_decode(R.e4m3_encode(q * FP8_SCALE)).astype(np.float64)
    full = qd @ R.e4m3_decode(codes).astype(np.float64).T / (FP8_SCALE * FP8_SCALE)
    ix = _index(x, "fp8")
    for name, mask in _masks(n, n + 2).items():
        s, i, p = _search(ix, q, k, ix.row_filter(mask=mask))
        _check(s, i, p, full, mask, k, 0, score_tol=5e-5, tie_tol=1e-4)
    ix.close()


@pytest.mark.parametrize("k", [40, 300])
def test_large_k_against_oracle(native_lib, k):
    n, d, b = 20000, 64, 7
    x = _unit(n, d, 3).astype(np.float16)
    q = _unit(b, d, 4).astype(np.float16)
    full = R.full_scores(q.astype(np.float32), x, R.DTYPE_F16)
    ix = _index(x, "fp16", id_base=5)
    for name in ("range", "rand50", "every_other", "rand1"):
        mask = _masks(n, 9)[name]
        s, i, p = _search(ix, q, k, ix.row_filter(mask=mask))
        _check(s, i, p, full, mask, k, 5)
    ix.close()


@pytest.mark.parametrize("k", [10, 40, 300])
def test_golden_ties_bit_exact_under_a_mask(native_lib, golden_dir, k):
    """Small-integer vectors: every product is exact, so positions, ids AND scores must equal a numpy restatement bit for bit
    (score desc, position asc over the allowed rows)."""
    g = np.load(f"{golden_dir}/retr_ties.npz")
    x, q, ids = g["x"].astype(np.float16), g["q"].astype(np.float16), g["ids"]
    n = x.shape[0]
    full = q.astype(np.float64) @ x.astype(np.float64).T
    ix = _index(x, "fp16", ids=ids)
    for mask in ((np.arange(n) % 3) != 1, np.arange(n) >= 37, np.arange(n) < 64):
        s, i, p = _search(ix, q, k, ix.row_filter(mask=mask))
        allowed = np.flatnonzero(mask)
        kk = min(k, allowed.size)
        for r in range(q.shape[0]):
            sc = full[r, allowed]
            order = allowed[np.lexsort((allowed, -sc))][:kk]
            assert np.array_equal(p[r, :kk], order)
            assert np.array_equal(i[r, :kk], ids[order])
            assert np.array_equal(s[r, :kk], full[r, order].astype(np.float32))
            assert np.all(p[r, kk:] == -1) and np.all(i[r, kk:] == -1) and np.all(np.isneginf(s[r, kk:]))
    ix.close()


def test_all_ones_equals_unfiltered_without_sketch(native_lib):
    n, d, b = 70001, 128, 64
    x = _unit(n, d, 11).astype(np.float16)
    q = _unit(b, d, 12).astype(np.float16)
    ix = _index(x, "fp16", id_base=3, sketch=False)
    rf = ix.row_filter(mask=np.ones(n, bool))
    for k in (1, 10, 12, 30):
        a = _search(ix, q, k)
        f = _search(ix, q, k, rf)
        for u, v in zip(a, f):
            assert np.array_equal(u, v), k
    ix.close()


def test_all_ones_equals_unfiltered_on_a_sketch_shard(native_lib):
    """A sketch shard reached at a small size (stage_min_tiles): the unfiltered search takes the sketch cascade and ends in the
    re-scoring arithmetic; the filtered one ends the same way (final_rescore), so an all-ones filter returns the same bits.  The
    sketch's pause state is neither read nor changed by filtered calls, and a filtered call between two unfiltered ones changes
    neither of them."""
    n, d, b = 300_000, 128, 32
    x = _unit(n, d, 21).astype(np.float16)
    q = _unit(b, d, 22).astype(np.float16)
    ix = _index(x, "fp16", sketch=True, options={"stage_min_tiles": 2, "final_rescore": 1})
    assert ix.sketch_state() == 0, "the test needs a shard that keeps a sketch"
    rf = ix.row_filter(mask=np.ones(n, bool))
    half = ix.row_filter(mask=(np.arange(n) % 2) == 0)
    for k in (1, 5, 10):
        a = _search(ix, q, k)
        state = ix.sketch_state()
        f = _search(ix, q, k, rf)
        for u, v in zip(a, f):
            assert np.array_equal(u, v), k
        for _ in range(20):
            _search(ix, q, k, half)
        assert ix.sketch_state() == state
        a2 = _search(ix, q, k)
        for u, v in zip(a, a2):
            assert np.array_equal(u, v), k
    ix.close()


def test_hip_graph_replay_follows_the_bitmap(native_lib):
    n, d, b, k = 20000, 64, 16, 10
    x = _unit(n, d, 31).astype(np.float16)
    q = _unit(b, d, 32).astype(np.float16)
    full = R.full_scores(q.astype(np.float32), x, R.DTYPE_F16)
    ix = _index(x, "fp16")
    first = np.zeros(n, bool)
    first[:3000] = True
    second = np.zeros(n, bool)
    second[12345:12345 + 700] = True
    rf = ix.row_filter(mask=first)
    dev = torch.device("cuda", 0)
    q_buf = torch.from_numpy(q).to(dev)
    out_s = torch.empty((b, k), dtype=torch.float32, device=dev)
    out_i = torch.empty((b, k), dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        ix.search(q_buf, k, out=(out_s, out_i), allow=rf)  # warm-up outside the capture: one-time kernel attributes
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ix.search(q_buf, k, out=(out_s, out_i), allow=rf)
    for mask in (second, first, second):
        rf.bits.copy_(ix.row_filter(mask=mask).bits)
        out_s.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        s, i = out_s.cpu().numpy(), out_i.cpu().numpy()
        _check(s, i, i, full, mask, k, 0)
    ix.close()


def test_poisoned_workspace(native_lib):
    n, d, b, k = 9000, 64, 20, 30
    x = _unit(n, d, 41).astype(np.float16)
    q = _unit(b, d, 42).astype(np.float16)
    full = R.full_scores(q.astype(np.float32), x, R.DTYPE_F16)
    ix = _index(x, "fp16", options={"poison_workspace": 0xA5})
    for name, mask in _masks(n, 43).items():
        s, i, p = _search(ix, q, k, ix.row_filter(mask=mask))
        _check(s, i, p, full, mask, k, 0)
    ix.close()


def test_errors(native_lib):
    from vietnamese_qa_system_amd import _native as N
    n, d = 1000, 64
    x = _unit(n, d, 51).astype(np.float16)
    ix = _index(x, "fp16")
    lib = N.load()
    q = torch.from_numpy(_unit(2, d, 52).astype(np.float16)).cuda()
    s = torch.empty((2, 1024), dtype=torch.float32, device="cuda")
    i = torch.empty((2, 1024), dtype=torch.int64, device="cuda")
    bits_dev = ix.row_filter(mask=np.ones(n, bool)).bits
    bits_host = np.full((n + 31) // 32, -1, dtype=np.int32)
    stream = torch.cuda.current_stream().cuda_stream
    for allow, k in ((None, 10), (bits_host.ctypes.data, 10), (bits_dev.data_ptr(), 0), (bits_dev.data_ptr(), 1025)):
        rc = lib.vqa_index_search_filtered(ix._handle, q.data_ptr(), N.VQA_F16, 2, k, allow, s.data_ptr(), i.data_ptr(), None, stream)
        assert rc == -1, (allow, k)
    with pytest.raises(ValueError):
        N.check(lib.vqa_index_search_filtered(ix._handle, q.data_ptr(), N.VQA_F16, 2, 10, None, s.data_ptr(), i.data_ptr(), None,
                                              stream), "vqa_index_search_filtered")
    with pytest.raises(ValueError):
        ix.search(q, 1025, allow=ix.row_filter(mask=np.ones(n, bool)))
    ix.close()
