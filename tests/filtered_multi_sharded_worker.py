"""One rank of the job tests/test_gpu_filtered_multi_embeddings.py starts with ``python -m torch.distributed.run --nproc-per-node 2``:
both ranks on cuda:0 over gloo.  Every rank keeps its row shard of the corpus (an odd row count: rank 1 starts at an odd row), slices
every distinct per-query filter to its rows and searches the batch in one call; the MERGED result (one all-gather, the same merge) is
held per query to an fp64 restatement over that query's rows of the whole corpus."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    from vietnamese_qa_system_amd import build
    assert build.is_fresh(), "build the library before starting the workers"

    import numpy as np
    import torch
    import torch.distributed as dist

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    from oracle import retrieval as R
    from vietnamese_qa_system_amd.embeddings import Embeddings
    from vietnamese_qa_system_amd.rowfilter import RowFilter
    from vietnamese_qa_system_amd.sharded import shard_bounds

    n, d, b, k = 20001, 768, 6, 10
    lo1, _ = shard_bounds(n, world, 1)
    assert lo1 % 32 != 0
    rng = np.random.default_rng(15)
    x = R.l2_normalize(rng.standard_normal((n, d)).astype(np.float32))
    q = R.l2_normalize(rng.standard_normal((b, d)).astype(np.float32)).astype(np.float16)
    straddle = np.zeros(n, bool)
    straddle[lo1 - 777: lo1 + 555] = True
    straddle[13] = straddle[n - 1] = True
    first = np.zeros(n, bool)
    first[:3000] = True
    second = np.zeros(n, bool)
    second[lo1 + 100: lo1 + 4000] = True
    rf = RowFilter.from_mask(straddle)
    masks = [straddle, None, first, straddle, second, None]
    filters = [rf, None, list(np.flatnonzero(first)), rf, list(np.flatnonzero(second)), None]
    e = Embeddings(dtype="fp16", min_score=None, normalize=False)
    e.index_vectors(None, x)
    got = e.batchsearch(q, k, filters=filters)
    full = q.astype(np.float64) @ x.astype(np.float16).astype(np.float64).T
    for j in range(b):
        mask = np.ones(n, bool) if masks[j] is None else masks[j]
        allowed = np.flatnonzero(mask)
        pos = np.array([[i for i, _ in got[j]]], dtype=np.int64)
        sc = np.array([[s for _, s in got[j]]], dtype=np.float32)
        assert np.all(mask[pos]), j
        R.check_topk(sc, np.searchsorted(allowed, pos), full[j:j + 1, allowed], k, score_tol=1e-5, tie_tol=2e-6)
    with open(os.path.join(args.out, f"rank{rank}.json"), "w") as f:
        json.dump({"rank": rank, "world": world, "checks": ["merged_fp16"]}, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
