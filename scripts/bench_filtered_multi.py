"""Filtered search with one filter per query on the headline shard: one JSON line.

    python scripts/bench_filtered_multi.py [--docs 10000000] [--dim 768] [--batch 256] [--k 10] [--steps 50] [--warmup 10]

The shard and queries are bench_filtered.py's (bench.py's shard: i.i.d. normal rows, L2-normalised, fp16, seed 1234; queries seed
99).  Legs, each one vqa_index_search_filtered_multi call per step against what a caller does without it:
  f1_contiguous_10pct: every query on one contiguous 10 % range, against vqa_index_search_filtered with the same bitmap;
  ranges_256x1pct:     query j on its own contiguous 1 % range (256 distinct ranges), against 256 B = 1 filtered calls;
  tenants_8x32:        8 tenants of 32 queries, each tenant a contiguous eighth of the rows;
  half_all_half_1pct:  half the queries on all rows (-1), the other half on one contiguous 1 % range.
Per leg: ms per step (HIP events around `steps` back-to-back calls), tiles of the union the scan reads, and an exact check of 8 queries
(spread over the batch) against an fp64 restatement over each query's own rows.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_filtered import build_shard, check  # noqa: E402


def timed(step, steps, warmup, dev):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from vietnamese_qa_system_amd.index import DeviceIndex
    from vietnamese_qa_system_amd.rowfilter import RowFilterBatch

    dev = torch.device("cuda", 0)
    n, d, b, k = args.docs, args.dim, args.batch, args.k
    shard = build_shard(n, d, 1234, dev)
    index = DeviceIndex(shard, id_base=1, dtype="fp16", device=0)
    gq = torch.Generator(device=dev)
    gq.manual_seed(99)
    q = torch.randn((b, d), generator=gq, device=dev, dtype=torch.float32)
    q = (q / q.norm(dim=1, keepdim=True)).to(torch.float16)

    def rng_mask(lo, rows):
        m = torch.zeros(n, dtype=torch.bool, device=dev)
        m[lo:lo + rows] = True
        return m

    one_pct = n // 100
    legs = {}
    m10 = rng_mask(n // 3, n // 10)
    legs["f1_contiguous_10pct"] = [m10] * b
    legs["ranges_256x1pct"] = [rng_mask((j * (n - one_pct)) // max(b - 1, 1), one_pct) for j in range(b)]
    tenants = [rng_mask(t * (n // 8), n // 8) for t in range(8)]
    legs["tenants_8x32"] = [tenants[j * 8 // b] for j in range(b)]
    m1 = rng_mask(n // 3, one_pct)
    legs["half_all_half_1pct"] = [None if j % 2 == 0 else m1 for j in range(b)]
    out = {"shard": {"n": n, "d": d, "dtype": "fp16", "batch": b, "k": k, "steps": args.steps, "warmup": args.warmup}, "legs": {}}
    probe = [j * b // 8 for j in range(8)]
    for name, masks in legs.items():
        cache = {}
        entries = []
        for m in masks:
            if m is None:
                entries.append(None)
                continue
            if id(m) not in cache:
                cache[id(m)] = index.row_filter(mask=m)
            entries.append(cache[id(m)])
        batch = RowFilterBatch(entries)
        union = torch.zeros(n, dtype=torch.bool, device=dev)
        for m in masks:
            union |= torch.ones_like(union) if m is None else m
        pad = torch.zeros((-n) % 256, dtype=torch.bool, device=dev)
        tiles = int(torch.cat([union, pad]).view(-1, 256).any(1).sum().item())
        ms = timed(lambda: index.search(q, k, return_positions=True, allow=batch), args.steps, args.warmup, dev)
        s, _, p = index.search(q, k, return_positions=True, allow=batch)
        torch.cuda.synchronize(dev)
        ok = all(check(shard, q[j:j + 1], torch.ones(n, dtype=torch.bool, device=dev) if masks[j] is None else masks[j], s[j:j + 1],
                       p[j:j + 1], k) for j in probe)
        leg = {"ms_per_step": round(ms, 4), "filters": batch.F, "union_tiles": tiles, "oracle_ok": ok}
        if name == "f1_contiguous_10pct":
            rf = entries[0]
            base = timed(lambda: index.search(q, k, return_positions=True, allow=rf), args.steps, args.warmup, dev)
            leg["shared_filter_ms"] = round(base, 4)
            leg["ratio_to_shared"] = round(ms / base, 3)
        if name == "ranges_256x1pct":
            def separate():
                for j in range(b):
                    index.search(q[j:j + 1], k, allow=entries[j])
            base = timed(separate, max(args.steps // 5, 2), 2, dev)
            leg["separate_calls_ms"] = round(base, 4)
            leg["speedup_vs_separate"] = round(base / ms, 2)
        out["legs"][name] = leg
    lg = out["legs"]
    out["target_f1_le_1.10x"] = lg["f1_contiguous_10pct"]["ratio_to_shared"] <= 1.10
    out["target_256_ranges_ge_10x"] = lg["ranges_256x1pct"]["speedup_vs_separate"] >= 10.0
    out["oracle_ok"] = all(v["oracle_ok"] for v in lg.values())
    print(json.dumps(out))
    index.close()
    return 0 if out["oracle_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
