"""Filtered search on the headline shard: one JSON line.

    python scripts/bench_filtered.py [--docs 10000000] [--dim 768] [--batch 256] [--k 10] [--steps 100] [--warmup 20]

The shard is bench.py's (i.i.d. normal rows, L2-normalised, fp16, seed 1234; queries seed 99).  Legs: the unfiltered search (default
plan: the sketch cascade), the exact path of the same handle (sketch paused), and filtered searches (vqa_index_search_filtered) with
all rows, a contiguous 10 % and 1 %, a random 1 % and a random 0.01 % of the rows allowed.  Per leg: ms per step (HIP events around
`steps` back-to-back searches), scan-kernel ms per step (the handle's timing events), tiles touched, bytes the scan reads
(tiles x 256 x d x 2 per pass), GB/s, and an exact check of 8 queries against an fp64 restatement over the allowed rows.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_shard(n, d, seed, device, chunk=1 << 18):
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    buf = torch.empty((n, d), dtype=torch.float16, device=device)
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        x = torch.randn((c1 - c0, d), generator=gen, device=device, dtype=torch.float32)
        x /= x.norm(dim=1, keepdim=True)
        buf[c0:c1] = x.to(buf.dtype)
    return buf


def check(shard, q, mask, s, p, k, chunk=1 << 20):
    """Exact top-k of the allowed rows in fp64 (chunked on the device) against the search's scores and positions."""
    n = shard.shape[0]
    q64 = q.double()
    best_s, best_p = [], []
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        sc = q64 @ shard[c0:c1].double().T
        sc[:, ~mask[c0:c1]] = -float("inf")
        v, i = torch.topk(sc, min(k + 1, c1 - c0), dim=1)
        best_s.append(v)
        best_p.append(i + c0)
    v, i = torch.topk(torch.cat(best_s, 1), k + 1, dim=1)
    ref_s = v.cpu().numpy()
    allowed = int(mask.sum().item())
    kk = min(k, allowed)
    s, p = s.cpu().numpy(), p.cpu().numpy()
    if kk == 0:
        return bool(np.all(p == -1))
    pos = torch.from_numpy(p[:, :kk]).to(shard.device)
    ok = bool(mask[pos].all().item())
    got64 = (q64[:, None, :] * shard[pos].double()).sum(-1).cpu().numpy()
    ok &= bool(np.abs(got64 - s[:, :kk]).max() <= 1e-5)
    ok &= bool(np.all(np.diff(got64, axis=1) <= 2e-6))
    # nothing outside the result beats its last score by more than the tie tolerance, and the k-th scores agree
    ok &= bool(np.all(np.abs(ref_s[:, kk - 1] - got64[:, -1]) <= 2e-6))
    ok &= bool(np.all(p[:, kk:] == -1))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from vietnamese_qa_system_amd.index import DeviceIndex

    dev = torch.device("cuda", 0)
    n, d, b, k = args.docs, args.dim, args.batch, args.k
    shard = build_shard(n, d, 1234, dev)
    index = DeviceIndex(shard, id_base=1, dtype="fp16", device=0)
    gq = torch.Generator(device=dev)
    gq.manual_seed(99)
    q = torch.randn((b, d), generator=gq, device=dev, dtype=torch.float32)
    q = (q / q.norm(dim=1, keepdim=True)).to(torch.float16)
    rng = np.random.default_rng(7)
    masks = {}
    masks["all"] = torch.ones(n, dtype=torch.bool, device=dev)
    for pct in (10, 1):
        m = torch.zeros(n, dtype=torch.bool, device=dev)
        lo = n // 3
        m[lo:lo + n * pct // 100] = True
        masks[f"contiguous_{pct}pct"] = m
    for name, frac in (("random_1pct", 0.01), ("random_0.01pct", 0.0001)):
        masks[name] = torch.from_numpy(rng.random(n) < frac).to(dev)
    legs = [("unfiltered", None, None), ("exact_paused", None, "pause")] + [(f"filter_{m}", m, None) for m in masks]
    out = {"shard": {"n": n, "d": d, "dtype": "fp16", "batch": b, "k": k, "steps": args.steps, "warmup": args.warmup}, "legs": {}}
    passes = -(-k // 12)
    for name, mname, mode in legs:
        rf = index.row_filter(mask=masks[mname]) if mname else None
        if mode == "pause":
            index.sketch_pause(1 << 30)

        def step():
            return index.search(q, k, return_positions=True, allow=rf)
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            s, i, p = step()
        e1.record()
        torch.cuda.synchronize(dev)
        ms = e0.elapsed_time(e1) / args.steps
        index.set_timing(True)
        for _ in range(args.warmup):
            step()
        kms, launches = index.get_timing()
        index.set_timing(False)
        kern = kms / args.warmup
        tiles = rf.tiles if rf is not None else (n + 255) // 256
        nbytes = tiles * 256 * d * 2 * (passes if rf is not None else 1)
        s, i, p = step()
        torch.cuda.synchronize(dev)
        mask = masks[mname] if mname else masks["all"]
        ok = check(shard, q[:8], mask, s[:8], p[:8], k)
        out["legs"][name] = {"ms_per_step": round(ms, 4), "scan_kernel_ms": round(kern, 4), "scan_launches_per_step": launches / args.warmup,
                             "allowed_rows": int(mask.sum().item()), "tiles_touched": tiles, "bytes_read": nbytes,
                             "gb_per_s": round(nbytes / (kern * 1e-3) / 1e9, 1) if kern > 0 and rf is not None else None, "oracle_ok": ok}
        if mode == "pause":
            index.sketch_pause(0)
    lg = out["legs"]
    out["all_rows_vs_exact_paused"] = round(lg["filter_all"]["ms_per_step"] / lg["exact_paused"]["ms_per_step"], 3)
    out["oracle_ok"] = all(v["oracle_ok"] for v in lg.values())
    print(json.dumps(out))
    index.close()
    return 0 if out["oracle_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
