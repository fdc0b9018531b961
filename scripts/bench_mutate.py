"""In-place updates of the headline shard: one JSON line.

    python scripts/bench_mutate.py [--docs 10000000] [--dim 768] [--steps 50] [--rounds 3] [--out FILE]

The shard is bench.py's (i.i.d. normal rows, L2-normalised, fp16, seed 1234; default sketch and row-major copy), created with room
for 100 000 more rows.  Legs, one after the other on the same handle: remove 1, 1 000 and 100 000 scattered rows, a contiguous run of
100 000, then append 1 000 and 100 000 rows into the capacity; and, for comparison, the only way to change an index without them:
a new handle created from the same device rows.  Per leg: wall ms of the call, device ms (events on the null stream around it), the
bytes it moves (moved rows read + written, dirty tiles re-cut) and an exact check of 8 queries (fp64 torch matmul over a device
mirror of the rows, moved by compaction_moves) with the leg's positions and ids.  Last, the search step (B = 256, k = 10) of the
mutated handle against a fresh handle of its rows, alternated over `rounds` rounds of `steps` steps.
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


def build_rows(n, d, seed, device, chunk=1 << 18):
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    buf = torch.empty((n, d), dtype=torch.float16, device=device)
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        x = torch.randn((c1 - c0, d), generator=gen, device=device, dtype=torch.float32)
        x /= x.norm(dim=1, keepdim=True)
        buf[c0:c1] = x.to(buf.dtype)
    return buf


def check(ix, rows, ids, q, k=10, chunk=1 << 20):
    """The handle's top-k of 8 queries against fp64 scores of the mirror rows: same ids (up to ties) and scores within 1e-5."""
    s, i, p = ix.search(q, k, return_positions=True)
    torch.cuda.synchronize()
    best_s, best_p = None, None
    qd = q.half().double()  # (the search scores the fp16-rounded queries)
    for c0 in range(0, rows.shape[0], chunk):
        sc = qd @ rows[c0:c0 + chunk].double().T
        v, j = sc.topk(min(k, sc.shape[1]), dim=1)
        j = j + c0
        if best_s is None:
            best_s, best_p = v, j
        else:
            v2, o = torch.cat([best_s, v], 1).topk(k, dim=1)
            best_s, best_p = v2, torch.cat([best_p, j], 1).gather(1, o)
    got = rows[p].double().mul(qd[:, None, :]).sum(-1)  # oracle score of every returned row
    ok = bool((got - s.double()).abs().max() <= 1e-5) and bool((got[:, -1] >= best_s[:, -1] - 2e-6).all())
    ok = ok and bool(torch.equal(ids[p], i)) and all(len(set(r)) == k for r in p.tolist())
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from vietnamese_qa_system_amd.index import DeviceIndex, compaction_moves
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, d = a.docs, a.dim
    cap = n + 100_000
    rows = build_rows(n, d, 1234, dev)
    extra = build_rows(101_000, d, 4321, dev)
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    gq = torch.Generator(device=dev)
    gq.manual_seed(99)
    q = torch.randn((256, d), generator=gq, device=dev)
    q /= q.norm(dim=1, keepdim=True)
    q8 = q[:8].contiguous()
    out = {"docs": n, "dim": d, "dtype": "fp16", "capacity": cap, "legs": {}}

    t0 = time.perf_counter()
    ix = DeviceIndex(rows, ids=ids, dtype="fp16", device=0, capacity=cap)
    torch.cuda.synchronize()
    out["create_s"] = round(time.perf_counter() - t0, 3)
    out["device_bytes"] = ix.device_bytes()
    out["sketch_scan"] = ix.launch_info(256, 10).sketch_scan
    row_bytes = ((d + 63) // 64 * 64) * 2
    tile_bytes = 256 * row_bytes

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - w0) * 1e3, e0.elapsed_time(e1)

    rng = np.random.default_rng(7)
    state = {"rows": rows, "ids": ids}

    def remove_leg(name, pos):
        nb = ix.n
        src, dst = compaction_moves(nb, pos)
        wall, devms = timed(lambda: ix.remove(pos))
        st, dt = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
        state["rows"][dt] = state["rows"][st]
        state["ids"][dt] = state["ids"][st]
        n1 = nb - len(pos)
        state["rows"], state["ids"] = state["rows"][:n1], state["ids"][:n1]
        dirty = len(set((dst >> 8).tolist()) | ({n1 >> 8} if n1 % 256 else set()))
        moved = int(dst.size)
        nbytes = 2 * moved * row_bytes * 2 + 2 * len(pos) * row_bytes + dirty * (tile_bytes + 256 * ((d + 127) // 128 * 128))
        out["legs"][name] = {"rows": int(len(pos)), "moved_rows": moved, "dirty_tiles": dirty, "wall_ms": round(wall, 3),
                             "device_ms": round(devms, 3), "bytes": nbytes, "gbs": round(nbytes / devms / 1e6, 1),
                             "check": check(ix, state["rows"], state["ids"], q8)}

    def append_leg(name, c):
        v = extra[:c]
        new_ids = torch.arange(10 ** 9, 10 ** 9 + c, dtype=torch.int64, device=dev)
        wall, devms = timed(lambda: ix.append(v, ids=new_ids))
        state["rows"] = torch.cat([state["rows"], v])
        state["ids"] = torch.cat([state["ids"], new_ids])
        out["legs"][name] = {"rows": c, "wall_ms": round(wall, 3), "device_ms": round(devms, 3),
                             "check": check(ix, state["rows"], state["ids"], q8)}

    remove_leg("remove_1_scattered", rng.choice(ix.n, 1, replace=False))
    remove_leg("remove_1000_scattered", rng.choice(ix.n, 1000, replace=False))
    remove_leg("remove_100000_scattered", rng.choice(ix.n, 100_000, replace=False))
    s0 = ix.n // 3
    remove_leg("remove_100000_contiguous", np.arange(s0, s0 + 100_000))
    append_leg("append_1000", 1000)
    append_leg("append_100000", 100_000)

    # the only way without in-place updates: a new handle from the same device rows
    fresh = None

    def rebuild():
        nonlocal fresh
        fresh = DeviceIndex(state["rows"], ids=state["ids"], dtype="fp16", device=0)
    wall, devms = timed(rebuild)
    out["legs"]["rebuild_from_device_rows"] = {"rows": int(state["rows"].shape[0]), "wall_ms": round(wall, 3), "device_ms": round(devms, 3),
                                               "check": check(fresh, state["rows"], state["ids"], q8)}
    r = out["legs"]
    out["remove_1000_vs_rebuild_device"] = round(r["rebuild_from_device_rows"]["device_ms"] / r["remove_1000_scattered"]["device_ms"], 1)
    out["remove_1000_vs_rebuild_wall"] = round(r["rebuild_from_device_rows"]["wall_ms"] / r["remove_1000_scattered"]["wall_ms"], 1)

    def step_ms(h):
        for _ in range(5):
            h.search(q, 10)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            h.search(q, 10)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    mut, frs = [], []
    for _ in range(a.rounds):
        mut.append(step_ms(ix))
        frs.append(step_ms(fresh))
    out["search_step_ms"] = {"mutated": [round(x, 4) for x in mut], "fresh": [round(x, 4) for x in frs],
                             "mutated_over_fresh": round(float(np.median(mut) / np.median(frs)), 4),
                             "sketch_scan": [ix.launch_info(256, 10).sketch_scan, fresh.launch_info(256, 10).sketch_scan],
                             "sketch_state": [ix.sketch_state(), fresh.sketch_state()]}
    out["all_checks_ok"] = all(v["check"] for v in out["legs"].values())
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ix.close()
    fresh.close()


if __name__ == "__main__":
    main()
