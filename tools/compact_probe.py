#!/usr/bin/env python3
"""What list compaction buys on a table that saw deletes, through the
public GammaEngine API only.

One IVFPQ table (tools/nbits_compare.py's corpus) is timed in three
states: freshly built, after deleting a random share of its documents
(every list still carries the dead entries — what a search pays without
compaction), and after compact(min_ratio). Per state: the search step
and the scan stage (last_timing() "scan_us"), medians over the timed
steps after warm-up, plus the entries the lists hold. The post-delete
state is the baseline; the fresh state shows the run-to-run floor.

Also records the wall time and stats of the compact() call itself and
checks that the search results before and after it are identical.

Writes one JSON document to --out and echoes one JSON line per state.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle as orc  # noqa: E402
from vearch_amd import GammaEngine  # noqa: E402
from vearch_amd.engine import lib  # noqa: E402


def log(msg):
    print(f"[compact] {msg}", file=sys.stderr, flush=True)


def list_entries(eng, nlist):
    return int(sum(lib().GammaDebugGetList(eng.h, ln, None, None)
                   for ln in range(nlist)))


def timed(eng, nq, args):
    total_ms, scan_us = [], []
    for step in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        eng.search_cached(nq, args.k, nprobe=args.nprobe, rerank=args.rerank)
        dt = time.perf_counter() - t0
        if step >= args.warmup:
            total_ms.append(dt * 1e3)
            scan_us.append(eng.last_timing()["scan_us"])
    ms = float(np.median(total_ms))
    return {"scan_ms": round(float(np.median(scan_us)) / 1e3, 4),
            "scan_ms_min_max": [round(min(scan_us) / 1e3, 4),
                                round(max(scan_us) / 1e3, 4)],
            "ms_per_step": round(ms, 3),
            "qps": round(args.nq / ms * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db-size", type=int, default=2_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rerank", type=int, default=200)
    ap.add_argument("--delete-frac", type=float, default=0.4)
    ap.add_argument("--min-ratio", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/compact_probe.json")
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("--steps must be >= 5 (medians)")

    n, d = args.db_size, args.d
    t0 = time.time()
    base = orc.gen_clustered(n, d, seed=42, ncl=10000)
    queries = orc.gen_queries(base, args.nq, seed=43)
    log(f"data gen {time.time() - t0:.1f}s")

    t0 = time.time()
    train_n = min(n, max(160_000, 39 * args.nlist))
    eng = GammaEngine(path="/tmp/gamma_compact_probe")
    eng.create_table(
        d, "IVFPQ",
        '{"ncentroids": %d, "nsubvector": %d, "metric_type": "L2", '
        '"training_threshold": %d, "bucket_max_size": 12800000}'
        % (args.nlist, args.m, train_n))
    for s in range(0, n, 1_000_000):
        eng.add(base[s:s + 1_000_000])
    eng.build_index()
    log(f"build {time.time() - t0:.1f}s")
    nq = eng.cache_queries(queries)

    states = []

    def record(name, **extra):
        line = {"state": name, "list_entries": list_entries(eng, args.nlist)}
        line.update(timed(eng, nq, args))
        line.update(extra)
        print(json.dumps(line), flush=True)
        states.append(line)
        return line

    record("built", live=n)

    rng = np.random.default_rng(44)
    victims = rng.permutation(n)[:int(n * args.delete_frac)]
    t0 = time.time()
    for v in victims:
        if eng.delete_doc(str(int(v))) != 0:
            raise RuntimeError(f"delete_doc({v}) failed")
    delete_s = time.time() - t0
    live = n - len(victims)
    log(f"deleted {len(victims)} docs in {delete_s:.1f}s")
    deleted = record("deleted", live=live, delete_s=round(delete_s, 2))
    d0, i0 = eng.search_cached(nq, args.k, nprobe=args.nprobe,
                               rerank=args.rerank)

    t0 = time.perf_counter()
    stats = eng.compact(args.min_ratio)
    compact_ms = (time.perf_counter() - t0) * 1e3
    log(f"compact({args.min_ratio}) {compact_ms:.1f} ms {stats}")
    compacted = record("compacted", live=live)
    d1, i1 = eng.search_cached(nq, args.k, nprobe=args.nprobe,
                               rerank=args.rerank)
    life = eng.compact_stats()
    eng.close()

    entry_ratio = compacted["list_entries"] / deleted["list_entries"]
    scan_ratio = compacted["scan_ms"] / deleted["scan_ms"]
    doc = {
        "db_size": n, "d": d, "m": args.m, "nlist": args.nlist,
        "nq": args.nq, "nprobe": args.nprobe, "k": args.k,
        "rerank": args.rerank, "delete_frac": args.delete_frac,
        "min_ratio": args.min_ratio, "steps": args.steps,
        "warmup": args.warmup,
        "note": "medians over timed steps after warm-up, one engine, "
                "states in sequence; baseline = state 'deleted'",
        "states": states,
        "compact_call_ms": round(compact_ms, 2),
        "compact_call_stats": stats,
        "compact_lifetime_stats": life,
        "results_identical_across_compact":
            bool(np.array_equal(i0, i1) and np.array_equal(d0, d1)),
        "list_entries_ratio_compacted_over_deleted": round(entry_ratio, 4),
        "scan_ratio_compacted_over_deleted": round(scan_ratio, 4),
        "step_ratio_compacted_over_deleted":
            round(compacted["ms_per_step"] / deleted["ms_per_step"], 4),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    log(f"wrote {args.out}")


if __name__ == "__main__":
    main()
