#!/usr/bin/env python3
"""IVFRABITQ next to the 8-bit IVFPQ ADC scan, through the public
GammaEngine API only.

One run builds two tables over the SAME float vectors (d = 128, L2), with
the same nlist and nprobe, plus a FLAT table for the exact ground truth:

  * IVFRABITQ, nb_bits = 1: the scan reads 4 B id + 24 B entry (16 B sign
    bits, A, Mul) + 4 B sval = 32 B per entry, one LDS lookup per nibble;
  * IVFPQ m = 32, 8-bit codes: 4 B id + 32 B code + 4 B S term = 40 B per
    entry, one LDS lookup per code byte.

Timed steps alternate between the tables (medians after warm-up), once with
recall_num = 0 (the scan selects k keys, no re-rank) and once with
recall_num = 100 (the scan selects 100 keys, the exact re-rank leg follows).
Recorded per table and recall_num: the stage times (coarse "assign", scan,
"post" = re-rank + final sort), recall@k against the FLAT table on the
first --gt-nq queries, and for the scan its effective byte rate = scanned
entries * bytes per entry / scan time (entries scanned per query = sum of
the probed lists' sizes, from the engine's own probes).

Writes one JSON document to --out and echoes one JSON line per table.
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

STAGES = ["h2d_us", "assign_us", "scan_us", "post_us", "d2h_us", "total_us"]
RECALL_NUMS = (0, 100)


def log(msg):
    print(f"[rbqprobe] {msg}", file=sys.stderr, flush=True)


def build(path, base, d, index_type, params):
    eng = GammaEngine(path=path)
    eng.create_table(d, index_type, params)
    for s in range(0, base.shape[0], 1_000_000):
        eng.add(base[s:s + 1_000_000])
    if index_type != "FLAT":
        eng.build_index()
    return eng


def scanned_per_query(eng, queries, nlist, nprobe):
    sizes = np.array([lib().GammaDebugGetList(eng.h, ln, None, None)
                      for ln in range(nlist)], dtype=np.int64)
    _, probes = eng.debug_coarse_assign(queries, nprobe)
    return float(sizes[probes].sum(axis=1).mean())


def recall_at(gt, ids, k):
    hits = sum(len(set(g.tolist()) & set(r[r >= 0].tolist()))
               for g, r in zip(gt[:, :k], ids[:, :k]))
    return hits / (gt.shape[0] * k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db-size", type=int, default=2_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--gt-nq", type=int, default=1000)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/rabitq_probe.json")
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("--steps must be >= 5 (medians)")
    n, d = args.db_size, args.d
    train_n = min(n, max(160_000, 39 * args.nlist))
    gt_nq = min(args.gt_nq, args.nq)

    t0 = time.time()
    base = orc.gen_clustered(n, d, seed=42, ncl=10000)
    q = orc.gen_queries(base, args.nq, seed=43)
    log(f"data gen {time.time() - t0:.1f}s")

    flat = build("/tmp/gamma_rbqprobe_flat", base, d, "FLAT",
                 '{"metric_type": "L2"}')
    _, gt = flat.raw_search(q[:gt_nq], args.k)
    flat.close()
    log("ground truth done")

    common = ('"ncentroids": %d, "metric_type": "L2", '
              '"training_threshold": %d, "bucket_max_size": 12800000'
              % (args.nlist, train_n))
    specs = [
        ("IVFRABITQ nb_bits=1 L2", "IVFRABITQ", '{%s, "nb_bits": 1}' % common,
         d // 8 + 8),
        ("IVFPQ m=%d 8-bit L2" % args.m, "IVFPQ",
         '{%s, "nsubvector": %d, "nbits_per_idx": 8}' % (common, args.m),
         args.m),
    ]
    tables = []
    for name, itype, params, code_bytes in specs:
        t0 = time.time()
        eng = build("/tmp/gamma_rbqprobe_" + itype, base, d, itype, params)
        tables.append({"table": name, "d": d, "code_bytes": code_bytes,
                       "scan_bytes_per_entry": 4 + code_bytes + 4,
                       "build_s": round(time.time() - t0, 1), "_eng": eng})
        log(f"built {name} {tables[-1]['build_s']}s")
    del base

    for t in tables:
        t["scanned_entries_per_query"] = round(scanned_per_query(
            t["_eng"], q, args.nlist, args.nprobe), 1)
        t["_nq"] = t["_eng"].cache_queries(q)
        t["_runs"] = {rn: {"stages": {s: [] for s in STAGES}, "ms": []}
                      for rn in RECALL_NUMS}
    for step in range(args.warmup + args.steps):
        for rn in RECALL_NUMS:
            for t in tables:  # alternate the tables
                t0 = time.perf_counter()
                t["_eng"].search_cached(t["_nq"], args.k, nprobe=args.nprobe,
                                        rerank=rn)
                dt = time.perf_counter() - t0
                if step >= args.warmup:
                    run = t["_runs"][rn]
                    run["ms"].append(dt * 1e3)
                    lt = t["_eng"].last_timing()
                    for s in STAGES:
                        run["stages"][s].append(lt[s])
    for t in tables:
        t["runs"] = []
        for rn in RECALL_NUMS:
            run = t["_runs"][rn]
            r = {"recall_num": rn}
            for s in STAGES:
                r[s.replace("_us", "_ms")] = round(
                    float(np.median(run["stages"][s])) / 1e3, 4)
            sc = run["stages"]["scan_us"]
            r["scan_ms_min_max"] = [round(min(sc) / 1e3, 4),
                                    round(max(sc) / 1e3, 4)]
            r["ms_per_step"] = round(float(np.median(run["ms"])), 3)
            scanned = t["scanned_entries_per_query"] * args.nq
            r["scan_gbytes_per_s"] = round(
                scanned * t["scan_bytes_per_entry"] / (r["scan_ms"] * 1e-3)
                / 1e9, 1)
            r["scan_gentries_per_s"] = round(
                scanned / (r["scan_ms"] * 1e-3) / 1e9, 2)
            _, ids = t["_eng"].raw_search(q[:gt_nq], args.k,
                                          nprobe=args.nprobe, rerank=rn)
            r["recall_at_k"] = round(recall_at(gt, ids, args.k), 4)
            t["runs"].append(r)
        t["_eng"].close()
        for key in [k for k in t if k.startswith("_")]:
            del t[key]
        print(json.dumps(t), flush=True)

    rb, pq = tables
    ratios = {str(rn): round(a["scan_gbytes_per_s"] / b["scan_gbytes_per_s"],
                             4)
              for rn, a, b in zip(RECALL_NUMS, rb["runs"], pq["runs"])}
    doc = {
        "db_size": n, "d": d, "nlist": args.nlist, "nq": args.nq,
        "gt_nq": gt_nq, "nprobe": args.nprobe, "k": args.k,
        "steps": args.steps, "warmup": args.warmup,
        "note": "medians over alternating timed steps; byte rate = scanned "
                "entries * bytes per entry / scan time; recall against a "
                "FLAT table over the same vectors",
        "results": tables,
        "byte_rate_ratio_rabitq_over_ivfpq8": ratios,
        "entry_rate_ratio_rabitq_over_ivfpq8": {
            str(rn): round(a["scan_gentries_per_s"]
                           / b["scan_gentries_per_s"], 4)
            for rn, a, b in zip(RECALL_NUMS, rb["runs"], pq["runs"])},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    log(f"wrote {args.out}")


if __name__ == "__main__":
    main()
