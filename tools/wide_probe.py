#!/usr/bin/env python3
"""The sliced-table 8-bit IVFPQ scan (k_ivfpq_scan_wide) against the
resident-table scan and the 4-bit scan on one d = 768 corpus, through the
public GammaEngine API only.

Rows (one run, all tables resident, timed steps alternating):
  M = 96,  8-bit, resident-table kernel (the baseline)
  M = 96,  8-bit, the same table forced onto the sliced kernel
           (GAMMA_SCAN_WIDE=1, read per launch)
  M = 192, 8-bit, sliced kernel
  M = 384, 8-bit, sliced kernel
  M = 384, 4-bit, the 4-bit kernel at 192 B per entry

Per row: the scan-stage time (last_timing() "scan_us", median over the
timed steps after warm-up; it includes the query-table build the launch
needs), the code bytes the scan walks per second (entries of the probed
lists x code bytes / scan time), and recall@10 against fp64 brute force on
a query subset, before and after the exact re-rank.

Writes one JSON document to --out and echoes one JSON line per row.
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

# (m, nbits, force_wide, kernel); rows sharing (m, nbits) share a table
ROWS = [(96, 8, False, "resident"), (96, 8, True, "wide (forced)"),
        (192, 8, False, "wide"), (384, 8, False, "wide"),
        (384, 4, False, "4-bit")]


def log(msg):
    print(f"[wide] {msg}", file=sys.stderr, flush=True)


class forced:
    """GAMMA_SCAN_WIDE=1 for the duration of a block (or nothing)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if self.on:
            os.environ["GAMMA_SCAN_WIDE"] = "1"

    def __exit__(self, *a):
        os.environ.pop("GAMMA_SCAN_WIDE", None)


def build(base, d, nlist, m, nbits, train_n):
    eng = GammaEngine(path=f"/tmp/gamma_wide_m{m}_b{nbits}")
    eng.create_table(
        d, "IVFPQ",
        '{"ncentroids": %d, "nsubvector": %d, "nbits_per_idx": %d, '
        '"metric_type": "L2", "training_threshold": %d, '
        '"bucket_max_size": 12800000}' % (nlist, m, nbits, train_n))
    for s in range(0, base.shape[0], 100_000):
        eng.add(base[s:s + 100_000])
    eng.build_index()
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db-size", type=int, default=400_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=2000)
    ap.add_argument("--nq-gt", type=int, default=200)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rerank", type=int, default=200)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/ivfpq_wide_probe.json")
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("--steps must be >= 5 (medians)")

    n, d = args.db_size, args.d
    t0 = time.time()
    base = orc.gen_clustered(n, d, seed=42, ncl=2000)
    queries = orc.gen_queries(base, args.nq, seed=43)
    log(f"data gen {time.time() - t0:.1f}s")
    t0 = time.time()
    _, gti = orc.flat_topk_f64(base, queries[:args.nq_gt], args.k, block=50)
    log(f"fp64 ground truth ({args.nq_gt} queries) {time.time() - t0:.1f}s")

    train_n = min(n, 39 * args.nlist)
    engines, lines = {}, []
    for m, nbits, force, kernel in ROWS:
        t0 = time.time()
        if (m, nbits) not in engines:
            engines[(m, nbits)] = build(base, d, args.nlist, m, nbits,
                                        train_n)
        eng = engines[(m, nbits)]
        code_bytes = m * nbits // 8
        line = {"m": m, "nbits": nbits, "kernel": kernel,
                "build_s": round(time.time() - t0, 1),
                "code_bytes": code_bytes}
        with forced(force):
            for key, rr in (("recall_at_10_no_rerank", 0),
                            ("recall_at_10_rerank", args.rerank)):
                _, gi = eng.raw_search(queries[:args.nq_gt], args.k,
                                       nprobe=args.nprobe, rerank=rr)
                line[key] = round(orc.recall_at(gti, gi, args.k), 4)
        # entries the scan walks for the timed batch
        sizes = np.array([len(eng.debug_list(ln, code_bytes)[0])
                          for ln in range(args.nlist)], dtype=np.int64)
        _, probes = eng.debug_coarse_assign(queries, args.nprobe)
        ok = (probes >= 0) & (probes < args.nlist)
        line["entries_scanned"] = int(sizes[probes[ok]].sum())
        log(f"ready {line}")
        lines.append(line)

    nq = {key: eng.cache_queries(queries) for key, eng in engines.items()}
    scan_us = [[] for _ in ROWS]
    for step in range(args.warmup + args.steps):
        for i, (m, nbits, force, _) in enumerate(ROWS):  # alternate
            eng = engines[(m, nbits)]
            with forced(force):
                eng.search_cached(nq[(m, nbits)], args.k,
                                  nprobe=args.nprobe, rerank=args.rerank)
            if step >= args.warmup:
                scan_us[i].append(eng.last_timing()["scan_us"])
    for i, line in enumerate(lines):
        ms = float(np.median(scan_us[i])) / 1e3
        line["scan_ms"] = round(ms, 4)
        line["scan_ms_min_max"] = [round(min(scan_us[i]) / 1e3, 4),
                                   round(max(scan_us[i]) / 1e3, 4)]
        line["code_gb_per_s"] = round(
            line["entries_scanned"] * line["code_bytes"] / ms / 1e6, 2)
        print(json.dumps(line), flush=True)
    for eng in engines.values():
        eng.close()

    doc = {
        "db_size": n, "d": d, "nlist": args.nlist, "nq": args.nq,
        "nq_gt": args.nq_gt, "nprobe": args.nprobe, "k": args.k,
        "rerank": args.rerank, "steps": args.steps, "warmup": args.warmup,
        "note": "medians over alternating timed steps; scan_ms includes "
                "the query-table build of launches that read one; recall "
                "vs fp64 exact brute force (numpy host)",
        "results": lines,
        "forced_wide_over_resident_m96":
            round(lines[1]["scan_ms"] / lines[0]["scan_ms"], 4),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    log(f"wrote {args.out}")


if __name__ == "__main__":
    main()
