#!/usr/bin/env python3
"""8-bit vs 4-bit IVFPQ codes on one corpus, through the public
GammaEngine API only.

Builds three tables over the same clustered corpus — (m=32, nbits=8),
(m=32, nbits=4), (m=64, nbits=4) — and records per table: the scan-stage
time (last_timing() "scan_us"), total ms per step and QPS (medians over
the timed steps, after warm-up), recall@10 with and without the exact
rerank against fp64 ground truth on a fixed query subset, and the bytes
the scan reads per entry (4 B id + code + 4 B S term).

All three engines are resident at once and the timed steps alternate
between them, so the 8-bit line is a same-run baseline under the same
machine conditions. m=32/4-bit vs m=32/8-bit is the equal-M comparison
(same table rows, half the code bytes); m=64/4-bit vs m=32/8-bit is the
equal-bytes comparison.

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

CONFIGS = [(32, 8), (32, 4), (64, 4)]  # (m, nbits); first = baseline


def log(msg):
    print(f"[nbits] {msg}", file=sys.stderr, flush=True)


def build(base, d, nlist, m, nbits, train_n):
    eng = GammaEngine(path=f"/tmp/gamma_nbits_m{m}_b{nbits}")
    eng.create_table(
        d, "IVFPQ",
        '{"ncentroids": %d, "nsubvector": %d, "nbits_per_idx": %d, '
        '"metric_type": "L2", "training_threshold": %d, '
        '"bucket_max_size": 12800000}' % (nlist, m, nbits, train_n))
    for s in range(0, base.shape[0], 1_000_000):
        eng.add(base[s:s + 1_000_000])
    eng.build_index()
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db-size", type=int, default=2_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--nq-gt", type=int, default=1000)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rerank", type=int, default=200)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/nbits4_compare.json")
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("--steps must be >= 5 (medians)")

    n, d = args.db_size, args.d
    t0 = time.time()
    base = orc.gen_clustered(n, d, seed=42, ncl=10000)
    queries = orc.gen_queries(base, args.nq, seed=43)
    log(f"data gen {time.time() - t0:.1f}s")
    t0 = time.time()
    _, gti = orc.flat_topk_f64(base, queries[:args.nq_gt], args.k, block=125)
    log(f"fp64 ground truth ({args.nq_gt} queries) {time.time() - t0:.1f}s")

    train_n = min(n, max(160_000, 39 * args.nlist))
    engines, lines = [], []
    for m, nbits in CONFIGS:
        t0 = time.time()
        eng = build(base, d, args.nlist, m, nbits, train_n)
        line = {"m": m, "nbits": nbits, "build_s": round(time.time() - t0, 1),
                "code_bytes": m * nbits // 8,
                "scan_bytes_per_entry": 4 + m * nbits // 8 + 4}
        for key, rr in (("recall_at_10_no_rerank", 0),
                        ("recall_at_10_rerank", args.rerank)):
            _, gi = eng.raw_search(queries[:args.nq_gt], args.k,
                                   nprobe=args.nprobe, rerank=rr)
            line[key] = round(orc.recall_at(gti, gi, args.k), 4)
        log(f"built {line}")
        engines.append(eng)
        lines.append(line)

    nq = [eng.cache_queries(queries) for eng in engines]
    scan_us = [[] for _ in engines]
    total_ms = [[] for _ in engines]
    for step in range(args.warmup + args.steps):
        for i, eng in enumerate(engines):  # alternate the tables
            t0 = time.perf_counter()
            eng.search_cached(nq[i], args.k, nprobe=args.nprobe,
                              rerank=args.rerank)
            dt = time.perf_counter() - t0
            if step >= args.warmup:
                total_ms[i].append(dt * 1e3)
                scan_us[i].append(eng.last_timing()["scan_us"])
    for i, line in enumerate(lines):
        ms = float(np.median(total_ms[i]))
        line["scan_ms"] = round(float(np.median(scan_us[i])) / 1e3, 4)
        line["scan_ms_min_max"] = [round(min(scan_us[i]) / 1e3, 4),
                                   round(max(scan_us[i]) / 1e3, 4)]
        line["ms_per_step"] = round(ms, 3)
        line["qps"] = round(args.nq / ms * 1e3, 1)
        print(json.dumps(line), flush=True)
    for eng in engines:
        eng.close()

    base8, eq_m, eq_b = lines
    doc = {
        "db_size": n, "d": d, "nlist": args.nlist, "nq": args.nq,
        "nq_gt": args.nq_gt, "nprobe": args.nprobe, "k": args.k,
        "rerank": args.rerank, "steps": args.steps, "warmup": args.warmup,
        "note": "medians over alternating timed steps; recall vs fp64 "
                "exact brute force (numpy host)",
        "results": lines,
        "equal_m_scan_ratio_4bit_over_8bit":
            round(eq_m["scan_ms"] / base8["scan_ms"], 4),
        "equal_m_condition_met_within_5pct":
            eq_m["scan_ms"] <= 1.05 * base8["scan_ms"],
        "equal_bytes_scan_ratio_m64_4bit_over_m32_8bit":
            round(eq_b["scan_ms"] / base8["scan_ms"], 4),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    log(f"wrote {args.out}")


if __name__ == "__main__":
    main()
