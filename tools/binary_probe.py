#!/usr/bin/env python3
"""BINARYIVF Hamming scan next to the 8-bit IVFPQ ADC scan, through the
public GammaEngine API only.

Two tables, both resident, timed steps alternating (medians after
warm-up), one process:

  * BINARYIVF, d = 256 bits: the scan reads 4 B id + 32 B code = 36 B per
    entry, one xor + popcount per word;
  * tools/nbits_compare.py's baseline IVFPQ table (d = 128, m = 32, 8-bit
    codes, L2): 4 B id + 32 B code + 4 B S term = 40 B per entry, one LDS
    table gather per code byte.

Both run the same nlist / nprobe / nq / k with no rerank leg, so the scan
stage (last_timing() "scan_us") selects the same k2 = k keys. Recorded per
table: the per-stage times, the entries scanned per query (sum of the
probed lists' sizes, from the engine's own probes), and the scan's
effective byte rate = entries * bytes-per-entry / scan time. The coarse
stage ("assign_us": Hamming matrix + select vs float GEMM + select) sits
in the same lines.

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


def log(msg):
    print(f"[binprobe] {msg}", file=sys.stderr, flush=True)


def gen_binary(n, d, seed, ncl=10000, flip=0.10, chunk=100_000):
    """cluster centres with ~10 % of the bits flipped per point, packed
    LSB-first into (n, d/8) uint8"""
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 2, size=(ncl, d), dtype=np.uint8)
    out = np.empty((n, d // 8), dtype=np.uint8)
    for s in range(0, n, chunk):
        m = min(chunk, n - s)
        bits = centres[rng.integers(0, ncl, size=m)]
        bits ^= (rng.random((m, d), dtype=np.float32) < flip).astype(np.uint8)
        out[s:s + m] = np.packbits(bits, axis=1, bitorder="little")
    return out


def build(path, base, d, index_type, params):
    eng = GammaEngine(path=path)
    eng.create_table(d, index_type, params)
    for s in range(0, base.shape[0], 1_000_000):
        eng.add(base[s:s + 1_000_000])
    eng.build_index()
    return eng


def scanned_per_query(eng, queries, nlist, nprobe):
    sizes = np.array([lib().GammaDebugGetList(eng.h, ln, None, None)
                      for ln in range(nlist)], dtype=np.int64)
    _, probes = eng.debug_coarse_assign(queries, nprobe)
    return float(sizes[probes].sum(axis=1).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db-size", type=int, default=2_000_000)
    ap.add_argument("--bits", type=int, default=256)
    ap.add_argument("--d-float", type=int, default=128)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/binaryivf_probe.json")
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("--steps must be >= 5 (medians)")
    n = args.db_size
    train_n = min(n, max(160_000, 39 * args.nlist))

    tables = []
    t0 = time.time()
    bbase = gen_binary(n, args.bits, seed=42)
    rng = np.random.default_rng(43)
    bq = bbase[rng.integers(0, n, size=args.nq)].copy()
    bq ^= np.packbits(rng.random((args.nq, args.bits)) < 0.05, axis=1,
                      bitorder="little")
    log(f"binary data gen {time.time() - t0:.1f}s")
    t0 = time.time()
    eng = build("/tmp/gamma_binprobe_bin", bbase, args.bits, "BINARYIVF",
                '{"ncentroids": %d, "training_threshold": %d, '
                '"bucket_max_size": 12800000}' % (args.nlist, train_n))
    tables.append({"table": "BINARYIVF", "d": args.bits,
                   "code_bytes": args.bits // 8,
                   "scan_bytes_per_entry": 4 + args.bits // 8,
                   "build_s": round(time.time() - t0, 1),
                   "_eng": eng, "_q": bq})
    log(f"built BINARYIVF {tables[-1]['build_s']}s")
    del bbase

    t0 = time.time()
    fbase = orc.gen_clustered(n, args.d_float, seed=42, ncl=10000)
    fq = orc.gen_queries(fbase, args.nq, seed=43)
    log(f"float data gen {time.time() - t0:.1f}s")
    t0 = time.time()
    eng = build("/tmp/gamma_binprobe_pq", fbase, args.d_float, "IVFPQ",
                '{"ncentroids": %d, "nsubvector": %d, "nbits_per_idx": 8, '
                '"metric_type": "L2", "training_threshold": %d, '
                '"bucket_max_size": 12800000}'
                % (args.nlist, args.m, train_n))
    tables.append({"table": "IVFPQ m=%d 8-bit L2" % args.m,
                   "d": args.d_float, "code_bytes": args.m,
                   "scan_bytes_per_entry": 4 + args.m + 4,
                   "build_s": round(time.time() - t0, 1),
                   "_eng": eng, "_q": fq})
    log(f"built IVFPQ {tables[-1]['build_s']}s")
    del fbase

    for t in tables:
        t["scanned_entries_per_query"] = round(scanned_per_query(
            t["_eng"], t["_q"], args.nlist, args.nprobe), 1)
        t["_nq"] = t["_eng"].cache_queries(t["_q"])
        t["_stages"] = {s: [] for s in STAGES}
        t["_ms"] = []
    for step in range(args.warmup + args.steps):
        for t in tables:  # alternate the tables
            t0 = time.perf_counter()
            t["_eng"].search_cached(t["_nq"], args.k, nprobe=args.nprobe)
            dt = time.perf_counter() - t0
            if step >= args.warmup:
                t["_ms"].append(dt * 1e3)
                lt = t["_eng"].last_timing()
                for s in STAGES:
                    t["_stages"][s].append(lt[s])
    for t in tables:
        for s in STAGES:
            t[s.replace("_us", "_ms")] = round(
                float(np.median(t["_stages"][s])) / 1e3, 4)
        sc = t["_stages"]["scan_us"]
        t["scan_ms_min_max"] = [round(min(sc) / 1e3, 4),
                                round(max(sc) / 1e3, 4)]
        t["ms_per_step"] = round(float(np.median(t["_ms"])), 3)
        t["qps"] = round(args.nq / t["ms_per_step"] * 1e3, 1)
        scanned = t["scanned_entries_per_query"] * args.nq
        t["scan_gbytes_per_s"] = round(
            scanned * t["scan_bytes_per_entry"] / (t["scan_ms"] * 1e-3) / 1e9,
            1)
        t["scan_gentries_per_s"] = round(
            scanned / (t["scan_ms"] * 1e-3) / 1e9, 2)
        t["_eng"].close()
        for key in [k for k in t if k.startswith("_")]:
            del t[key]
        print(json.dumps(t), flush=True)

    b, p = tables
    ratio = b["scan_gbytes_per_s"] / p["scan_gbytes_per_s"]
    doc = {
        "db_size": n, "nlist": args.nlist, "nq": args.nq,
        "nprobe": args.nprobe, "k": args.k, "steps": args.steps,
        "warmup": args.warmup,
        "note": "medians over alternating timed steps, no rerank leg; "
                "byte rate = scanned entries * bytes per entry / scan time",
        "results": tables,
        "byte_rate_ratio_binary_over_ivfpq8": round(ratio, 4),
        "binary_within_5pct_of_ivfpq8_byte_rate": ratio >= 0.95,
        "coarse_ms_hamming_vs_float": [b["assign_ms"], p["assign_ms"]],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    log(f"wrote {args.out}")


if __name__ == "__main__":
    main()
