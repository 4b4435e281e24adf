#!/usr/bin/env python3
"""IVFRABITQ next to the 8-bit IVFPQ ADC scan, through the public
GammaEngine API only.

One run builds two tables over the SAME float vectors (d = 128, L2), with
the same nlist and nprobe, plus a FLAT table for the exact ground truth:

  * IVFRABITQ, nb_bits = 1: the scan reads 4 B id + 24 B entry (16 B sign
    bits, A, Mul) + 4 B sval = 32 B per entry, one LDS lookup per nibble;
    --nb-bits 1,4,8 adds a table per further width (d * nb_bits / 8 + 8 B
    entries, the table-free scan) to the same run;
  * IVFPQ m = 32, 8-bit codes: 4 B id + 32 B code + 4 B S term = 40 B per
    entry, one LDS lookup per code byte.

Timed steps alternate between the tables (medians after warm-up), once with
recall_num = 0 (the scan selects k keys, no re-rank) and once with
recall_num = 100 (the scan selects 100 keys, the exact re-rank leg follows);
--recall-num takes other values in its place, several in one run, e.g.
1024,2048,8192 to time the deep top-k path (IVFRABITQ only: the IVFPQ table
sits out the values beyond 1024) next to the 1024 one.
Recorded per table and recall_num: the stage times (coarse "assign", scan,
"post" = re-rank + final sort), recall@k against the FLAT table on the
first --gt-nq queries, and for the scan its effective byte rate = scanned
entries * bytes per entry / scan time (entries scanned per query = sum of
the probed lists' sizes, from the engine's own probes).

Every IVFRABITQ table records whether its scan takes the tiled entry
movement (gk::rabitq_scan_is_tiled). --tiled-ab times each nb_bits 4 / 8
table a second time, in the same alternation, with GAMMA_RBQ_TILED set
against the default: 0 (streamed) where the default is tiled, 1 (tiled)
where the entry is register-resident. Such runs carry "tiled_knob".

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
from vearch_amd import GammaEngine, ktest  # noqa: E402
from vearch_amd.engine import lib  # noqa: E402

STAGES = ["h2d_us", "assign_us", "scan_us", "post_us", "d2h_us", "total_us"]


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
    ap.add_argument("--nb-bits", default="1",
                    help="comma-separated IVFRABITQ code widths (1, 4, 8): "
                         "one table each, all timed in the same run")
    ap.add_argument("--recall-num", default="100",
                    help="comma-separated recall_num values timed next to "
                         "recall_num = 0 (up to 8192; beyond 1024 IVFRABITQ "
                         "only)")
    ap.add_argument("--tiled-ab", action="store_true",
                    help="time the nb_bits 4 / 8 tables under the opposite "
                         "GAMMA_RBQ_TILED too")
    ap.add_argument("--out", default="profiles/rabitq_probe.json")
    args = ap.parse_args()
    recall_nums = (0,) + tuple(int(r) for r in args.recall_num.split(","))
    if any(not 0 < r <= 8192 for r in recall_nums[1:]):
        ap.error("--recall-num takes values in 1..8192")
    widths = [int(b) for b in args.nb_bits.split(",")]
    if not widths or any(b not in (1, 4, 8) for b in widths):
        ap.error("--nb-bits takes 1, 4 and 8")
    if args.steps < 5:
        ap.error("--steps must be >= 5 (medians)")
    if "GAMMA_RBQ_TILED" in os.environ:
        ap.error("unset GAMMA_RBQ_TILED: the probe sets it per run")
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
    specs = [("IVFRABITQ nb_bits=%d L2" % b, "IVFRABITQ",
              '{%s, "nb_bits": %d}' % (common, b), d * b // 8 + 8, b)
             for b in widths] + [
        ("IVFPQ m=%d 8-bit L2" % args.m, "IVFPQ",
         '{%s, "nsubvector": %d, "nbits_per_idx": 8}' % (common, args.m),
         args.m, 0),
    ]
    tables = []
    for name, itype, params, code_bytes, nb in specs:
        t0 = time.time()
        wide = itype == "IVFRABITQ" and code_bytes != d // 8 + 8
        eng = build("/tmp/gamma_rbqprobe_" + itype
                    + ("_%d" % code_bytes if wide else ""), base, d, itype,
                    params)
        tables.append({"table": name, "d": d, "code_bytes": code_bytes,
                       "scan_bytes_per_entry": 4 + code_bytes + 4,
                       "build_s": round(time.time() - t0, 1), "_eng": eng})
        # the knobs this table is timed under: None = the environment's
        tables[-1]["_knobs"] = [None]
        if nb:
            tiled = ktest.rabitq_scan_is_tiled(nb, d)
            tables[-1]["scan_tiled"] = tiled
            if args.tiled_ab and nb > 1:
                tables[-1]["_knobs"].append("0" if tiled else "1")
        log(f"built {name} {tables[-1]['build_s']}s")
    del base

    for t in tables:
        t["scanned_entries_per_query"] = round(scanned_per_query(
            t["_eng"], q, args.nlist, args.nprobe), 1)
        t["_nq"] = t["_eng"].cache_queries(q)
        t["_runs"] = {(rn, kn): {"stages": {s: [] for s in STAGES}, "ms": []}
                      for rn in recall_nums for kn in t["_knobs"]
                      if rn <= 1024 or t["table"].startswith("IVFRABITQ")}

    def search(t, rn, kn, fn):  # the knob is read at every launch
        if kn is not None:
            os.environ["GAMMA_RBQ_TILED"] = kn
        try:
            return fn(rn)
        finally:
            os.environ.pop("GAMMA_RBQ_TILED", None)

    for step in range(args.warmup + args.steps):
        for rn in recall_nums:
            for t, kn in [(t, kn) for kn in (None, "0", "1")
                          for t in tables]:  # alternate the tables
                if (rn, kn) not in t["_runs"]:
                    continue
                t0 = time.perf_counter()
                search(t, rn, kn, lambda rn: t["_eng"].search_cached(
                    t["_nq"], args.k, nprobe=args.nprobe, rerank=rn))
                dt = time.perf_counter() - t0
                if step >= args.warmup:
                    run = t["_runs"][(rn, kn)]
                    run["ms"].append(dt * 1e3)
                    lt = t["_eng"].last_timing()
                    for s in STAGES:
                        run["stages"][s].append(lt[s])
    for t in tables:
        t["runs"] = []
        for (rn, kn), run in t["_runs"].items():
            r = {"recall_num": rn}
            if kn is not None:
                r["tiled_knob"] = int(kn)
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
            _, ids = search(t, rn, kn, lambda rn: t["_eng"].raw_search(
                q[:gt_nq], args.k, nprobe=args.nprobe, rerank=rn))
            r["recall_at_k"] = round(recall_at(gt, ids, args.k), 4)
            t["runs"].append(r)
        t["_eng"].close()
        for key in [k for k in t if k.startswith("_")]:
            del t[key]
        print(json.dumps(t), flush=True)

    rb, pq = tables[0], tables[-1]

    def ratio(key, ta, tb):  # per recall_num that both tables ran
        rb_ = {r["recall_num"]: r for r in tb["runs"]
               if "tiled_knob" not in r}
        return {str(r["recall_num"]) + ("" if "tiled_knob" not in r else
                                        " tiled_knob=%d" % r["tiled_knob"]):
                round(r[key] / rb_[r["recall_num"]][key], 4)
                for r in ta["runs"] if r["recall_num"] in rb_}

    ratios = ratio("scan_gbytes_per_s", rb, pq)
    doc = {
        "db_size": n, "d": d, "nlist": args.nlist, "nq": args.nq,
        "gt_nq": gt_nq, "nprobe": args.nprobe, "k": args.k,
        "steps": args.steps, "warmup": args.warmup,
        "note": "medians over alternating timed steps; byte rate = scanned "
                "entries * bytes per entry / scan time; recall against a "
                "FLAT table over the same vectors",
        "results": tables,
        "byte_rate_ratio_rabitq_over_ivfpq8": ratios,
        "entry_rate_ratio_rabitq_over_ivfpq8":
            ratio("scan_gentries_per_s", rb, pq),
    }
    if len(widths) > 1:  # the wider codes against the first width given
        doc["byte_rate_ratio_over_nb_bits_%d" % widths[0]] = {
            t["table"]: ratio("scan_gbytes_per_s", t, rb)
            for t in tables[1:-1]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    log(f"wrote {args.out}")


if __name__ == "__main__":
    main()
