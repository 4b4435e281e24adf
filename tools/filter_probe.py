"""Filtered-search timing probe (SURVEY §8f-2 perf evidence; round-2
plan item 4). Uses only the validated product path: docs with a scalar
tag field, protobuf Search with a term filter at several selectivities,
wall-clock per batch. Run on a GPU box:

    python tools/filter_probe.py
    python tools/filter_probe.py --filter-first profiles/filter_first.json
"""
import os
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oracle as orc  # noqa: E402
from vearch_amd import GammaEngine, fbsenc  # noqa: E402


def main():
    n, d = 400_000, 64
    base = orc.gen_clustered(n, d, seed=42, ncl=2000)
    eng = GammaEngine(path="/tmp/gamma_filterprobe")
    eng.create_table(
        d, "IVFPQ",
        '{"ncentroids": 512, "nsubvector": 16, "metric_type": "L2", '
        '"training_threshold": 80000}',
        scalar_fields=[("tag", fbsenc.DATA_INT)])
    t0 = time.time()
    for vid in range(n):
        eng.add_doc(str(vid), base[vid],
                    fields=[("tag", struct.pack("<i", vid % 1000),
                             fbsenc.DATA_INT)])
    print(f"ingest {n} docs with tags: {time.time() - t0:.1f}s")
    eng.build_index()
    q = orc.gen_queries(base, 64, seed=5)

    def timed(label, **kw):
        eng.search_pb(q, topn=10, **kw)  # warm (also builds the index)
        ts = []
        for _ in range(10):
            t = time.time()
            eng.search_pb(q, topn=10, **kw)
            ts.append((time.time() - t) * 1e3)
        ts.sort()
        print(f"{label:42s} p50={ts[5]:7.2f} ms/64q "
              f"({64 / (ts[5] / 1e3):8.0f} QPS)")

    timed("unfiltered")
    # term filter: 1/1000 of docs match
    timed("term filter (0.1% selectivity)",
          term_filters=[("tag", b"\x07\x00\x00\x00")])
    # range filters at three selectivities
    for lo, hi, lbl in ((0, 9, "1%"), (0, 99, "10%"), (0, 499, "50%")):
        timed(f"range filter ({lbl} selectivity)",
              range_filters=[("tag", struct.pack("<i", lo),
                              struct.pack("<i", hi), True, True)])
    eng.close()


def filter_first_probe(out_path, steps=9):
    """The same range-filtered request with `filter_first` on and off,
    alternating in one process, on an IVFPQ and a FLAT table of the data
    above. Per (table, selectivity, mode): medians and min-max over `steps`
    of the scan time (last_timing scan_us) and the wall step time of one
    64-query protobuf Search, results per query, and recall@10 against the
    fp64 top-10 of the matching docs."""
    import json

    import numpy as np

    n, d, nq, k = 400_000, 64, 64, 10
    base = orc.gen_clustered(n, d, seed=42, ncl=2000)
    q = orc.gen_queries(base, nq, seed=5)
    tags = np.arange(n) % 1000
    widths = (1, 10, 20, 50, 100, 200, 500)  # of 1000 tags: 0.1 % .. 50 %
    truth = {w: np.flatnonzero(tags < w) for w in widths}
    truth = {w: m[orc.flat_topk_f64(base[m], q, k)[1]]
             for w, m in truth.items()}
    tables = {
        "IVFPQ": '{"ncentroids": 512, "nsubvector": 16, "metric_type": "L2", '
                 '"training_threshold": 80000}',
        "FLAT": '{"metric_type": "L2"}',
    }
    rows = []
    for kind, params in tables.items():
        eng = GammaEngine(path="/tmp/gamma_ffprobe_" + kind)
        eng.create_table(d, kind, params,
                         scalar_fields=[("tag", fbsenc.DATA_INT)])
        for vid in range(n):
            eng.add_doc(str(vid), base[vid],
                        fields=[("tag", struct.pack("<i", int(tags[vid])),
                                 fbsenc.DATA_INT)])
        eng.build_index()
        for w in widths:
            rf = [("tag", struct.pack("<i", 0), struct.pack("<i", w - 1),
                   True, True)]
            modes = {"off": '{"nprobe": 32}',
                     "on": '{"nprobe": 32, "filter_first": 1048576}'}
            acc = {m: {"scan_us": [], "step_ms": []} for m in modes}
            for m, ip in modes.items():  # warm both paths
                eng.search_pb(q, topn=k, index_params=ip, range_filters=rf)
            for _ in range(steps):
                for m, ip in modes.items():
                    t = time.perf_counter()
                    res = eng.search_pb(q, topn=k, index_params=ip,
                                        range_filters=rf)
                    acc[m]["step_ms"].append((time.perf_counter() - t) * 1e3)
                    acc[m]["scan_us"].append(eng.last_timing()["scan_us"])
                    acc[m]["res"] = res
            for m in modes:
                ids = [[int(it["fields"]["_id"]) for it in r["items"]]
                       for r in acc[m]["res"]]
                hit = sum(len(set(g.tolist()) & set(r))
                          for g, r in zip(truth[w], ids))
                row = {"table": kind, "candidates": n * w // 1000,
                       "filter_first": m, "steps": steps,
                       "results_per_query": sum(map(len, ids)) / nq,
                       "recall_at_10": hit / (nq * k)}
                for key in ("scan_us", "step_ms"):
                    v = sorted(acc[m][key])
                    row[key] = {"median": v[len(v) // 2], "min": v[0],
                                "max": v[-1]}
                rows.append(row)
                print(json.dumps(row), flush=True)
        eng.close()
    with open(out_path, "w") as f:
        json.dump({"n": n, "d": d, "nq": nq, "topn": k, "nprobe": 32,
                   "rows": rows}, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--filter-first":
        filter_first_probe(sys.argv[2])
    else:
        main()
