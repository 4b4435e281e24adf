"""Share of scanned entries that the list bound of the 8-bit L2 scan skips
(gk::ivfpq_scan with its pruning block, DESIGN.md "Kernels" item 3) on a
prepared bench index: loads the dump that `bench.py --index-dir DIR` wrote,
rebuilds lists, S terms and coarse probes through the kernel test hooks and
runs the counting kernel for GAMMA_SCAN_PRUNE_HEAD = 1, 2 and 4. Counted,
not timed. Prints one JSON line: per head the mean, 99.9 % and worst (least
skipped) query's share of probed entries skipped, and whether the keys
equal those of GAMMA_SCAN_PRUNE=0.

    python tools/scan_prune_probe.py --index-dir DIR [--workload W]
        [--queries N]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def time_iid(path, rounds=7):
    """Where nothing prunes: the scan stage (HIP events, eng.last_timing)
    on an i.i.d. Gaussian table, d = 128, N = 2M, nlist = 4096, M = 32,
    nprobe = 32, 10 000 queries, recall_num 200; GAMMA_SCAN_PRUNE 0 / 1
    alternating, `rounds` each behind two warm-up searches per side."""
    from vearch_amd import GammaEngine
    d, n, nlist, M, nprobe, nq, k, k2 = 128, 2_000_000, 4096, 32, 32, \
        10_000, 10, 200
    rng = np.random.default_rng(17)
    eng = GammaEngine(path=path)
    eng.create_table(
        d, "IVFPQ",
        '{"ncentroids": %d, "nsubvector": %d, "metric_type": "L2", '
        '"training_threshold": %d}' % (nlist, M, 200_000))
    for c0 in range(0, n, 500_000):
        eng.add(rng.standard_normal((500_000, d), dtype=np.float32))
    eng.build_index()
    q = rng.standard_normal((nq, d), dtype=np.float32)
    res, us = {}, {"off": [], "on": []}
    for r in range(rounds + 2):
        for side in ("off", "on"):
            os.environ["GAMMA_SCAN_PRUNE"] = "1" if side == "on" else "0"
            res[side] = eng.raw_search(q, k, nprobe=nprobe, rerank=k2)
            if r >= 2:
                us[side].append(round(eng.last_timing()["scan_us"], 1))
    os.environ.pop("GAMMA_SCAN_PRUNE")
    eng.close()
    out = {"table": "iid gaussian d=128 N=2M nlist=4096 M=32 nprobe=32 "
                    "nq=10000 recall_num=200",
           "outputs_equal": bool(
               np.array_equal(res["on"][0], res["off"][0]) and
               np.array_equal(res["on"][1], res["off"][1]))}
    for side, v in us.items():
        out[side] = {"scan_us": v, "median": float(np.median(v)),
                     "spread": round(max(v) - min(v), 1)}
    out["on_within_off_median_plus_spread"] = bool(
        out["on"]["median"] <= out["off"]["median"] + out["off"]["spread"])
    print(json.dumps(out), flush=True)


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--index-dir", required=True)
    ap.add_argument("--workload", default="ivfpq_d128_n10m_nprobe32")
    ap.add_argument("--queries", type=int, default=0,
                    help="first N queries of the dump (0 = all)")
    ap.add_argument("--time-iid", action="store_true",
                    help="time the scan stage on an i.i.d. Gaussian table "
                         "built under --index-dir instead of counting")
    args = ap.parse_args()
    if args.time_iid:
        return time_iid(args.index_dir)
    cfg = dict(bench.WORKLOADS[args.workload])
    d, M, nlist, nprobe = cfg["d"], cfg["m"], cfg["nlist"], cfg["nprobe"]
    k2 = cfg.get("rerank", 200) or 200

    from vearch_amd import GammaEngine, ktest as kt

    eng = GammaEngine(path=args.index_dir)
    eng.create_table(d, cfg["kind"], bench.index_params(cfg))
    eng.load()
    cent, books = eng.debug_model(nlist, d, M)
    q = np.load(os.path.join(args.index_dir, "queries.npy"))
    if args.queries:
        q = q[:args.queries]
    pdists, probes = eng.debug_coarse_assign(q, nprobe)
    btab = kt.pq_tables_b(cent, books, M, 256)
    raw = []
    for ln in range(nlist):
        ids, codes = eng.debug_list(ln, M)
        ids = np.asarray(ids, dtype=np.int64)
        ids32 = np.where(ids < 0, (ids & 0x7FFFFFFF) | 0x80000000,
                         ids).astype(np.uint32)
        raw.append((ids32, np.asarray(codes, dtype=np.uint8).reshape(-1, M)))
    eng.close()
    # the S terms of all entries in one launch (the B table travels once)
    sizes = [len(i) for i, _ in raw]
    asg = np.repeat(np.arange(nlist, dtype=np.int32), sizes)
    sv = kt.pq_sterm(np.concatenate([c for _, c in raw]), btab, M, 256,
                     asg=asg)
    del btab
    cuts = np.cumsum([0] + sizes)
    lists = [(raw[ln][0], raw[ln][1], sv[cuts[ln]:cuts[ln + 1]])
             for ln in range(nlist)]

    out = {"workload": args.workload, "nq": int(q.shape[0]), "k2": k2,
           "nprobe": nprobe}
    os.environ["GAMMA_SCAN_PRUNE"] = "0"
    ref, _ = kt.ivfpq_scan_prune(lists, probes, pdists, q, cent, books, 1, k2)
    os.environ.pop("GAMMA_SCAN_PRUNE")
    for head in (1, 2, 4):
        os.environ["GAMMA_SCAN_PRUNE_HEAD"] = str(head)
        keys, st = kt.ivfpq_scan_prune(lists, probes, pdists, q, cent, books,
                                       1, k2, count=True)
        share = st[:, 1] / np.maximum(st[:, 2], 1)
        out["head_%d" % head] = {
            "skipped_share_of_all_entries":
                round(float(st[:, 1].sum() / max(st[:, 2].sum(), 1)), 4),
            "share_mean": round(float(share.mean()), 4),
            "share_p001": round(float(np.quantile(share, 0.001)), 4),
            "share_worst": round(float(share.min()), 4),
            "lists_skipped_mean": round(float(st[:, 0].mean()), 2),
            "keys_equal_off": bool(np.array_equal(keys, ref)),
        }
    os.environ.pop("GAMMA_SCAN_PRUNE_HEAD")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
