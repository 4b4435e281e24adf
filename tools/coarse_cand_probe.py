"""Candidate volume of the seed-filtered coarse assign (gk::coarse_select)
on a prepared bench index: loads the dump that `bench.py --index-dir DIR`
wrote, takes its centroids and its query batch, runs one coarse_select
through the kernel test hook and prints, as one JSON line, the mean and
the maximum of the per-query candidate counters, how many queries ran past
`cap`, and whether the keys equal the plain full-width pair's.

    python tools/coarse_cand_probe.py --index-dir DIR [--workload W]
        [--n1 4096,2048,1024] [--cap 1024]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--index-dir", required=True)
    ap.add_argument("--workload", default="ivfpq_d128_n10m_nprobe32")
    ap.add_argument("--n1", default="4096")
    ap.add_argument("--cap", type=int, default=1024)
    args = ap.parse_args()
    cfg = dict(bench.WORKLOADS[args.workload])

    import torch
    from vearch_amd import GammaEngine, ktest as kt

    eng = GammaEngine(path=args.index_dir)
    eng.create_table(cfg["d"], cfg["kind"], bench.index_params(cfg))
    eng.load()
    cent, _ = eng.debug_model(cfg["nlist"], cfg["d"], cfg["m"])
    eng.close()
    q = np.load(os.path.join(args.index_dir, "queries.npy"))
    nq, nprobe = q.shape[0], cfg["nprobe"]

    Qd = torch.from_numpy(q).cuda()
    Bd = torch.from_numpy(cent).cuda()
    qn = torch.from_numpy(kt.row_norms(q)).cuda()
    bn = torch.from_numpy(kt.row_norms(cent)).cuda()
    want = kt.keys_to_np(kt.select_from_dots(
        kt.dots_mfma(Qd, Bd), cfg["nlist"], nprobe, True, False,
        qnorms=qn, bnorms=bn))
    out = {"workload": args.workload, "nq": nq, "nlist": cfg["nlist"],
           "nprobe": nprobe, "cap": args.cap, "by_n1": {}}
    for n1 in [int(x) for x in args.n1.split(",")]:
        if not kt.coarse_can_filter(nq, cfg["nlist"], cfg["d"], nprobe, n1):
            out["by_n1"][str(n1)] = None
            continue
        keys, cnt, flag = kt.coarse_select(Qd, Bd, nprobe, True, False, n1,
                                           args.cap, qnorms=qn, bnorms=bn)
        out["by_n1"][str(n1)] = {
            "cand_mean": round(float(cnt.mean()), 2),
            "cand_max": int(cnt.max()),
            "cand_p999": int(np.quantile(cnt, 0.999)),
            "queries_over_cap": int((cnt > args.cap).sum()),
            "overflow_flag": flag,
            "keys_equal_full_width": bool(
                np.array_equal(kt.keys_to_np(keys), want)),
        }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
