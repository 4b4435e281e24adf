"""Survivors of the primed wave select (gk::select_from_dots, k2 <= 192) on
a prepared bench index: loads the dump that `bench.py --index-dir DIR`
wrote, takes its centroids and its query batch, selects the top-nprobe of
the first --cols centroid columns through the counting kernel test hook,
primed and with GAMMA_SELECT_PRIME=0, and prints one JSON line: per mode the
mean, 99.9 % and maximum of the keys the walk admitted per query, how many
rows flushed before the closing sort, and whether the two key sets are equal.

    python tools/select_prime_probe.py --index-dir DIR [--workload W]
        [--cols 4096]
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
    ap.add_argument("--cols", type=int, default=4096)
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
    cols = min(args.cols, cfg["nlist"])

    Qd = torch.from_numpy(q).cuda()
    Bd = torch.from_numpy(np.ascontiguousarray(cent[:cols])).cuda()
    qn = torch.from_numpy(kt.row_norms(q)).cuda()
    bn = torch.from_numpy(kt.row_norms(cent[:cols])).cuda()
    dots = kt.dots_mfma(Qd, Bd)
    out = {"workload": args.workload, "nq": nq, "cols": cols,
           "nprobe": nprobe}
    keys = {}
    for mode in ("primed", "unprimed"):
        if mode == "unprimed":
            os.environ["GAMMA_SELECT_PRIME"] = "0"
        else:
            os.environ.pop("GAMMA_SELECT_PRIME", None)
        st, pushed, flushes = kt.select_wave_stats(
            dots, cols, nprobe, True, False, qnorms=qn, bnorms=bn)
        keys[mode] = kt.keys_to_np(st)
        out[mode] = {
            "pushed_mean": round(float(pushed.mean()), 2),
            "pushed_p999": int(np.quantile(pushed, 0.999)),
            "pushed_max": int(pushed.max()),
            "rows_flushing_mid_walk": int((flushes > 0).sum()),
        }
    os.environ.pop("GAMMA_SELECT_PRIME", None)
    out["keys_equal"] = bool(np.array_equal(keys["primed"],
                                            keys["unprimed"]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
