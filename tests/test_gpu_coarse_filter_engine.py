"""Engine-level: coarse assign and a whole raw search return the same bits
whether IVFIndex::coarse_assign takes the seed-filtered path
(gk::coarse_select) or, with GAMMA_FUSE_COARSE=0, the full dots matrix.

Every setting runs in a fresh child process that builds the same small
IVFPQ table. At nlist = 1024 the default 4096 seed columns leave the table
on the old path under either setting, so a third child sets
GAMMA_COARSE_SEED_COLS=256, under which the filter does run; its results
must equal the other two as well. The children run side by side."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import numpy as np
import oracle as orc
from vearch_amd import GammaEngine, ktest

out, path = sys.argv[1], sys.argv[2]
N, D, NLIST, M, NPROBE, NQ, K = 40000, 32, 1024, 8, 16, 200, 10
base = orc.gen_clustered(N, D, seed=42, ncl=400)
q = orc.gen_queries(base, NQ, seed=1)
eng = GammaEngine(path=path)
eng.create_table(
    D, "IVFPQ",
    '{"ncentroids": %d, "nsubvector": %d, "metric_type": "L2", '
    '"training_threshold": %d}' % (NLIST, M, N))
eng.add(base)
eng.build_index()
cent, _ = eng.debug_model(NLIST, D, M)
pd, pl = eng.debug_coarse_assign(q, NPROBE)
res = {"cent": cent, "pd": pd, "pl": pl,
       "filters": np.array(ktest.coarse_can_filter(NQ, NLIST, D, NPROBE))}
for name, metric in (("l2", 1), ("ip", 2)):
    d, i = eng.raw_search(q, K, nprobe=NPROBE, rerank=100, metric=metric)
    res["d_" + name], res["i_" + name] = d, i
eng.close()
np.savez(out, **res)
"""

SETTINGS = {
    "default": {},
    "off": {"GAMMA_FUSE_COARSE": "0"},
    "seed256": {"GAMMA_COARSE_SEED_COLS": "256"},
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("coarse_filter")
    procs = {}
    for name, extra in SETTINGS.items():
        env = {k: v for k, v in os.environ.items()
               if not k.startswith("GAMMA_")}
        env.update(extra)
        procs[name] = subprocess.Popen(
            [sys.executable, "-c", CHILD, str(tmp / (name + ".npz")),
             str(tmp / ("table_" + name))],
            cwd=REPO, env=env, stdout=subprocess.PIPE,
            stderr=subprocess.STDOUT, text=True)
    res = {}
    for name, p in procs.items():
        log, _ = p.communicate(timeout=300)
        assert p.returncode == 0, (name, log[-2000:])
        res[name] = dict(np.load(tmp / (name + ".npz")))
    return res


def test_children_took_the_paths_they_were_meant_to(runs):
    assert not runs["default"]["filters"]  # nlist < 2 * 4096
    assert not runs["off"]["filters"]
    assert runs["seed256"]["filters"]
    for name in ("off", "seed256"):  # the same table everywhere
        assert np.array_equal(runs[name]["cent"], runs["default"]["cent"])


@pytest.mark.parametrize("name", ["off", "seed256"])
def test_coarse_assign_is_unchanged(runs, name):
    a, b = runs["default"], runs[name]
    assert np.array_equal(a["pl"], b["pl"])
    assert np.array_equal(a["pd"].view(np.uint32), b["pd"].view(np.uint32))
    assert (a["pl"] >= 0).all() and (np.diff(a["pd"], axis=1) >= 0).all()


@pytest.mark.parametrize("name", ["off", "seed256"])
def test_raw_search_is_unchanged(runs, name):
    a, b = runs["default"], runs[name]
    for m in ("l2", "ip"):
        assert np.array_equal(a["i_" + m], b["i_" + m])
        assert np.array_equal(a["d_" + m].view(np.uint32),
                              b["d_" + m].view(np.uint32))
